"""Drop-in for ``open3d.ml.torch.ops`` on the point-cloud hot path.

Every function keeps the Open3D signature, argument meaning, output dtypes and
namedtuple field names the reference models bind to, and runs
on the HIP kernels of libo3dml_amd.so.  Inputs may live on the CPU (the
reference calls some ops from DataLoader workers on CPU tensors); they are then
staged to the GPU and the results returned on the CPU.  There is no CPU
compute path.
"""
import threading
from collections import OrderedDict, namedtuple

import numpy as np
import torch

from . import _lib
from ._util import (back_to, check_points, gpu_device, index_bits, metric_code, ptr,
                    row_splits_host, scalar, stream_handle, to_dev, workspace)

BuildSpatialHashTableResult = namedtuple(
    "build_spatial_hash_table", ["hash_table_index", "hash_table_cell_splits", "hash_table_splits"])
FixedRadiusSearchResult = namedtuple(
    "fixed_radius_search", ["neighbors_index", "neighbors_row_splits", "neighbors_distance"])
KnnSearchResult = namedtuple("knn_search", ["neighbors_index", "neighbors_row_splits", "neighbors_distance"])
RadiusSearchResult = namedtuple("radius_search", ["neighbors_index", "neighbors_row_splits", "neighbors_distance"])
VoxelizeResult = namedtuple(
    "voxelize", ["voxel_coords", "voxel_point_indices", "voxel_point_row_splits", "voxel_batch_splits"])
GridSubsampleResult = namedtuple("grid_subsample", ["points", "lengths", "features", "classes"])


# ---------------------------------------------------------------------------
# spatial hash table + fixed radius search  
# ---------------------------------------------------------------------------
def build_spatial_hash_table(points, radius, points_row_splits=None, hash_table_size_factor=1 / 64,
                             max_hash_table_size=33554432):
    """Open3D ``ops.build_spatial_hash_table`` (used by layers.FixedRadiusSearch;
    reference caller kpconv.py:2021-2023).  Cell size 2*radius; bins sized
    ``min(max(factor*N_b, 1), max_hash_table_size)`` per batch item.
    Returns (hash_table_index int32 [N], hash_table_cell_splits int32 [T+1],
    hash_table_splits int32 [B+1] on the CPU)."""
    dev = gpu_device(points)
    check_points("points", points)
    lib = _lib.load()
    n = points.shape[0]
    r = scalar(radius)
    if not r > 0:
        raise RuntimeError("radius must be > 0")
    prs = row_splits_host(points_row_splits, n)
    B = len(prs) - 1
    splits = np.zeros(B + 1, np.uint32)
    T = lib.o3dml_hash_table_splits(B, prs.ctypes.data, float(hash_table_size_factor),
                                    int(max_hash_table_size), splits.ctypes.data)
    pts = to_dev(points, dev)
    prs_d = to_dev(prs, dev)
    hts_d = to_dev(splits.view(np.int32), dev)
    index = torch.empty(n, dtype=torch.int32, device=dev)
    cells = torch.empty(T + 1, dtype=torch.int32, device=dev)
    ws = workspace(lib.o3dml_build_spatial_hash_table_workspace_size(n, T), dev)
    _lib.call("o3dml_build_spatial_hash_table", ptr(pts), n, r, B, ptr(prs_d), ptr(hts_d), splits.ctypes.data, T,
              ptr(index), ptr(cells), ptr(ws), ws.numel(), stream_handle(dev))
    return BuildSpatialHashTableResult(back_to(index, points), back_to(cells, points),
                                       torch.from_numpy(splits.astype(np.int32)))


def _same_cloud(points, queries, prs, qrs):
    return (points.data_ptr() == queries.data_ptr() and points.shape == queries.shape
            and np.array_equal(prs, qrs))


def _frs_count(points, queries, radius, points_row_splits, queries_row_splits, hash_table_splits,
               hash_table_index, hash_table_cell_splits, metric, ignore_query_point, return_distances):
    """Phase 1 of fixed_radius_search: neighbour counts -> device row splits.
    Returns (row_splits int64 [M+1] on the GPU, state for _frs_fill)."""
    dev = gpu_device(points, queries)
    check_points("points", points)
    check_points("queries", queries)
    mcode = metric_code(metric)
    lib = _lib.load()
    n, m = points.shape[0], queries.shape[0]
    r = scalar(radius)
    if not r > 0:
        raise RuntimeError("radius must be > 0")
    prs = row_splits_host(points_row_splits, n)
    qrs = row_splits_host(queries_row_splits, m)
    if len(prs) != len(qrs):
        raise RuntimeError("points_row_splits and queries_row_splits must have the same length")
    if hash_table_index is None:
        ht = build_spatial_hash_table(points, r, prs)
        hash_table_splits, hash_table_index, hash_table_cell_splits = (
            ht.hash_table_splits, ht.hash_table_index, ht.hash_table_cell_splits)
    same = _same_cloud(points, queries, prs, qrs)
    pts = to_dev(points, dev)
    qry = pts if same else to_dev(queries, dev)
    prs_d = to_dev(prs, dev)
    qrs_d = prs_d if same else to_dev(qrs, dev)
    hts_d = to_dev(hash_table_splits, dev, torch.int32)
    hti_d = to_dev(hash_table_index, dev, torch.int32)
    hcs_d = to_dev(hash_table_cell_splits, dev, torch.int32)
    B = len(prs) - 1
    st = stream_handle(dev)
    rs = torch.empty(m + 1, dtype=torch.int64, device=dev)
    ws = workspace(lib.o3dml_fixed_radius_search_workspace_size(n, m, B), dev)
    common = (ptr(pts), n, ptr(qry), m, r, B, ptr(prs_d), ptr(qrs_d), prs.ctypes.data, ptr(hts_d), ptr(hti_d),
              ptr(hcs_d), mcode, int(bool(ignore_query_point)), int(same), int(bool(return_distances)))
    _lib.call("o3dml_fixed_radius_search_count", *common, ptr(rs), ptr(ws), ws.numel(), st)
    # keep every buffer the fill phase reads alive in the state
    return rs, (common, ws, st, dev, (pts, qry, prs_d, qrs_d, hts_d, hti_d, hcs_d), prs, bool(return_distances))


def _frs_alloc(state, total, index_dtype):
    dev, with_dist = state[3], state[6]
    bits = index_bits(index_dtype)
    idx = torch.empty(total, dtype=torch.int32 if bits == 32 else torch.int64, device=dev)
    dist = torch.empty(total if with_dist else 0, dtype=torch.float32, device=dev)
    return idx, dist


def _frs_launch_fill(rs, state, idx, dist, capacity, parts):
    """Phase 2 (o3dml_fixed_radius_search_fill_bounded): parts 1 = row copy,
    2 = the re-run of rows longer than 64; capacity < 0: exact buffers,
    else a guess made before the total was read (nothing written if short)."""
    common, ws, st, _dev, _keep, _prs, with_dist = state
    bits = 32 if idx.dtype == torch.int32 else 64
    _lib.call("o3dml_fixed_radius_search_fill_bounded", *common, ptr(rs), bits, ptr(idx),
              ptr(dist) if with_dist else None, capacity, parts, ptr(ws), ws.numel(), st)


# One pinned host buffer per (device, host thread) for the totals read (a
# fresh pinned allocation per call can block the host until the device is
# idle, which would delay the fill launch behind the search); a thread reads
# its buffer before its next call writes it, and threads never share one.
_PINNED = {}


def _pinned_slot(device, n):
    key = (device, threading.get_ident())
    buf = _PINNED.get(key)
    if buf is None or buf.numel() < n:
        buf = torch.empty(max(n, 8), dtype=torch.int64, pin_memory=True)
        _PINNED[key] = buf
    return buf[:n]


# Neighbours per query of the last search per (radius, metric, points,
# queries): the capacity guess that lets the fill be queued before the host
# reads the total, so the GPU does not idle through that read.  A guess that
# proves too small costs one more (exact) fill; the rows are always the exact
# ones.  The key holds the cloud sizes, so a dense cloud's density is never
# applied to another call shape; a guess above _FRS_GUESS_MAX_BYTES reads the
# total first instead, and a result far below its capacity is returned as a
# compact copy (a view would keep the whole speculative buffer alive).
_FRS_DENSITY = {}
_FRS_HAD_OVER = {}  # call shapes whose last search had rows longer than 64
_FRS_GUESS_MAX_BYTES = 1 << 30
_FRS_SLACK = 1.25


def _frs_count_fill(rs, state, key, m, index_dtype, extra=None):
    """Fill with the total read after the (bounded, speculative) row copy when a
    density guess exists, else read first.  The overflow count (the plan's
    first int64) comes in the same host transfer, so the re-run of rows longer
    than 64 is launched only when there are any.  extra: more device scalars
    read in that transfer.  Returns (idx, dist, [total] + extra values)."""
    guess = _FRS_DENSITY.get(key)
    ws, st = state[1], state[2]
    # the totals go to pinned host memory right behind the count; the host
    # waits for them only, not for the fill queued after them
    if extra:
        n_over_dev = ws[:8].view(torch.int64)
        vals_dev = torch.stack([rs[-1], n_over_dev[0]] + list(extra))
        host = _pinned_slot(rs.device, vals_dev.numel())
        host.copy_(vals_dev, non_blocking=True)
    else:  # one small kernel writes both into the pinned buffer
        host = _pinned_slot(rs.device, 2)
        _lib.call("o3dml_fixed_radius_search_totals", ptr(rs), m, ptr(ws), host.data_ptr(), st)
    ready = torch.cuda.Event()
    ready.record(torch.cuda.current_stream(rs.device))
    cap = 0 if guess is None else int(m * guess * 1.0625) + 1024
    elem = (4 if index_bits(index_dtype) == 32 else 8) + (4 if state[6] else 0)
    if guess is None or m == 0 or cap * elem > _FRS_GUESS_MAX_BYTES:
        ready.synchronize()
        vals = host.tolist()
        idx, dist = _frs_alloc(state, int(vals[0]), index_dtype)
        _frs_launch_fill(rs, state, idx, dist, -1, 1 | (2 if vals[1] else 0))
    else:
        idx, dist = _frs_alloc(state, cap, index_dtype)
        _frs_launch_fill(rs, state, idx, dist, cap, 1)
        ready.synchronize()
        vals = host.tolist()
        total = int(vals[0])
        if total <= cap:
            if vals[1]:
                _frs_launch_fill(rs, state, idx, dist, cap, 2)
            compact = cap > _FRS_SLACK * total + 1024
            idx = idx[:total].clone() if compact else idx[:total]
            dist = (dist[:total].clone() if compact else dist[:total]) if dist.numel() else dist
        else:
            idx, dist = _frs_alloc(state, total, index_dtype)
            _frs_launch_fill(rs, state, idx, dist, -1, 1 | (2 if vals[1] else 0))
    if m > 0:
        _FRS_DENSITY[key] = int(vals[0]) / m
        if len(_FRS_DENSITY) > 64:
            _FRS_DENSITY.pop(next(iter(_FRS_DENSITY)))
    return idx, dist, [vals[0]] + vals[2:]


def fixed_radius_search(points, queries, radius, points_row_splits=None, queries_row_splits=None,
                        hash_table_splits=None, hash_table_index=None, hash_table_cell_splits=None,
                        index_dtype=torch.int32, metric="L2", ignore_query_point=False,
                        return_distances=False):
    """Open3D ``ops.fixed_radius_search``: for every query all
    points with dist <= radius (L2: squared distance <= r^2; L1; Linf), in the
    query's batch item.  Neighbour order: hash bins ascending, point id
    ascending inside a bin (the canonical order).  Distances are
    squared for L2.  Returns (neighbors_index [P], neighbors_row_splits int64
    [M+1], neighbors_distance [P] or [0])."""
    index_bits(index_dtype)
    rs, state = _frs_count(points, queries, radius, points_row_splits, queries_row_splits, hash_table_splits,
                           hash_table_index, hash_table_cell_splits, metric, ignore_query_point, return_distances)
    idx, dist, _ = _frs_count_fill(rs, state, (scalar(radius), metric_code(metric), points.shape[0], queries.shape[0]),
                                   queries.shape[0], index_dtype)
    return FixedRadiusSearchResult(back_to(idx, points), back_to(rs, points), back_to(dist, points))


def fixed_radius_search_dense(points, queries, radius, points_row_splits, queries_row_splits, hash_table=None):
    """Fixed-radius neighbours as a dense int32 matrix [M, max row length]
    padded with len(points) — kpconv.py batch_neighbors (:2002-2034) in one
    call: one host read for both the total and the width (the reference reads
    them separately), fill, densify.  GPU tensors in and out."""
    ht = hash_table
    rs, state = _frs_count(points, queries, radius, points_row_splits, queries_row_splits,
                           None if ht is None else ht.hash_table_splits,
                           None if ht is None else ht.hash_table_index,
                           None if ht is None else ht.hash_table_cell_splits, "L2", False, False)
    m = queries.shape[0]
    if m == 0:
        return torch.zeros((0, 0), dtype=torch.int32, device=rs.device)
    # the total and the width in one host read, after the fill is queued
    idx, _, (_total, width) = _frs_count_fill(rs, state, (scalar(radius), -1, points.shape[0], m), m, torch.int32,
                                              extra=[(rs[1:] - rs[:-1]).max()])
    width = int(width)
    return ragged_to_dense(idx.reshape(-1, 1), rs, width,
                           torch.tensor([points.shape[0]], dtype=torch.int32)).squeeze(2)


# layers.FixedRadiusSearch without a given table: the table build, the count,
# the totals and the speculative row copy in ONE library call
# (o3dml_fixed_radius_search_layer), the batch layout (row splits, table
# splits, their device copies, the workspace size) cached per layout — a
# small search costs one ctypes call and three allocations on the host.
_LAYER_PLANS = OrderedDict()
_LAYER_EVENTS = {}


def _splits_key(rs, n):
    if rs is None:
        return None, np.array([0, n], np.int64)
    if isinstance(rs, torch.Tensor) and rs.device.type == "cpu" and rs.dtype == torch.int64 and rs.dim() == 1:
        a = rs.numpy()
        return a.tobytes(), a
    a = row_splits_host(rs, n)
    return a.tobytes(), a


def _layer_plan(dev, st, n, m, points_row_splits, queries_row_splits, factor, max_table):
    pkey, prs = _splits_key(points_row_splits, n)
    qkey, qrs = (pkey, prs) if queries_row_splits is points_row_splits else _splits_key(queries_row_splits, m)
    key = (dev.index, st, n, m, pkey, qkey, float(factor), int(max_table))
    plan = _LAYER_PLANS.get(key)
    if plan is not None:
        _LAYER_PLANS.move_to_end(key)
        return plan
    # copies: the arrays may be views of the caller's tensors
    prs = row_splits_host(prs, n).copy()
    qrs = row_splits_host(qrs, m).copy()
    if len(prs) != len(qrs):
        raise RuntimeError("points_row_splits and queries_row_splits must have the same length")
    lib = _lib.load()
    B = len(prs) - 1
    splits = np.zeros(B + 1, np.uint32)
    T = lib.o3dml_hash_table_splits(B, prs.ctypes.data, float(factor), int(max_table), splits.ctypes.data)
    same_splits = np.array_equal(prs, qrs)
    # pinned, non-blocking uploads (a pageable copy would wait for the stream
    # to drain: KPFCNN's collate meets a new layout in every layer, its
    # subsampled sizes follow the random grid orientation)
    prs_d = to_dev(prs, dev)
    qrs_d = prs_d if same_splits else to_dev(qrs, dev)
    hts_d = to_dev(splits.view(np.int32), dev)
    plan = (prs, qrs, splits, T, prs_d, qrs_d, hts_d, same_splits,
            lib.o3dml_fixed_radius_search_layer_workspace_size(n, m, B, T))
    _LAYER_PLANS[key] = plan
    if len(_LAYER_PLANS) > 32:
        _LAYER_PLANS.popitem(last=False)
    return plan


class _LayerSearch:
    """A counted search of the one-call path: the arguments every later call
    repeats, the workspace, row splits and the hash table it was given or
    built (int32 [N + T + 1]: index, then cell splits)."""
    __slots__ = ("head", "tail", "ws", "ws_bytes", "rs", "tab", "keep", "n", "m", "dev", "st")


def _layer_count(points, queries, radius, points_row_splits, queries_row_splits, hash_table_size_factor=1 / 64,
                 max_hash_table_size=33554432, metric="L2", ignore_query_point=False, return_distances=False,
                 table=None, totals=None, sizes=None, count_done=None, index_bits_=32, idx=None, dist=None,
                 capacity=-1, stage=0):
    """Stage 0 of o3dml_fixed_radius_search_layer: the table build (or
    ``table``, a previous _LayerSearch over the same points at this radius),
    the count, totals (pinned) and/or sizes (device) and, with capacity >= 0,
    the speculative row copy.  Returns the _LayerSearch for the fills."""
    dev = gpu_device(points, queries)
    check_points("points", points)
    check_points("queries", queries)
    mcode = metric_code(metric)
    r = scalar(radius)
    if not r > 0:
        raise RuntimeError("radius must be > 0")
    n, m = points.shape[0], queries.shape[0]
    st = stream_handle(dev)
    prs, _qrs, splits, T, prs_d, qrs_d, hts_d, same_splits, ws_bytes = _layer_plan(
        dev, st, n, m, points_row_splits, queries_row_splits, hash_table_size_factor, max_hash_table_size)
    pts = points if points.device == dev and points.is_contiguous() else to_dev(points, dev)
    same = same_splits and points.data_ptr() == queries.data_ptr() and n == m
    qry = pts if same else (queries if queries.device == dev and queries.is_contiguous() else to_dev(queries, dev))
    x = _LayerSearch()
    x.ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    x.ws_bytes = ws_bytes
    x.rs = torch.empty(m + 1, dtype=torch.int64, device=dev)
    build = table is None
    x.tab = torch.empty(n + T + 1, dtype=torch.int32, device=dev) if build else table.tab
    x.head = (ptr(pts), n, ptr(qry), m, r, len(prs) - 1, ptr(prs_d), ptr(qrs_d), prs.ctypes.data, ptr(hts_d),
              splits.ctypes.data, T, ptr(x.tab), ptr(x.tab) + 4 * n)
    x.tail = (mcode, int(bool(ignore_query_point)), int(same), int(bool(return_distances)), ptr(x.rs))
    x.keep = (pts, qry, prs, prs_d, qrs_d, hts_d, splits)
    x.n, x.m, x.dev, x.st = n, m, dev, st
    _lib.call("o3dml_fixed_radius_search_layer", *x.head, int(build), *x.tail, None if totals is None else
              totals.data_ptr(), None if sizes is None else ptr(sizes), index_bits_, ptr(idx), ptr(dist), capacity,
              stage, count_done, ptr(x.ws), ws_bytes, st)
    return x


def _layer_fill(x, idx, dist, capacity, parts, index_bits_=32):
    """Stage 1..3 (parts) of a counted _LayerSearch into CSR buffers."""
    _lib.call("o3dml_fixed_radius_search_layer", *x.head, 0, *x.tail, None, None, index_bits_, ptr(idx), ptr(dist),
              capacity, parts, None, ptr(x.ws), x.ws_bytes, x.st)


def _layer_fill_dense(x, width, pad, parts):
    """The counted search as KPConv's dense neighbour matrix int32 [M, width]
    padded with `pad` (o3dml_fixed_radius_search_fill_dense)."""
    out = torch.empty((x.m, width), dtype=torch.int32, device=x.dev)
    h = x.head
    if x.m:
        _lib.call("o3dml_fixed_radius_search_fill_dense", h[2], h[1], h[3], h[4], h[5], h[6], h[7], h[8], h[9],
                  h[13], x.tail[0], x.tail[1], x.tail[4], width, pad, ptr(out), parts, ptr(x.ws), x.ws_bytes, x.st)
    return out


def _fixed_radius_search_layer(points, queries, radius, points_row_splits, queries_row_splits,
                               hash_table_size_factor, max_hash_table_size, index_dtype, metric,
                               ignore_query_point, return_distances):
    """layers.FixedRadiusSearch forward (table built here): the same result as
    build_spatial_hash_table + fixed_radius_search."""
    dev = gpu_device(points, queries)
    bits = index_bits(index_dtype)
    r = scalar(radius)
    m = queries.shape[0]
    key = (r, metric_code(metric), points.shape[0], m)
    guess = _FRS_DENSITY.get(key)
    # the previous call of this shape had rows longer than 64: their re-run is
    # queued with the copy (stage 4) so it runs beside it on the side stream
    early_over = key in _FRS_HAD_OVER
    elem = (4 if bits == 32 else 8) + (4 if return_distances else 0)
    cap = -1 if guess is None else int(m * guess * 1.0625) + 1024
    if cap * elem > _FRS_GUESS_MAX_BYTES:
        cap = -1
    itype = torch.int32 if bits == 32 else torch.int64
    idx = torch.empty(max(cap, 0), dtype=itype, device=dev)
    dist = torch.empty(max(cap, 0) if return_distances else 0, dtype=torch.float32, device=dev)
    host = _pinned_slot(dev, 2)
    ekey = (dev, threading.get_ident())  # per host thread, like the pinned totals
    ev = _LAYER_EVENTS.get(ekey)
    if ev is None:  # recorded by the library after the count, before the row copy
        ev = _LAYER_EVENTS[ekey] = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))  # creates the HIP event on this device
    x = _layer_count(points, queries, r, points_row_splits, queries_row_splits, hash_table_size_factor,
                     max_hash_table_size, metric, ignore_query_point, return_distances, totals=host,
                     count_done=ev.cuda_event, index_bits_=bits, idx=idx,
                     dist=dist if return_distances else None, capacity=cap, stage=4 if early_over else 0)
    ev.synchronize()
    total, n_over = host.tolist()
    if n_over:
        _FRS_HAD_OVER[key] = True
        if len(_FRS_HAD_OVER) > 64:
            _FRS_HAD_OVER.pop(next(iter(_FRS_HAD_OVER)))
    else:
        _FRS_HAD_OVER.pop(key, None)
    if cap < 0 or total > cap:  # no guess, or it was short: exact buffers, both parts
        idx = torch.empty(total, dtype=itype, device=dev)
        dist = torch.empty(total if return_distances else 0, dtype=torch.float32, device=dev)
        _layer_fill(x, idx, dist if return_distances else None, -1, 1 | (2 if n_over else 0), bits)
    else:
        if n_over and not early_over:
            _layer_fill(x, idx, dist if return_distances else None, cap, 2, bits)
        compact = cap > _FRS_SLACK * total + 1024
        idx = idx[:total].clone() if compact else idx[:total]
        if return_distances:
            dist = dist[:total].clone() if compact else dist[:total]
    if m > 0:
        _FRS_DENSITY[key] = total / m
        if len(_FRS_DENSITY) > 64:
            _FRS_DENSITY.pop(next(iter(_FRS_DENSITY)))
    return FixedRadiusSearchResult(back_to(idx, points), back_to(x.rs, points), back_to(dist, points))


# ---------------------------------------------------------------------------
# kNN
# ---------------------------------------------------------------------------
def knn_search(points, queries, k, points_row_splits=None, queries_row_splits=None,
               index_dtype=torch.int32, metric="L2", ignore_query_point=False, return_distances=False):
    """Open3D ``ops.knn_search``: per query the min(k, N_b) nearest points of
    its batch item, ascending (distance, index); distances squared for L2.
    Returns (neighbors_index [P], neighbors_row_splits int64 [M+1],
    neighbors_distance [P] or [0]).  Reference callers:
    point_transformer.py:724-729 (and, through core.nns, randlanet.py:218-229)."""
    dev = gpu_device(points, queries)
    check_points("points", points)
    check_points("queries", queries)
    bits = index_bits(index_dtype)
    mcode = metric_code(metric)
    k = int(k)
    if k < 1:
        raise RuntimeError("k must be >= 1")
    lib = _lib.load()
    n, m = points.shape[0], queries.shape[0]
    prs = row_splits_host(points_row_splits, n)
    qrs = row_splits_host(queries_row_splits, m)
    if len(prs) != len(qrs):
        raise RuntimeError("points_row_splits and queries_row_splits must have the same length")
    same = _same_cloud(points, queries, prs, qrs)
    pts = to_dev(points, dev)
    qry = pts if same else to_dev(queries, dev)
    prs_d = to_dev(prs, dev)
    qrs_d = prs_d if same else to_dev(qrs, dev)
    B = len(prs) - 1
    st = stream_handle(dev)
    rs = torch.empty(m + 1, dtype=torch.int64, device=dev)
    ws = workspace(lib.o3dml_knn_search_workspace_size(n, m, k, B), dev)
    _lib.call("o3dml_knn_search_count", ptr(pts), n, ptr(qry), m, k, B, ptr(prs_d), ptr(qrs_d), prs.ctypes.data,
              qrs.ctypes.data, mcode, int(bool(ignore_query_point)), int(same), ptr(rs), ptr(ws), ws.numel(), st)
    if ignore_query_point:
        total = int(rs[-1].item())
    else:  # min(k, N_b) per query: known on the host, no device read
        total = int(sum((qrs[b + 1] - qrs[b]) * min(k, prs[b + 1] - prs[b]) for b in range(B)))
    idx = torch.empty(total, dtype=torch.int32 if bits == 32 else torch.int64, device=dev)
    dist = torch.empty(total if return_distances else 0, dtype=torch.float32, device=dev)
    _lib.call("o3dml_knn_search_fill", ptr(pts), n, ptr(qry), m, k, B, ptr(qrs_d), prs.ctypes.data,
              qrs.ctypes.data, mcode, int(bool(ignore_query_point)), ptr(rs), bits, ptr(idx),
              ptr(dist) if return_distances else None, ptr(ws), ws.numel(), st)
    return KnnSearchResult(back_to(idx, points), back_to(rs, points), back_to(dist, points))


def radius_search(points, queries, radii, points_row_splits=None, queries_row_splits=None,
                  index_dtype=torch.int32, metric="L2", ignore_query_point=False, return_distances=False,
                  normalize_distances=False):
    """Open3D ``ops.radius_search`` (per-query radius; Open3D ml ops API,
    SURVEY §2.2 — no reference model calls it): per query q every point of its
    batch item with dist <= radii[q] (L2 squared against radii[q]^2), rows in
    ascending (distance, index) order; normalize_distances divides by radii[q]
    (L2: radii[q]^2).  Returns (neighbors_index [P], neighbors_row_splits int64
    [M+1], neighbors_distance [P] or [0])."""
    dev = gpu_device(points, queries, radii)
    check_points("points", points)
    check_points("queries", queries)
    bits = index_bits(index_dtype)
    mcode = metric_code(metric)
    lib = _lib.load()
    n, m = points.shape[0], queries.shape[0]
    rad = to_dev(torch.as_tensor(radii), dev, torch.float32).reshape(-1)
    if rad.numel() != m:
        raise RuntimeError(f"radii must have one entry per query ({m}), got {rad.numel()}")
    prs = row_splits_host(points_row_splits, n)
    qrs = row_splits_host(queries_row_splits, m)
    if len(prs) != len(qrs):
        raise RuntimeError("points_row_splits and queries_row_splits must have the same length")
    pts = to_dev(points, dev)
    qry = to_dev(queries, dev)
    prs_d = to_dev(prs, dev)
    qrs_d = to_dev(qrs, dev)
    B = len(prs) - 1
    st = stream_handle(dev)
    rs = torch.empty(m + 1, dtype=torch.int64, device=dev)
    ws = workspace(lib.o3dml_radius_search_workspace_size(n, m, B), dev)
    _lib.call("o3dml_radius_search_count", ptr(pts), n, ptr(qry), m, ptr(rad), B, ptr(prs_d), ptr(qrs_d), mcode,
              int(bool(ignore_query_point)), ptr(rs), ptr(ws), ws.numel(), st)
    host = _pinned_slot(rs.device, 2)
    _lib.call("o3dml_radius_search_totals", ptr(rs), m, ptr(ws), host.data_ptr(), st)
    torch.cuda.current_stream(dev).synchronize()
    total, max_row = (int(v) for v in host.tolist())
    long_rows = max_row > 8192
    idx = torch.empty(total, dtype=torch.int32 if bits == 32 else torch.int64, device=dev)
    dist = torch.empty(total if (return_distances or long_rows) else 0, dtype=torch.float32, device=dev)
    _lib.call("o3dml_radius_search_fill", ptr(pts), n, ptr(qry), m, ptr(rad), B, ptr(qrs_d), mcode,
              int(bool(ignore_query_point)), int(bool(normalize_distances)), ptr(rs), max_row, bits, ptr(idx),
              ptr(dist) if dist.numel() else None, ptr(ws), ws.numel(), st)
    if long_rows:  # rows past the LDS list were written unsorted
        rows = rs.cpu().numpy()
        _lib.call("o3dml_radius_search_sort_long_rows", n, m, B, rows.ctypes.data, bits, ptr(idx), ptr(dist),
                  ptr(ws), ws.numel(), st)
    if not return_distances:
        dist = torch.empty(0, dtype=torch.float32, device=dev)
    return RadiusSearchResult(back_to(idx, points), back_to(rs, points), back_to(dist, points))


# ---------------------------------------------------------------------------
# ragged helpers
# ---------------------------------------------------------------------------
def ragged_to_dense(values, row_splits, out_col_size, default_value):
    """Open3D ``ops.ragged_to_dense``: rows of a ragged tensor into
    [M, out_col_size, ...], truncated / padded with default_value
    (kpconv.py:2030-2032, point_pillars.py:364-366)."""
    dev = gpu_device(values, row_splits)
    vals = to_dev(values, dev)
    rs = to_dev(row_splits, dev, torch.int64)
    inner_shape = tuple(vals.shape[1:])
    inner = int(np.prod(inner_shape)) if inner_shape else 1
    dflt = to_dev(torch.as_tensor(default_value), dev, vals.dtype)
    if dflt.numel() == 1 and inner != 1:
        dflt = dflt.reshape(1).expand(inner).contiguous()
    if dflt.numel() != inner:
        raise RuntimeError(f"default_value must have shape {list(inner_shape)}, got {list(dflt.shape)}")
    M = rs.shape[0] - 1
    out_col_size = int(out_col_size)
    out = torch.empty((M, out_col_size) + inner_shape, dtype=vals.dtype, device=dev)
    _lib.call("o3dml_ragged_to_dense", ptr(vals), ptr(rs), M, out_col_size, inner, vals.element_size(), ptr(dflt), ptr(out),
              stream_handle(dev))
    return back_to(out, values)


def reduce_subarrays_sum(values, row_splits):
    """Open3D ``ops.reduce_subarrays_sum``: per-row sums (fp32, left to right;
    empty rows give 0) — sparseconvnet.py:319-324."""
    dev = gpu_device(values, row_splits)
    if values.dtype != torch.float32:
        raise RuntimeError(f"reduce_subarrays_sum: values must be float32, got {values.dtype}")
    vals = to_dev(values, dev)
    rs = to_dev(row_splits, dev, torch.int64)
    M = rs.shape[0] - 1
    out = torch.empty(M, dtype=torch.float32, device=dev)
    _lib.call("o3dml_reduce_subarrays_sum", ptr(vals), ptr(rs), M, ptr(out), stream_handle(dev))
    return back_to(out, values)


# ---------------------------------------------------------------------------
# voxelize
# ---------------------------------------------------------------------------
def _host_f32(x, ndim, name):
    a = np.ascontiguousarray(np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x,
                                        dtype=np.float32).reshape(-1))
    if a.size != ndim:
        raise RuntimeError(f"{name} must have {ndim} entries, got {a.size}")
    return a


def voxelize(points, row_splits, voxel_size, points_range_min, points_range_max,
             max_points_per_voxel=9223372036854775807, max_voxels=9223372036854775807):
    """Open3D ``ops.voxelize`` (point_pillars.py:352-357, sparseconvnet.py:293-298).
    Returns (voxel_coords int32 [V,D], voxel_point_indices int64 [P],
    voxel_point_row_splits int64 [V+1], voxel_batch_splits int64 [B+1]).
    Voxels ordered by (batch, linear id, dim 0 fastest); points of a voxel by
    index; caps keep the first voxels / points in that order."""
    dev = gpu_device(points)
    if points.dim() != 2 or points.dtype != torch.float32:
        raise RuntimeError("voxelize: points must be float32 [N, D]")
    lib = _lib.load()
    n, ndim = points.shape
    rs = row_splits_host(row_splits, n)
    B = len(rs) - 1
    vs = _host_f32(voxel_size, ndim, "voxel_size")
    mn = _host_f32(points_range_min, ndim, "points_range_min")
    mx = _host_f32(points_range_max, ndim, "points_range_max")
    pts = to_dev(points, dev)
    rs_d = to_dev(rs, dev)
    st = stream_handle(dev)
    ws = workspace(lib.o3dml_voxelize_workspace_size(n, B), dev)
    counts = np.zeros(2, np.int64)
    _lib.call("o3dml_voxelize_count", ptr(pts), n, ndim, B, ptr(rs_d), vs.ctypes.data, mn.ctypes.data,
              mx.ctypes.data, int(max_points_per_voxel), int(max_voxels), counts.ctypes.data, ptr(ws), ws.numel(), st)
    V, P = int(counts[0]), int(counts[1])
    coords = torch.empty((V, ndim), dtype=torch.int32, device=dev)
    pidx = torch.empty(P, dtype=torch.int64, device=dev)
    prs = torch.empty(V + 1, dtype=torch.int64, device=dev)
    bsp = torch.empty(B + 1, dtype=torch.int64, device=dev)
    _lib.call("o3dml_voxelize_fill", n, ndim, B, vs.ctypes.data, mn.ctypes.data, mx.ctypes.data, V, ptr(coords),
              ptr(pidx), ptr(prs), ptr(bsp), ptr(ws), ws.numel(), st)
    return VoxelizeResult(back_to(coords, points), back_to(pidx, points), back_to(prs, points), back_to(bsp, points))


def calculate_grid(in_positions):
    """Stride-2 output grid of sparseconvnet ``Convolution`` (reference
    sparseconvnet.py:388-401): unique all-even non-negative parents of
    trunc(pos) + {-1,0}^3, lexicographically sorted, + 0.5.  f32 [M,3]."""
    dev = gpu_device(in_positions)
    check_points("in_positions", in_positions)
    lib = _lib.load()
    n = in_positions.shape[0]
    pos = to_dev(in_positions, dev)
    st = stream_handle(dev)
    ws = workspace(lib.o3dml_calculate_grid_workspace_size(n), dev)
    m = np.zeros(1, np.int64)
    _lib.call("o3dml_calculate_grid_count", ptr(pos), n, m.ctypes.data, ptr(ws), ws.numel(), st)
    out = torch.empty((int(m[0]), 3), dtype=torch.float32, device=dev)
    _lib.call("o3dml_calculate_grid_fill", n, ptr(out), ptr(ws), ws.numel(), st)
    return back_to(out, in_positions)


# ---------------------------------------------------------------------------
# grid subsampling — backend of contrib.subsample(_batch)
# ---------------------------------------------------------------------------
def grid_subsample(points, lengths, sampleDl, features=None, classes=None, max_p=0):
    """KPConv grid subsampling per batch element (lengths int64 [B]).
    Returns (points [S,3], lengths int64 [B], features [S,F] | None,
    classes int32 [S,L] | None); cells in ascending key order, first max_p
    cells per element."""
    dev = gpu_device(points)
    check_points("points", points)
    lib = _lib.load()
    n = points.shape[0]
    lengths = np.asarray(lengths.cpu() if isinstance(lengths, torch.Tensor) else lengths, np.int64).reshape(-1)
    rs = np.zeros(len(lengths) + 1, np.int64)
    rs[1:] = np.cumsum(lengths)
    rs = row_splits_host(rs, n)
    B = len(rs) - 1
    pts = to_dev(points, dev)
    rs_d = to_dev(rs, dev)
    st = stream_handle(dev)
    ws = workspace(lib.o3dml_grid_subsample_workspace_size(n, B), dev)
    nout = np.zeros(1, np.int64)
    _lib.call("o3dml_grid_subsample_count", ptr(pts), n, B, ptr(rs_d), rs.ctypes.data, float(sampleDl), int(max_p),
              nout.ctypes.data, ptr(ws), ws.numel(), st)
    S = int(nout[0])
    fd = 0 if features is None else int(features.reshape(n, -1).shape[1])
    ld = 0 if classes is None else int(classes.reshape(n, -1).shape[1])
    f = None if features is None else to_dev(features.reshape(n, fd), dev, torch.float32)
    c = None if classes is None else to_dev(classes.reshape(n, ld), dev, torch.int32)
    out_p = torch.empty((S, 3), dtype=torch.float32, device=dev)
    out_f = torch.empty((S, fd), dtype=torch.float32, device=dev) if fd else None
    out_c = torch.empty((S, ld), dtype=torch.int32, device=dev) if ld else None
    out_l = torch.empty(B, dtype=torch.int64, device=dev)
    _lib.call("o3dml_grid_subsample_fill", ptr(pts), n, B, ptr(f), fd, ptr(c), ld, ptr(out_p), ptr(out_f),
              ptr(out_c), ptr(out_l), ptr(ws), ws.numel(), st)
    return GridSubsampleResult(back_to(out_p, points), back_to(out_l, points),
                               None if out_f is None else back_to(out_f, points),
                               None if out_c is None else back_to(out_c, points))


# ---------------------------------------------------------------------------
# PointNet++ ops
# ---------------------------------------------------------------------------
def _check_bn3(name, t):
    if t.dim() != 3 or t.shape[2] != 3 or t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be float32 [B, N, 3], got {t.dtype} {list(t.shape)}")


def furthest_point_sampling(points, sample_size):
    """Open3D ``ops.furthest_point_sampling`` (pointnet2_utils.py:55): points
    [B,N,3] -> int32 [B, sample_size]; greedy from index 0, squared L2, ties
    -> smallest index."""
    dev = gpu_device(points)
    _check_bn3("points", points)
    lib = _lib.load()
    B, N, _ = points.shape
    m = int(sample_size)
    pts = to_dev(points, dev)
    out = torch.empty((B, m), dtype=torch.int32, device=dev)
    ws = workspace(lib.o3dml_furthest_point_sampling_workspace_size(B, N), dev)
    _lib.call("o3dml_furthest_point_sampling", ptr(pts), B, N, m, ptr(out), ptr(ws), ws.numel(), stream_handle(dev))
    return back_to(out, points)


def ball_query(xyz, center, radius, nsample):
    """Open3D ``ops.ball_query`` (pointnet2_utils.py:212): first nsample points
    (index order) with d^2 < r^2, padded with the first hit, 0 if none."""
    dev = gpu_device(xyz, center)
    _check_bn3("xyz", xyz)
    _check_bn3("center", center)
    B, N, _ = xyz.shape
    M = center.shape[1]
    x, c = to_dev(xyz, dev), to_dev(center, dev)
    out = torch.empty((B, M, int(nsample)), dtype=torch.int32, device=dev)
    _lib.call("o3dml_ball_query", ptr(x), ptr(c), B, N, M, float(radius), int(nsample), ptr(out), stream_handle(dev))
    return back_to(out, xyz)


def three_nn(query_pts, data_pts):
    """Open3D ``ops.three_nn`` (pointnet2_utils.py:129): -> (dist2 [B,n,3], idx int32 [B,n,3])."""
    dev = gpu_device(query_pts, data_pts)
    _check_bn3("query_pts", query_pts)
    _check_bn3("data_pts", data_pts)
    B, n, _ = query_pts.shape
    m = data_pts.shape[1]
    q, d = to_dev(query_pts, dev), to_dev(data_pts, dev)
    dist = torch.empty((B, n, 3), dtype=torch.float32, device=dev)
    idx = torch.empty((B, n, 3), dtype=torch.int32, device=dev)
    _lib.call("o3dml_three_nn", ptr(q), ptr(d), B, n, m, ptr(dist), ptr(idx), stream_handle(dev))
    return back_to(dist, query_pts), back_to(idx, query_pts)


def three_interpolate(feats, idx, weights):
    """Open3D ``ops.three_interpolate`` (pointnet2_utils.py:162): feats [B,C,m],
    idx/weights [B,n,3] -> [B,C,n]."""
    dev = gpu_device(feats, idx, weights)
    B, C, m = feats.shape
    n = idx.shape[1]
    f = to_dev(feats, dev, torch.float32)
    i = to_dev(idx, dev, torch.int32)
    w = to_dev(weights, dev, torch.float32)
    out = torch.empty((B, C, n), dtype=torch.float32, device=dev)
    _lib.call("o3dml_three_interpolate", ptr(f), ptr(i), ptr(w), B, C, m, n, ptr(out), stream_handle(dev))
    return back_to(out, feats)


def three_interpolate_grad(grad_out, idx, weights, M):
    """Open3D ``ops.three_interpolate_grad`` (pointnet2_utils.py:184):
    grad_out [B,C,n] -> [B,C,M].  fp32 atomic accumulation, as the reference;
    under ``torch.use_deterministic_algorithms(True)`` a fixed-order gather
    (pairs grouped by source point with a stable radix sort) instead."""
    dev = gpu_device(grad_out, idx, weights)
    B, C, n = grad_out.shape
    g = to_dev(grad_out, dev, torch.float32)
    i = to_dev(idx, dev, torch.int32)
    w = to_dev(weights, dev, torch.float32)
    out = torch.empty((B, C, int(M)), dtype=torch.float32, device=dev)
    if torch.are_deterministic_algorithms_enabled():
        ws = workspace(_lib.load().o3dml_three_interpolate_grad_workspace_size(B, n, int(M)), dev)
        _lib.call("o3dml_three_interpolate_grad_det", ptr(g), ptr(i), ptr(w), B, C, n, int(M), ptr(out), ptr(ws),
                  ws.numel(), stream_handle(dev))
        return back_to(out, grad_out)
    _lib.call("o3dml_three_interpolate_grad", ptr(g), ptr(i), ptr(w), B, C, n, int(M), ptr(out), stream_handle(dev))
    return back_to(out, grad_out)


# ---------------------------------------------------------------------------
# PVCNN ops (pvcnn.py:14, 37, 57)
# ---------------------------------------------------------------------------
def _f32_3d(name, t, what):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 3:
        raise RuntimeError(f"{name} must be float32 {what}, got "
                           f"{getattr(t, 'dtype', type(t))} {list(getattr(t, 'shape', []))}")


def trilinear_devoxelize_forward(resolution, is_training, coords, features):
    """Open3D ``ops.trilinear_devoxelize_forward`` (pvcnn.py:37): coords
    [B,3,N] in grid units (clamped to [0, r-1]), features [B,C,r,r,r] or
    [B,C,r^3] -> (outs [B,C,N], inds int32 [B,8,N], wgts [B,8,N]).  Corner
    k = 4 bx + 2 by + bz; the high corner of an axis is lo + (frac > 0), so an
    integer coordinate never indexes past the grid.  inds / wgts are written
    when is_training and are zeros otherwise (the reference never reads them
    in eval mode)."""
    dev = gpu_device(coords, features)
    r = int(resolution)
    if r < 1:
        raise RuntimeError(f"trilinear_devoxelize_forward: resolution must be >= 1, got {r}")
    _f32_3d("coords", coords, "[B, 3, N]")
    if coords.shape[1] != 3:
        raise RuntimeError(f"coords must be float32 [B, 3, N], got {list(coords.shape)}")
    if not isinstance(features, torch.Tensor) or features.dtype != torch.float32 or features.dim() not in (3, 5):
        raise RuntimeError("features must be float32 [B, C, r, r, r] or [B, C, r^3], got "
                           f"{getattr(features, 'dtype', type(features))} {list(getattr(features, 'shape', []))}")
    B, _, N = coords.shape
    C = features.shape[1]
    spatial = tuple(features.shape[2:])
    if features.shape[0] != B or spatial not in ((r, r, r), (r ** 3,)):
        raise RuntimeError(f"features {list(features.shape)} do not match coords {list(coords.shape)} at "
                           f"resolution {r}")
    c = to_dev(coords.detach(), dev)
    f = to_dev(features.detach(), dev)
    outs = torch.empty((B, C, N), dtype=torch.float32, device=dev)
    inds = torch.empty((B, 8, N), dtype=torch.int32, device=dev)
    wgts = torch.empty((B, 8, N), dtype=torch.float32, device=dev)
    _lib.call("o3dml_trilinear_devoxelize_forward", ptr(c), ptr(f), B, C, N, r, int(bool(is_training)), ptr(outs),
              ptr(inds), ptr(wgts), stream_handle(dev))
    return back_to(outs, coords), back_to(inds, coords), back_to(wgts, coords)


def trilinear_devoxelize_backward(grad_y, indices, weights, resolution):
    """Open3D ``ops.trilinear_devoxelize_backward`` (pvcnn.py:57): grad_y
    [B,C,N], indices int32 / weights [B,8,N] -> [B,C,r^3].  Each voxel sums its
    entries in ascending position of the [8,N] layout (per-voxel lists from a
    stable sort; no float atomics): bitwise reproducible.  Indices outside
    [0, r^3) contribute nothing.  Worst case: with every point on one corner
    a single lane sums 8 N terms per channel."""
    dev = gpu_device(grad_y, indices, weights)
    r = int(resolution)
    if r < 1:
        raise RuntimeError(f"trilinear_devoxelize_backward: resolution must be >= 1, got {r}")
    _f32_3d("grad_y", grad_y, "[B, C, N]")
    _f32_3d("weights", weights, "[B, 8, N]")
    B, C, N = grad_y.shape
    if not isinstance(indices, torch.Tensor) or indices.dtype != torch.int32 or tuple(indices.shape) != (B, 8, N):
        raise RuntimeError(f"indices must be int32 [{B}, 8, {N}], got "
                           f"{getattr(indices, 'dtype', type(indices))} {list(getattr(indices, 'shape', []))}")
    if tuple(weights.shape) != (B, 8, N):
        raise RuntimeError(f"weights must be float32 [{B}, 8, {N}], got {list(weights.shape)}")
    g = to_dev(grad_y.detach(), dev)
    i = to_dev(indices, dev)
    w = to_dev(weights.detach(), dev)
    out = torch.empty((B, C, r ** 3), dtype=torch.float32, device=dev)
    if out.numel():
        ws = workspace(_lib.load().o3dml_trilinear_devoxelize_backward_workspace_size(B, N, r), dev)
        _lib.call("o3dml_trilinear_devoxelize_backward", ptr(g), ptr(i), ptr(w), B, C, N, r, ptr(out), ptr(ws),
                  ws.numel(), stream_handle(dev))
    return back_to(out, grad_y)


# ---------------------------------------------------------------------------
# sparse convolution — see sparse_conv.py
def nms(boxes, scores, nms_overlap_thresh):
    """Open3D ``ops.nms`` (objdet_helper.py:27, called at :346): rotated BEV NMS.
    boxes f32 [N,5] (x1,y1,x2,y2,yaw), scores f32 [N] -> int64 kept indices in
    descending-score order (stable for ties); IoU > threshold suppresses.

    Scores are ranked by a total order: -0 equals +0 and NaN ranks below -inf
    (so a NaN-scored box is visited last, never first).  The suppression mask
    is N*ceil(N/64)*8 bytes of workspace (N^2/8: 1.25 MiB at 3,200 boxes,
    512 MiB at the cap); N is limited to 65,536 boxes and a larger call raises
    RuntimeError before anything is allocated."""
    dev = gpu_device(boxes, scores)
    if boxes.dim() != 2 or boxes.shape[1] != 5:
        raise RuntimeError("nms: boxes must be [N, 5], got %s" % (tuple(boxes.shape),))
    if scores.dim() != 1 or scores.shape[0] != boxes.shape[0]:
        raise RuntimeError("nms: scores must be [N] matching boxes")
    lib = _lib.load()
    n = boxes.shape[0]
    if n > 65536:
        raise RuntimeError("nms: %d boxes exceed the 65,536-box cap (N^2/8-byte suppression mask)" % n)
    b = to_dev(boxes, dev, torch.float32)
    s = to_dev(scores, dev, torch.float32)
    keep = torch.empty((max(n, 1),), dtype=torch.int64, device=dev)
    count = torch.zeros((1,), dtype=torch.int64, device=dev)
    ws = workspace(lib.o3dml_nms_workspace_size(n), dev)
    _lib.call("o3dml_nms", ptr(b), ptr(s), n, float(nms_overlap_thresh), ptr(keep), ptr(count), ptr(ws),
              ws.numel(), stream_handle(dev))
    return back_to(keep[:int(count.item())], boxes)


# ---------------------------------------------------------------------------
# RoI point pooling (PointRCNN, roipool3d_utils.py:24)
# ---------------------------------------------------------------------------
ROI_POOL_MAX_SAMPLES = 8192


def _roi_pool(xyz, boxes3d, pts_feature, sampled_pts_num, with_index):
    dev = gpu_device(xyz, boxes3d, pts_feature)
    for name, t, last in (("xyz", xyz, 3), ("boxes3d", boxes3d, 7), ("pts_feature", pts_feature, None)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 3 or (
                last is not None and t.shape[2] != last):
            raise RuntimeError(f"roi_pool: {name} must be float32 [B, *, {'C' if last is None else last}], got "
                               f"{getattr(t, 'dtype', type(t))} {list(getattr(t, 'shape', []))}")
        if not t.is_contiguous():
            raise RuntimeError(f"roi_pool: {name} must be contiguous")
    B, N, _ = xyz.shape
    M, C, S = boxes3d.shape[1], pts_feature.shape[2], int(sampled_pts_num)
    if boxes3d.shape[0] != B or pts_feature.shape[0] != B or pts_feature.shape[1] != N:
        raise RuntimeError(f"roi_pool: xyz {list(xyz.shape)}, boxes3d {list(boxes3d.shape)} and pts_feature "
                           f"{list(pts_feature.shape)} do not share B and N")
    if not 1 <= S <= ROI_POOL_MAX_SAMPLES:
        raise RuntimeError(f"roi_pool: sampled_pts_num must be in 1..{ROI_POOL_MAX_SAMPLES}, got {S}")
    x, b, f = to_dev(xyz.detach(), dev), to_dev(boxes3d.detach(), dev), to_dev(pts_feature.detach(), dev)
    pooled = torch.empty((B, M, S, 3 + C), dtype=torch.float32, device=dev)
    flag = torch.empty((B, M), dtype=torch.int32, device=dev)
    idx = torch.empty((B, M, S), dtype=torch.int32, device=dev) if with_index else None
    if B * M:
        _lib.call("o3dml_roi_pool", ptr(x), ptr(b), ptr(f), B, N, M, C, S, ptr(pooled), ptr(flag), ptr(idx),
                  stream_handle(dev))
    return back_to(pooled, xyz), back_to(flag, xyz), None if idx is None else back_to(idx, xyz)


def roi_pool_indexed(xyz, boxes3d, pts_feature, sampled_pts_num):
    """roi_pool plus the pooled point index per slot: -> (pooled_features,
    pooled_empty_flag, index int32 [B, M, sampled_pts_num], -1 in an empty
    box).  Not an Open3D name."""
    return _roi_pool(xyz, boxes3d, pts_feature, sampled_pts_num, True)


def roi_pool(xyz, boxes3d, pts_feature, sampled_pts_num):
    """Open3D ``ops.roi_pool`` (roipool3d_utils.py:24): xyz [B,N,3], boxes3d
    [B,M,7] = (x, y, z, h, w, l, ry) in the camera frame (y the bottom face),
    pts_feature [B,N,C] -> (pooled_features f32 [B,M,S,3+C], pooled_empty_flag
    int32 [B,M]).  Per box the first S points inside it in ascending index
    (closed bounds, float32, a 10 m per-axis prefilter around the centre), as
    rows [xyz | feature]; fewer than S repeat cyclically, none gives flag 1
    and zeros.  The contract is spelled out in csrc/roi_pool.hip."""
    pooled, flag, _ = _roi_pool(xyz, boxes3d, pts_feature, sampled_pts_num, False)  # no index written
    return pooled, flag


# ---------------------------------------------------------------------------
from .sparse_conv import sparse_conv, sparse_conv_transpose  # noqa: E402,F401


__all__ = ["build_spatial_hash_table", "fixed_radius_search", "knn_search", "radius_search", "ragged_to_dense",
           "reduce_subarrays_sum", "voxelize", "grid_subsample", "calculate_grid", "furthest_point_sampling",
           "ball_query", "three_nn", "three_interpolate", "three_interpolate_grad", "nms", "sparse_conv",
           "sparse_conv_transpose", "trilinear_devoxelize_forward", "trilinear_devoxelize_backward", "roi_pool"]
