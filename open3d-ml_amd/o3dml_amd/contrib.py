"""Drop-in for ``open3d.ml.contrib``: ``subsample`` / ``subsample_batch``
(KPConv grid subsampling) and the pairwise rotated-box
IoU ``iou_bev_cuda`` / ``iou_3d_cuda`` / ``iou_bev_cpu`` / ``iou_3d_cpu``.
numpy in, numpy out, as the reference calls them (dataprocessing.py:33-49,
kpconv.py:2099-2155; metrics/mAP.py:85-89, datasets/utils/operations.py:430).
Subsampling and the ``_cuda`` / ``_batch`` IoU run on the GPU; the ``_cpu``
IoU is the library's host routine (an API Open3D has, for data-loader workers
and machines without a GPU, not a fallback of the GPU path)."""
import numpy as np
import torch

from . import _lib, ops
from ._util import ptr, require_gpu, row_splits_host, stream_handle, to_dev


def _run(points, batches, features, classes, sampleDl, max_p):
    pts = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32))
    feat = None if features is None else torch.from_numpy(
        np.ascontiguousarray(np.asarray(features, np.float32).reshape(len(points), -1)))
    cls = None
    if classes is not None:
        cls = torch.from_numpy(np.ascontiguousarray(np.asarray(classes, np.int32).reshape(len(points), -1)))
    return ops.grid_subsample(pts, torch.from_numpy(np.asarray(batches, np.int64)), float(sampleDl),
                              features=feat, classes=cls, max_p=int(max_p))


def subsample(points, features=None, classes=None, sampleDl=0.1, verbose=0):
    """Grid subsampling (barycentres) -> points[, features][, classes]."""
    points = np.asarray(points, np.float32)
    out = _run(points, [len(points)], features, classes, sampleDl, 0)
    res = [out.points.numpy()]
    if features is not None:
        res.append(out.features.numpy())
    if classes is not None:
        c = out.classes.numpy()
        res.append(c.reshape(-1) if np.asarray(classes).ndim == 1 else c)
    return res[0] if len(res) == 1 else tuple(res)


def subsample_batch(points, batches, features=None, classes=None, sampleDl=0.1, method="barycenters", max_p=0,
                    verbose=0):
    """Per-batch-element grid subsampling -> (points, lengths int32[, features][, classes])."""
    if method != "barycenters":
        raise RuntimeError(f"subsample_batch: unsupported method {method!r}")
    points = np.asarray(points, np.float32)
    out = _run(points, batches, features, classes, sampleDl, max_p)
    res = [out.points.numpy(), out.lengths.numpy().astype(np.int32)]
    if features is not None:
        res.append(out.features.numpy())
    if classes is not None:
        c = out.classes.numpy()
        res.append(c.reshape(-1) if np.asarray(classes).ndim == 1 else c)
    return tuple(res)


# ---- pairwise rotated-box IoU (csrc/box_iou.hpp holds the contract) --------
_BEV, _3D = 0, 1
_WIDTH = {_BEV: 5, _3D: 7}
_NAME = {_BEV: "iou_bev", _3D: "iou_3d"}


def _boxes(what, arg, x, mode):
    a = np.ascontiguousarray(np.asarray(x), dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != _WIDTH[mode]:
        raise RuntimeError(f"{what}: {arg} must have shape [N, {_WIDTH[mode]}], got {list(a.shape)}")
    return a


def _iou_host(a, b, mode):
    out = np.empty((len(a), len(b)), np.float32)
    if out.size:
        _lib.call("o3dml_box_iou_host", a.ctypes.data, len(a), b.ctypes.data, len(b), mode, out.ctypes.data)
    return out


def _iou_device(a, a_rs, b, b_rs, mode):
    """All frames' [n_f, m_f] blocks back to back (float32, host) and their
    offsets: one launch, one device-to-host copy."""
    off = np.zeros(len(a_rs), np.int64)
    np.cumsum(np.diff(a_rs) * np.diff(b_rs), out=off[1:])
    total = int(off[-1])
    if total == 0:
        return np.empty(0, np.float32), off
    dev = torch.device("cuda", torch.cuda.current_device())
    a_d, b_d = to_dev(torch.from_numpy(a), dev), to_dev(torch.from_numpy(b), dev)
    a_rs_d, b_rs_d, off_d = to_dev(a_rs, dev), to_dev(b_rs, dev), to_dev(off, dev)
    out = torch.empty(total, dtype=torch.float32, device=dev)
    _lib.call("o3dml_box_iou_ragged", ptr(a_d), len(a), ptr(a_rs_d), ptr(b_d), len(b), ptr(b_rs_d), ptr(off_d),
              len(a_rs) - 1, total, mode, ptr(out), stream_handle(dev))
    return out.cpu().numpy(), off


def _iou_cuda(boxes_a, boxes_b, mode):
    what = _NAME[mode] + "_cuda"
    a, b = _boxes(what, "boxes_a", boxes_a, mode), _boxes(what, "boxes_b", boxes_b, mode)
    require_gpu()
    flat, _ = _iou_device(a, np.array([0, len(a)], np.int64), b, np.array([0, len(b)], np.int64), mode)
    return flat.reshape(len(a), len(b))


def _iou_cpu(boxes_a, boxes_b, mode):
    what = _NAME[mode] + "_cpu"
    return _iou_host(_boxes(what, "boxes_a", boxes_a, mode), _boxes(what, "boxes_b", boxes_b, mode), mode)


def _iou_batch(boxes_a, a_row_splits, boxes_b, b_row_splits, mode):
    what = _NAME[mode] + "_batch"
    a, b = _boxes(what, "boxes_a", boxes_a, mode), _boxes(what, "boxes_b", boxes_b, mode)
    a_rs, b_rs = row_splits_host(a_row_splits, len(a)), row_splits_host(b_row_splits, len(b))
    if len(a_rs) != len(b_rs):
        raise RuntimeError(f"{what}: a_row_splits has {len(a_rs) - 1} frames, b_row_splits {len(b_rs) - 1}")
    require_gpu()
    flat, off = _iou_device(a, a_rs, b, b_rs, mode)
    nf, mf = np.diff(a_rs), np.diff(b_rs)
    return [flat[off[f]:off[f + 1]].reshape(nf[f], mf[f]) for f in range(len(nf))]


def iou_bev_cuda(boxes_a, boxes_b):
    """Rotated BEV IoU of every pair, on the GPU: boxes_a [N,5], boxes_b [M,5]
    rows (cx, cy, w, l, ry) -> float32 [N,M].  Disjoint boxes give exactly 0."""
    return _iou_cuda(boxes_a, boxes_b, _BEV)


def iou_3d_cuda(boxes_a, boxes_b):
    """3D IoU of every pair, on the GPU: boxes_a [N,7], boxes_b [M,7] rows
    (x, y, z, w, h, l, ry) in the camera frame (y the bottom face, footprint
    in x-z) -> float32 [N,M]."""
    return _iou_cuda(boxes_a, boxes_b, _3D)


def iou_bev_cpu(boxes_a, boxes_b):
    """iou_bev_cuda's contract on the host: no GPU needed, safe in forked
    data-loader workers (box_collision_test, operations.py:430)."""
    return _iou_cpu(boxes_a, boxes_b, _BEV)


def iou_3d_cpu(boxes_a, boxes_b):
    """iou_3d_cuda's contract on the host."""
    return _iou_cpu(boxes_a, boxes_b, _3D)


def iou_bev_batch(boxes_a, a_row_splits, boxes_b, b_row_splits):
    """BEV IoU of many frames in one launch and one device-to-host copy: frame
    f pairs rows a_row_splits[f]:a_row_splits[f+1] of boxes_a with rows
    b_row_splits[f]:b_row_splits[f+1] of boxes_b -> list of float32 [n_f, m_f]
    (views of one buffer), bit-identical to per-frame iou_bev_cuda calls."""
    return _iou_batch(boxes_a, a_row_splits, boxes_b, b_row_splits, _BEV)


def iou_3d_batch(boxes_a, a_row_splits, boxes_b, b_row_splits):
    """iou_bev_batch for 3D IoU ([.,7] rows)."""
    return _iou_batch(boxes_a, a_row_splits, boxes_b, b_row_splits, _3D)
