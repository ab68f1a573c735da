"""Fixed-radius search: the stream cursor of the search kernel, which reads a
group's bucket list in rounds of 64 points from per-entry run tables (where a
bucket's unread part starts, how much of it is left, and whether the bucket
went whole into the previous bucket's last round).  The shapes are the
smallest at which that schedule can go wrong; cases 1-3 first check on the CPU
that the list they are about exists in their data.  Every case is bit-exact
against the oracle: row splits, indices and, where asked for, distances."""
import numpy as np
import pytest
import torch

import oracle as O

pytestmark = pytest.mark.gpu

METRICS = ["L2", "L1", "Linf"]


def _uniform(rng, n):
    return rng.random((n, 3), dtype=np.float32)


def _in_one_voxel(rng, k, r):
    """k points 0.3 r wide, well inside one voxel (edge 2 r) of the unit cube."""
    vox = 2.0 * r
    cell = np.floor(rng.random(3) * (1.0 / vox - 1.0))
    return ((cell + 0.4) * vox + rng.random((k, 3)) * 0.3 * r).astype(np.float32)


def _visit_lengths(pts, q, r, factor):
    """Bucket lengths along the visit list of query q over the single batch item
    pts: the rule of the oracle's orc_query_bins (the query's voxel and those of
    the eight corners q +- r, hashed, sorted, repeats dropped) in numpy."""
    _, cell_splits, splits = O.build_spatial_hash_table(pts, r, None, factor)
    tsize = int(splits[1]) - int(splits[0])
    r32 = np.float32(r)
    inv = np.float32(1.0) / (np.float32(2.0) * r32)
    corners = [q.astype(np.float32)]
    for dz in (-1, 1):
        for dy in (-1, 1):
            for dx in (-1, 1):
                corners.append((q + r32 * np.float32([dx, dy, dz])).astype(np.float32))
    bins = set()
    for c in corners:
        v = [int(x) for x in np.floor(c * inv).astype(np.int32)]
        h = ((v[0] * 73856096) ^ (v[1] * 193649663) ^ (v[2] * 83492791)) & 0xffffffff  # 32-bit wrap-around
        if h >= 1 << 31:  # the 32-bit hash sign-extended to 64 bits, then taken as unsigned
            h += (1 << 64) - (1 << 32)
        bins.add(int(splits[0]) + h % tsize)
    return [int(cell_splits[b + 1]) - int(cell_splits[b]) for b in sorted(bins)]


def _check(cuda, pts, qry, r, prs, qrs, metric, full, factor=1 / 64):
    """One search against the oracle; `full`: ignore_query_point, distances and
    int64 indices, otherwise none of them."""
    from o3dml_amd import layers
    dt, ndt = (torch.int64, np.int64) if full else (torch.int32, np.int32)
    nns = layers.FixedRadiusSearch(metric=metric, ignore_query_point=full, return_distances=full, index_dtype=dt)
    res = nns(torch.from_numpy(pts).to(cuda), torch.from_numpy(qry).to(cuda), r, torch.from_numpy(prs),
              torch.from_numpy(qrs), hash_table_size_factor=factor)
    oi, ors, od = O.fixed_radius_search(pts, qry, r, prs, qrs, metric=metric, ignore_query_point=full,
                                        return_distances=full, index_dtype=ndt, hash_table_size_factor=factor)
    assert res.neighbors_index.dtype == dt
    assert np.array_equal(res.neighbors_row_splits.cpu().numpy(), ors)
    assert np.array_equal(res.neighbors_index.cpu().numpy(), oi)
    if full:
        assert np.array_equal(res.neighbors_distance.cpu().numpy(), od)
    return ors


def _self(cuda, pts, r, metric, full, factor=1 / 64):
    rs = np.array([0, len(pts)], np.int64)
    return _check(cuda, pts, pts, r, rs, rs, metric, full, factor)


@pytest.mark.parametrize("metric", METRICS)
def test_frs_rounds_many_tiny_segments(cuda, metric):
    """2,000 uniform points, r = 0.05, one bucket per two points: a list has up
    to nine buckets of about two points, so a round ends one bucket, takes the
    next whole, and the one after starts afresh, all the way down the list."""
    pts = _uniform(np.random.default_rng(0), 2000)
    r, factor = 0.05, 1 / 2
    lists = [[n for n in _visit_lengths(pts, q, r, factor) if n > 0] for q in pts[:64]]
    assert any(len(ls) >= 3 and sum(ls) < 64 for ls in lists)
    _self(cuda, pts, r, metric, False, factor)


@pytest.mark.parametrize("full", [False, True])
def test_frs_rounds_long_entries_and_multiples(cuda, full):
    """Clusters of 64, 128, 129 and 300 points, each inside one voxel, among 500
    uniform points at r = 0.02 with one bucket per point: buckets of exactly
    k x 64 points (a last round with every lane taken), of k x 64 + 1, and rows
    longer than the 64-entry temp rows."""
    rng = np.random.default_rng(0)
    r, factor = 0.02, 1.0
    sizes = (64, 128, 129, 300)
    clusters = [_in_one_voxel(rng, k, r) for k in sizes]
    pts = np.concatenate(clusters + [_uniform(rng, 500)])
    assert 128 in _visit_lengths(pts, clusters[1][0], r, factor)
    ors = _self(cuda, pts, r, "L2", full, factor)
    assert np.diff(ors).max() > 64


def test_frs_rounds_more_than_64_rounds(cuda):
    """8,192 points in [0, 0.3)^3 at r = 0.05 in 8 buckets of about 1,000: a
    group streams more than 64 rounds, a batch of seven several hundred."""
    pts = (_uniform(np.random.default_rng(0), 8192) * np.float32(0.3)).astype(np.float32)
    r, factor = 0.05, 1 / 1024
    assert max(sum(_visit_lengths(pts, q, r, factor)) for q in pts[:64]) > 64 * 64
    _self(cuda, pts, r, "L2", False, factor)


def test_frs_rounds_two_items_lists_end_apart(cuda):
    """Batch items of 3,000 and 37 points: the second item's one-bucket lists
    and the zero entries after them sit next to the first item's longer ones."""
    rng = np.random.default_rng(0)
    pts = np.concatenate([_uniform(rng, 3000), _uniform(rng, 37)])
    rs = np.array([0, 3000, 3037], np.int64)
    _check(cuda, pts, pts, 0.05, rs, rs, "L2", False)


def test_frs_rounds_queries_not_points(cuda):
    """1,000 queries over 5,000 points: the Morton query order, the same cursor."""
    rng = np.random.default_rng(0)
    pts, qry = _uniform(rng, 5000), _uniform(rng, 1000)
    _check(cuda, pts, qry, 0.05, np.array([0, 5000], np.int64), np.array([0, 1000], np.int64), "L2", False)
