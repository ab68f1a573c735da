"""Fixed-radius search: the batched group set-up of the search kernel (all
groups of a 64-query chunk found first, the bucket lists of seven groups built
in one pass).  Every case is bit-exact against the oracle: row splits, indices
and, where asked for, distances."""
import numpy as np
import pytest
import torch

import oracle as O

pytestmark = pytest.mark.gpu

METRICS = ["L2", "L1", "Linf"]


def _uniform(rng, n):
    return rng.random((n, 3), dtype=np.float32)


def _sparse():
    """3,000 points, r = 0.02: nearly every (voxel, octant) group is a single
    query, so a chunk has about as many groups as queries and takes several
    batches of seven (at this size a wave takes 16 queries: 7 + 7 + 2)."""
    return _uniform(np.random.default_rng(0), 3000), 0.02


def _bench_like():
    """8,192 points, r = 0.1: the points per octant of the 65,536-point r = 0.05
    bench scenes, so groups of about eight queries that start and end inside
    chunks (at this size a wave takes 16 queries; the bench batch itself, 64
    per wave with a full and a partial batch, is test_frs_bench_batch_bit_exact)."""
    return _uniform(np.random.default_rng(0), 8192), 0.1


def _clusters():
    """4,000 uniform points, tight clusters (0.004 wide) of 1 .. 64 points and a
    100-point blob 0.01 wide, r = 0.06: groups from one query to a full wave,
    and rows longer than the 64-entry temp rows (re-run one query per wave)."""
    rng = np.random.default_rng(0)
    parts = [_uniform(rng, 4000)]
    for k in (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64):
        c = rng.random(3, dtype=np.float32) * 0.9 + 0.05
        parts.append((c + rng.random((k, 3), dtype=np.float32) * 0.004).astype(np.float32))
    c = rng.random(3, dtype=np.float32) * 0.9 + 0.05
    parts.append((c + rng.random((100, 3), dtype=np.float32) * 0.01).astype(np.float32))
    return np.concatenate(parts), 0.06


SHAPES = {"sparse": _sparse, "bench_like": _bench_like, "clusters": _clusters}


def _check(cuda, pts, qry, r, prs, qrs, metric, full):
    """One search against the oracle; `full`: ignore_query_point, distances and
    int64 indices, otherwise none of them."""
    from o3dml_amd import layers
    dt, ndt = (torch.int64, np.int64) if full else (torch.int32, np.int32)
    nns = layers.FixedRadiusSearch(metric=metric, ignore_query_point=full, return_distances=full, index_dtype=dt)
    res = nns(torch.from_numpy(pts).to(cuda), torch.from_numpy(qry).to(cuda), r, torch.from_numpy(prs),
              torch.from_numpy(qrs))
    oi, ors, od = O.fixed_radius_search(pts, qry, r, prs, qrs, metric=metric, ignore_query_point=full,
                                        return_distances=full, index_dtype=ndt)
    assert res.neighbors_index.dtype == dt
    assert np.array_equal(res.neighbors_row_splits.cpu().numpy(), ors)
    assert np.array_equal(res.neighbors_index.cpu().numpy(), oi)
    if full:
        assert np.array_equal(res.neighbors_distance.cpu().numpy(), od)
    return ors


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_frs_groups_self_search(cuda, shape, metric, full):
    pts, r = SHAPES[shape]()
    rs = np.array([0, len(pts)], np.int64)
    ors = _check(cuda, pts, pts, r, rs, rs, metric, full)
    if shape == "clusters":
        # the case is there for the long rows: it may not pass by missing them
        assert np.diff(ors).max() > 64


@pytest.mark.parametrize("metric", METRICS)
def test_frs_groups_general_query_order(cuda, metric):
    """Queries that are not the points, items of 4,000 and 8,000 points (tables
    that are no powers of two) and an empty item between them: the Morton
    order of the general path, where equal bin lists need not be adjacent."""
    rng = np.random.default_rng(0)
    pts = _uniform(rng, 12000)
    qry = _uniform(rng, 9000)
    prs = np.array([0, 4000, 4000, 12000], np.int64)
    qrs = np.array([0, 3000, 3000, 9000], np.int64)
    _check(cuda, pts, qry, 0.1, prs, qrs, metric, metric == "L1")


def test_frs_groups_many_batches_of_full_chunks(cuda):
    """2^18 points at the density of the sparse case (r = 0.0045): enough
    queries for 64 per wave, so a chunk of mostly single-query groups takes
    about nine batches."""
    pts = _uniform(np.random.default_rng(0), 1 << 18)
    rs = np.array([0, len(pts)], np.int64)
    _check(cuda, pts, pts, 0.0045, rs, rs, "L2", False)


@pytest.mark.parametrize("mode", ["0", "1"])
def test_frs_groups_forced_order(cuda, mode, monkeypatch):
    """The many-groups case with the self-search query order forced either way."""
    monkeypatch.setenv("O3DML_FRS_SELF_ORDER", mode)
    pts, r = _sparse()
    rs = np.array([0, len(pts)], np.int64)
    _check(cuda, pts, pts, r, rs, rs, "L2", True)


@pytest.mark.parametrize("full", [False, True])
def test_frs_groups_chunk_sizes(cuda, full):
    """Items of 1, 63 and 65 points in one batch: partial chunks, and so few
    queries that a wave takes 16."""
    sizes = [1, 63, 65]
    pts = _uniform(np.random.default_rng(0), sum(sizes))
    rs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    _check(cuda, pts, pts, 0.3, rs, rs, "L2", full)
