"""Fixed-radius search: the one-pass set-up of a chunk's groups in the search
kernel (group leaders found by comparing every lane with its left neighbour,
runs with equal lists merged by the compare loop, the groups' boxes and lane
splits kept in lane tables).  Every case is
bit-exact against the oracle: row splits, indices and, where asked for,
distances."""
import numpy as np
import pytest
import torch

import oracle as O

pytestmark = pytest.mark.gpu

METRICS = ["L2", "L1", "Linf"]


def _uniform(rng, n):
    return rng.random((n, 3), dtype=np.float32)


def _cluster(rng, k, width):
    c = rng.random(3, dtype=np.float32) * 0.9 + 0.05
    return (c + rng.random((k, 3), dtype=np.float32) * width).astype(np.float32)


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


def _self(cuda, pts, r, metric, full):
    rs = np.array([0, len(pts)], np.int64)
    return _check(cuda, pts, pts, r, rs, rs, metric, full)


@pytest.mark.parametrize("metric", METRICS)
def test_frs_setup_equal_lists_not_adjacent(cuda, metric):
    """Queries that alternate between two tight clusters 256 r-cells apart
    along x (r = 0.01, centres 0.105 and 2.665): the cell coordinates wrap at
    2^8, so both clusters have one Morton key and the stable sort leaves them
    interleaved: every query is a run of its own, and the runs' lists repeat.
    The 64 points sit in the first cluster: its queries find all of them, the
    other cluster's queries none."""
    rng = np.random.default_rng(0)
    r = 0.01
    near = np.float32([0.105, 0.105, 0.105])
    away = np.float32([2.665, 0.105, 0.105])
    jitter = lambda n: ((rng.random((n, 3), dtype=np.float32) - 0.5) * 0.002).astype(np.float32)  # noqa: E731
    pts = near + jitter(64)
    qry = np.empty((128, 3), np.float32)
    qry[0::2] = near + jitter(64)
    qry[1::2] = away + jitter(64)
    ors = _check(cuda, pts, qry, r, np.array([0, 64], np.int64), np.array([0, 128], np.int64), metric, False)
    assert np.array_equal(np.diff(ors), np.tile([64, 0], 64))


def test_frs_setup_groups_at_every_lane(cuda):
    """2^18 points at r = 0.0045 (64 queries per wave, mostly single-query
    groups), 1,500 tight clusters (0.0008 wide) of 1 .. 64 points among them:
    groups of every size begin and end at every lane of a chunk, the row
    boundaries 15 / 16, 31 / 32 and 47 / 48 included."""
    rng = np.random.default_rng(0)
    pts = _uniform(rng, 1 << 18)
    at = 0
    for i in range(1500):
        k = i % 64 + 1
        pts[at:at + k] = _cluster(rng, k, 0.0008)
        at += k
    _self(cuda, pts, 0.0045, "L2", False)


def _clusters():
    """4,000 uniform points, tight clusters (0.004 wide) of 1 .. 64 points and a
    100-point blob 0.01 wide, r = 0.06: so few queries that a wave takes 16
    and lanes 16-63 join no group."""
    rng = np.random.default_rng(0)
    parts = [_uniform(rng, 4000)]
    for k in (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64):
        parts.append(_cluster(rng, k, 0.004))
    parts.append(_cluster(rng, 100, 0.01))
    return np.concatenate(parts), 0.06


@pytest.mark.parametrize("full", [False, True])
def test_frs_setup_few_queries_per_wave(cuda, full):
    pts, r = _clusters()
    _self(cuda, pts, r, "L2", full)


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("metric", METRICS)
def test_frs_setup_boxes_across_zero(cuda, metric, full):
    """4,000 points in [-0.5, 0.5)^3, 64 of them with +0.0 or -0.0 in one or
    more coordinates: group boxes that straddle zero or have a zero edge of
    either sign (the keys of the box reduce put -0 below +0)."""
    rng = np.random.default_rng(0)
    pts = (_uniform(rng, 4000) - np.float32(0.5)).astype(np.float32)
    rows = rng.choice(len(pts), 64, replace=False)
    for i, row in enumerate(rows):
        coords = [c for c in range(3) if (i % 7 + 1) >> c & 1]  # every non-empty subset of x, y, z
        for c in coords:
            pts[row, c] = np.float32(-0.0) if (i + c) % 2 else np.float32(0.0)
    assert np.signbit(pts[pts == 0]).any() and not np.signbit(pts[pts == 0]).all()
    _self(cuda, pts, 0.1, metric, full)


@pytest.mark.parametrize("full", [False, True])
def test_frs_setup_large_groups(cuda, full):
    """A 100-point blob 0.01 wide in 2,000 uniform points, r = 0.06: groups of
    more than 16 members and rows longer than the 64-entry temp rows."""
    rng = np.random.default_rng(0)
    pts = np.concatenate([_uniform(rng, 2000), _cluster(rng, 100, 0.01)])
    ors = _self(cuda, pts, 0.06, "L2", full)
    assert np.diff(ors).max() > 64


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("mode", ["0", "1"])
def test_frs_setup_batches_forced_order(cuda, mode, full, monkeypatch):
    """3,000 points, r = 0.02: about one group per query, so a chunk takes
    several box tables of seven groups; both self-search query orders."""
    monkeypatch.setenv("O3DML_FRS_SELF_ORDER", mode)
    pts = _uniform(np.random.default_rng(0), 3000)
    _self(cuda, pts, 0.02, "L2", full)
