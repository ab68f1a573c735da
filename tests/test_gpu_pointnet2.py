"""PointNet++ kernels (csrc/pointnet2.hip) at ties, boundaries and odd shapes:
furthest-point sampling, ball_query and three_nn bit for bit against float64
numpy references on inputs whose fp32 arithmetic is exact (tests/
exact_cases.py, validated against the oracle by tests/test_exact_cases.py),
three_interpolate and its two gradients within derived rounding bounds of
float64, and the status paths that return before any launch."""
import numpy as np
import pytest
import torch

import exact_cases as X
import oracle as O

pytestmark = pytest.mark.gpu


def _t(a, dev):
    return torch.tensor(a).to(dev)  # a copy: the cases are read-only


# ------------------------------------------------------------------ FPS
@pytest.mark.parametrize("name", list(X.fps_cases()))
def test_fps_exact(cuda, name):
    """Every ITEMS instantiation at both edges (n = 1024 k and 1024 k + 1), the
    global-memory fallback (n > 32768), m > n, m = 1, m = n, duplicates and
    distances beyond the 1e10 the min-distances start from: ties go to the
    smallest index in the per-lane order, the shuffle tree and the LDS
    exchange alike."""
    from o3dml_amd import ops
    c = X.fps_cases()[name]
    got = ops.furthest_point_sampling(_t(c["xyz"], cuda), c["m"]).cpu().numpy()
    assert got.dtype == np.int32 and got.shape == c["ref"].shape
    assert np.array_equal(got, c["ref"]), f"{int((got != c['ref']).sum())} of {got.size} entries differ"
    if c["kind"] == "perm":
        assert all(np.array_equal(np.sort(r), np.arange(c["m"])) for r in got)


def test_fps_random_floats_by_property(cuda):
    """General fp32 input: no bitwise claim, but each pick must be a furthest
    point up to the fp32 error of a squared distance (one rounding per
    difference and three in the fma chain, about 5 * 2^-24 = 3e-7 < 1e-6)."""
    from o3dml_amd import ops
    c = X.fps_random_case()
    got = ops.furthest_point_sampling(_t(c["xyz"], cuda), c["m"]).cpu().numpy()
    assert got.shape == (3, 64)
    assert X.fps_property_violations(c["xyz"], got, margin=1e-6) == []


# ------------------------------------------------------------------ ball_query
@pytest.mark.parametrize("name", list(X.ball_cases()))
def test_ball_query_exact(cuda, name):
    """Rows with no, some, exactly nsample and more than nsample hits, pairs
    with d2 == r2 (excluded), queries of one workgroup finishing in different
    tiles, n and M off the 256 tile."""
    from o3dml_amd import ops
    c = X.ball_cases()[name]
    got = ops.ball_query(_t(c["xyz"], cuda), _t(c["ctr"], cuda), c["r"], c["nsample"]).cpu().numpy()
    assert got.dtype == np.int32 and got.shape == c["ref"].shape
    rows = (got != c["ref"]).any(-1)
    assert not rows.any(), f"{int(rows.sum())} of {rows.size} rows differ"


# ------------------------------------------------------------------ three_nn
@pytest.mark.parametrize("name", list(X.three_nn_cases()))
def test_three_nn_exact(cuda, name):
    """Fewer than three known points (inf / index 0 in the missing slots), m
    around the 256 tile, and ties between third and fourth place in a third
    to a half of the rows: the earlier index wins."""
    from o3dml_amd import ops
    c = X.three_nn_cases()[name]
    d, i = ops.three_nn(_t(c["unknown"], cuda), _t(c["known"], cuda))
    d, i = d.cpu().numpy(), i.cpu().numpy()
    assert i.dtype == np.int32 and d.dtype == np.float32
    rows = (i != c["idx"]).any(-1)
    assert not rows.any(), f"indices of {int(rows.sum())} of {rows.size} rows differ"
    assert np.array_equal(d, c["dist"])


# ------------------------------------------------------------------ three_interpolate
INTERP = [(n, C) for n in X.interp_index_sets() for C in (1, 7)]


@pytest.mark.parametrize("name,C", INTERP)
def test_three_interpolate_forward(cuda, name, C):
    """|out - float64| <= 4 * 2^-24 * sum_t |w_t f_t| per element (three
    roundings of the fma chain and one spare), and bit-equal to the oracle's
    fmaf chain."""
    from o3dml_amd import ops
    c = X.interp_case(name, C)
    got = ops.three_interpolate(_t(c["feats"], cuda), _t(c["idx"], cuda), _t(c["w"], cuda)).cpu().numpy()
    assert got.shape == c["out"].shape
    excess = X.interp_forward_excess(got, c)
    print(f"{name} C={C}: max error beyond the bound {excess:.3e} (<= 0 passes)")
    assert excess <= 0
    assert np.array_equal(got, O.three_interpolate(c["feats"], c["idx"], c["w"]))


def _grad_capi(cuda, c, det, fill):
    """The C entry called directly on an output pre-filled with `fill`."""
    from o3dml_amd import _lib
    from o3dml_amd._util import ptr, stream_handle, workspace
    g, i, w = _t(c["grad"], cuda), _t(c["idx"], cuda), _t(c["w"], cuda)
    B, C, n = g.shape
    out = torch.full((B, C, c["m"]), fill, dtype=torch.float32, device=cuda)
    if det:
        ws = workspace(_lib.load().o3dml_three_interpolate_grad_workspace_size(B, n, c["m"]), cuda)
        _lib.call("o3dml_three_interpolate_grad_det", ptr(g), ptr(i), ptr(w), B, C, n, c["m"], ptr(out), ptr(ws),
                  ws.numel(), stream_handle(cuda))
    else:
        _lib.call("o3dml_three_interpolate_grad", ptr(g), ptr(i), ptr(w), B, C, n, c["m"], ptr(out),
                  stream_handle(cuda))
    return out.cpu().numpy()


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
@pytest.mark.parametrize("name,C", INTERP)
def test_three_interpolate_grad(cuda, name, C, det):
    """|grad - float64| <= (P + 2) * 2^-24 * sum |g w| over the P pairs landing
    on an element (P rounded products summed in any order); elements with no
    pair exactly 0; the output fully written (C entry on a NaN-filled
    buffer); the deterministic variant bit-equal across runs."""
    from o3dml_amd import ops
    c = X.interp_case(name, C)
    args = (_t(c["grad"], cuda), _t(c["idx"], cuda), _t(c["w"], cuda), c["m"])
    before = torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(det)
        got = ops.three_interpolate_grad(*args).cpu().numpy()
        again = ops.three_interpolate_grad(*args).cpu().numpy() if det else None
    finally:
        torch.use_deterministic_algorithms(before)
    assert got.shape == c["gf"].shape
    excess = X.interp_grad_excess(got, c)
    print(f"{name} C={C} det={det}: max error beyond the bound {excess:.3e} (<= 0 passes), "
          f"up to {int(c['pairs'].max())} pairs per element")
    assert excess <= 0
    raw = _grad_capi(cuda, c, det, float("nan"))
    assert X.interp_grad_excess(raw, c) <= 0  # inf if a NaN or a non-zero untouched element is left
    if det:
        assert np.array_equal(got, again) and np.array_equal(got, raw)


# ------------------------------------------------------------------ status paths
def test_status_paths(cuda):
    """Checks that return before any launch."""
    from o3dml_amd import ops
    f = lambda *s: torch.zeros(s, dtype=torch.float32, device=cuda)  # noqa: E731
    with pytest.raises(RuntimeError, match="empty cloud"):
        ops.furthest_point_sampling(f(2, 0, 3), 4)
    with pytest.raises(RuntimeError, match="nsample"):
        ops.ball_query(f(2, 10, 3), f(2, 5, 3), 1.0, 0)
    for bad in (f(2, 10, 3).double(), f(10, 3), f(2, 10, 2), f(2, 10, 3).int()):
        with pytest.raises(RuntimeError, match=r"float32 \[B, N, 3\]"):
            ops.furthest_point_sampling(bad, 4)
        with pytest.raises(RuntimeError, match=r"float32 \[B, N, 3\]"):
            ops.ball_query(bad, f(2, 5, 3), 1.0, 4)
        with pytest.raises(RuntimeError, match=r"float32 \[B, N, 3\]"):
            ops.ball_query(f(2, 10, 3), bad, 1.0, 4)
        with pytest.raises(RuntimeError, match=r"float32 \[B, N, 3\]"):
            ops.three_nn(bad, f(2, 10, 3))
        with pytest.raises(RuntimeError, match=r"float32 \[B, N, 3\]"):
            ops.three_nn(f(2, 10, 3), bad)
    # B = 0 and M = 0: empty results, nothing launched
    assert tuple(ops.furthest_point_sampling(f(0, 10, 3), 4).shape) == (0, 4)
    assert tuple(ops.furthest_point_sampling(f(2, 10, 3), 0).shape) == (2, 0)
    assert tuple(ops.furthest_point_sampling(f(2, 0, 3), 0).shape) == (2, 0)
    assert tuple(ops.ball_query(f(0, 10, 3), f(0, 5, 3), 1.0, 4).shape) == (0, 5, 4)
    assert tuple(ops.ball_query(f(2, 10, 3), f(2, 0, 3), 1.0, 4).shape) == (2, 0, 4)
    d, i = ops.three_nn(f(0, 5, 3), f(0, 10, 3))
    assert tuple(d.shape) == (0, 5, 3) and tuple(i.shape) == (0, 5, 3)
    d, i = ops.three_nn(f(2, 0, 3), f(2, 10, 3))
    assert tuple(d.shape) == (2, 0, 3) and i.dtype == torch.int32
    assert tuple(ops.three_interpolate(f(0, 4, 10), i[:0], d[:0]).shape) == (0, 4, 0)
    gf = ops.three_interpolate_grad(f(2, 4, 0), i, d, 10).cpu()  # no pairs: all zeros
    assert tuple(gf.shape) == (2, 4, 10) and not gf.any()
