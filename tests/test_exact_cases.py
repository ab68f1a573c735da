"""The float64 numpy references of tests/exact_cases.py against the C oracle,
bit for bit, on the exact-arithmetic inputs the GPU tests use, and the
properties those inputs are built for (ties, rows of every fill class, points
on voxel faces, the product-stride key layout, ...).  Runs without a GPU: it
validates the references before they judge a kernel, and fails if an edit to
a seed or a shape loses the edge a case exists for."""
import numpy as np
import pytest

import exact_cases as X
import oracle as O


# ------------------------------------------------------------------ FPS
@pytest.mark.parametrize("name", list(X.fps_cases()))
def test_fps_reference_equals_oracle(name):
    c = X.fps_cases()[name]
    assert np.array_equal(c["ref"], O.furthest_point_sampling(c["xyz"], c["m"]))


@pytest.mark.parametrize("n", X.FPS_LATTICE_SIZES)
def test_fps_lattice_discriminates_tie_direction(n):
    """A reference that breaks ties towards the largest index must give a
    different answer, or the case could not tell the two apart."""
    c = X.fps_cases()[f"lattice-{n}"]
    assert c["m"] == min(48, n + 5)
    diff = int((X.ref_fps(c["xyz"], c["m"], tie="last") != c["ref"]).sum())
    print(f"n={n}: {diff} of {c['ref'].size} entries differ under largest-index ties")
    if n == 1:
        assert diff == 0 and not c["ref"].any()
    else:
        assert diff >= 8


def test_fps_case_conditions():
    cs = X.fps_cases()
    # m > n: once every distinct site is taken all min-distances are 0 and the
    # argmax falls back to index 0
    for name, n in (("lattice-1", 1), ("short-40", 40)):
        c = cs[name]
        assert c["m"] > n == c["xyz"].shape[1] and not c["ref"][:, n:].any()
        assert all(np.array_equal(np.sort(r[:n]), np.arange(n)) for r in c["ref"])
    for n in (65, 1025):
        c = cs[f"perm-{n}"]
        assert c["m"] == n
        assert all(len(np.unique(x, axis=0)) == n for x in c["xyz"])
        assert all(np.array_equal(np.sort(r), np.arange(n)) for r in c["ref"])
    assert not cs["identical-1025"]["ref"].any()
    c = cs["two-clusters-2049"]
    assert all(len(np.unique(x, axis=0)) == 2 for x in c["xyz"])
    first_other = [int(np.flatnonzero((x != x[0]).any(1))[0]) for x in c["xyz"]]
    assert np.array_equal(c["ref"], [[0, k] + [0] * 6 for k in first_other])
    # scaled cloud: distances pass the 1e10 the min-distances start from, all
    # still exact in fp32, and the cap changes the answer
    c = cs["scaled-1025"]
    x = c["xyz"].astype(np.float64)
    d2 = ((x - x[:, :1])**2).sum(-1)
    assert d2.max() > 1e10 and np.array_equal(d2, d2.astype(np.float32)) and np.float32(1e10) == 1e10
    assert not np.array_equal(X.ref_fps(c["xyz"], c["m"], cap=np.inf), c["ref"])
    assert cs["m1-65"]["m"] == 1


def test_fps_property_check_accepts_oracle_rejects_wrong():
    c = X.fps_random_case()
    good = O.furthest_point_sampling(c["xyz"], c["m"])
    assert X.fps_property_violations(c["xyz"], good) == []
    bad = good.copy()
    bad[1, 40] = bad[1, 3]
    assert X.fps_property_violations(c["xyz"], bad)


# ------------------------------------------------------------------ ball_query
@pytest.mark.parametrize("name", list(X.ball_cases()))
def test_ball_query_reference_equals_oracle(name):
    c = X.ball_cases()[name]
    assert np.array_equal(c["ref"], O.ball_query(c["xyz"], c["ctr"], c["r"], c["nsample"]))


def test_ball_query_case_conditions():
    cs = X.ball_cases()
    assert {k: (v["xyz"].shape[1], v["ctr"].shape[1], v["nsample"], v["r"]) for k, v in cs.items()} == \
        {k: v[:4] for k, v in X.BALL_SHAPES.items()}
    classes = set()
    for name, c in cs.items():
        h, ns = c["hits"], c["nsample"]
        here = {k for k, m in (("none", h == 0), ("partial", (h > 0) & (h < ns)), ("exact", h == ns),
                               ("over", h > ns)) if m.any()}
        eq = int((X.ball_d2(c["xyz"], c["ctr"]) == X.ball_r2(c["r"])).sum())
        print(f"{name}: fill classes {sorted(here)}, {eq} pairs with d2 == r2, "
              f"{X.ball_split_workgroups(c)} split workgroups")
        classes |= here
        if name != "255-1-1":
            assert eq > 0  # pairs exactly on the sphere: excluded by the strict <
    assert classes == {"none", "partial", "exact", "over"}
    assert X.ball_split_workgroups(cs["dense-1000-16"]) >= 1
    assert sum(c["ctr"].shape[1] % 256 != 0 for c in cs.values()) >= 2


# ------------------------------------------------------------------ three_nn
@pytest.mark.parametrize("name", list(X.three_nn_cases()))
def test_three_nn_reference_equals_oracle(name):
    c = X.three_nn_cases()[name]
    od, oi = O.three_nn(c["unknown"], c["known"])
    assert np.array_equal(c["idx"], oi) and np.array_equal(c["dist"], od)
    m = c["known"].shape[1]
    print(f"{name}: {c['tie34']:.2f} of the rows tie between third and fourth place")
    if m > 3:
        assert c["tie34"] >= 0.25
    else:
        assert np.isinf(c["dist"][:, :, m:]).all() and not c["idx"][:, :, m:].any()


# ------------------------------------------------------------------ three_interpolate
INTERP = [(n, C) for n in X.interp_index_sets() for C in (1, 7)]


@pytest.mark.parametrize("name,C", INTERP)
def test_interpolate_references_bound_the_oracle(name, C):
    c = X.interp_case(name, C)
    assert X.interp_forward_excess(O.three_interpolate(c["feats"], c["idx"], c["w"]), c) <= 0
    assert X.interp_grad_excess(O.three_interpolate_grad(c["grad"], c["idx"], c["w"], c["m"]), c) <= 0


def test_interpolate_case_conditions():
    s = X.interp_index_sets()
    rep = s["repeats"][0]
    same = (rep[..., 0] == rep[..., 1]).astype(int) + (rep[..., 1] == rep[..., 2]) + (rep[..., 0] == rep[..., 2])
    assert (same == 1).any() and (same == 3).any()  # an index twice, and three times, within a triple
    c = X.interp_case("single-target", 7)
    assert c["pairs"][:, 4].tolist() == [1500] * 3 and c["pairs"].sum() == 4500
    c = X.interp_case("half-untouched", 7)
    assert (c["pairs"][:, 1::2] == 0).all() and (c["pairs"] == 0).mean() >= 0.5
    # the bounds have teeth: one fp32 ulp-sized relative error on a large element is caught
    c = X.interp_case("nn-513-700", 7)
    g = c["gf"].astype(np.float32)
    assert X.interp_grad_excess(g, c) <= 0
    g2 = g.copy()
    k = np.unravel_index(np.argmax(c["pairs"][:, None, :] * np.ones_like(g)), g.shape)
    g2[k] += np.float32(2 * (c["pairs"][k[0], k[2]] + 3) * X.EPS * c["gf_abs"][k])
    assert X.interp_grad_excess(g2, c) > 0
    c = X.interp_case("half-untouched", 7)
    g3 = c["gf"].astype(np.float32)
    g3[0, 0, 1] = 1e-30  # an element no pair lands on must be exactly 0
    assert X.interp_grad_excess(g3, c) == float("inf")


# ------------------------------------------------------------------ voxelize
@pytest.mark.parametrize("run", X.VOX_RUNS, ids=X.vox_run_id)
def test_voxelize_reference_equals_oracle(run):
    name, caps = run
    c = X.vox_cases()[name]
    ref = X.vox_ref(name, caps)
    orc = O.voxelize(c["pts"], c["rs"], c["vs"], c["mn"], c["mx"], *caps)
    for a, b in zip(ref, orc):
        assert a.dtype == b.dtype and np.array_equal(a, b)


@pytest.mark.parametrize("ndim", X.VOX_NDIMS)
def test_voxelize_grid_case_conditions(ndim):
    c = X.vox_grid_case(ndim)
    pts, vs, mn, mx = (c[k].astype(np.float64) for k in ("pts", "vs", "mn", "mx"))
    assert np.array_equal(pts * 8, np.round(pts * 8)) and len(set(c["vs"][:4].tolist())) == min(ndim, 4)
    assert np.array_equal(np.log2(vs), np.round(np.log2(vs)))  # power-of-two sizes: quotient == product
    assert c["rs"][1] == c["rs"][2] and len(c["rs"]) == 4  # B = 3, the middle item empty
    span = (mx - mn) / vs
    assert span[0] != np.trunc(span[0]) and np.array_equal(span[1:], np.trunc(span[1:]))
    coords, pidx, prs, bs = X.vox_ref(f"grid-{ndim}d", (X.BIG, X.BIG))
    kept = np.zeros(len(pts), bool)
    kept[pidx] = True
    below, on_min, on_face, on_max, partial, on_max_last = c["special"]
    assert kept[[on_min, on_face]].all() and not kept[[below, on_max, partial, on_max_last]].any()
    assert pts[on_min, 0] == mn[0] and pts[on_max, 0] == mx[0] and pts[on_max_last, -1] == mx[-1]
    assert pts[below, 0] < mn[0] and mn[0] + np.trunc(span[0]) * vs[0] <= pts[partial, 0] < mx[0]
    face_voxel = coords[np.searchsorted(prs, np.flatnonzero(pidx == on_face)[0], side="right") - 1]
    assert face_voxel[0] == 3 and (pts[on_face, 0] - mn[0]) / vs[0] == 3.0
    # points on faces and outside are common, not only the hand-placed ones
    frac = (pts[:2000] - mn) / vs
    assert (frac == np.floor(frac)).any(1).mean() > 0.2 and 0.05 < 1 - kept[:2000].mean() < 0.8
    assert (np.diff(prs) > 1).sum() >= min(20, len(coords))  # voxels with several points
    per_item = np.diff(bs)
    assert per_item[0] > 5 and per_item[1] == 0 and 0 < per_item[2] < 5  # around max_voxels = 5
    assert (np.diff(prs) > 3).any()  # max_points_per_voxel = 3 cuts something


def test_voxelize_key_layout_conditions():
    cs = X.vox_cases()
    for name, nb in (("scn-300", 300), ("scn4d-20", 20)):
        assert len(cs[name]["rs"]) - 1 == nb
        p2, p1 = X.key_budget(cs[name])
        assert p2 >= 2**56 > p1, name  # product strides, and they fit
    for name in ("scn-3", "scn4d-3"):
        assert X.key_budget(cs[name])[0] < 2**56, name  # the control keeps power-of-two strides
    c = cs["scn-300"]
    assert np.all(np.diff(c["rs"]) >= 3) and np.all(np.diff(c["rs"]) <= 10)
    assert (c["pts"] == np.float32(40959.5)).all(1).any() and (c["pts"] == 40960).any()
    coords = X.vox_ref("scn-300", (X.BIG, X.BIG))[0]
    assert (coords == 40959).any(0).all() and (coords == 0).any(0).all()
    assert len(np.unique(coords % 7, axis=0)) > 50  # the decode sees many different remainders
    prs = X.vox_ref("scn-300", (X.BIG, X.BIG))[2]
    assert (np.diff(prs) > 1).sum() >= 50
    assert np.array_equal(cs["scn-3"]["pts"], c["pts"])


def test_voxelize_empty_case_conditions():
    for name in ("empty-n0", "empty-two-items", "all-outside", "max-below-min"):
        coords, pidx, prs, bs = X.vox_ref(name, (X.BIG, X.BIG))
        assert len(coords) == 0 and len(pidx) == 0 and prs.tolist() == [0] and not bs.any(), name
    c = X.vox_cases()["max-below-min"]
    assert c["mx"][1] < c["mn"][1]
    bs = X.vox_ref("empty-first-last", (X.BIG, X.BIG))[3]
    assert np.diff(bs)[[0, 3]].tolist() == [0, 0] and (np.diff(bs)[[1, 2]] > 5).all()
    coords, pidx, prs, bs = X.vox_ref("one-voxel-5000", (X.BIG, X.BIG))
    assert len(coords) == 1 and np.array_equal(pidx, np.arange(5000))
    for d in X.VOX_NDIMS:
        assert len(X.vox_ref(f"grid-{d}d", (X.BIG, 0))[0]) == 0
