"""Inputs on which fp32 arithmetic is exact, and float64 numpy references
written from the contracts in include/o3dml_amd.h, for the PointNet++ ops and
voxelize.

Coordinates are small integers times a power of two, so every difference,
square and three-term sum of a squared distance is exact in fp32: equal
distances and points on a boundary are the rule, and the expected result does
not depend on fma contraction, evaluation order or fp32 versus fp64.  The
references below share no code with oracle/o3d_oracle.c; tests/
test_exact_cases.py checks them against it on the CPU, together with the
properties the cases are built for, before tests/test_gpu_pointnet2.py and
tests/test_gpu_voxelize.py use them to judge the kernels.

Everything is built once per process (lru_cache) and must be treated as
read-only.
"""
import functools

import numpy as np

BIG = 2**63 - 1
EPS = 2.0**-24  # fp32 unit roundoff


def lattice(rng, shape, hi=64, step=0.125):
    """float32 points on the lattice step * {0..hi-1}^3."""
    return (rng.integers(0, hi, tuple(shape) + (3,)) * step).astype(np.float32)


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


# --------------------------------------------------------------------------
# furthest point sampling
# --------------------------------------------------------------------------
def ref_fps(xyz, m, tie="first", cap=1e10):
    """Greedy from index 0; min-distance initialised to `cap` (1e10 by the
    contract); the next point is the argmax of the min-distances, the smallest
    index on ties (tie="last": the largest, a deliberately wrong variant)."""
    x = np.asarray(xyz, np.float64)
    B, n, _ = x.shape
    out = np.zeros((B, m), np.int32)
    for b in range(B):
        md = np.full(n, cap, np.float64)
        old = 0
        for j in range(1, m):
            md = np.minimum(md, ((x[b] - x[b, old])**2).sum(1))
            old = int(np.argmax(md)) if tie == "first" else n - 1 - int(np.argmax(md[::-1]))
            out[b, j] = old
    return out


FPS_LATTICE_SIZES = (1, 63, 65, 1024, 1025, 2048, 2049, 4097, 8193, 16385, 32768, 32769)


def _distinct_sites(rng, B, n):
    s = np.stack([rng.choice(64**3, n, replace=False) for _ in range(B)])
    return (np.stack([s % 64, (s // 64) % 64, s // 4096], -1) * 0.125).astype(np.float32)


@functools.lru_cache(maxsize=None)
def fps_cases():
    """name -> dict(xyz [3,n,3], m, ref [3,m], kind)."""
    cases = {}

    def add(name, xyz, m, kind):
        ref = ref_fps(xyz, m)
        _freeze(xyz, ref)
        cases[name] = dict(xyz=xyz, m=m, ref=ref, kind=kind)

    for n in FPS_LATTICE_SIZES:
        add(f"lattice-{n}", lattice(np.random.default_rng(1000 + n), (3, n)), min(48, n + 5), "lattice")
    add("short-40", _distinct_sites(np.random.default_rng(2002), 3, 40), 48, "short")  # m > n, past n = 1
    add("m1-65", lattice(np.random.default_rng(2001), (3, 65)), 1, "m1")
    for n in (65, 1025):
        add(f"perm-{n}", _distinct_sites(np.random.default_rng(2100 + n), 3, n), n, "perm")
    same = np.broadcast_to(np.array([[1.5, -2.25, 0.75], [0, 0, 0], [-4, 8, 0.125]], np.float32)[:, None, :],
                           (3, 1025, 3)).copy()
    add("identical-1025", same, 16, "identical")
    rng = np.random.default_rng(2201)
    ab = lattice(rng, (3, 2))  # two sites per cloud
    ab[:, 1] += 1.0  # never the same site
    pick = rng.integers(0, 2, (3, 2049))
    pick[:, 0] = 0
    pick[:, 7] = 1
    add("two-clusters-2049", np.take_along_axis(ab, pick[:, :, None].repeat(3, 2), 1), 8, "clusters")
    add("scaled-1025", (lattice(np.random.default_rng(2301), (3, 1025)) * 65536.0).astype(np.float32), 48, "scaled")
    return cases


@functools.lru_cache(maxsize=None)
def fps_random_case():
    xyz = np.random.default_rng(2401).random((3, 5000, 3), dtype=np.float32)
    _freeze(xyz)
    return dict(xyz=xyz, m=64)


def fps_property_violations(xyz, idx, margin=1e-6):
    """For general fp32 input: each chosen point's float64 distance to the
    earlier chosen set must be >= (1 - margin) times the maximum over all
    points, and indices in range and distinct.  Returns a list of messages."""
    x = np.asarray(xyz, np.float64)
    bad = []
    for b in range(x.shape[0]):
        ii = np.asarray(idx[b], np.int64)
        n = x.shape[1]
        if ii[0] != 0 or ii.min() < 0 or ii.max() >= n:
            bad.append(f"cloud {b}: start {ii[0]} or index out of [0, {n})")
            continue
        if len(np.unique(ii)) != len(ii):
            bad.append(f"cloud {b}: repeated index")
        md = np.full(n, np.inf)
        for j in range(1, len(ii)):
            md = np.minimum(md, ((x[b] - x[b, ii[j - 1]])**2).sum(1))
            if not md[ii[j]] >= (1.0 - margin) * md.max():
                bad.append(f"cloud {b} pick {j}: distance {md[ii[j]]!r} < max {md.max()!r}")
    return bad


# --------------------------------------------------------------------------
# ball_query
# --------------------------------------------------------------------------
def ball_d2(xyz, ctr):
    """float64 squared distances [B, M, n]."""
    x = np.asarray(xyz, np.float64)
    c = np.asarray(ctr, np.float64)
    return ((c[:, :, None, :] - x[:, None, :, :])**2).sum(-1)


def ball_r2(r):
    return np.float64(np.float32(r) * np.float32(r))  # as the ABI computes it


def ref_ball_query(xyz, ctr, r, nsample):
    """The first nsample points, in index order, with d2 < r2 strictly; the row
    padded with the first hit; all 0 when there is none."""
    hit = ball_d2(xyz, ctr) < ball_r2(r)
    B, M, _ = hit.shape
    out = np.zeros((B, M, nsample), np.int32)
    for b in range(B):
        for j in range(M):
            k = np.flatnonzero(hit[b, j])[:nsample]
            if len(k):
                out[b, j] = k[0]
                out[b, j, :len(k)] = k
    return out


# name: (n, M, nsample, r, lattice sites per axis at 0.5 spacing)
BALL_SHAPES = {
    "255-1-1": (255, 1, 1, 1.0, 12),
    "256-257-16": (256, 257, 16, 1.0, 9),
    "257-300-64": (257, 300, 64, 0.5, 4),
    "1000-77-8": (1000, 77, 8, 1.0, 12),
    "dense-1000-16": (1000, 300, 16, 1.0, 8),
    "dense-1000-64": (1000, 300, 64, 1.0, 8),
}


@functools.lru_cache(maxsize=None)
def ball_cases():
    """name -> dict(xyz [3,n,3], ctr [3,M,3], r, nsample, ref, hits [3,M])."""
    cases = {}
    for k, (name, (n, M, ns, r, hi)) in enumerate(BALL_SHAPES.items()):
        rng = np.random.default_rng(3000 + k)
        xyz = lattice(rng, (3, n), hi, 0.5)
        ctr = lattice(rng, (3, M), hi, 0.5)
        ref = ref_ball_query(xyz, ctr, r, ns)
        hits = (ball_d2(xyz, ctr) < ball_r2(r)).sum(-1)
        _freeze(xyz, ctr, ref, hits)
        cases[name] = dict(xyz=xyz, ctr=ctr, r=r, nsample=ns, ref=ref, hits=hits)
    return cases


def ball_split_workgroups(case, tile=256):
    """Number of (cloud, 256-query workgroup) pairs in which some query has
    nsample hits within the first tile of points while another still lacks
    them before the last tile."""
    hit = ball_d2(case["xyz"], case["ctr"]) < ball_r2(case["r"])
    n = hit.shape[2]
    last = (n - 1) // tile * tile
    if last == 0:
        return 0
    full_first = hit[:, :, :tile].sum(-1) >= case["nsample"]
    need_last = hit[:, :, :last].sum(-1) < case["nsample"]
    cnt = 0
    for b in range(hit.shape[0]):
        for w in range(0, hit.shape[1], tile):
            cnt += bool(full_first[b, w:w + tile].any() and need_last[b, w:w + tile].any())
    return cnt


# --------------------------------------------------------------------------
# three_nn
# --------------------------------------------------------------------------
def ref_three_nn(unknown, known):
    """The three smallest (d2, index) pairs per query, the earlier index first
    among equal distances; a missing slot is (inf, 0).  Also returns the
    sorted float64 distances for the tie statistics."""
    d2 = ball_d2(known, unknown)  # [B, n, m]
    B, n, m = d2.shape
    order = np.argsort(d2, axis=-1, kind="stable")
    srt = np.take_along_axis(d2, order, -1)
    dist = np.full((B, n, 3), np.inf, np.float32)
    idx = np.zeros((B, n, 3), np.int32)
    k = min(3, m)
    dist[:, :, :k] = srt[:, :, :k]
    idx[:, :, :k] = order[:, :, :k]
    return dist, idx, srt


THREE_NN_SHAPES = ((1, 1), (257, 2), (300, 3), (100, 255), (100, 257), (513, 700))  # (queries n, known m)


@functools.lru_cache(maxsize=None)
def three_nn_cases():
    """name -> dict(unknown [3,n,3], known [3,m,3], dist, idx, tie34)."""
    cases = {}
    for n, m in THREE_NN_SHAPES:
        rng = np.random.default_rng(4000 + 7 * n + m)
        unknown = lattice(rng, (3, n), 16, 0.25)
        known = lattice(rng, (3, m), 16, 0.25)
        dist, idx, srt = ref_three_nn(unknown, known)
        tie34 = float((srt[:, :, 2] == srt[:, :, 3]).mean()) if m > 3 else 0.0
        _freeze(unknown, known, dist, idx)
        cases[f"{n}-{m}"] = dict(unknown=unknown, known=known, dist=dist, idx=idx, tie34=tie34)
    return cases


# --------------------------------------------------------------------------
# three_interpolate and its gradient
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def interp_index_sets():
    """name -> (idx int32 [3,n,3], m); every index in [0, m)."""
    sets = {f"nn-{k}": (c["idx"], c["known"].shape[1]) for k, c in three_nn_cases().items()}
    rng = np.random.default_rng(5001)
    a, b = rng.integers(0, 10, (2, 3, 64))
    b = np.where(a == b, (b + 1) % 10, b)
    rep = np.stack([a, a, b], -1)
    rep[:, 16:32] = np.stack([a, b, a], -1)[:, 16:32]
    rep[:, 32:48] = np.stack([b, a, a], -1)[:, 32:48]
    rep[:, 48:] = np.stack([a, a, a], -1)[:, 48:]
    sets["repeats"] = (rep.astype(np.int32), 10)
    sets["single-target"] = (np.full((3, 500, 3), 4, np.int32), 9)  # 1500 pairs on one element
    sets["half-untouched"] = ((rng.integers(0, 100, (3, 300, 3)) * 2).astype(np.int32), 200)
    for idx, m in sets.values():
        assert idx.min() >= 0 and idx.max() < m
        _freeze(idx)
    return sets


@functools.lru_cache(maxsize=None)
def interp_case(name, C):
    """dict(idx, m, feats [3,C,m], w [3,n,3], grad [3,C,n]) and the float64
    references: out / out_abs [3,C,n] (sum and sum of magnitudes of the three
    products), gf / gf_abs [3,C,m] and pairs [3,m] (the pairs landing on each
    source point)."""
    idx, m = interp_index_sets()[name]
    B, n, _ = idx.shape
    rng = np.random.default_rng(5100 + 16 * sorted(interp_index_sets()).index(name) + C)
    feats = rng.standard_normal((B, C, m)).astype(np.float32)
    w = rng.random((B, n, 3)).astype(np.float32)
    grad = rng.standard_normal((B, C, n)).astype(np.float32)
    f64, w64, g64 = feats.astype(np.float64), w.astype(np.float64), grad.astype(np.float64)
    out = np.zeros((B, C, n))
    out_abs = np.zeros((B, C, n))
    gf = np.zeros((B, C, m))
    gf_abs = np.zeros((B, C, m))
    pairs = np.zeros((B, m), np.int64)
    for b in range(B):
        for t in range(3):
            prod = w64[b, :, t][None, :] * f64[b][:, idx[b, :, t]]  # [C, n]
            out[b] += prod
            out_abs[b] += np.abs(prod)
            gw = g64[b] * w64[b, :, t][None, :]  # [C, n]
            for c in range(C):
                np.add.at(gf[b, c], idx[b, :, t], gw[c])
                np.add.at(gf_abs[b, c], idx[b, :, t], np.abs(gw[c]))
            np.add.at(pairs[b], idx[b, :, t], 1)
    case = dict(idx=idx, m=m, feats=feats, w=w, grad=grad, out=out, out_abs=out_abs, gf=gf, gf_abs=gf_abs,
                pairs=pairs)
    _freeze(*[v for v in case.values() if isinstance(v, np.ndarray)])
    return case


def interp_forward_excess(got, case):
    """max over elements of |got - float64| - 4 eps sum|w f| (three roundings
    of the fma chain and one spare); <= 0 passes."""
    return float((np.abs(got.astype(np.float64) - case["out"]) - 4 * EPS * case["out_abs"]).max(initial=-1.0))


def interp_grad_excess(got, case):
    """max over elements of |got - float64| - (P + 2) eps sum|g w| over the P
    pairs landing there (P rounded products summed in any order); <= 0
    passes, and elements with P = 0 must be exactly 0 (returns inf if not)."""
    P = case["pairs"][:, None, :].astype(np.float64)
    err = np.abs(got.astype(np.float64) - case["gf"])
    untouched = np.broadcast_to(P == 0, err.shape)
    if np.any(got[untouched] != 0) or np.any(np.signbit(got[untouched])) or not np.all(np.isfinite(got)):
        return float("inf")
    return float((err - (P + 2) * EPS * case["gf_abs"])[~untouched].max(initial=-1.0))


# --------------------------------------------------------------------------
# voxelize
# --------------------------------------------------------------------------
def ref_voxelize(points, row_splits, voxel_size, range_min, range_max, max_ppv=BIG, max_voxels=BIG):
    """coord = floor((p - min) / vs); valid iff 0 <= coord_d < trunc((max_d -
    min_d) / vs_d) for every d; voxels ordered by (batch, coord[ndim-1], ...,
    coord[0]) with no linear key; points of a voxel by index; then the first
    max_voxels voxels per batch item and max_ppv points per voxel.  Exact and
    unambiguous for power-of-two voxel sizes."""
    p = np.asarray(points, np.float32).astype(np.float64)
    rs = np.asarray(row_splits, np.int64)
    vs, mn, mx = (np.asarray(a, np.float32).astype(np.float64) for a in (voxel_size, range_min, range_max))
    n, ndim = p.shape
    nb = len(rs) - 1
    coord = np.floor((p - mn) / vs)
    ext = np.trunc((mx - mn) / vs)
    ids = np.flatnonzero(((coord >= 0) & (coord < ext)).all(1))
    c = coord[ids].astype(np.int64)
    b = np.searchsorted(rs, ids, side="right") - 1  # the item whose [rs[b], rs[b+1]) holds the point
    order = np.lexsort((ids,) + tuple(c[:, d] for d in range(ndim)) + (b,))  # last key is the primary one
    ids, c, b = ids[order], c[order], b[order]
    coords, pidx, prs, bsplits = [], [], [0], np.zeros(nb + 1, np.int64)
    in_item = np.zeros(nb, np.int64)
    s = 0
    while s < len(ids):
        e = s + 1
        while e < len(ids) and b[e] == b[s] and np.array_equal(c[e], c[s]):
            e += 1
        if in_item[b[s]] < max_voxels:
            in_item[b[s]] += 1
            coords.append(c[s])
            pidx.extend(ids[s:min(e, s + max_ppv)])
            prs.append(len(pidx))
        s = e
    bsplits[1:] = np.cumsum(in_item)
    return (np.asarray(coords, np.int32).reshape(-1, ndim), np.asarray(pidx, np.int64), np.asarray(prs, np.int64),
            bsplits)


_VS = (0.5, 0.25, 1.0, 2.0)
_MIN = (-2.5, -1.25, 0.0, -3.0)
_CELLS = (11, 7, 3, 2)
VOX_NDIMS = (1, 2, 3, 4, 8)
VOX_CAPS = ((BIG, BIG), (1, BIG), (3, 5), (BIG, 0), (1, 1))


def _grid(ndim):
    vs = np.array([_VS[d % 4] for d in range(ndim)], np.float32)
    mn = np.array([_MIN[d % 4] for d in range(ndim)], np.float32)
    mx = (mn + vs * np.array([_CELLS[d % 4] for d in range(ndim)], np.float32)).astype(np.float32)
    mx[0] += 0.25  # half a voxel of dim 0 beyond the last whole one: dropped
    return vs, mn, mx


@functools.lru_cache(maxsize=None)
def vox_grid_case(ndim):
    """About 2000 points at multiples of 1/8 in three batch items (the middle
    one empty, the last one small), a different power-of-two voxel size per
    dimension and a dim-0 range that is no multiple of its voxel size."""
    rng = np.random.default_rng(6000 + ndim)
    vs, mn, mx = _grid(ndim)
    lo8, hi8 = np.round(mn * 8).astype(np.int64), np.round(mx * 8).astype(np.int64)
    n = 2000
    inside = rng.integers(lo8, hi8 + 1, (n, ndim))  # max itself included
    wide = rng.integers(lo8 - 16, hi8 + 17, (n, ndim))
    pts8 = np.where(rng.random((n, ndim)) < 0.93, inside, wide)
    dup = rng.random(n) < 0.3  # repeated points: voxels with several points also in 8 dims
    pts8[dup] = pts8[rng.integers(0, n, dup.sum())]
    centre8 = np.round((mn + 0.5 * vs) * 8).astype(np.int64)  # centre of voxel 0: valid in every dim
    special = np.tile(centre8, (6, 1))
    special[0, 0] = lo8[0] - 1  # just below min
    special[1, 0] = lo8[0]  # exactly on min: valid, coord 0
    special[2, 0] = lo8[0] + int(vs[0] * 8) * 3  # exactly on a voxel face: the upper voxel
    special[3, 0] = hi8[0]  # exactly on max: invalid
    special[4, 0] = hi8[0] - 1  # inside the dropped partial voxel: invalid
    special[5, ndim - 1] = hi8[ndim - 1]  # on max of the last dim
    tail = np.tile(centre8, (6, 1))  # the small last item: 3 voxels, 2 points each
    tail[2:4, 0] += int(vs[0] * 8)
    tail[4:6, 0] += int(vs[0] * 8) * 2
    pts = (np.concatenate([pts8, special, tail]) / 8.0).astype(np.float32)
    rs = np.array([0, n + 6, n + 6, n + 12], np.int64)
    _freeze(pts, rs, vs, mn, mx)
    return dict(pts=pts, rs=rs, vs=vs, mn=mn, mx=mx, special=np.arange(n, n + 6))


@functools.lru_cache(maxsize=None)
def vox_ref(name, caps):
    c = vox_cases()[name]
    out = ref_voxelize(c["pts"], c["rs"], c["vs"], c["mn"], c["mx"], *caps)
    _freeze(*out)
    return out


def pow2ceil(x):
    p = 1
    while p < x:
        p *= 2
    return p


def key_budget(case):
    """((nb+1) prod pow2ceil(ext), (nb+1) prod ext): the power-of-two key layout
    is used iff the first is below 2^56; the plain product strides need the
    second below it."""
    ext = np.trunc((case["mx"].astype(np.float64) - case["mn"]) / case["vs"]).astype(np.int64)
    nb = len(case["rs"]) - 1
    p2 = p1 = nb + 1
    for e in ext:
        p2 *= pow2ceil(int(e))
        p1 *= int(e)
    return p2, p1


def _scn_like(ndim, top, nb, seed):
    """nb batch items of 3-10 points at k + 0.5 in [0, top)^ndim, vs = 1: the
    top voxel, repeated voxels and a point on range_max included."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(3, 11, nb)
    rs = np.zeros(nb + 1, np.int64)
    rs[1:] = np.cumsum(lens)
    n = int(rs[-1])
    k = rng.integers(0, top, (n, ndim))
    k[rng.random((n, ndim)) < 0.15] = top - 1  # the last voxel of an axis
    k[rng.random((n, ndim)) < 0.15] = 0
    pts = (k + 0.5).astype(np.float32)
    rep = rng.random(n) < 0.3
    rep[0] = False
    pts[rep] = pts[np.flatnonzero(rep) - 1]  # same voxel as the previous point (often the same item)
    pts[1] = top - 0.5
    pts[2, 0] = top  # on range_max: invalid
    one = np.ones(ndim, np.float32)
    case = dict(pts=pts, rs=rs, vs=one, mn=0 * one, mx=top * one)
    _freeze(*case.values())
    return case


def _regroup(case, nb):
    """The same points in nb batch items of (almost) equal size."""
    n = len(case["pts"])
    rs = np.linspace(0, n, nb + 1).astype(np.int64)
    _freeze(rs)
    return dict(case, rs=rs)


@functools.lru_cache(maxsize=None)
def vox_cases():
    """name -> dict(pts [N,ndim], rs, vs, mn, mx)."""
    cases = {f"grid-{d}d": vox_grid_case(d) for d in VOX_NDIMS}
    cases["scn-300"] = _scn_like(3, 40960, 300, 6101)  # product strides
    cases["scn-3"] = _regroup(cases["scn-300"], 3)  # control: power-of-two strides
    cases["scn4d-20"] = _scn_like(4, 4097, 20, 6102)  # product strides, 4 dims
    cases["scn4d-3"] = _regroup(cases["scn4d-20"], 3)
    g3 = vox_grid_case(3)
    f32 = np.float32

    def c(pts, rs, vs=g3["vs"], mn=g3["mn"], mx=g3["mx"]):
        d = dict(pts=np.asarray(pts, f32).reshape(-1, len(vs)), rs=np.asarray(rs, np.int64), vs=np.asarray(vs, f32),
                 mn=np.asarray(mn, f32), mx=np.asarray(mx, f32))
        _freeze(*d.values())
        return d

    cases["empty-n0"] = c(np.zeros((0, 3)), [0, 0])
    cases["empty-two-items"] = c(np.zeros((0, 3)), [0, 0, 0])
    cases["all-outside"] = c(g3["pts"][:500] + f32(100.0), [0, 200, 500])
    mx_bad = g3["mx"].copy()
    mx_bad[1] = g3["mn"][1] - 1.0
    cases["max-below-min"] = c(g3["pts"][:500], [0, 200, 500], mx=mx_bad)
    cases["empty-first-last"] = c(g3["pts"][:700], [0, 0, 300, 700, 700])
    heap = np.tile(np.array([[0.25, 0.5, 0.75]]), (5000, 1))  # all in one voxel of a [0,1)^3 grid of size 1
    heap += np.random.default_rng(6201).integers(0, 2, (5000, 3)) * 0.125
    cases["one-voxel-5000"] = c(heap, [0, 5000], vs=[1, 1, 1], mn=[0, 0, 0], mx=[4, 4, 4])
    return cases


# (case, caps) pairs run by both the CPU and the GPU tests
VOX_RUNS = tuple((f"grid-{d}d", caps) for d in VOX_NDIMS for caps in VOX_CAPS) + tuple(
    (name, (BIG, BIG)) for name in ("scn-300", "scn-3", "scn4d-20", "scn4d-3", "empty-n0", "empty-two-items",
                                    "all-outside", "max-below-min", "empty-first-last", "one-voxel-5000")) + (
                                        ("scn-300", (2, 3)), ("one-voxel-5000", (7, BIG)), ("empty-first-last", (3, 5)))


def vox_run_id(run):
    name, caps = run
    return name + "-" + "x".join("big" if v == BIG else str(v) for v in caps)
