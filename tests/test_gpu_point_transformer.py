"""PointTransformer on the GPU: the ragged FPS bitwise against the per-cloud op
and the oracle, the four gather kernels against the float64 restatements of
tests/test_point_transformer.py, the plan constructor, and the eval() forward
against the reference's float64 logits (tests/golden/point_transformer.npz)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_point_transformer import (EPS, G, aggregate_ref, group_ref, interpolate_ref, layer_case,  # noqa: E402
                                    relation_ref)

pytestmark = pytest.mark.gpu

LAYER_SHAPES = [(1, 1, 8, 8), (65, 8, 32, 8), (257, 16, 48, 8), (130, 16, 512, 8), (64, 17, 64, 8)]


def n(x):
    return x.detach().cpu().numpy()


# ----------------------------------------------------------------- ragged FPS
def _fps_batches():
    rng = np.random.default_rng(5)
    cloud = lambda k: rng.random((k, 3), dtype=np.float32) * np.array([4, 3, 2.5], np.float32)  # noqa: E731
    block = cloud(300)
    return {
        "small_and_empty": [cloud(k) for k in (1, 3, 63, 1025, 4100)],
        "threshold": [cloud(2049), cloud(1024)],
        "global_memory": [cloud(33000), cloud(100)],
        "repeated_block": [np.concatenate([block, block, cloud(40), block]), cloud(77)],
    }


@pytest.mark.parametrize("name", ["small_and_empty", "threshold", "global_memory", "repeated_block"])
def test_ragged_fps_bitwise(cuda, name):
    """m_b = n_b // 4 samples per cloud in one launch: the bits of
    ops.furthest_point_sampling on each cloud alone plus its offset, and of
    the oracle, whichever register variant the largest cloud selects."""
    import oracle as O
    from o3dml_amd import ops
    from o3dml_amd.point_transformer import furthest_point_sample_ragged
    clouds = _fps_batches()[name]
    rs = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    nrs = np.concatenate([[0], np.cumsum([len(c) // 4 for c in clouds])]).astype(np.int64)
    xyz = torch.from_numpy(np.concatenate(clouds)).to(cuda)
    got = furthest_point_sample_ragged(xyz, rs, nrs)
    assert got.dtype == torch.int32 and tuple(got.shape) == (int(nrs[-1]),)
    assert torch.equal(got, furthest_point_sample_ragged(xyz, torch.from_numpy(rs), torch.from_numpy(nrs)))
    got = n(got)
    for b, c in enumerate(clouds):
        m = len(c) // 4
        mine = got[nrs[b]:nrs[b + 1]]
        alone = n(ops.furthest_point_sampling(xyz[rs[b]:rs[b + 1]][None], m))[0] + rs[b]
        assert np.array_equal(mine, alone), (name, b)
        assert np.array_equal(mine, O.furthest_point_sampling(c[None], m)[0] + rs[b]), (name, b)
    if name == "repeated_block":  # ties: a repeated point is taken at its first copy
        first = got[:nrs[1]]
        assert np.all((first < 300) | ((first >= 600) & (first < 640)))


def test_ragged_fps_errors_and_empty(cuda):
    from o3dml_amd.point_transformer import furthest_point_sample_ragged
    xyz = torch.rand(10, 3, device=cuda)
    with pytest.raises(RuntimeError, match="cloud 1 is empty"):
        furthest_point_sample_ragged(xyz, [0, 10, 10], [0, 2, 3])
    assert furthest_point_sample_ragged(xyz, [0, 10, 10], [0, 0, 0]).numel() == 0
    assert n(furthest_point_sample_ragged(xyz, [0, 10, 10], [0, 1, 1])).tolist() == [0]
    with pytest.raises(RuntimeError, match="new_row_splits"):
        furthest_point_sample_ragged(xyz, [0, 10], [0, 2, 3])


# ------------------------------------------------------- relation / aggregate
def _layer(cuda, shape):
    """The case rounded to float32 (what the GPU sees), its float64 copy for
    the restatement, and the op arguments on the GPU."""
    from o3dml_amd.point_transformer import Neighbours
    z = layer_case(*shape)
    r32 = lambda t: t.float()  # noqa: E731
    P32 = {k: tuple(r32(x) for x in v) if isinstance(v, tuple) else r32(v) for k, v in z["P"].items()}
    z32 = {k: r32(v) if k not in ("idx", "P") else v for k, v in z.items()}
    z64 = {k: v.double() if k not in ("idx", "P") else v for k, v in z32.items()}
    z64["P"] = {k: tuple(x.double() for x in v) if isinstance(v, tuple) else v.double() for k, v in P32.items()}
    d = lambda t: t.to(cuda)  # noqa: E731

    def fold(bn):
        g, b, mean, var = (d(x) for x in bn)
        scale = g * torch.rsqrt(var + EPS)
        return scale, b - mean * scale

    pos = (d(P32["w1"]), d(P32["b1"]), *fold(P32["bn_p"]), d(P32["w2"]), d(P32["b2"]))
    plan = Neighbours(d(z["idx"]), z32["xyz_src"].shape[0])
    return z32, z64, pos, fold(P32["bn_w"]), plan, d


@pytest.mark.parametrize("shape", LAYER_SHAPES)
def test_relation_and_aggregate_against_float64(cuda, shape):
    """Per element within 1e-4 of the largest magnitude of the expected
    tensor; one aggregate with the logits scaled by 50 (softmax must not
    overflow); two runs bit-equal."""
    from o3dml_amd.point_transformer import aggregate, group, relation
    nq, ns, c, s = shape
    z32, z64, pos, (sw, tw), plan, d = _layer(cuda, shape)
    xq, xs = d(z32["xyz_q"]), d(z32["xyz_src"])
    want = relation_ref(z64["xyz_q"], z64["xyz_src"], z64["idx"], z64["k"], z64["q"], z64["P"]).numpy()
    got = relation(plan, xq, xs, d(z32["k"]), d(z32["q"]), pos, sw, tw)
    assert tuple(got.shape) == (nq, ns, c) and not got.requires_grad
    e = np.abs(n(got) - want).max() / np.abs(want).max()
    print("relation", shape, e)
    assert e <= 1e-4
    assert torch.equal(got, relation(plan, xq, xs, d(z32["k"]), d(z32["q"]), pos, sw, tw))
    for mult in (1.0, 50.0):
        want = aggregate_ref(z64["xyz_q"], z64["xyz_src"], z64["idx"], z64["v"], z64["w"] * mult, z64["P"], s).numpy()
        w = d(z32["w"] * mult)
        got = aggregate(plan, xq, xs, d(z32["v"]), w, pos, s)
        assert tuple(got.shape) == (nq, c) and torch.isfinite(got).all()
        e = np.abs(n(got) - want).max() / np.abs(want).max()
        print("aggregate", shape, mult, e)
        assert e <= 1e-4
        assert torch.equal(got, aggregate(plan, xq, xs, d(z32["v"]), w, pos, s))
    want = group_ref(z64["xyz_q"], z64["xyz_src"], z64["idx"], z64["v"]).numpy()
    got = group(plan, xq, xs, d(z32["v"]))
    assert tuple(got.shape) == (nq, ns, 3 + c)
    assert np.abs(n(got) - want).max() <= 1e-4 * np.abs(want).max()
    assert torch.equal(got[:, :, 3:], d(z32["v"])[plan.index.long().reshape(-1)].view(nq, ns, c))


def test_layer_ops_reject_bad_shapes(cuda):
    from o3dml_amd.point_transformer import Neighbours, aggregate, knn_interpolate, relation
    z32, _, pos, (sw, tw), plan, d = _layer(cuda, (65, 8, 32, 8))
    xq, xs = d(z32["xyz_q"]), d(z32["xyz_src"])
    with pytest.raises(RuntimeError, match="multiple of share_planes"):
        aggregate(plan, xq, xs, d(z32["v"]), d(z32["w"]), pos, 5)
    with pytest.raises(RuntimeError, match="feat_q must be float32"):
        relation(plan, xq, xs, d(z32["k"]), d(z32["q"]).double(), pos, sw, tw)
    wide = Neighbours(torch.zeros((4, 65), dtype=torch.int32, device=cuda), 65)
    with pytest.raises(RuntimeError, match="nsample must be in 1..64"):
        relation(wide, xq[:4], xs, d(z32["k"]), d(z32["q"])[:4], pos, sw, tw)
    with pytest.raises(RuntimeError, match="needs a plan with distances"):
        knn_interpolate(plan, d(z32["v"]))
    nine = Neighbours(torch.zeros((4, 9), dtype=torch.int32, device=cuda), 65, torch.ones((4, 9), device=cuda))
    with pytest.raises(RuntimeError, match="k must be in 1..8"):
        knn_interpolate(nine, d(z32["v"]))


# -------------------------------------------------------------- interpolation
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("c", [32, 48])
@pytest.mark.parametrize("nq", [1, 257])
def test_knn_interpolate_against_float64(cuda, k, c, nq):
    """Plans from knn_search with distances (bit-exact against the oracle); a
    query with three equidistant sources, and with nq = 257 queries that
    coincide with a source point (d = 0)."""
    import oracle as O
    from o3dml_amd.point_transformer import Neighbours, knn_interpolate
    rng = np.random.default_rng(7 + k + c)
    src = (rng.random((40, 3), dtype=np.float32) + 5).astype(np.float32)
    src[:3] = np.eye(3, dtype=np.float32)  # three sources at distance 1 from the origin
    qry = (rng.random((nq, 3), dtype=np.float32) * 2 + 4).astype(np.float32)
    qry[0] = 0
    if nq > 1:
        qry[1:21] = src[10:30]
    feat = rng.standard_normal((40, c)).astype(np.float32)
    plan = Neighbours.from_knn(torch.from_numpy(src).to(cuda), torch.from_numpy(qry).to(cuda), k, distances=True)
    oi, _, od = O.knn_search(src, qry, k, return_distances=True)
    assert np.array_equal(n(plan.index).reshape(-1), oi) and np.array_equal(n(plan.distance).reshape(-1), od)
    assert od.reshape(nq, k)[0].tolist() == [1.0] * k and (nq == 1 or od.reshape(nq, k)[1, 0] == 0.0)
    want = interpolate_ref(torch.from_numpy(feat).double(), plan.index.cpu().long(), plan.distance.cpu().double())
    got = knn_interpolate(plan, torch.from_numpy(feat).to(cuda))
    assert tuple(got.shape) == (nq, c)
    assert np.abs(n(got) - want.numpy()).max() <= 1e-4 * np.abs(want.numpy()).max()
    assert torch.equal(got, knn_interpolate(plan, torch.from_numpy(feat).to(cuda)))
    ones = knn_interpolate(plan, torch.ones((40, c), device=cuda))  # each row's weights sum to 1
    assert float((ones - 1).abs().max()) <= 1e-6


# ----------------------------------------------------------------------- plan
def test_plan_constructor_checks_the_index_range(cuda):
    from o3dml_amd.point_transformer import Neighbours
    idx = torch.zeros((5, 4), dtype=torch.int32, device=cuda)
    assert Neighbours(idx, 7).index.dtype == torch.int32
    assert Neighbours(idx.long() + 6, 7).index.dtype == torch.int32
    for bad in (-1, 7):
        idx2 = idx.clone()
        idx2[3, 2] = bad
        with pytest.raises(RuntimeError, match=r"index entries must lie in \[0, 7\)"):
            Neighbours(idx2, 7)
    with pytest.raises(RuntimeError, match="fewer than k"):
        Neighbours.from_knn(torch.rand(5, 3, device=cuda), torch.rand(2, 3, device=cuda), 6)


# ---------------------------------------------------------------------- model
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(G, "point_transformer.npz"))


@pytest.fixture(scope="module")
def model(cuda, golden):
    import pt_weights
    from o3dml_amd.point_transformer import PointTransformer
    z = golden
    m = PointTransformer(blocks=[int(b) for b in z["blocks"]], in_channels=int(z["in_channels"]),
                         num_classes=int(z["num_classes"]))
    m.load_state_dict(pt_weights.state_dict_for(m), strict=True)
    return m.to(cuda).eval()


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


def test_model_eval_against_float64_reference(cuda, golden, model):
    """First every level's sampled rows equal the stored ones (a mismatch there
    must not show up as a logit error); then the logit rows within
    max(8 x the reference's own float32 error, 1e-4) of the largest of the
    float64 rows.  Scaling one positional Linear by 1 + 1e-2 must break that
    bound.  A second forward is bitwise equal and copies nothing to the host."""
    z = golden
    batch = {"point": torch.from_numpy(z["points"]).to(cuda), "feat": torch.from_numpy(z["feat"]).to(cuda),
             "row_splits": torch.from_numpy(z["row_splits"])}
    logits = model(batch)
    assert tuple(logits.shape) == (len(z["points"]), int(z["num_classes"])) and not logits.requires_grad
    sampled = model.sampled_indices()
    assert len(sampled) == 4
    for lvl, s in enumerate(sampled, 1):
        assert s.dtype == torch.int32 and np.array_equal(n(s), z[f"fps_level{lvl}"]), lvl
    step, bound = int(z["row_step"]), max(8 * float(z["ref32_err_rows"]), 1e-4)
    e = _rel(n(logits)[::step], z["f64_logit_rows"])
    print("logit rows", e, "bound", bound)
    assert e <= bound

    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = model(batch)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.equal(again, logits)

    w = model.state_dict()["encoders.1.1.transformer2.linear_p.3.weight"]
    keep = w.clone()
    try:
        w.mul_(1 + 1e-2)
        e2 = _rel(n(model(batch))[::step], z["f64_logit_rows"])
    finally:
        w.copy_(keep)
    print("with linear_p.3.weight scaled by 1.01:", e2)
    assert e2 > bound


def test_model_other_batch_and_errors(cuda, model):
    """Attribute access, in_channels features checked, a cloud too small for
    the deepest level named before anything runs."""
    import types
    pts = torch.rand(4096, 3, device=cuda)
    out = model(types.SimpleNamespace(point=pts, feat=torch.rand(4096, 3, device=cuda),
                                      row_splits=torch.tensor([0, 4096])))
    assert tuple(out.shape) == (4096, 13) and torch.isfinite(out).all()
    with pytest.raises(RuntimeError, match="level 4"):
        model({"point": pts[:4000], "feat": pts[:4000], "row_splits": torch.tensor([0, 4000])})
    with pytest.raises(RuntimeError, match="feat must be float32"):
        model({"point": pts, "feat": torch.rand(4096, 4, device=cuda), "row_splits": torch.tensor([0, 4096])})
