"""PointTransformer without a GPU: the module tree against the reference's
stored state_dict layout, level_row_splits, the loud failures, and the float64
torch restatements of the four gather ops that tests/test_gpu_point_transformer.py
holds the HIP kernels to.  The restatements follow the reference's layer
(ml3d/torch/models/point_transformer.py:427-467, :650-697, :737-776) on raw
BatchNorm tensors; a test here checks them against torch modules applied as
the reference applies them (BatchNorm1d on the transposed tensor)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, G)

EPS = 1e-5


# ------------------------------------------------------------ restatements
def bn_eval(x, bn):
    """BatchNorm in eval form over the last axis; bn = (weight, bias, mean, var)."""
    g, b, mean, var = bn
    return (x - mean) / torch.sqrt(var + EPS) * g + b


def point_r_ref(xyz_q, xyz_src, idx, P):
    """linear_p on the relative coordinates: (n, nsample, c)."""
    d = xyz_src[idx.reshape(-1)].view(idx.shape[0], idx.shape[1], 3) - xyz_q.unsqueeze(1)
    h = torch.relu(bn_eval(d @ P["w1"].T + P["b1"], P["bn_p"]))
    return h @ P["w2"].T + P["b2"]


def relation_ref(xyz_q, xyz_src, idx, feat_k, feat_q, P):
    n, ns = idx.shape
    w = feat_k[idx.reshape(-1)].view(n, ns, -1) - feat_q.unsqueeze(1) + point_r_ref(xyz_q, xyz_src, idx, P)
    return torch.relu(bn_eval(w, P["bn_w"]))


def aggregate_ref(xyz_q, xyz_src, idx, feat_v, weight, P, s):
    n, ns = idx.shape
    c = feat_v.shape[1]
    w = torch.softmax(weight, dim=1)
    v = feat_v[idx.reshape(-1)].view(n, ns, c) + point_r_ref(xyz_q, xyz_src, idx, P)
    return (v.view(n, ns, s, c // s) * w.unsqueeze(2)).sum(1).view(n, c)


def interpolate_ref(feat, idx, dist):
    dist_recip = 1.0 / (dist + 1e-8)
    weight = dist_recip / torch.sum(dist_recip, dim=1, keepdim=True)
    out = torch.zeros((idx.shape[0], feat.shape[1]), dtype=feat.dtype)
    for i in range(idx.shape[1]):
        out += feat[idx[:, i]] * weight[:, i].unsqueeze(-1)
    return out


def group_ref(xyz_q, xyz_src, idx, feat):
    n, ns = idx.shape
    g = xyz_src[idx.reshape(-1)].view(n, ns, 3) - xyz_q.unsqueeze(1)
    return torch.cat((g, feat[idx.reshape(-1)].view(n, ns, -1)), -1)


def layer_case(n, ns, c, s, seed=0, n_src=None):
    """float64 inputs of one Transformer layer: random indices (repeats
    included), rows 0 and n // 2 with idx[i, :] = i, and the last row naming
    the last source row only."""
    n_src = n if n_src is None else n_src
    rng = np.random.default_rng(seed + 1000 * n + c)
    f = lambda *sh: torch.from_numpy(rng.standard_normal(sh))  # noqa: E731
    idx = rng.integers(0, n_src, (n, ns))
    idx[0, :] = 0
    idx[n // 2, :] = min(n // 2, n_src - 1)
    idx[-1, :] = n_src - 1
    bn = lambda k: (1 + 0.1 * f(k), 0.1 * f(k), 0.1 * f(k), 1 + 0.5 * torch.from_numpy(rng.random(k)))  # noqa: E731
    P = {"w1": f(3, 3) / 3 ** 0.5, "b1": 0.05 * f(3), "bn_p": bn(3), "w2": f(c, 3) / 3 ** 0.5, "b2": 0.05 * f(c),
         "bn_w": bn(c)}
    return {"xyz_q": 2 * f(n, 3), "xyz_src": 2 * f(n_src, 3), "idx": torch.from_numpy(idx), "k": f(n_src, c),
            "q": f(n, c), "v": f(n_src, c), "w": f(n, ns, c // s), "P": P}


# -------------------------------------------------------------------- tests
def test_restatements_match_the_modules():
    """The restatements against nn modules in float64 applied as the reference
    applies them: BatchNorm1d in eval() on the transposed (n, c, nsample)
    tensor, Softmax(dim=1), and the view / unsqueeze product of :464-465."""
    n, ns, c, s = 9, 5, 16, 8
    z = layer_case(n, ns, c, s)
    P = z["P"]

    def bn_mod(k, t):
        m = torch.nn.BatchNorm1d(k).double().eval()
        with torch.no_grad():
            m.weight.copy_(t[0]), m.bias.copy_(t[1]), m.running_mean.copy_(t[2]), m.running_var.copy_(t[3])
        return m

    with torch.no_grad():
        d = group_ref(z["xyz_q"], z["xyz_src"], z["idx"], z["k"])
        point_r, feat_k = d[:, :, 0:3], d[:, :, 3:]
        point_r = point_r @ P["w1"].T + P["b1"]
        point_r = bn_mod(3, P["bn_p"])(point_r.transpose(1, 2).contiguous()).transpose(1, 2).contiguous()
        point_r = torch.relu(point_r) @ P["w2"].T + P["b2"]
        w = feat_k - z["q"].unsqueeze(1) + point_r
        w = torch.relu(bn_mod(c, P["bn_w"])(w.transpose(1, 2).contiguous()).transpose(1, 2).contiguous())
        assert torch.allclose(w, relation_ref(z["xyz_q"], z["xyz_src"], z["idx"], z["k"], z["q"], P), atol=1e-12)
        sm = torch.nn.Softmax(dim=1)(z["w"])
        feat_v = z["v"][z["idx"].reshape(-1)].view(n, ns, c)
        want = ((feat_v + point_r).view(n, ns, s, c // s) * sm.unsqueeze(2)).sum(1).view(n, c)
        got = aggregate_ref(z["xyz_q"], z["xyz_src"], z["idx"], z["v"], z["w"], P, s)
        assert torch.allclose(want, got, atol=1e-12)
        # channel ch takes the softmax column ch mod (c / s)
        j = torch.softmax(z["w"], 1)
        one = sum(j[3, t, 11 % (c // s)] * (feat_v[3, t, 11] + point_r[3, t, 11]) for t in range(ns))
        assert abs(float(one - got[3, 11])) < 1e-12


def test_interpolate_restatement_weights():
    feat = torch.eye(4, dtype=torch.float64)
    idx = torch.tensor([[0, 1, 2], [3, 3, 3]])
    dist = torch.tensor([[0.0, 1.0, 1.0], [2.0, 2.0, 2.0]], dtype=torch.float64)
    out = interpolate_ref(feat, idx, dist)
    assert torch.allclose(out.sum(1), torch.ones(2, dtype=torch.float64), atol=1e-12)
    assert out[0, 0] > 1 - 1e-7 and abs(float(out[1, 3]) - 1) < 1e-12


def test_state_dict_layout_matches_the_reference():
    from o3dml_amd.point_transformer import PointTransformer
    want = json.load(open(os.path.join(G, "point_transformer_state_dict.json")))["PointTransformer"]
    got = [[k, list(v.shape)] for k, v in PointTransformer().state_dict().items()]
    assert got == want
    assert sum(p.numel() for p in PointTransformer().parameters()) == 4854145


def test_pt_weights_load_strict():
    import pt_weights
    from o3dml_amd.point_transformer import PointTransformer
    m = PointTransformer()
    sd = pt_weights.state_dict_for(m)
    m.load_state_dict(sd, strict=True)
    assert 1.0 <= float(sd["encoders.1.1.bn1.running_var"].min()) and float(sd["cls.1.running_var"].max()) <= 1.5
    assert abs(float(sd["encoders.1.1.transformer2.linear_w.0.weight"].mean()) - 1) < 0.1  # a BatchNorm
    assert abs(float(sd["encoders.1.1.transformer2.linear_w.2.weight"].mean())) < 0.1  # a Linear
    again = pt_weights.state_dict_for(PointTransformer())
    assert all(torch.equal(sd[k], again[k]) for k in sd)


def test_level_row_splits():
    from o3dml_amd.point_transformer import level_row_splits
    lv = level_row_splits([0, 4500, 10501])
    assert [np.diff(x).tolist() for x in lv] == [[4500, 6001], [1125, 1500], [281, 375], [70, 93], [17, 23]]
    assert all(x.dtype == np.int64 and x[0] == 0 for x in lv)
    assert [np.diff(x).tolist() for x in level_row_splits(torch.tensor([0, 4096]))][-1] == [16]
    with pytest.raises(RuntimeError, match=r"level 4.*cloud 0"):
        level_row_splits([0, 4095])
    with pytest.raises(RuntimeError, match=r"level 0.*cloud 1"):
        level_row_splits([0, 5000, 5007])


def test_ops_fail_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from o3dml_amd import point_transformer as pt
    xyz, feat = torch.zeros(8, 3), torch.zeros(8, 8)
    idx = torch.zeros((8, 2), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no ROCm GPU"):
        pt.furthest_point_sample_ragged(xyz, [0, 8], [0, 2])
    with pytest.raises(RuntimeError, match="no ROCm GPU"):
        pt.Neighbours(idx, 8)
    with pytest.raises(RuntimeError, match="no ROCm GPU"):
        pt.Neighbours.from_knn(xyz, xyz, 2)
    pos = (torch.zeros(3, 3), torch.zeros(3), torch.zeros(3), torch.zeros(3), torch.zeros(8, 3), torch.zeros(8))
    with pytest.raises(RuntimeError, match="no ROCm GPU"):
        pt.relation(None, xyz, xyz, feat, feat, pos, torch.ones(8), torch.zeros(8))
    with pytest.raises(RuntimeError, match="no ROCm GPU"):
        pt.aggregate(None, xyz, xyz, feat, torch.zeros(8, 2, 1), pos, 8)
    with pytest.raises(RuntimeError, match="no ROCm GPU"):
        pt.knn_interpolate(None, feat)
    with pytest.raises(RuntimeError, match="no ROCm GPU"):
        pt.group(None, xyz, xyz, feat)
    with pytest.raises(RuntimeError, match="no ROCm GPU"):
        pt.PointTransformer().eval()({"point": xyz, "feat": torch.zeros(8, 3), "row_splits": torch.tensor([0, 8])})


def test_ops_are_not_open3d_names():
    from o3dml_amd import ops
    for name in ("furthest_point_sample_ragged", "relation", "aggregate", "knn_interpolate", "group"):
        assert name not in ops.__all__


def test_train_mode_forward_raises():
    from o3dml_amd.point_transformer import Bottleneck, PointTransformer
    m = PointTransformer().train()
    batch = {"point": torch.zeros(8, 3), "feat": torch.zeros(8, 3), "row_splits": torch.tensor([0, 8])}
    with pytest.raises(NotImplementedError, match="PointTransformer: training is not built yet"):
        m(batch)
    with pytest.raises(NotImplementedError, match="training is not built yet"):
        Bottleneck(8, 8).train()([torch.zeros(8, 3), torch.zeros(8, 8), np.array([0, 8])])
