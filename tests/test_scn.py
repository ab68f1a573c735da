"""SparseConvUnet module tree vs the reference (tests/golden/scn.npz, made by
make_golden_scn.py from ml3d/torch/models/sparseconvnet.py): identical
state_dict keys and shapes for the residual and the plain UNet, so reference
checkpoints load unchanged.  The logits are checked on the GPU
(test_gpu_scn.py).  Also on the CPU: the eval caches follow replaced
parameter / buffer objects, the training fixture keeps the conditions its
generator asserts, and the reference sparse-conv stand-in's autograd form
equals its detached float64 branch."""
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "scn.npz"))


def model(residual):
    from o3dml_amd.sparseconvnet import SparseConvUnet
    return SparseConvUnet(multiplier=8, residual_blocks=residual, conv_block_reps=1, num_classes=5)


@pytest.mark.parametrize("tag,residual", [("res", True), ("plain", False)])
def test_state_dict_manifest(tag, residual):
    sd = model(residual).state_dict()
    assert list(sd.keys()) == [str(k) for k in G[f"{tag}_keys"]]
    assert [",".join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in G[f"{tag}_shapes"]]


def test_graph_mode_rejects_unknown_values(monkeypatch):
    """O3DML_SCN_GRAPH takes "0", "1", "3" or nothing (= "3"); "2" (a removed
    mode) and any other value raise and name the three."""
    from o3dml_amd.sparseconvnet import _graph_mode
    monkeypatch.delenv("O3DML_SCN_GRAPH", raising=False)
    assert _graph_mode() == "3"
    for mode in ("0", "1", "3"):
        monkeypatch.setenv("O3DML_SCN_GRAPH", mode)
        assert _graph_mode() == mode
    for mode in ("2", "on"):
        monkeypatch.setenv("O3DML_SCN_GRAPH", mode)
        with pytest.raises(ValueError) as err:
            _graph_mode()
        assert all(f'"{ok}"' in str(err.value) for ok in ("0", "1", "3")) and repr(mode) in str(err.value)


def test_replaced_tensors_drop_the_eval_caches():
    """A parameter or buffer replaced by another tensor object (not modified
    in place) changes _param_key and drops whatever was captured on the old
    tensors; an in-place update changes the key and keeps the captures (they
    are keyed on it)."""
    import torch
    m = model(True).eval()
    name = "_o3dml_scn_plan_bodies"

    def key_with_capture():
        k = m._param_key()
        m.__dict__[name] = {"captured": k}
        assert m._param_key() == k and name in m.__dict__
        return k

    k = key_with_capture()
    with torch.no_grad():
        m.linear.linear.bias.add_(1.0)
    assert m._param_key() != k and name in m.__dict__
    k = key_with_capture()
    conv = m.unet.net[0].sub_sparse_conv1.net
    conv.kernel = torch.nn.Parameter(conv.kernel.detach() * 1.5)
    assert m._param_key() != k and name not in m.__dict__
    k = key_with_capture()
    m.batch_norm.bn.running_var = m.batch_norm.bn.running_var * 2.0
    assert m._param_key() != k and name not in m.__dict__
    k = key_with_capture()
    m.load_state_dict({n: v.detach().clone() for n, v in m.state_dict().items()}, assign=True)
    assert name not in m.__dict__ and m._param_key() != k


def test_folded_bn_follows_replaced_tensors():
    """The folded BatchNorm is refreshed when a tensor is replaced by a fresh
    one whose version counter equals the old one's (both 0)."""
    import torch
    from o3dml_amd.sparseconvnet import _folded_bn
    block = model(True).eval().batch_norm
    bn = block.bn
    bn.running_var = bn.running_var + 0.5  # as after .to(device): version 0
    scale, shift = _folded_bn(block)
    assert _folded_bn(block)[0] is scale  # cached
    fresh = bn.running_var * 4.0 + 1.0
    assert fresh._version == bn.running_var._version == 0
    bn.running_var = fresh
    scale2, shift2 = _folded_bn(block)
    assert torch.equal(scale2, bn.weight.detach() / torch.sqrt(fresh + bn.eps)) and not torch.equal(scale2, scale)
    assert torch.equal(shift2, bn.bias.detach() - bn.running_mean * scale2)
    with torch.no_grad():
        bn.running_mean.add_(1.0)  # in place: the version counter
    assert torch.equal(_folded_bn(block)[1], bn.bias.detach() - bn.running_mean * scale2)


def test_train_fixture_keeps_its_conditions():
    """tests/golden/scn_train.npz as make_golden_scn_train.py must leave it:
    room A above voxel.hip's kDeepMax = 8192 at level 0 and below from level 1
    on, no level empty, about a third of the voxels with 2 - 3 points, and the
    reference's own fp32-vs-fp64 errors small enough to keep the GPU test's
    bound tight (none above 1e-2, at most 5 % of the parameter tensors with a
    gradient-norm or full-gradient error above 5e-4)."""
    T = np.load(os.path.join(HERE, "golden", "scn_train.npz"))
    TG = np.load(os.path.join(HERE, "golden", "scn_train_grads.npz"))
    lv = T["room_a_levels"]
    assert len(lv) == 7 and lv[0] > 8192 >= lv[1] and lv.min() > 0
    pos, lengths = T["pos"], T["lengths"]
    assert lengths.sum() == len(pos) == len(T["feat"]) == len(T["labels"]) and T["feat"].shape[1] == 3
    assert np.array_equal(pos - np.floor(pos), np.full_like(pos, 0.5))
    _, counts = np.unique(pos[:lengths[0]], axis=0, return_counts=True)
    assert len(counts) == lv[0] and counts.max() == 3 and 0.28 < (counts > 1).mean() < 0.39
    assert T["labels"].min() >= 0 and T["labels"].max() < 20
    for mode in ("eval", "train"):
        p = f"scn_{mode}_"
        rows = -(-len(pos) // int(T["row_step"]))
        assert T[p + "f64_logit_rows"].shape == TG[p + "logit_rows"].shape == (rows, 20)
        assert len(T[p + "grad_names"]) == len(T[p + "f64_grad_norms"]) == len(T[p + "ref32_err_norms"])
        errs = [float(np.max(T[k])) for k in T.files if k.startswith(p + "ref32_err_")]
        assert max(errs) <= 1e-2
        for k in T["full_grad_names"]:
            assert p + "f64_grad:" + str(k) in TG.files and p + "ref32_err_grad:" + str(k) in T.files
        # a parameter tensor counts when its norm error OR its full-gradient error is above 5e-4
        full = {str(k): float(T[p + "ref32_err_grad:" + str(k)]) for k in T["full_grad_names"]}
        per_tensor = [max(float(e), full.get(str(k), 0.0)) for k, e in zip(T[p + "grad_names"], T[p + "ref32_err_norms"])]
        assert set(full) <= set(map(str, T[p + "grad_names"]))
        assert np.mean(np.array(per_tensor) > 5e-4) <= 0.05
    assert len(T["scn_train_bn_names"]) == len(T["scn_train_ref32_err_bn"]) == 78


def test_reference_stub_autograd_form():
    """tools/ref_loader.py's sparse-conv stand-in (the fixture generators'):
    with autograd it equals its detached float64 branch bit for bit and passes
    gradcheck, for the submanifold, strided and transposed convolutions."""
    import sys
    import torch
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    import oracle as O
    import ref_loader
    rng = np.random.default_rng(2)
    v = np.unique(rng.integers(0, 5, (200, 3)), axis=0)[:14]
    pos = torch.from_numpy(v.astype(np.float32) + 0.5)
    grid = torch.from_numpy(O.calculate_grid(pos.numpy()))
    g = torch.Generator().manual_seed(2)
    for cls, ks, off, ip, op in [(ref_loader._SparseConvStub, [3, 3, 3], 0.0, pos, pos),
                                 (ref_loader._SparseConvStub, [2, 2, 2], -0.5, pos, grid),
                                 (ref_loader._SparseConvTransposeStub, [2, 2, 2], -0.5, grid, pos)]:
        layer = cls(2, 3, ks, use_bias=True, offset=torch.full((3,), off)).double()
        x = torch.randn((ip.shape[0], 2), generator=g, dtype=torch.float64)
        k0 = torch.randn(layer.kernel.shape, generator=g, dtype=torch.float64)
        b0 = torch.randn(3, generator=g, dtype=torch.float64)

        def f(x, k, b):
            return torch.func.functional_call(layer, {"kernel": k, "bias": b}, (x, ip, op, 1.0))
        with torch.no_grad():
            a = f(x, k0, b0)
        leaves = [t.clone().requires_grad_(True) for t in (x, k0, b0)]
        b = f(*leaves)
        assert b.requires_grad and a.abs().max() > 0 and torch.equal(a, b.detach())
        assert torch.autograd.gradcheck(f, leaves)
