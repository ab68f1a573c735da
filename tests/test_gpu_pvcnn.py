"""PVCNN on the GPU.  Op level: trilinear devoxelize forward / backward and mean
voxelize forward / backward against the numpy restatements of test_pvcnn.py,
bit for bit.  Model level: one train step and one eval forward + backward of
o3dml_amd.pvcnn.PVCNN(width_multiplier=0.25) on the stored weights against the
reference's float64 run (tests/golden/pvcnn.npz)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_pvcnn import (G, SHAPES, devox_backward_ref, devox_forward_ref, make_case,  # noqa: E402
                        vox_backward_ref, vox_forward_ref)

pytestmark = pytest.mark.gpu

_CASES = {}


def case(B, C, N, r):
    """Inputs and float32 restatement results of one shape, computed once."""
    key = (B, C, N, r)
    if key not in _CASES:
        coords, feat, grad, vox, pfeat, ggrid = make_case(B, C, N, r)
        outs, inds, wgts = devox_forward_ref(coords, feat, r)
        gfeat = devox_backward_ref(grad, inds, wgts, r)
        grid, cnt = vox_forward_ref(pfeat, vox, r)
        gp = vox_backward_ref(ggrid, vox, cnt, r)
        d = dict(coords=coords, feat=feat, grad=grad, vox=vox, pfeat=pfeat, ggrid=ggrid, outs=outs, inds=inds,
                 wgts=wgts, gfeat=gfeat, grid=grid, cnt=cnt, gp=gp)
        for v in d.values():
            v.setflags(write=False)
        _CASES[key] = d
    return _CASES[key]


def t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


def n(x):
    return x.detach().cpu().numpy()


# ---------------------------------------------------------------- op level
@pytest.mark.parametrize("B,C,N,r", SHAPES)
def test_devoxelize_forward_backward_bitwise(cuda, B, C, N, r):
    from o3dml_amd import ops
    c = case(B, C, N, r)
    coords, feat = t(c["coords"], cuda), t(c["feat"], cuda)
    outs, inds, wgts = ops.trilinear_devoxelize_forward(r, True, coords, feat)
    assert outs.dtype == torch.float32 and inds.dtype == torch.int32 and wgts.dtype == torch.float32
    assert np.array_equal(n(inds), c["inds"])
    assert np.array_equal(n(wgts), c["wgts"])
    assert np.array_equal(n(outs), c["outs"])
    # [B,C,r,r,r] features are the same call; eval mode: same outs, zero-filled inds / wgts at full shape
    o2, i2, w2 = ops.trilinear_devoxelize_forward(r, False, coords, feat.reshape(B, C, r, r, r))
    assert torch.equal(o2, outs) and i2.shape == inds.shape and w2.shape == wgts.shape
    assert not i2.any() and not w2.any()
    grad = t(c["grad"], cuda)
    g = ops.trilinear_devoxelize_backward(grad, inds, wgts, r)
    assert g.shape == (B, C, r ** 3) and np.array_equal(n(g), c["gfeat"])
    # run twice: bitwise equal
    o3, i3, w3 = ops.trilinear_devoxelize_forward(r, True, coords, feat)
    assert torch.equal(o3, outs) and torch.equal(i3, inds) and torch.equal(w3, wgts)
    assert torch.equal(ops.trilinear_devoxelize_backward(grad, inds, wgts, r), g)
    # torch.ops.open3d.* returns exactly what o3dml_amd.ops returns
    import o3dml_amd
    o3dml_amd.register_torch_ops()
    for a, b in zip(torch.ops.open3d.trilinear_devoxelize_forward(r, True, coords, feat), (outs, inds, wgts)):
        assert torch.equal(a, b)
    assert torch.equal(torch.ops.open3d.trilinear_devoxelize_backward(grad, inds, wgts, r), g)


@pytest.mark.parametrize("B,C,N,r", SHAPES)
def test_avg_voxelize_bitwise(cuda, B, C, N, r):
    from o3dml_amd.pvcnn import AvgVoxelization, VoxelPlan
    c = case(B, C, N, r)
    plan = VoxelPlan(t(c["vox"], cuda), r)
    assert plan.cnt.dtype == torch.int32 and np.array_equal(n(plan.cnt), c["cnt"])
    feat = t(c["pfeat"], cuda).requires_grad_(True)
    grid = AvgVoxelization.apply(feat, plan)
    assert grid.shape == (B, C, r, r, r)
    assert np.array_equal(n(grid).reshape(B, C, -1), c["grid"])
    (gp,) = torch.autograd.grad(grid, feat, t(c["ggrid"], cuda).reshape(grid.shape))
    assert np.array_equal(n(gp), c["gp"])
    # the plan is reused; a second plan and run are bitwise equal
    again = AvgVoxelization.apply(feat, plan)
    other = AvgVoxelization.apply(feat, VoxelPlan(t(c["vox"], cuda), r))
    assert torch.equal(again, grid) and torch.equal(other, grid)


def test_avg_voxelize_one_voxel_and_one_point_per_voxel(cuda):
    from o3dml_amd.pvcnn import VoxelPlan, avg_voxelize
    rng = np.random.default_rng(7)
    B, C, N, r = 2, 5, 1500, 12
    feat = rng.standard_normal((B, C, N)).astype(np.float32)
    ggrid = rng.standard_normal((B, C, r ** 3)).astype(np.float32)
    one = np.zeros((B, 3, N), np.int32)
    one[:, 0], one[:, 1], one[:, 2] = 3, 11, 7           # every point in voxel (3, 11, 7)
    perm = np.stack([rng.permutation(r ** 3)[:N] for _ in range(B)])
    own = np.stack([perm // (r * r), (perm // r) % r, perm % r], 1).astype(np.int32)  # every point its own voxel
    outside = own.copy()
    outside[:, :, :40] += np.where(own[:, :, :40] == 0, -3, 0) + np.where(own[:, :, :40] == r - 1, 5, 0)
    for vox in (one, own, outside):
        want, cnt = vox_forward_ref(feat, vox, r)
        f = t(feat, cuda).requires_grad_(True)
        plan = VoxelPlan(t(vox, cuda), r)
        grid = avg_voxelize(f, plan)
        assert np.array_equal(n(plan.cnt), cnt)
        assert np.array_equal(n(grid).reshape(B, C, -1), want)
        (g,) = torch.autograd.grad(grid, f, t(ggrid, cuda).reshape(grid.shape))
        assert np.array_equal(n(g), vox_backward_ref(ggrid, vox, cnt, r))
    assert cnt.max() == 1 and np.array_equal(vox_forward_ref(feat, own, r)[0], want)  # clamped back onto `own`


def test_devoxelize_backward_one_coordinate_and_bad_indices(cuda):
    from o3dml_amd import ops
    rng = np.random.default_rng(8)
    B, C, N, r = 2, 3, 700, 6
    grad = rng.standard_normal((B, C, N)).astype(np.float32)
    feat = rng.standard_normal((B, C, r ** 3)).astype(np.float32)
    coords = np.empty((B, 3, N), np.float32)
    coords[:, 0], coords[:, 1], coords[:, 2] = 2.25, 4.5, 0.125     # all points at one coordinate
    outs, inds, wgts = ops.trilinear_devoxelize_forward(r, True, t(coords, cuda), t(feat, cuda))
    want_o, want_i, want_w = devox_forward_ref(coords, feat, r)
    assert np.array_equal(n(outs), want_o) and np.array_equal(n(inds), want_i) and np.array_equal(n(wgts), want_w)
    g = ops.trilinear_devoxelize_backward(t(grad, cuda), inds, wgts, r)
    assert np.array_equal(n(g), devox_backward_ref(grad, want_i, want_w, r))
    assert np.count_nonzero(n(g)[0, 0]) == 8
    # caller-made indices holding -1 and r3: those entries contribute nothing
    coords = (rng.random((B, 3, N), dtype=np.float32) * (r - 1)).astype(np.float32)
    _, inds, wgts = devox_forward_ref(coords, feat, r)
    bad = inds.copy()
    bad[:, 0, ::3] = -1
    bad[:, 6, 1::4] = r ** 3
    bad[1, 3, :5] = np.iinfo(np.int32).min
    g = ops.trilinear_devoxelize_backward(t(grad, cuda), t(bad, cuda), t(wgts, cuda), r)
    assert np.array_equal(n(g), devox_backward_ref(grad, bad, wgts, r))


def test_empty_inputs_and_limits(cuda):
    from o3dml_amd import ops
    from o3dml_amd.pvcnn import VoxelPlan, avg_voxelize
    r = 3
    for B, C, N in ((0, 4, 10), (2, 0, 10), (2, 4, 0)):
        coords = torch.zeros((B, 3, N), device=cuda)
        feat = torch.randn((B, C, r ** 3), device=cuda)
        outs, inds, wgts = ops.trilinear_devoxelize_forward(r, True, coords, feat)
        assert outs.shape == (B, C, N) and inds.shape == (B, 8, N) and wgts.shape == (B, 8, N)
        g = ops.trilinear_devoxelize_backward(torch.randn((B, C, N), device=cuda), inds, wgts, r)
        assert g.shape == (B, C, r ** 3) and not g.any()
        grid = avg_voxelize(torch.randn((B, C, N), device=cuda), VoxelPlan(torch.zeros((B, 3, N), dtype=torch.int32,
                                                                                       device=cuda), r))
        assert grid.shape == (B, C, r, r, r) and not grid.any()
    # limits are raised before any launch: r3 > 2^31 - 1, B * r3 >= 2^32 - 1 (nothing of that size is allocated)
    from o3dml_amd import _lib
    from o3dml_amd._util import stream_handle
    st = stream_handle(cuda)
    for B, N, rr in ((1, 8, 1291), (4, 8, 1100), (1, 1 << 29, 2), (1, 8, 0)):
        with pytest.raises(RuntimeError):
            _lib.call("o3dml_trilinear_devoxelize_forward", None, None, B, 1, N, rr, 1, None, None, None, st)
        with pytest.raises(RuntimeError):
            _lib.call("o3dml_trilinear_devoxelize_backward", None, None, None, B, 1, N, rr, None, None, 0, st)
    with pytest.raises(RuntimeError):
        _lib.call("o3dml_avg_voxelize_plan", None, 1, 8, 1291, None, None, 0, st)
    torch.cuda.synchronize()


@pytest.mark.parametrize("B,C,N,r", SHAPES[1:3])
def test_autograd_functions_against_float64(cuda, B, C, N, r):
    """The two autograd functions' gradients against the float64 restatement,
    per element within 1e-4 of the largest."""
    from o3dml_amd.pvcnn import AvgVoxelization, DevoxelizePlan, VoxelPlan, trilinear_devoxelize
    c = case(B, C, N, r)
    _, i64, w64 = devox_forward_ref(c["coords"], c["feat"], r, np.float64)
    want = devox_backward_ref(c["grad"], i64, w64, r, np.float64)
    feat = t(c["feat"], cuda).reshape(B, C, r, r, r).requires_grad_(True)
    coords = t(c["coords"], cuda)
    out = trilinear_devoxelize(feat, coords, r, True)
    (g,) = torch.autograd.grad(out, feat, t(c["grad"], cuda))
    assert g.shape == feat.shape
    assert np.abs(n(g).reshape(B, C, -1) - want).max() <= 1e-4 * np.abs(want).max()
    # a shared plan (indices written once, lists built once) gives the same bits, twice
    plan = DevoxelizePlan(coords, r)
    for _ in range(2):
        o2 = trilinear_devoxelize(feat, coords, r, True, plan)
        (g2,) = torch.autograd.grad(o2, feat, t(c["grad"], cuda))
        assert torch.equal(o2, out) and torch.equal(g2, g)
    # eval mode without grad: same values
    with torch.no_grad():
        assert torch.equal(trilinear_devoxelize(feat, coords, r, False), out)
    _, cnt = vox_forward_ref(c["pfeat"], c["vox"], r, np.float64)
    want = vox_backward_ref(c["ggrid"], c["vox"], cnt, r, np.float64)
    pf = t(c["pfeat"], cuda).requires_grad_(True)
    grid = AvgVoxelization.apply(pf, VoxelPlan(t(c["vox"], cuda), r))
    (gp,) = torch.autograd.grad(grid, pf, t(c["ggrid"], cuda).reshape(grid.shape))
    assert np.abs(n(gp) - want).max() <= 1e-4 * np.abs(want).max()


# ---------------------------------------------------------------- model level
def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(G, "pvcnn.npz"))


@pytest.fixture(scope="module")
def model(cuda, golden):
    from o3dml_amd.pvcnn import PVCNN
    z = golden
    m = PVCNN(num_classes=int(z["num_classes"]), width_multiplier=float(z["width_multiplier"]),
              voxel_resolution_multiplier=float(z["voxel_resolution_multiplier"]))
    sd = m.state_dict()
    for k in z["weight_names"]:
        sd[str(k)] = torch.from_numpy(z["w:" + str(k)])
    m.load_state_dict(sd)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = float(z["dropout_p"])
    return m.to(cuda)


def _step(m, z, cuda, train):
    m.train(train)
    m.zero_grad()
    pts = torch.from_numpy(z["points"]).to(cuda)
    feat = torch.cat([pts, torch.from_numpy(z["extra"]).to(cuda)], 1)
    logits = m({"point": pts, "feat": feat})
    nc = logits.shape[-1]
    loss = torch.nn.functional.cross_entropy(logits.reshape(-1, nc), torch.from_numpy(z["labels"]).to(cuda).reshape(-1))
    loss.backward()
    return logits, loss


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_model_step_against_float64_reference(cuda, golden, model, mode):
    """Every stored quantity within max(8 x the reference's own float32 error,
    1e-4 relative) of the reference's float64 run (MIOpen's and the CPU's
    convolutions are two independent float32 evaluations of the same
    well-conditioned instance, hence the 8), the generator's 1e-2 / 5 % above
    5e-4 conditions on the build's errors as well, and the parameters whose
    float64 gradient is (analytically) zero bounded absolutely."""
    z = golden
    start = {k: v.clone() for k, v in model.state_dict().items()}
    try:
        logits, loss = _step(model, z, cuda, mode == "train")
        p = f"pv_{mode}_"
        step = int(z["row_step"])
        bound = lambda key: max(8 * float(z[p + key]), 1e-4)  # noqa: E731
        assert tuple(logits.shape) == (z["labels"].shape[0], z["labels"].shape[1], int(z["num_classes"]))
        rows = n(logits).reshape(-1, logits.shape[-1])[::step]
        e_rows = _rel(rows, z[p + "f64_logit_rows"])
        e_loss = abs(loss.item() - float(z[p + "f64_loss"])) / abs(float(z[p + "f64_loss"]))
        print(mode, "rows", e_rows, "bound", bound("ref32_err_rows"), "loss", e_loss, "bound", bound("ref32_err_loss"))
        names = [str(k) for k in z[p + "grad_names"]]
        params = dict(model.named_parameters())
        assert names == list(params)
        n64 = z[p + "f64_grad_norms"]
        mine = np.array([float(params[k].grad.double().norm().item()) for k in names])
        live = n64 > 1e-6 * n64.max()
        e_norm = np.where(live, np.abs(mine - n64) / np.maximum(n64, 1e-300), 0.0)
        b_norm = np.maximum(8 * z[p + "ref32_err_norms"], 1e-4)
        worst = int(np.argmax(e_norm / b_norm))
        print(mode, "live", int(live.sum()), "norm error max", e_norm.max(), "worst vs bound", names[worst],
              e_norm[worst], b_norm[worst], "above 5e-4:", int((e_norm > 5e-4).sum()))
        e_full = {}
        for k in z["full_grad_names"]:
            k = str(k)
            e_full[k] = _rel(n(params[k].grad), z[p + "f64_grad:" + k])
            print(mode, "full gradient", k, e_full[k], "bound", bound("ref32_err_grad:" + k))
        assert e_rows <= bound("ref32_err_rows")
        assert e_loss <= bound("ref32_err_loss")
        assert np.all(mine[~live] <= 1e-5 * n64.max()), mine[~live]
        assert np.all(e_norm <= b_norm), [(names[i], e_norm[i], b_norm[i]) for i in np.nonzero(e_norm > b_norm)[0]]
        for k, e in e_full.items():
            assert e <= bound("ref32_err_grad:" + k), (k, e)
        every = [e_rows, e_loss, float(e_norm.max())] + list(e_full.values())
        tensor_errs = [max(e, e_full.get(k, 0.0)) for k, e, lv in zip(names, e_norm, live) if lv]
        if mode == "train":
            sd = model.state_dict()
            for k, ref_err in zip(z[p + "bn_names"], z[p + "ref32_err_bn"]):
                e = _rel(n(sd[str(k)]), z[p + "f64_bn:" + str(k)])
                every.append(e)
                assert e <= max(8 * float(ref_err), 1e-4), (str(k), e)
            print(mode, "bn error max", max(every[-len(z[p + "bn_names"]):]))
        assert max(every) <= 1e-2
        assert sum(e > 5e-4 for e in tensor_errs) <= 0.05 * len(tensor_errs)
    finally:
        model.load_state_dict(start)


def test_model_point_voxel_transfers_reproducible(cuda, golden, model):
    """Two identical train steps: the voxelize outputs of every block's input
    and, on one fixed voxel grid, the devoxelize output and gradient are
    bitwise equal.  MIOpen's Conv3d forward proved deterministic on the MI355X
    (logits, conv output and the first conv's weight gradient all bitwise equal
    between the two steps), so the whole-model logits are compared bit for bit
    too; the weight gradient (MIOpen's backward) is only printed."""
    from o3dml_amd.pvcnn import PVConv, trilinear_devoxelize
    start = {k: v.clone() for k, v in model.state_dict().items()}
    seen = []
    first = [b for b in model.point_features if isinstance(b, PVConv)][0]
    hooks = [first.voxelization.register_forward_hook(lambda mod, inp, out: seen.append([o for o in out[:2]])),
             first.voxel_layers.register_forward_hook(lambda mod, inp, out: seen.append([out.detach().clone()]))]
    try:
        runs = []
        for _ in range(2):
            model.load_state_dict(start)
            seen.clear()
            logits, _ = _step(model, golden, cuda, True)
            runs.append(([x.detach().clone() for x in seen[0]], seen[1][0], logits.detach().clone(),
                         first.voxel_layers[0].weight.grad.clone()))
        (vox_a, grid_a, log_a, gw_a), (vox_b, grid_b, log_b, gw_b) = runs
        assert torch.equal(vox_a[0], vox_b[0]) and torch.equal(vox_a[1], vox_b[1])
        print("logits bitwise equal:", torch.equal(log_a, log_b), "conv grid bitwise equal:",
              torch.equal(grid_a, grid_b), "first conv weight gradient bitwise equal:", torch.equal(gw_a, gw_b))
        assert torch.equal(log_a, log_b) and torch.equal(grid_a, grid_b)
        outs = []
        for _ in range(2):
            g = grid_a.clone().requires_grad_(True)
            o = trilinear_devoxelize(g, vox_a[1], first.resolution, True)
            (gg,) = torch.autograd.grad(o, g, torch.ones_like(o) * 0.37)
            outs.append((o.detach(), gg))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    finally:
        for h in hooks:
            h.remove()
        model.load_state_dict(start)
