"""The gradients of ops.voxel_conv3d on the GPU against autograd through
torch.nn.functional.conv3d(padding=1) in float64 on the CPU.  The bound is that
of tests/test_gpu_voxel_conv3d.py: largest absolute difference over largest
reference magnitude <= 1e-4 per tensor, which the float32 evaluation on the CPU
has to keep too.  ops.voxel_conv3d_wgrad takes no buffers, so its first run goes
through the C ABI with dweight, dbias and the workspace pre-filled with NaN; the
run through ops has to equal it bitwise."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
BOUND = 1e-4
B = 2


def make(r, cin, cout, seed=0):
    # a third of the voxels empty; no mask at r = 1, where seed 0 empties both voxels and every reference is zero
    g = torch.Generator().manual_seed(seed)
    grid, gout = torch.randn(B, cin, r, r, r, generator=g), torch.randn(B, cout, r, r, r, generator=g)
    if r > 1:
        grid = grid * (torch.rand(B, 1, r, r, r, generator=g) > 1 / 3)
        gout = gout * (torch.rand(B, 1, r, r, r, generator=g) > 1 / 3)
    weight = torch.randn(cout, cin, 3, 3, 3, generator=g) / (27 * cin) ** 0.5
    return grid, gout, weight, 0.1 * torch.randn(cout, generator=g)


def reference(grid, gout, weight, bias, dtype, slope=None):
    """(dgrid, dweight, dbias) of sum(gout * act(conv3d(grid, weight, bias)))"""
    leaves = [t.to(dtype).requires_grad_() for t in (grid, weight, bias)]
    y = F.conv3d(*leaves, padding=1)
    return torch.autograd.grad(y if slope is None else F.leaky_relu(y, slope), leaves, gout.to(dtype))


def err(a, ref):
    return float((a.double().cpu() - ref).abs().max() / ref.abs().max())


def check(cuda, r, cin, cout, bias=True):
    from o3dml_amd import _lib, ops
    from o3dml_amd._util import ptr, stream_handle
    grid, gout, weight, b = make(r, cin, cout)
    ref = reference(grid, gout, weight, b, torch.float64)
    e32 = [err(a, f) for a, f in zip(reference(grid, gout, weight, b, torch.float32), ref)]
    assert max(e32) <= BOUND, e32
    dg, dgo, dw_ = grid.to(cuda), gout.to(cuda), weight.to(cuda)
    n = int(_lib.load().o3dml_voxel_conv3d_wgrad_workspace_size(B, cin, cout, r))
    nan = dict(fill_value=float("nan"), device=cuda)
    ws, dw, db = torch.full((n,), **nan), torch.full(weight.shape, **nan), torch.full((cout,), **nan)
    _lib.call("o3dml_voxel_conv3d_wgrad", ptr(dg), ptr(dgo), B, cin, cout, r, ptr(dw), ptr(db) if bias else None,
              ptr(ws), n, stream_handle(cuda))
    dw2, db2 = ops.voxel_conv3d_wgrad(dg, dgo, bias=bias)
    dx, dx2 = ops.voxel_conv3d_grad_input(dgo, dw_), ops.voxel_conv3d_grad_input(dgo, dw_)
    e = [err(dx, ref[0]), err(dw, ref[1])] + ([err(db, ref[2])] if bias else [])
    print(f"r {r} {cin} -> {cout}: dX, dW, db {e} (float32 on the CPU {e32}), bound {BOUND}")
    assert max(e) <= BOUND and dx.shape == grid.shape
    assert torch.equal(dw, dw2) and torch.equal(dx, dx2)  # run to run bitwise
    assert torch.equal(db, db2) if bias else db2 is None and bool(db.isnan().all())


# Slabs S and box by the launch rule (boxes = B ceil(r/2) ceil(r/4) ceil(r/ZT), S = min(ceil(256 / blocks),
# boxes / 2), at least 1); 9 -> 16 is one block.  r 1, 2: 2 boxes of 2 x 4 x 16, S = 1.  r 3: 4 boxes, S = 2.
# r 5: 12 boxes, S = 6.  r 16: 64 boxes, S = 32.  r 17: 90 boxes of 2 x 4 x 32, S = 45.  r 32: 256 boxes of
# 2 x 4 x 32, S = 128.  r 33: 918 boxes of 2 x 4 x 16 in S = 256 slabs of 3 or 4 boxes (does not divide).
@pytest.mark.parametrize("r", [1, 2, 3, 5, 16, 17, 32, 33])
def test_resolutions(cuda, r):
    check(cuda, r, 9, 16)


# All at 12 boxes of 2 x 4 x 16 but the last.  (5, 1, 1), (5, 9, 64) with 2 blocks, (5, 64, 64) with 4 and
# (5, 67, 33) with 2 x 3: S = 6.  (5, 130, 130): 25 blocks, ceil(256 / 25) = 11 -> S = 6.  (16, 64, 128): 64
# boxes, 8 blocks, S = 32.
@pytest.mark.parametrize("r, cin, cout", [(5, 1, 1), (5, 9, 64), (5, 64, 64), (5, 67, 33), (5, 130, 130),
                                          (16, 64, 128)])
def test_channels(cuda, r, cin, cout):
    check(cuda, r, cin, cout)


def test_no_bias(cuda):
    check(cuda, 5, 9, 16, bias=False)


def test_autograd_with_leaky_relu(cuda):
    from o3dml_amd import ops
    grid, gout, weight, b = make(5, 9, 16)
    ref = reference(grid, gout, weight, b, torch.float64, 0.1)
    e32 = [err(a, f) for a, f in zip(reference(grid, gout, weight, b, torch.float32, 0.1), ref)]
    leaves = [t.to(cuda).requires_grad_() for t in (grid, weight, b)]
    got = torch.autograd.grad(ops.voxel_conv3d(*leaves, negative_slope=0.1), leaves, gout.to(cuda))
    e = [err(a, f) for a, f in zip(got, ref)]
    print("dX, dW, db", e, "float32 on the CPU", e32, "bound", BOUND)
    assert max(e32) <= BOUND and max(e) <= BOUND
    with pytest.raises(RuntimeError, match="negative_slope > 0"):
        ops.voxel_conv3d(*leaves, negative_slope=0.0)


def test_channels_above_the_limit_raise(cuda):
    from o3dml_amd import ops
    small = torch.zeros(1, 8, 2, 2, 2, device=cuda)
    with pytest.raises(RuntimeError, match="grad_input.*513"):
        ops.voxel_conv3d_grad_input(small, torch.zeros(8, 513, 3, 3, 3, device=cuda))
    with pytest.raises(RuntimeError, match="wgrad.*513"):
        ops.voxel_conv3d_wgrad(small, torch.zeros(1, 513, 2, 2, 2, device=cuda))


def counted(fn):
    # (result of fn(), launches of voxel_conv3d, launches of voxel_conv3d_wgrad while it ran)
    from o3dml_amd import _lib
    lib = _lib.load()
    lib.o3dml_timing_enable(1)
    try:
        lib.o3dml_timing_reset()
        res = fn()
        torch.cuda.synchronize()
        t = _lib.kernel_times(["voxel_conv3d", "voxel_conv3d_wgrad"])
        return res, t["voxel_conv3d"][1], t["voxel_conv3d_wgrad"][1]
    finally:
        lib.o3dml_timing_enable(0)


@pytest.mark.parametrize("train", [True, False])
def test_module_switch(cuda, train):
    """fused_grad on against off on the same inputs: output, feature and
    parameter gradients, running statistics, launch counts.  No pre-activation
    of the off run may lie within 1e-5 of its layer's rms from zero: a
    LeakyReLU branch would flip on a float32 rounding."""
    from o3dml_amd.pvcnn import PVConv
    torch.manual_seed(0)  # the first seed at which the condition on the pre-activations holds in both modes
    pv = PVConv(9, 16, 3, resolution=8)
    for m in pv.modules():  # randomised BatchNorm, as tests/test_gpu_voxel_conv3d.py builds it
        if isinstance(m, torch.nn.BatchNorm3d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0, 0.1)
    pv = pv.to(cuda).train(train)
    coords, feat = torch.rand(2, 3, 200, device=cuda), torch.randn(2, 9, 200, device=cuda)
    gout = torch.randn(2, 16, 200, device=cuda)

    def run(on, feat_grad):
        m, f = copy.deepcopy(pv), feat.clone().requires_grad_(feat_grad)
        m.fused_grad = on
        margins = []
        for bn in [x for x in m.voxel_layers if isinstance(x, torch.nn.BatchNorm3d)]:
            bn.register_forward_hook(
                lambda _m, _i, o: margins.append(float(o.detach().abs().min() / o.detach().pow(2).mean().sqrt())))

        def step():
            out = m((f, coords))[0]
            leaves = dict(m.named_parameters(), **({"features": f} if feat_grad else {}))
            return dict(zip(leaves, torch.autograd.grad(out, list(leaves.values()), gout)), out=out.detach())
        res, fwd, wgrad = counted(step)
        res.update({k: b for k, b in m.state_dict().items() if "voxel_layers" in k and "running" in k})
        return res, (fwd, wgrad), margins

    assert run(True, False)[1] == (3, 2)  # the first layer's data gradient is skipped
    on, launches_on, _ = run(True, True)
    off, launches_off, margins = run(False, True)
    errs = {k: err(on[k], off[k].double().cpu()) for k in off}
    if train:  # batch statistics remove a constant: the exact gradient of a convolution's bias is zero, both runs
        # hold rounding noise, which is held to the bound relative to that layer's weight gradient
        for conv in ("voxel_layers.0", "voxel_layers.3", "point_features.layers.0"):
            errs[conv + ".bias"] = float((on[conv + ".bias"] - off[conv + ".bias"]).abs().max()
                                         / off[conv + ".weight"].abs().max())
    print("train" if train else "eval", "errors", errs, "margins", margins, "bound", BOUND)
    assert len(margins) == 2 and min(margins) > 1e-5, margins
    assert launches_on == (4, 2) and launches_off == (0, 0)
    assert len(errs) == 2 + len(list(pv.parameters())) + 4 and set(on) == set(off) and max(errs.values()) <= BOUND


def test_model_train_step(cuda):
    """The train step of tests/golden/pvcnn.npz with fused_grad on, by the keys
    and the rule of tests/test_gpu_pvcnn.py test_model_step_against_float64_
    reference[train]: max(8 x the reference's float32 error, 1e-4)."""
    from o3dml_amd.pvcnn import PVCNN, PVConv
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pvcnn.npz"))
    m = PVCNN(num_classes=int(z["num_classes"]), width_multiplier=float(z["width_multiplier"]),
              voxel_resolution_multiplier=float(z["voxel_resolution_multiplier"]))
    sd = m.state_dict()
    for k in z["weight_names"]:
        sd[str(k)] = torch.from_numpy(z["w:" + str(k)])
    m.load_state_dict(sd)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = float(z["dropout_p"])
        if isinstance(mod, PVConv):
            mod.fused_grad = True
    m = m.to(cuda).train()
    pts = torch.from_numpy(z["points"]).to(cuda)
    feat = torch.cat([pts, torch.from_numpy(z["extra"]).to(cuda)], 1)
    labels = torch.from_numpy(z["labels"]).to(cuda).reshape(-1)

    def step():
        logits = m({"point": pts, "feat": feat})
        loss = F.cross_entropy(logits.reshape(-1, logits.shape[-1]), labels)
        loss.backward()
        return logits, loss
    (logits, loss), _, wgrads = counted(step)
    p = "pv_train_"
    rel = lambda a, ref: float(np.abs(a.detach().double().cpu().numpy() - ref).max() / np.abs(ref).max())  # noqa: E731
    bound = lambda e32: max(8 * float(e32), 1e-4)  # noqa: E731
    found = {"rows": (rel(logits.reshape(-1, logits.shape[-1])[::int(z["row_step"])], z[p + "f64_logit_rows"]),
                      bound(z[p + "ref32_err_rows"])),
             "loss": (abs(loss.item() - float(z[p + "f64_loss"])) / abs(float(z[p + "f64_loss"])),
                      bound(z[p + "ref32_err_loss"]))}
    params, n64 = dict(m.named_parameters()), z[p + "f64_grad_norms"]
    for k, want, e32 in zip(z[p + "grad_names"], n64, z[p + "ref32_err_norms"]):
        norm = float(params[str(k)].grad.double().norm())
        live = want > 1e-6 * n64.max()
        found["norm:" + str(k)] = (abs(norm - want) / want, bound(e32)) if live else (norm, 1e-5 * n64.max())
    for k in z["full_grad_names"]:
        found["grad:" + str(k)] = (rel(params[str(k)].grad, z[p + "f64_grad:" + str(k)]),
                                   bound(z[p + "ref32_err_grad:" + str(k)]))
    for k, e32 in zip(z[p + "bn_names"], z[p + "ref32_err_bn"]):
        found["bn:" + str(k)] = (rel(m.state_dict()[str(k)], z[p + "f64_bn:" + str(k)]), bound(e32))
    worst = max(found, key=lambda k: found[k][0] / found[k][1])
    print("worst against its bound", worst, found[worst], "wgrad launches", wgrads)
    assert wgrads == 8 and not [k for k, (e, bnd) in found.items() if not e <= bnd]
