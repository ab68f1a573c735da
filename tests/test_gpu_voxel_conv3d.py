"""ops.voxel_conv3d on the GPU against torch.nn.functional.conv3d(padding=1) +
bias + LeakyReLU in float64 on the CPU.  The bound is the project's: largest
absolute difference over largest reference magnitude <= 1e-4; the float32
evaluation on the CPU has to keep it too, so the bound is one float32
arithmetic can meet.  The output buffer is handed in pre-filled with NaN, so an
element the kernel does not write fails the bound."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
BOUND = 1e-4
B = 2  # the batch stride is exercised throughout


def make(r, cin, cout, bias_shift=0.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    grid = torch.randn(B, cin, r, r, r, generator=g)
    grid = grid * (torch.rand(B, 1, r, r, r, generator=g) > 1 / 3)  # empty voxels, as an averaged grid has
    weight = torch.randn(cout, cin, 3, 3, 3, generator=g) / (27 * cin) ** 0.5
    bias = 0.1 * torch.randn(cout, generator=g) + bias_shift
    return grid, weight, bias


def composed(grid, weight, bias, slope, dtype):
    y = F.conv3d(grid.to(dtype), weight.to(dtype), bias.to(dtype), padding=1)
    return y if slope is None else F.leaky_relu(y, slope)


def err(a, ref):
    return float((a.double() - ref).abs().max() / ref.abs().max())


def check(cuda, r, cin, cout, slope=0.1, bias_shift=0.0):
    from o3dml_amd import ops
    args = make(r, cin, cout, bias_shift)
    ref = composed(*args, slope, torch.float64)
    e32 = err(composed(*args, slope, torch.float32), ref)
    assert e32 <= BOUND, e32
    dev = [t.to(cuda) for t in args]
    out = ops.voxel_conv3d(*dev, negative_slope=slope, out=torch.full(ref.shape, float("nan"), device=cuda))
    again = ops.voxel_conv3d(*dev, negative_slope=slope)
    e = err(out.cpu(), ref)
    print(f"r {r} {cin} -> {cout} slope {slope}: {e:.3g} (float32 on the CPU {e32:.3g}), bound {BOUND}")
    assert tuple(out.shape) == tuple(ref.shape) and e <= BOUND
    assert torch.equal(out, again)  # run to run bitwise
    return ref


# below the filter, around the tile edges 16 and 32 (two y rows per tile at 16), the two model resolutions
@pytest.mark.parametrize("r", [1, 2, 3, 5, 16, 17, 32, 33])
def test_resolutions(cuda, r):
    check(cuda, r, 9, 16)


# odd and padded widths, Cin above one chunk of 8 (with a remainder), nine channel tiles; (64, 128) at r = 16
# takes the small box.  All of these have so few boxes at B = 2 that the launch rule ends at one channel tile per
# wave (NC = 1) with the tiles spread over blockIdx.y.
@pytest.mark.parametrize("r, cin, cout", [(5, 1, 1), (5, 9, 64), (5, 64, 64), (5, 67, 33), (5, 130, 130),
                                          (5, 16, 257), (16, 64, 128)])
def test_channels(cuda, r, cin, cout):
    check(cuda, r, cin, cout)


# The kernel instances (ZT, NV, NC) with more than one channel tile per wave, by the launch rule at B = 2 (boxes x
# channel groups >= 256 with the block named): test_resolutions runs (32, 2, 1) at r = 32, (16, 2, 1) at 33,
# (32, 1, 1) at 17 and (16, 1, 1) at 16 and below, so with these all twelve run.
@pytest.mark.parametrize("r, cin, cout", [
    (32, 8, 64),    # (32, 2, 2): 256 boxes of 2 x 4 x 32, 1 group; the model's r = 32 instance
    (32, 8, 130),   # (32, 2, 4): 5 tiles in 2 groups, the last group holds one tile (clamped tiles, not stored)
    (17, 8, 128),   # (32, 1, 2): 162 boxes of 2 x 2 x 32, 2 groups
    (17, 8, 256),   # (32, 1, 4): 162 boxes, 2 groups
    (16, 8, 256),   # (16, 1, 2): 64 boxes of 2 x 4 x 16, 4 groups; the model's r = 16, 64 -> 64 instance
    (16, 8, 512),   # (16, 1, 4): 64 boxes, 4 groups; the model's r = 16, -> 128 instance
    (33, 8, 64),    # (16, 2, 2): 486 boxes of 4 x 4 x 16, 1 group
    (33, 8, 160),   # (16, 2, 4): 5 tiles in 2 groups, the last group holds one tile
])
def test_channel_tiles_per_wave(cuda, r, cin, cout):
    check(cuda, r, cin, cout)


def test_cout_above_the_limit_raises(cuda):
    from o3dml_amd import ops
    grid, weight, bias = [t.to(cuda) for t in make(5, 16, 513)]
    with pytest.raises(RuntimeError, match="513"):
        ops.voxel_conv3d(grid, weight, bias, 0.1)


def test_no_activation(cuda):
    check(cuda, 5, 9, 16, slope=None)


def test_negative_branch(cuda):
    ref = check(cuda, 5, 9, 16, slope=0.1, bias_shift=-2.0)
    assert float((ref < 0).float().mean()) > 0.9


def randomise_bn(module):
    for m in module.modules():
        if isinstance(m, torch.nn.BatchNorm3d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0, 0.1)


def counted(fn):
    """(result of fn(), launches of voxel_conv3d while it ran)"""
    from o3dml_amd import _lib
    lib = _lib.load()
    lib.o3dml_timing_enable(1)
    try:
        lib.o3dml_timing_reset()
        res = fn()
        torch.cuda.synchronize()
        return res, _lib.kernel_times(["voxel_conv3d"])["voxel_conv3d"][1]
    finally:
        lib.o3dml_timing_enable(0)


def test_module_switch(cuda):
    """The same result fused and composed in eval() under no_grad, the kernel's
    timing counter counting the fused launches only; with grad enabled and in
    train() the fused path is not taken."""
    from o3dml_amd.pvcnn import PVConv
    torch.manual_seed(0)
    pv = PVConv(9, 16, 3, resolution=8)
    randomise_bn(pv)
    pv = pv.to(cuda).eval()
    coords, feat = torch.rand(2, 3, 200, device=cuda), torch.randn(2, 9, 200, device=cuda)

    def run():
        return pv((feat, coords))[0]

    res, launches = [], []
    for fused in (True, False):
        pv.fused = fused
        with torch.no_grad():
            out, n = counted(run)
        res.append(out)
        launches.append(n)
    e = err(res[0].cpu(), res[1].cpu().double())
    print("fused against composed", e, "bound", BOUND)
    assert tuple(res[0].shape) == (2, 16, 200) and e <= BOUND and launches == [2, 0]
    pv.fused = True
    assert counted(run)[1] == 0  # grad enabled, the parameters require grad
    pv.train()
    with torch.no_grad():
        assert counted(run)[1] == 0


def test_model_eval_no_grad(cuda):
    """The golden eval logits of tests/golden/pvcnn.npz with every voxel
    convolution on the kernel, within the bound tests/test_gpu_pvcnn.py holds
    the torch path to; one launch per Conv3d of the model (its four PVConv
    blocks have eight)."""
    import os
    from o3dml_amd.pvcnn import PVCNN, PVConv
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pvcnn.npz"))
    m = PVCNN(num_classes=int(z["num_classes"]), width_multiplier=float(z["width_multiplier"]),
              voxel_resolution_multiplier=float(z["voxel_resolution_multiplier"]))
    sd = m.state_dict()
    for k in z["weight_names"]:
        sd[str(k)] = torch.from_numpy(z["w:" + str(k)])
    m.load_state_dict(sd)
    m = m.to(cuda).eval()
    for mod in m.modules():
        if isinstance(mod, PVConv):
            mod.fused = True
    convs = sum(isinstance(mod, torch.nn.Conv3d) for mod in m.modules())
    pts = torch.from_numpy(z["points"]).to(cuda)
    feat = torch.cat([pts, torch.from_numpy(z["extra"]).to(cuda)], 1)
    with torch.no_grad():
        logits, launches = counted(lambda: m({"point": pts, "feat": feat}))
    rows = logits.reshape(-1, logits.shape[-1])[::int(z["row_step"])].cpu().double().numpy()
    ref = z["pv_eval_f64_logit_rows"]
    e = float(np.abs(rows - ref).max() / np.abs(ref).max())
    bound = max(8 * float(z["pv_eval_ref32_err_rows"]), 1e-4)
    print("eval logit rows", e, "bound", bound, "launches", launches)
    assert e <= bound and launches == convs == 8
