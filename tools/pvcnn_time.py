"""Time the PVCNN point <-> voxel ops (csrc/pvcnn.hip) against the same ops
written as the reference writes them in torch, on the same GPU, and the
default model's train step and eval forward.  Prints one JSON line.

Shapes: B = 8, N = 40,960 with (C = 64, r = 32) and (C = 128, r = 16).  Times
are HIP-event medians in ms.  ``bytes`` is the algorithmic traffic (each input
read once, each output written once) and ``hbm_frac`` = bytes / time over the
nominal 8 TB/s of an MI355X.  The torch rows: avg_voxelize as pvcnn.py:579-619
(one scatter_add_ per channel, then the count), its autograd backward, a
gather devoxelize and an index_add_ devoxelize backward.

``voxel_conv``: ops.voxel_conv3d (csrc/voxel_conv3d.hip) at the five layer
shapes of the default model's voxel branch at B = 8, and at B = 1 for the
r = 16 shapes, against the torch composition on the same tensors (Conv3d +
eval BatchNorm3d + LeakyReLU, MIOpen; warmed up until it has picked its
algorithm), the two alternating in one loop: medians with [min, max].
``kernel_ms`` is the kernel's own time from the library's timing counter
(voxel_conv3d), ``flop`` = 2 * 27 * Cin * Cout * B * r^3 and ``matrix_peak``
= flop / kernel time over the 157.3 TF/s dense f32 matrix rate of one MI355X
(256 CUs x 4 SIMDs x 4096 flop per 64-cycle v_mfma_f32_32x32x2_f32 at
2.4 GHz, the figure tools/prcnn_time.py uses).  ``model.eval_fused`` /
``eval_composed``: the eval forward under no_grad with PVConv.fused on and
off, alternating.

``voxel_conv_grad``: at the same eight shapes, ops.voxel_conv3d_wgrad
(csrc/voxel_conv3d_grad.hip; its kernels' own times from the counters
voxel_conv3d_wgrad and voxel_conv3d_wgrad_reduce, ``wgrad_matrix_peak`` = flop
/ wgrad kernel time over the same 157.3 TF/s) and ops.voxel_conv3d_grad_input
against torch's conv3d backward through autograd (weight, bias and input
gradients in one call, MIOpen), alternating on the same tensors.
``model.train_fused_grad`` / ``train_composed``: the train step with
PVConv.fused_grad on and off, alternating; ``composed_profile``: one off step
under torch.profiler, the device time of the 5-D aten::convolution_backward
calls as a share of the step; ``train_fused_grad_differing``: the parameters
whose gradients differ bitwise between two backward passes from the same state
with fused_grad on (the Conv1d weights, whose gradient is MIOpen's).

    python tools/pvcnn_time.py [--iters 20] [--skip-model] [--skip-ops] [--model-batch 8]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "open3d-ml_amd"))

HBM_BYTES_PER_S = 8.0e12
MFMA_F32_PEAK = 157.3e12  # dense f32 matrix rate of one MI355X


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def row(ms, nbytes=None):
    r = {"ms": round(ms, 4)}
    if nbytes is not None:
        r["bytes"] = int(nbytes)
        r["hbm_frac"] = round(nbytes / (ms * 1e-3) / HBM_BYTES_PER_S, 4)
    return r


def torch_avg_voxelize(feat, coords, r):
    """pvcnn.py:579-619: C + 1 scatter_add_ launches from a Python loop."""
    coords = coords.to(torch.int64)
    B, C = feat.shape[:2]
    grid = torch.zeros((B, C, r, r, r), device=feat.device)
    batch_id = torch.arange(B, device=feat.device).reshape(-1, 1)
    h = (batch_id * r * r * r + coords[:, 0] * r * r + coords[:, 1] * r + coords[:, 2]).reshape(-1)
    for i in range(C):
        grid[:, i] = torch.zeros(B * r ** 3, device=feat.device).scatter_add_(
            0, h, feat[:, i].reshape(-1)).reshape(B, r, r, r)
    count = torch.zeros(B * r ** 3, device=feat.device).scatter_add_(
        0, h, torch.ones_like(feat[:, 0].reshape(-1))).reshape(B, 1, r, r, r).clamp(min=1)
    return grid / count


def torch_devox(feat, inds, wgts):
    """outs[b,c,i] = sum_k wgts[b,k,i] * feat[b,c,inds[b,k,i]] (feat [B,C,r3])."""
    B, C, _ = feat.shape
    N = inds.shape[2]
    idx = inds.long().reshape(B, 1, 8 * N).expand(-1, C, -1)
    return (feat.gather(2, idx).reshape(B, C, 8, N) * wgts[:, None]).sum(2)


def torch_devox_backward(grad, inds, wgts, r3):
    B, C, N = grad.shape
    out = torch.zeros((B, C, r3), device=grad.device)
    src = (grad[:, :, None, :] * wgts[:, None]).reshape(B, C, 8 * N)
    for b in range(B):
        out[b].index_add_(1, inds[b].reshape(-1).long(), src[b])
    return out


def ops_at(B, C, N, r, iters, dev):
    from o3dml_amd import ops
    from o3dml_amd.pvcnn import AvgVoxelization, DevoxelizePlan, VoxelPlan
    g = torch.Generator(device="cpu").manual_seed(0)
    r3 = r ** 3
    coords = (torch.rand((B, 3, N), generator=g) * (r - 1)).to(dev)
    feat = torch.randn((B, C, r3), generator=g).to(dev)
    pfeat = torch.randn((B, C, N), generator=g).to(dev)
    grad = torch.randn((B, C, N), generator=g).to(dev)
    ggrid = torch.randn((B, C, r, r, r), generator=g).to(dev)
    vox = torch.round(coords).to(torch.int32)
    f4 = 4
    out = {}
    outs, inds, wgts = ops.trilinear_devoxelize_forward(r, True, coords, feat)
    io = (B * C * r3 + B * C * N) * f4
    out["devox_forward_train"] = row(timed(lambda: ops.trilinear_devoxelize_forward(r, True, coords, feat), iters),
                                     io + B * N * (12 + 64))
    out["devox_backward"] = row(timed(lambda: ops.trilinear_devoxelize_backward(grad, inds, wgts, r), iters),
                                io + B * N * 64)
    plan = DevoxelizePlan(coords, r)
    plan.inds, plan.wgts = inds, wgts
    lists = plan.backward_lists()
    from o3dml_amd import _lib
    from o3dml_amd._util import ptr, stream_handle
    gf = torch.empty((B, C, r3), device=dev)
    out["devox_backward_lists_built"] = row(timed(lambda: _lib.call(
        "o3dml_trilinear_devoxelize_backward_planned", ptr(grad), ptr(wgts), ptr(lists), B, C, N, r, ptr(gf),
        stream_handle(dev)), iters), io + B * N * 64)
    out["voxel_plan"] = row(timed(lambda: VoxelPlan(vox, r), iters), B * N * 12 + B * r3 * 4)
    vplan = VoxelPlan(vox, r)
    out["avg_voxelize_forward"] = row(timed(lambda: AvgVoxelization.apply(pfeat, vplan), iters), io + B * N * 4)
    pf = pfeat.clone().requires_grad_(True)
    grid = AvgVoxelization.apply(pf, vplan)
    out["avg_voxelize_backward"] = row(timed(lambda: torch.autograd.grad(grid, pf, ggrid, retain_graph=True), iters),
                                       io + B * N * 12)
    # the same ops as the reference writes them in torch
    out["torch_avg_voxelize_forward"] = row(timed(lambda: torch_avg_voxelize(pfeat, vox, r), max(3, iters // 4)))
    tgrid = torch_avg_voxelize(pf, vox, r)
    out["torch_avg_voxelize_backward"] = row(timed(lambda: torch.autograd.grad(tgrid, pf, ggrid, retain_graph=True),
                                                   max(3, iters // 4)))
    out["torch_devox_forward"] = row(timed(lambda: torch_devox(feat, inds, wgts), iters))
    out["torch_devox_backward_index_add"] = row(timed(lambda: torch_devox_backward(grad, inds, wgts, r3), iters))
    ref = torch_devox_backward(grad, inds, wgts, r3)
    mine = ops.trilinear_devoxelize_backward(grad, inds, wgts, r)
    out["check_backward_rel"] = float((mine - ref).abs().max() / ref.abs().max())
    out["check_voxelize_rel"] = float((AvgVoxelization.apply(pfeat, vplan) - torch_avg_voxelize(pfeat, vox, r)
                                       ).abs().max())
    return out


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def spread(times):
    return {"ms": round(statistics.median(times), 4), "min": round(min(times), 4), "max": round(max(times), 4)}


CONV_SHAPES = [(8, 32, 9, 64), (8, 32, 64, 64), (8, 16, 64, 64), (8, 16, 64, 128), (8, 16, 128, 128),
               (1, 16, 64, 64), (1, 16, 64, 128), (1, 16, 128, 128)]  # (B, r, Cin, Cout)


def conv_at(B, r, cin, cout, iters, dev):
    from o3dml_amd import _lib, ops
    from o3dml_amd.point_transformer import fold_bn
    torch.manual_seed(0)
    seq = torch.nn.Sequential(torch.nn.Conv3d(cin, cout, 3, stride=1, padding=1),
                              torch.nn.BatchNorm3d(cout, eps=1e-4), torch.nn.LeakyReLU(0.1, True))
    seq[1].running_mean.normal_(0, 0.1)
    seq[1].running_var.uniform_(0.5, 1.5)
    seq = seq.to(dev).eval()
    grid = torch.randn(B, cin, r, r, r, device=dev) * (torch.rand(B, 1, r, r, r, device=dev) > 1 / 3)
    with torch.no_grad():
        scale, shift = fold_bn(seq[1])
        w = (seq[0].weight * scale.view(-1, 1, 1, 1, 1)).contiguous()
        b = seq[0].bias * scale + shift
        packed = ops.voxel_conv3d_pack(w, b)

        def fused():
            return ops.voxel_conv3d(grid, w, b, 0.1, packed=packed)

        def composed():
            return seq(grid.clone())  # the LeakyReLU is in place, as in the model

        for _ in range(5):
            fused()
            composed()
        ref = composed()
        check = float((fused() - ref).abs().max() / ref.abs().max())
        tf, tc = [], []
        for _ in range(iters):
            tf.append(event_ms(fused))
            tc.append(event_ms(composed))
        clone_ms = statistics.median([event_ms(lambda: grid.clone()) for _ in range(iters)])
        lib = _lib.load()
        lib.o3dml_timing_enable(1)
        try:
            lib.o3dml_timing_reset()
            for _ in range(iters):
                fused()
            torch.cuda.synchronize()
            ms, cnt = _lib.kernel_times(["voxel_conv3d"])["voxel_conv3d"]
        finally:
            lib.o3dml_timing_enable(0)
    flop = 2 * 27 * cin * cout * B * r ** 3
    kernel = ms / cnt
    return {"B": B, "r": r, "cin": cin, "cout": cout, "flop": flop, "fused": spread(tf), "composed": spread(tc),
            "composed_clone_ms": round(clone_ms, 4), "kernel_ms": round(kernel, 4),
            "matrix_peak": round(flop / (kernel * 1e-3) / MFMA_F32_PEAK, 4), "check_rel": check}


def conv_grad_at(B, r, cin, cout, iters, dev):
    """The convolution's backward at one layer shape: ops.voxel_conv3d_wgrad and
    ops.voxel_conv3d_grad_input against torch's conv3d backward through
    autograd (weight, bias and input gradients; MIOpen), alternating."""
    from o3dml_amd import _lib, ops
    torch.manual_seed(0)
    grid = torch.randn(B, cin, r, r, r, device=dev) * (torch.rand(B, 1, r, r, r, device=dev) > 1 / 3)
    gout = torch.randn(B, cout, r, r, r, device=dev)
    w = (torch.randn(cout, cin, 3, 3, 3, device=dev) / (27 * cin) ** 0.5).requires_grad_()
    b = torch.zeros(cout, device=dev, requires_grad=True)
    gin = grid.clone().requires_grad_()
    packed_t = ops.voxel_conv3d_pack(w.detach().flip(2, 3, 4).transpose(0, 1).contiguous())
    y = torch.nn.functional.conv3d(gin, w, b, padding=1)

    def wgrad():
        return ops.voxel_conv3d_wgrad(grid, gout)

    def dgrad():
        return ops.voxel_conv3d_grad_input(gout, w, packed=packed_t)

    def miopen():
        return torch.autograd.grad(y, (gin, w, b), gout, retain_graph=True)

    for _ in range(5):
        wgrad(), dgrad(), miopen()
    ref = miopen()
    rel = lambda a, c: float((a - c).abs().max() / c.abs().max())  # noqa: E731
    check = {"dx": rel(dgrad(), ref[0]), "dw": rel(wgrad()[0], ref[1]), "db": rel(wgrad()[1], ref[2])}
    tw, td, tm = [], [], []
    for _ in range(iters):
        tw.append(event_ms(wgrad))
        td.append(event_ms(dgrad))
        tm.append(event_ms(miopen))
    names = ["voxel_conv3d_wgrad", "voxel_conv3d_wgrad_reduce"]
    lib = _lib.load()
    lib.o3dml_timing_enable(1)
    try:
        lib.o3dml_timing_reset()
        for _ in range(iters):
            wgrad()
        torch.cuda.synchronize()
        kt = _lib.kernel_times(names)
    finally:
        lib.o3dml_timing_enable(0)
    flop = 2 * 27 * cin * cout * B * r ** 3
    kernel = kt[names[0]][0] / kt[names[0]][1]
    return {"B": B, "r": r, "cin": cin, "cout": cout, "flop": flop, "wgrad": spread(tw), "dgrad": spread(td),
            "torch_backward": spread(tm), "wgrad_kernel_ms": round(kernel, 4),
            "wgrad_reduce_kernel_ms": round(kt[names[1]][0] / kt[names[1]][1], 4),
            "wgrad_matrix_peak": round(flop / (kernel * 1e-3) / MFMA_F32_PEAK, 4), "check_rel": check}


def model_train_switch(m, train, iters):
    """The train step with PVConv.fused_grad on and off, alternating, and the
    off step's time inside convolution backward (torch.profiler, the device
    time of the 5-D aten::convolution_backward calls over the step's median)."""
    from o3dml_amd.pvcnn import PVConv
    from torch.profiler import ProfilerActivity, profile
    blocks = [b for b in m.modules() if isinstance(b, PVConv)]
    times = {True: [], False: []}
    for on in (True, False) * 2:
        for b in blocks:
            b.fused_grad = on
        train()
    for _ in range(iters):
        for on in (True, False):
            for b in blocks:
                b.fused_grad = on
            times[on].append(event_ms(train))
    # two backward passes from the same state with fused_grad on: the parameters whose gradients differ bitwise
    for b in blocks:
        b.fused_grad = True
    grads = []
    for _ in range(2):
        torch.manual_seed(1)  # the Dropout masks
        train(step=False)
        grads.append({k: p.grad.clone() for k, p in m.named_parameters()})
    for b in blocks:
        b.fused_grad = False
    res = {"train_fused_grad": spread(times[True]), "train_composed": spread(times[False]),
           "train_fused_grad_differing": [k for k in grads[0] if not torch.equal(grads[0][k], grads[1][k])]}
    try:  # the off step under the profiler, last: a profiler that fails to start costs only this field
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA], record_shapes=True) as prof:
            train()
            torch.cuda.synchronize()
        events = prof.key_averages(group_by_input_shape=True)
        dev_time = lambda e: getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0)  # noqa: E731
        conv3d = lambda e, key: e.key == key and e.input_shapes and len(e.input_shapes[0]) == 5  # noqa: E731
        conv_bwd = sum(dev_time(e) for e in events if conv3d(e, "aten::convolution_backward")) * 1e-3
        conv_fwd = sum(dev_time(e) for e in events if conv3d(e, "aten::convolution")) * 1e-3
        res["composed_profile"] = {"conv3d_backward_ms": round(conv_bwd, 3), "conv3d_forward_ms": round(conv_fwd, 3),
                                   "conv3d_backward_share_of_step": round(conv_bwd / res["train_composed"]["ms"], 4)}
    except Exception as e:  # noqa: BLE001
        res["composed_profile"] = {"error": repr(e)}
        print(f"pvcnn_time: no profile of the composed step, conv3d_backward_share_of_step is missing: {e!r}",
              file=sys.stderr)
    return res


def model_eval_switch(m, run, iters):
    from o3dml_amd.pvcnn import PVConv
    blocks = [b for b in m.modules() if isinstance(b, PVConv)]
    times = {True: [], False: []}
    for fused in (True, False) * 2:  # warm-up of both settings
        for b in blocks:
            b.fused = fused
        run()
    for _ in range(iters):
        for fused in (True, False):
            for b in blocks:
                b.fused = fused
            times[fused].append(event_ms(run))
    for b in blocks:
        b.fused = True
    return {"eval_fused": spread(times[True]), "eval_composed": spread(times[False])}


def model_times(B, N, iters, dev):
    from o3dml_amd.pvcnn import PVCNN
    torch.manual_seed(0)
    m = PVCNN().to(dev)
    pts = torch.rand((B, 3, N), device=dev) * torch.tensor([4, 3, 2.5], device=dev)[None, :, None]
    feat = torch.cat([pts, torch.rand((B, 6, N), device=dev)], 1)
    labels = torch.randint(0, 13, (B * N,), device=dev)
    opt = torch.optim.Adam(m.parameters(), 1e-3)

    def train(step=True):
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.cross_entropy(m({"point": pts, "feat": feat}).reshape(-1, 13), labels)
        loss.backward()
        if step:
            opt.step()

    def evaluate():
        with torch.no_grad():
            m({"point": pts, "feat": feat})

    m.train()
    t_train = timed(train, iters, warmup=2)
    switch = model_train_switch(m, train, max(iters, 5))
    m.eval()
    res = {"batch": B, "points": N, "train_step": row(t_train), "eval_forward": row(timed(evaluate, iters, warmup=2))}
    res.update(switch)
    res.update(model_eval_switch(m, evaluate, max(iters, 10)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--skip-ops", action="store_true", help="leave out the point <-> voxel op rows")
    ap.add_argument("--model-batch", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pvcnn_time: no ROCm GPU is visible")
    dev = torch.device("cuda", 0)
    res = {"tool": "pvcnn_time", "device": torch.cuda.get_device_name(0), "iters": args.iters, "B": 8, "N": 40960}
    if not args.skip_ops:
        res["C64_r32"] = ops_at(8, 64, 40960, 32, args.iters, dev)
        res["C128_r16"] = ops_at(8, 128, 40960, 16, args.iters, dev)
    res["voxel_conv"] = [conv_at(*shape, args.iters, dev) for shape in CONV_SHAPES]
    res["voxel_conv_grad"] = [conv_grad_at(*shape, args.iters, dev) for shape in CONV_SHAPES]
    if not args.skip_model:
        res["model"] = model_times(args.model_batch, 40960, max(3, args.iters // 4), dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
