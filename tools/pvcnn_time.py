"""Time the PVCNN point <-> voxel ops (csrc/pvcnn.hip) against the same ops
written as the reference writes them in torch, on the same GPU, and the
default model's train step and eval forward.  Prints one JSON line.

Shapes: B = 8, N = 40,960 with (C = 64, r = 32) and (C = 128, r = 16).  Times
are HIP-event medians in ms.  ``bytes`` is the algorithmic traffic (each input
read once, each output written once) and ``hbm_frac`` = bytes / time over the
nominal 8 TB/s of an MI355X.  The torch rows: avg_voxelize as pvcnn.py:579-619
(one scatter_add_ per channel, then the count), its autograd backward, a
gather devoxelize and an index_add_ devoxelize backward.

    python tools/pvcnn_time.py [--iters 20] [--skip-model] [--model-batch 8]
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


def model_times(B, N, iters, dev):
    from o3dml_amd.pvcnn import PVCNN
    torch.manual_seed(0)
    m = PVCNN().to(dev)
    pts = torch.rand((B, 3, N), device=dev) * torch.tensor([4, 3, 2.5], device=dev)[None, :, None]
    feat = torch.cat([pts, torch.rand((B, 6, N), device=dev)], 1)
    labels = torch.randint(0, 13, (B * N,), device=dev)
    opt = torch.optim.Adam(m.parameters(), 1e-3)

    def train():
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.cross_entropy(m({"point": pts, "feat": feat}).reshape(-1, 13), labels)
        loss.backward()
        opt.step()

    def evaluate():
        with torch.no_grad():
            m({"point": pts, "feat": feat})

    m.train()
    t_train = timed(train, iters, warmup=2)
    m.eval()
    return {"batch": B, "points": N, "train_step": row(t_train), "eval_forward": row(timed(evaluate, iters, warmup=2))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--model-batch", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pvcnn_time: no ROCm GPU is visible")
    dev = torch.device("cuda", 0)
    res = {"tool": "pvcnn_time", "device": torch.cuda.get_device_name(0), "iters": args.iters, "B": 8, "N": 40960}
    res["C64_r32"] = ops_at(8, 64, 40960, 32, args.iters, dev)
    res["C128_r16"] = ops_at(8, 128, 40960, 16, args.iters, dev)
    if not args.skip_model:
        res["model"] = model_times(args.model_batch, 40960, max(3, args.iters // 4), dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
