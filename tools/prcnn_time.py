"""Time PointRCNN inference.  Prints one JSON line, times in ms (host clock
around work that ends in a device synchronise; medians over --iters after a
warm-up of every shape):

  roi_pool             ops.roi_pool at the shape of ml3d/configs/
                       pointrcnn_kitti.yml (B = 1, N = 16384, M = 100, S = 512,
                       C = 130) on a synthetic frame, beside the same pooling
                       composed from torch ops on the same GPU (membership mask,
                       a sort for the ordered first S, gathers), alternating;
                       whether both give the same rows; the op's algorithmic
                       bytes (the pooled rows written, the cloud and its
                       features read once) over its time, as GB/s and as a
                       fraction of the 8 TB/s HBM peak;
  sa_levels            ops.sa_mlp_max at the eleven level / scale shapes of the
                       yml (RPN: one cloud of 16384 points; RCNN: 100 rois of
                       512 points), index from this library's FPS and ball
                       query, beside the composition it replaces on the same
                       index (row gather, folded Linears + ReLU, max),
                       alternating after a warm-up of each; the kernel's own
                       time (timing counter sa_mlp_max); FLOPs and algorithmic
                       bytes (cloud, index, centres, weights read once, the
                       output written) from the shape, and the least time the
                       hardware could take (FLOPs over the 157.3 TF/s f32
                       matrix peak or bytes over the 8 TB/s HBM peak,
                       whichever is larger and named in `bound`) over the
                       kernel time;
  fp_modules           ops.fp_mlp at the four feature-propagation shapes of the
                       yml's RPN backbone (B = 1; dist2 and idx from this
                       library's three_nn, not timed), beside the composition
                       it replaces (weights from dist2, three_interpolate on
                       the transposed features, concatenate, folded Linears +
                       ReLU), alternating after a warm-up of each; the kernel's
                       own time (timing counter fp_mlp); FLOPs of the layers
                       over the f32 matrix peak against the kernel time;
  frame_forward_ms     the eval() forward (mode "RCNN") plus get_bboxes of the
                       yml's model on one frame of --points points (default
                       16384), weights from tests/golden/prcnn_weights.py, with
                       the fused set abstraction and feature propagation;
                       frame_forward_composed_ms the same with every level's
                       `fused` flag off, frame_forward_fp_composed_ms with
                       only the feature-propagation modules' flags off, the
                       three alternating in one loop, each with its [min, max];
  frame_ops_ms         per forward, the time inside this library's ops (each
                       call bracketed by device synchronises, so the sum is an
                       upper bound of their share) and the calls.

The composition is the comparison: the reference's own roi_pool is a native
Open3D op that is not available here.

    python tools/prcnn_time.py [--iters 10] [--points 16384]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "open3d-ml_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

HBM_PEAK = 8.0e12
MFMA_F32_PEAK = 157.3e12  # dense f32 matrix rate of one MI355X
OPS = ["furthest_point_sampling", "ball_query", "three_nn", "three_interpolate", "fp_mlp", "sa_mlp_max", "nms",
       "roi_pool_indexed"]


def clock(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def composed_roi_pool(xyz, boxes, feat, S):
    """The roi_pool contract on torch ops: -> (pooled, flag, idx)."""
    B, N, _ = xyz.shape
    hh, hw, hl = boxes[..., 3:4] * 0.5, boxes[..., 4:5] * 0.5, boxes[..., 5:6] * 0.5
    dx = xyz[:, None, :, 0] - boxes[..., 0:1]
    dy = xyz[:, None, :, 1] - (boxes[..., 1:2] - hh)
    dz = xyz[:, None, :, 2] - boxes[..., 2:3]
    cs, sn = torch.cos(boxes[..., 6:7]), torch.sin(boxes[..., 6:7])
    xr, zr = dx * cs - dz * sn, dx * sn + dz * cs
    mask = ((dx.abs() <= 10) & (dy.abs() <= hh) & (dz.abs() <= 10) & (xr >= -hl) & (xr <= hl) & (zr >= -hw) &
            (zr <= hw))  # [B, M, N]
    cnt = mask.sum(-1, keepdim=True)
    ar = torch.arange(N, device=xyz.device)
    first = torch.where(mask, ar, N).sort(dim=-1).values[..., :S]  # members ascending, then N
    if first.shape[-1] < S:
        first = torch.nn.functional.pad(first, (0, S - first.shape[-1]), value=N)
    slot = torch.arange(S, device=xyz.device).expand_as(first)
    slot = torch.where(cnt >= S, slot, slot % cnt.clamp(min=1))
    idx = first.gather(-1, slot).clamp(max=N - 1)
    rows = torch.cat([xyz, feat], dim=2)
    pooled = torch.stack([rows[b][idx[b]] for b in range(B)]) * (cnt > 0).unsqueeze(-1)
    return pooled, (cnt.squeeze(-1) == 0).int(), torch.where(cnt > 0, idx, -1).int()


def sa_levels(cfg, dev, rng, iters):
    """One entry per level and scale of the yml's RPN backbone and RCNN head."""
    from o3dml_amd import _lib, ops, point_rcnn
    import torch.nn as nn
    shapes = []
    sa = cfg["rpn"]["backbone"]["SA_config"]
    n_in, c_in = 16384, cfg["rpn"]["backbone"]["in_channels"]
    for k, m in enumerate([4096, 1024, 256, 64]):
        for radius, S, mlp in zip(sa["radius"][k], sa["nsample"][k], sa["mlps"][k]):
            shapes.append((f"rpn{k + 1}_r{radius}", 1, n_in, m, S, c_in, radius, list(mlp), True))
        n_in, c_in = m, sum(mlp[-1] for mlp in sa["mlps"][k])
    sa = cfg["rcnn"]["SA_config"]
    n_in, c_in = 512, cfg["rcnn"]["in_channels"]
    for k, m in enumerate(sa["npoints"]):
        shapes.append((f"rcnn{k + 1}", 100, n_in, m, sa["nsample"][k], c_in, sa["radius"][k], list(sa["mlps"][k]),
                       False))
        n_in, c_in = m, sa["mlps"][k][-1]
    lib = _lib.load()
    out = []
    for name, B, N, M, S, C, radius, mlp, bn in shapes:
        widths = [C + 3] + mlp
        if B == 1:
            xyz = torch.from_numpy(frame(16384, rng)[None, :N].copy()).to(dev)
        else:  # a roi's points in its canonical frame
            xyz = torch.from_numpy(((rng.random((B, N, 3)) - 0.5) * [4.0, 2.0, 6.0]).astype(np.float32)).to(dev)
        feat = torch.from_numpy(rng.standard_normal((B, N, C)).astype(np.float32)).to(dev) if C else None
        seq = point_rcnn.gen_CNN(widths, conv=nn.Conv2d, batch_norm=nn.BatchNorm2d if bn else None,
                                 bias=not bn).to(dev).eval()
        with torch.no_grad():
            if M == -1:  # GroupAll
                M, S, new_xyz, idx = 1, N, None, None
                rows = torch.arange(B * N, device=dev)
            else:
                fps = ops.furthest_point_sampling(xyz, M)
                new_xyz = torch.gather(xyz, 1, fps.long().unsqueeze(2).expand(-1, -1, 3))
                idx = ops.ball_query(xyz, new_xyz, radius, S)
                rows = (idx.long() + (torch.arange(B, device=dev) * N).view(B, 1, 1)).view(-1)
            weights, biases = point_rcnn.fused_chain(seq)
            packed = ops.sa_mlp_pack(weights, biases)

            def fused():
                return ops.sa_mlp_max(xyz, new_xyz, feat, idx, weights, biases, packed=packed)

            def composed():
                g = xyz.reshape(B * N, 3)[rows].view(B, M, S, 3)
                if new_xyz is not None:
                    g = g - new_xyz.unsqueeze(2)
                if feat is not None:
                    g = torch.cat([g, feat.reshape(B * N, C)[rows].view(B, M, S, C)], dim=3)
                return point_rcnn.run_channels_last(seq, g).max(dim=2).values

            a, b = fused(), composed()
            err = float((a - b).abs().max() / b.abs().max())
            fused(), composed()
            tf, tc = [], []
            for _ in range(iters):
                tf.append(clock(fused))
                tc.append(clock(composed))
            lib.o3dml_timing_enable(1)
            lib.o3dml_timing_reset()
            for _ in range(iters):
                fused()
            torch.cuda.synchronize()
            ms, cnt = _lib.kernel_times(["sa_mlp_max"])["sa_mlp_max"]
            lib.o3dml_timing_enable(0)
        kernel_ms = ms / max(cnt, 1)
        flops = 2 * B * M * S * sum(i * o for i, o in zip(widths[:-1], widths[1:]))
        nbytes = 4 * (B * N * (3 + C) + (0 if idx is None else B * M * S + 3 * B * M) + packed.numel() +
                      B * M * widths[-1])
        t_flop, t_byte = flops / MFMA_F32_PEAK, nbytes / HBM_PEAK
        out.append({"level": name, "shape": [B, N, M, S], "widths": widths,
                    "fused_ms": round(statistics.median(tf), 4), "kernel_ms": round(kernel_ms, 4),
                    "composed_ms": round(statistics.median(tc), 4), "max_rel_diff": err, "flops": flops,
                    "algorithmic_bytes": nbytes, "bound": "matrix" if t_flop >= t_byte else "hbm",
                    "fraction_of_matrix_peak": round(t_flop / (kernel_ms * 1e-3), 4),
                    "fraction_of_hbm_peak": round(t_byte / (kernel_ms * 1e-3), 4)})
    return out


def fp_modules(cfg, dev, rng, iters):
    """One entry per feature-propagation module of the yml's RPN backbone."""
    from o3dml_amd import _lib, ops, point_rcnn
    import torch.nn as nn
    bb = cfg["rpn"]["backbone"]
    npts = [16384, 4096, 1024, 256, 64]
    skip = [bb["in_channels"]] + [sum(m[-1] for m in mlps) for mlps in bb["SA_config"]["mlps"]]
    fp = [list(m) for m in bb["fp_mlps"]]
    lib = _lib.load()
    out = []
    for k in range(len(fp)):
        n, m, C1 = npts[k], npts[k + 1], skip[k]
        C2 = fp[k + 1][-1] if k + 1 < len(fp) else skip[-1]
        widths = [C2 + C1] + fp[k]
        cloud = torch.from_numpy(frame(16384, rng)[None]).to(dev)
        unknown, known = cloud[:, :n].contiguous(), cloud[:, :m].contiguous()
        kf = torch.from_numpy(rng.standard_normal((1, m, C2)).astype(np.float32)).to(dev)
        uf = torch.from_numpy(rng.standard_normal((1, n, C1)).astype(np.float32)).to(dev) if C1 else None
        seq = point_rcnn.gen_CNN(widths, conv=nn.Conv2d, batch_norm=nn.BatchNorm2d, bias=False).to(dev).eval()
        with torch.no_grad():
            dist2, idx = ops.three_nn(unknown, known)
            weights, biases = point_rcnn.fused_chain(seq, ops.FP_MLP_IN)
            packed = ops.sa_mlp_pack(weights, biases, ops.FP_MLP_IN, "fp_mlp")

            def fused():
                return ops.fp_mlp(uf, kf, dist2, idx, weights, biases, packed=packed)

            def composed():
                recip = 1.0 / (torch.sqrt(dist2) + 1e-8)
                weight = recip / torch.sum(recip, dim=2, keepdim=True)
                h = ops.three_interpolate(kf.transpose(1, 2).contiguous(), idx, weight).transpose(1, 2)
                return point_rcnn.run_channels_last(seq, h if uf is None else torch.cat([h, uf], dim=2))

            a, b = fused(), composed()
            err = float((a - b).abs().max() / b.abs().max())
            fused(), composed()
            tf, tc = [], []
            for _ in range(iters):
                tf.append(clock(fused))
                tc.append(clock(composed))
            lib.o3dml_timing_enable(1)
            lib.o3dml_timing_reset()
            for _ in range(iters):
                fused()
            torch.cuda.synchronize()
            ms, cnt = _lib.kernel_times(["fp_mlp"])["fp_mlp"]
            lib.o3dml_timing_enable(0)
        kernel_ms = ms / max(cnt, 1)
        flops = 2 * n * sum(i * o for i, o in zip(widths[:-1], widths[1:]))
        out.append({"module": f"fp{k + 1}", "shape": [1, n, m, C2, C1], "widths": widths,
                    "fused_ms": round(statistics.median(tf), 4), "kernel_ms": round(kernel_ms, 4),
                    "composed_ms": round(statistics.median(tc), 4), "max_rel_diff": err, "flops": flops,
                    "fraction_of_matrix_peak": round(flops / MFMA_F32_PEAK / (kernel_ms * 1e-3), 4)})
    return out


def frame(points, rng):
    """A synthetic camera-frame cloud: ground clutter over 40 x 70 m and 20
    car-sized blobs holding half of the points."""
    blobs = points // 40
    parts = [rng.random((points - 20 * blobs, 3)) * [40, 3, 68] + [-20, -1, 2]]
    for _ in range(20):
        c = rng.random(3) * [36, 0.5, 60] + [-18, 0.8, 5]
        parts.append(c + (rng.random((blobs, 3)) - 0.5) * [3.6, 1.5, 1.8])
    pts = np.concatenate(parts)
    return pts[rng.permutation(len(pts))].astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--points", type=int, default=16384)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prcnn_time: no ROCm GPU is visible")
    import prcnn_weights
    from o3dml_amd import ops, point_rcnn
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    res = {"tool": "prcnn_time", "device": torch.cuda.get_device_name(0), "iters": args.iters, "points": args.points}

    # ---- the op at the yml shape
    B, N, M, S, C = 1, 16384, 100, 512, 130
    pts = frame(N, rng)
    xyz = torch.from_numpy(pts[None]).to(dev)
    feat = torch.from_numpy(rng.standard_normal((B, N, C)).astype(np.float32)).to(dev)
    centre = pts[rng.choice(N, M, replace=False)] + rng.standard_normal((M, 3)) * [1.0, 0.1, 1.0]
    boxes = np.concatenate([centre[:, :1], centre[:, 1:2] + 1.8, centre[:, 2:3],
                            np.tile([3.5, 3.6, 5.9], (M, 1)) * (1 + 0.1 * rng.standard_normal((M, 3))),
                            rng.random((M, 1)) * 2 * np.pi - np.pi], axis=1).astype(np.float32)
    boxes = torch.from_numpy(boxes[None]).to(dev)
    with torch.no_grad():
        a, b = ops.roi_pool_indexed(xyz, boxes, feat, S), composed_roi_pool(xyz, boxes, feat, S)
        same = bool(torch.equal(a[2], b[2]) and torch.equal(a[1], b[1]) and torch.equal(a[0], b[0]))
        cnt = [(len(torch.unique(i[i >= 0]))) for i in a[2][0]]
        fused = lambda: ops.roi_pool(xyz, boxes, feat, S)  # noqa: E731
        composed = lambda: composed_roi_pool(xyz, boxes, feat, S)  # noqa: E731
        fused(), composed()
        tf, tc = [], []
        for _ in range(args.iters):
            tf.append(clock(fused))
            tc.append(clock(composed))
    lib_ms = _kernel_ms(fused, args.iters)
    nbytes = B * M * S * (3 + C) * 4 + B * N * (3 + C) * 4 + B * M * (7 + 1) * 4
    res["roi_pool"] = {"shape": [B, N, M, S, C], "op_ms": round(statistics.median(tf), 4),
                       "kernel_ms": lib_ms, "composed_torch_ms": round(statistics.median(tc), 3),
                       "same_result": same, "boxes_empty_partial_full": [sum(c == 0 for c in cnt),
                                                                         sum(0 < c < S for c in cnt),
                                                                         sum(c >= S for c in cnt)],
                       "algorithmic_bytes": nbytes, "kernel_GBps": round(nbytes / (lib_ms * 1e-3) / 1e9, 1),
                       "fraction_of_hbm_peak": round(nbytes / (lib_ms * 1e-3) / HBM_PEAK, 4)}

    # ---- the model on one frame
    # the yml's configuration: the fixture's, with the sizes the fixture shrinks put back
    cfg = json.loads(str(np.load(os.path.join(ROOT, "tests", "golden", "point_rcnn.npz"))["config"]))
    cfg = {k: cfg[k] for k in ("classes", "score_thres", "rpn", "rcnn")}
    cfg["rpn"]["backbone"]["SA_config"]["npoints"] = [4096, 1024, 256, 64]
    cfg["rpn"]["head"].update(nms_pre=9000, nms_post_val=100)
    model = point_rcnn.PointRCNN(npoints=args.points, **cfg)
    model.load_state_dict(prcnn_weights.state_dict_for(model), strict=True)
    model = model.to(dev).eval()
    cloud = torch.from_numpy(frame(args.points, rng)[None]).to(dev)
    run = lambda: model.get_bboxes(model(cloud))  # noqa: E731
    res["sa_levels"] = sa_levels(cfg, dev, rng, args.iters)
    res["fp_modules"] = fp_modules(cfg, dev, rng, args.iters)
    levels = [m for m in model.modules() if isinstance(m, point_rcnn.PointnetSAModuleMSG)]
    props = [m for m in model.modules() if isinstance(m, point_rcnn.PointnetFPModule)]

    def switch(on):  # True: all fused; False: all composed; "fp": only the feature propagation composed
        for m in levels:
            m.fused = bool(on)
        for m in props:
            m.fused = on is True

    times = {True: [], False: [], "fp": []}
    for on in times:
        switch(on)
        run()
    for _ in range(args.iters):
        for on in times:
            switch(on)
            times[on].append(clock(run))
    switch(True)
    for on, key in ((True, "frame_forward_ms"), (False, "frame_forward_composed_ms"),
                    ("fp", "frame_forward_fp_composed_ms")):
        res[key] = round(statistics.median(times[on]), 3)
        res[key.replace("_ms", "_min_max_ms")] = [round(min(times[on]), 3), round(max(times[on]), 3)]
    spent = {k: [0.0, 0] for k in OPS}
    real = {k: getattr(ops, k) for k in OPS}

    def wrap(name):
        def f(*a, **kw):
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = real[name](*a, **kw)
            torch.cuda.synchronize()
            spent[name][0] += (time.perf_counter() - t) * 1e3
            spent[name][1] += 1
            return out
        return f

    try:
        for k in OPS:
            setattr(ops, k, wrap(k))
        total = statistics.median(clock(run) for _ in range(args.iters))
    finally:
        for k in OPS:
            setattr(ops, k, real[k])
    res["frame_ops_ms"] = {k: [round(ms / args.iters, 3), n // args.iters] for k, (ms, n) in spent.items()}
    res["frame_forward_synchronised_ms"] = round(total, 3)
    print(json.dumps(res))


def _kernel_ms(fn, iters):
    """The roi_pool kernel's own time per call (HIP events around the launch)."""
    from o3dml_amd import _lib
    lib = _lib.load()
    lib.o3dml_timing_enable(1)
    lib.o3dml_timing_reset()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    ms, cnt = _lib.kernel_times(["roi_pool"])["roi_pool"]
    lib.o3dml_timing_enable(0)
    return round(ms / max(cnt, 1), 4)


if __name__ == "__main__":
    main()
