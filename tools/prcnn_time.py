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
  frame_forward_ms     the eval() forward (mode "RCNN") plus get_bboxes of the
                       yml's model on one frame of --points points (default
                       16384), weights from tests/golden/prcnn_weights.py;
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
OPS = ["furthest_point_sampling", "ball_query", "three_nn", "three_interpolate", "nms", "roi_pool_indexed"]


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
    run()
    res["frame_forward_ms"] = round(statistics.median(clock(run) for _ in range(args.iters)), 3)
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
