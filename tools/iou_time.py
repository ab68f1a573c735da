"""Time detection evaluation on a KITTI-val-shaped synthetic set: 3,769 frames
of about 50 predictions x 12 targets (seeded; predictions are jittered copies
of the targets plus clutter, three classes, difficulties 0-2).  Prints one
JSON line, times in ms (host clock around work that ends in the device-to-host
copy; medians over --iters):

  (a) per_frame_loop   the reference-style loop, one iou_bev_cuda and one
                       iou_3d_cuda call per frame (metrics/mAP.py:85-89);
  (b) batched          one iou_bev_batch and one iou_3d_batch call;
  (c) map_*            o3dml_amd.metrics.mAP end to end (GPU overlaps), with
                       its split into filtering, overlaps and host matching,
                       and the same with the host IoU routine;
  kernel_*             the box_iou kernel alone (HIP events around the launch,
                       o3dml_timing), and pairs per second.
(a) and (b) are also checked to be bit-identical.

    python tools/iou_time.py [--iters 5] [--frames 3769]
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

SIZES = {0: (0.6, 1.7, 0.8), 1: (0.6, 1.7, 1.8), 2: (1.6, 1.5, 3.9)}  # w, h, l
BEV = [0, 2, 3, 5, 6]


def make_set(frames, seed=0):
    rng = np.random.default_rng(seed)
    pred, target = [], []
    for _ in range(frames):
        nt = int(rng.integers(6, 19))
        tl = rng.choice([0, 1, 2, 2], size=nt)
        tb = np.zeros((nt, 7), np.float32)
        tb[:, 0], tb[:, 1], tb[:, 2] = rng.uniform(-30, 30, nt), rng.uniform(1.2, 2.0, nt), rng.uniform(5, 65, nt)
        tb[:, 3:6] = np.asarray([SIZES[c] for c in tl]) * rng.uniform(0.85, 1.15, (nt, 3))
        tb[:, 6] = rng.uniform(-np.pi, np.pi, nt)
        td = rng.choice([0, 1, 2], size=nt)
        hit = rng.random(nt) < 0.85
        pb = tb[hit].copy()
        pb[:, [0, 2]] += rng.normal(0, 0.15, (len(pb), 2)).astype(np.float32)
        pb[:, 6] += rng.normal(0, 0.08, len(pb)).astype(np.float32)
        nc = max(0, int(rng.integers(40, 61)) - len(pb))
        cl = rng.choice([0, 1, 2], size=nc)
        cb = np.zeros((nc, 7), np.float32)
        cb[:, 0], cb[:, 1], cb[:, 2] = rng.uniform(-30, 30, nc), rng.uniform(1.2, 2.0, nc), rng.uniform(5, 65, nc)
        cb[:, 3:6] = np.asarray([SIZES[c] for c in cl]).reshape(nc, 3) * rng.uniform(0.85, 1.15, (nc, 3))
        cb[:, 6] = rng.uniform(-np.pi, np.pi, nc)
        pred.append({"bbox": np.concatenate([pb, cb]), "label": np.concatenate([tl[hit], cl]),
                     "score": rng.uniform(0.05, 1.0, len(pb) + nc).astype(np.float32),
                     "difficulty": np.concatenate([td[hit], rng.choice([0, 1, 2], size=nc)])})
        target.append({"bbox": tb, "label": tl, "difficulty": td})
    return pred, target


def timed(fn, iters):
    fn()  # warm-up
    times = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    return round(statistics.median(times), 3), round(min(times), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--frames", type=int, default=3769)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("iou_time: no ROCm GPU is visible")
    from o3dml_amd import _lib, contrib, metrics
    pred, target = make_set(args.frames)
    a = [p["bbox"] for p in pred]
    b = [t["bbox"] for t in target]
    a_rs = np.concatenate([[0], np.cumsum([len(x) for x in a])])
    b_rs = np.concatenate([[0], np.cumsum([len(x) for x in b])])
    A, B = np.concatenate(a), np.concatenate(b)
    A5, B5 = np.ascontiguousarray(A[:, BEV]), np.ascontiguousarray(B[:, BEV])
    pairs = int(np.sum(np.diff(a_rs) * np.diff(b_rs)))
    res = {"tool": "iou_time", "device": torch.cuda.get_device_name(0), "iters": args.iters, "frames": args.frames,
           "pairs_per_mode": pairs, "mean_pred": round(len(A) / args.frames, 1),
           "mean_target": round(len(B) / args.frames, 1)}

    def loop():
        return [(contrib.iou_bev_cuda(x[:, BEV], y[:, BEV]), contrib.iou_3d_cuda(x, y)) for x, y in zip(a, b)]

    def batched():
        return contrib.iou_bev_batch(A5, a_rs, B5, b_rs), contrib.iou_3d_batch(A, a_rs, B, b_rs)

    per_frame, (bev_b, i3d_b) = loop(), batched()
    res["loop_equals_batched"] = all(x.tobytes() == p[0].tobytes() and y.tobytes() == p[1].tobytes()
                                     for x, y, p in zip(bev_b, i3d_b, per_frame))
    res["per_frame_loop_ms"], res["per_frame_loop_min_ms"] = timed(loop, max(2, args.iters // 2))
    res["batched_ms"], res["batched_min_ms"] = timed(batched, args.iters)

    lib = _lib.load()
    lib.o3dml_timing_enable(1)
    lib.o3dml_timing_reset()
    for _ in range(args.iters):
        batched()
    ms, cnt = _lib.kernel_times(["box_iou"])["box_iou"]
    lib.o3dml_timing_enable(0)
    res["kernel_ms_mean_of_bev_and_3d"] = round(ms / max(cnt, 1), 4)
    res["kernel_launches_timed"] = cnt
    res["kernel_pairs_per_s"] = round(pairs / (ms / max(cnt, 1) * 1e-3)) if ms > 0 else None

    kw = dict(classes=[0, 1, 2], difficulties=[0, 1, 2], min_overlap=[0.5, 0.5, 0.7])
    for bev in (True, False):
        tag = "bev" if bev else "3d"
        res[f"map_{tag}_ms"], res[f"map_{tag}_min_ms"] = timed(lambda: metrics.mAP(pred, target, bev=bev, **kw),
                                                              max(2, args.iters // 2))
    # where mAP's time goes (bev): the three steps timed apart
    t0 = time.perf_counter()
    frames = [metrics._prefilter(p, t, kw["classes"], {}) for p, t in zip(pred, target)]
    t1 = time.perf_counter()
    ov = metrics._overlaps(frames, True)
    t2 = time.perf_counter()
    for (p, t), o in zip(frames, ov):
        metrics._frame_rows(p, t, o, kw["classes"], kw["difficulties"], kw["min_overlap"], {})
    t3 = time.perf_counter()
    res["map_bev_split_ms"] = {"filter": round((t1 - t0) * 1e3, 1), "overlaps_gpu": round((t2 - t1) * 1e3, 1),
                               "matching_host": round((t3 - t2) * 1e3, 1)}
    gpu = metrics.mAP(pred, target, bev=True, **kw)
    metrics._use_gpu = lambda: False
    res["map_bev_host_iou_ms"], _ = timed(lambda: metrics.mAP(pred, target, bev=True, **kw), 2)
    res["map_gpu_vs_host_iou_max_diff"] = float(np.abs(gpu - metrics.mAP(pred, target, bev=True, **kw)).max())
    res["map_bev"] = np.round(gpu[..., 0], 3).tolist()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
