"""Time farthest-point sampling of single clouds.  Prints one JSON line, times
in ms: medians over --iters calls after a warm-up of every shape, HIP events
around each call's launches.

Per case  n -> m:
  direct_ms        ops.furthest_point_sampling(..., method="direct"): the
                   register variants up to 32,768 points, fps_cloud_global above;
  pruned_ms        method="pruned": set-up and kernel;
  pruned_setup_ms  of that, box + keys + sort + gather (o3dml_timing);
  visited_per_round  mean buckets visited per round, of `buckets`;
  equal            the two results are the same bits.
On a tree without the pruned path (no `method` argument) only direct_ms is
reported, so the same tool times the commit before it.

Cases: a synthetic room of 80,000 points (floor, ceiling, four walls and a
few boxes of furniture, 1 cm noise) and its first sampled level of 20,000;
33,000, 16,384 and 4,096 points of the same room; 80,000 points uniform in a
cube, where pruning bites least.

    python tools/fps_time.py [--iters 7]
"""
import argparse
import inspect
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "open3d-ml_amd"))


def room(n, seed=0):
    rng = np.random.default_rng(seed)
    size = np.array([8, 6, 3], np.float32)
    pts = rng.random((n, 3), dtype=np.float32) * size
    kind = rng.integers(0, 8, n)
    for k, (axis, value) in enumerate([(2, 0), (2, 3), (0, 0), (0, 8), (1, 0), (1, 6)]):
        pts[kind == k, axis] = value
    box = kind >= 6  # furniture: points on the surfaces of a few 1 m boxes
    corner = rng.integers(0, 5, (n, 3)).astype(np.float32) * np.array([1.5, 1.2, 0], np.float32)
    local = rng.random((n, 3), dtype=np.float32)
    face = rng.integers(0, 3, n)
    local[np.arange(n), face] = rng.integers(0, 2, n)
    pts[box] = (corner + local)[box]
    return pts + rng.normal(0, 0.01, (n, 3)).astype(np.float32)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def median_ms(fn, iters):
    fn()
    return round(statistics.median(event_ms(fn)[0] for _ in range(iters)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fps_time: no ROCm GPU is visible")
    from o3dml_amd import _lib, ops
    from o3dml_amd import point_transformer as pt
    dev = torch.device("cuda", 0)
    has_pruned = "method" in inspect.signature(ops.furthest_point_sampling).parameters
    res = {"tool": "fps_time", "device": torch.cuda.get_device_name(0), "iters": args.iters, "pruned": has_pruned}
    lib = _lib.load()

    big = room(80000)
    direct = (lambda x, m: ops.furthest_point_sampling(x, m, method="direct")) if has_pruned \
        else ops.furthest_point_sampling
    level1 = big[direct(torch.from_numpy(big[None]).to(dev), 20000)[0].cpu().numpy()]
    cube = np.random.default_rng(1).random((80000, 3), dtype=np.float32)
    cases = [("room_80000_20000", big, 20000), ("room_20000_5000", level1, 5000),
             ("room_33000_8250", room(33000, 2), 8250), ("room_16384_4096", room(16384, 3), 4096),
             ("room_4096_1024", room(4096, 4), 1024), ("cube_80000_20000", cube, 20000)]
    for name, pts, m in cases:
        x = torch.from_numpy(np.ascontiguousarray(pts[None])).to(dev)
        n = x.shape[1]
        r = {"direct_ms": median_ms(lambda: direct(x, m), args.iters)}
        if has_pruned:
            pruned = lambda: ops.furthest_point_sampling(x, m, method="pruned")  # noqa: E731
            r["pruned_ms"] = median_ms(pruned, args.iters)
            lib.o3dml_timing_enable(1)
            lib.o3dml_timing_reset()
            for _ in range(args.iters):
                pruned()
            torch.cuda.synchronize()
            ms, cnt = _lib.kernel_times(["fps_pruned_setup"])["fps_pruned_setup"]
            lib.o3dml_timing_enable(0)
            r["pruned_setup_ms"] = round(ms / cnt, 3)
            rows, visited = pt.furthest_point_sample_ragged(x[0], [0, n], [0, m], method="pruned",
                                                            return_visited=True)
            r["buckets"] = -(-n // 64)
            r["visited_per_round"] = round(int(visited.item()) / (m - 1), 1)
            r["equal"] = bool(torch.equal(rows.view(1, m), direct(x, m)))
        res[name] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
