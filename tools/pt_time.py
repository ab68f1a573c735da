"""Time PointTransformer inference.  Prints one JSON line, times in ms (host
clock around work that ends in a device synchronise; medians over --iters
after a warm-up of every shape):

  fixture_forward_ms   eval() forward on the batch of
                       tests/golden/point_transformer.npz (4,500 + 6,001 points);
  room_forward_ms      the same on one synthetic room of --points points
                       (default 80,000, the reference's max_voxels), uniform in
                       an 8 x 6 x 3 box;
  room_kernels_ms      per forward of the room, the HIP kernels' own time (HIP
                       events around the launches, o3dml_timing) and launches;
  layer_c64 / c256     one Transformer layer at --points points, nsample 16:
                       the fused path (relation, the two small Linears,
                       aggregate) beside the same layer composed from torch ops
                       on the GPU as the reference writes it
                       (point_transformer.py:427-467), both given the same
                       neighbour index, alternating; and their largest
                       difference relative to the largest output.

The composition is the comparison: the reference itself searches on the CPU
and is not runnable here.

    python tools/pt_time.py [--iters 10] [--points 80000]
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

KERNELS = ["knn_search", "fps_ragged", "pt_group", "pt_relation", "pt_aggregate", "pt_knn_interpolate"]


def clock(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def timed(fn, iters):
    fn()
    return round(statistics.median(clock(fn) for _ in range(iters)), 3)


def composed_layer(layer, point, feat, idx):
    """Transformer.forward as the reference writes it, on torch ops, with the
    neighbour index given (eval mode)."""
    n, ns = idx.shape
    flat = idx.reshape(-1).long()
    feat_q, feat_k, feat_v = layer.linear_q(feat), layer.linear_k(feat), layer.linear_v(feat)
    point_r = point[flat, :].view(n, ns, 3) - point.unsqueeze(1)
    feat_k = feat_k[flat, :].view(n, ns, -1)
    feat_v = feat_v[flat, :].view(n, ns, -1)
    for i, mod in enumerate(layer.linear_p):
        point_r = mod(point_r.transpose(1, 2).contiguous()).transpose(1, 2).contiguous() if i == 1 else mod(point_r)
    w = feat_k - feat_q.unsqueeze(1) + point_r
    for i, mod in enumerate(layer.linear_w):
        w = mod(w.transpose(1, 2).contiguous()).transpose(1, 2).contiguous() if i % 3 == 0 else mod(w)
    w = layer.softmax(w)
    c, s = feat_v.shape[2], layer.share_planes
    return ((feat_v + point_r).view(n, ns, s, c // s) * w.unsqueeze(2)).sum(1).view(n, c)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--points", type=int, default=80000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pt_time: no ROCm GPU is visible")
    import pt_weights
    from o3dml_amd import _lib
    from o3dml_amd.point_transformer import Neighbours, PointTransformer, Transformer
    dev = torch.device("cuda", 0)
    res = {"tool": "pt_time", "device": torch.cuda.get_device_name(0), "iters": args.iters, "points": args.points}

    model = PointTransformer()
    model.load_state_dict(pt_weights.state_dict_for(model), strict=True)
    model = model.to(dev).eval()
    z = np.load(os.path.join(ROOT, "tests", "golden", "point_transformer.npz"))
    fixture = {"point": torch.from_numpy(z["points"]).to(dev), "feat": torch.from_numpy(z["feat"]).to(dev),
               "row_splits": torch.from_numpy(z["row_splits"])}
    rng = np.random.default_rng(0)
    room_pts = rng.random((args.points, 3), dtype=np.float32) * np.array([8, 6, 3], np.float32)
    room = {"point": torch.from_numpy(room_pts).to(dev),
            "feat": torch.from_numpy(rng.random((args.points, 3), dtype=np.float32)).to(dev),
            "row_splits": torch.tensor([0, args.points])}
    res["fixture_forward_ms"] = timed(lambda: model(fixture), args.iters)
    res["room_forward_ms"] = timed(lambda: model(room), args.iters)

    lib = _lib.load()
    lib.o3dml_timing_enable(1)
    lib.o3dml_timing_reset()
    for _ in range(args.iters):
        model(room)
    torch.cuda.synchronize()
    times = _lib.kernel_times(KERNELS)
    lib.o3dml_timing_enable(0)
    res["room_kernels_ms"] = {k: [round(ms / args.iters, 3), cnt // args.iters] for k, (ms, cnt) in times.items()}

    point = room["point"]
    plan = Neighbours.from_knn(point, point, 16, [0, args.points], [0, args.points])
    for c in (64, 256):
        layer = Transformer(c, c, 8, 16)
        layer.load_state_dict(pt_weights.state_dict_for(layer))
        layer = layer.to(dev).eval()
        feat = torch.from_numpy(rng.standard_normal((args.points, c)).astype(np.float32)).to(dev)
        fused = lambda: layer([point, feat, None, plan])  # noqa: E731
        with torch.no_grad():
            composed = lambda: composed_layer(layer, point, feat, plan.index)  # noqa: E731
            a, b = fused(), composed()
            diff = float((a - b).abs().max() / b.abs().max())
            composed()
            tf, tc = [], []
            for _ in range(args.iters):  # alternating, the same call
                tf.append(clock(fused))
                tc.append(clock(composed))
        res[f"layer_c{c}"] = {"fused_ms": round(statistics.median(tf), 3),
                              "composed_torch_ms": round(statistics.median(tc), 3), "max_rel_diff": diff}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
