"""Time PointTransformer gradients.  Prints one JSON line, times in ms (host
clock around work that ends in a device synchronise; medians over --iters
after a warm-up of every shape):

  fixture_step_ms      forward under recording_grad(), cross entropy and
                       backward on the batch of tests/golden/point_transformer.npz
                       (4,500 + 6,001 points), beside fixture_forward_ms, the
                       plain eval() forward;
  fixture_kernels_ms   per step of the fixture, the HIP kernels' own time (HIP
                       events around the launches, o3dml_timing) and launches;
  layer_c64 / c256     one Transformer layer at --points points, nsample 16,
                       forward + backward (gradients of the input features and
                       of every parameter): the fused path under
                       recording_grad() beside the same layer composed from
                       torch ops under autograd (tools/pt_time.py
                       composed_layer), both given the same neighbour index,
                       alternating; the fused path's per-kernel split and the
                       time of its torch part for linear_p[0..2] (run once per
                       op); and rel_diff, fused against composed: d feat per
                       element relative to its largest element (largest, share
                       above 1e-4, and the relative L2 difference) and the
                       largest such figure over the parameter gradients.

    python tools/pt_grad_time.py [--iters 10] [--points 80000]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "open3d-ml_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pt_time import clock, composed_layer, timed  # noqa: E402

KERNELS = ["knn_search", "fps_ragged", "pt_group", "pt_relation", "pt_aggregate", "pt_knn_interpolate",
           "pt_invert_plan", "pt_gather_sum", "pt_relation_backward", "pt_aggregate_backward"]
LAYER_KERNELS = ["pt_relation", "pt_aggregate", "pt_invert_plan", "pt_gather_sum", "pt_relation_backward",
                 "pt_aggregate_backward"]


def kernel_split(lib, _lib, fn, names, iters):
    lib.o3dml_timing_enable(1)
    lib.o3dml_timing_reset()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    times = _lib.kernel_times(names)
    lib.o3dml_timing_enable(0)
    return {k: [round(ms / iters, 3), cnt // iters] for k, (ms, cnt) in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--points", type=int, default=80000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pt_grad_time: no ROCm GPU is visible")
    import pt_weights
    from o3dml_amd import _lib
    from o3dml_amd.point_transformer import (Neighbours, PointTransformer, Transformer, _pos_hidden_backward,
                                             position_encoding, recording_grad)
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    res = {"tool": "pt_grad_time", "device": torch.cuda.get_device_name(0), "iters": args.iters,
           "points": args.points}

    model = PointTransformer()
    model.load_state_dict(pt_weights.state_dict_for(model), strict=True)
    model = model.to(dev).eval()
    z = np.load(os.path.join(ROOT, "tests", "golden", "point_transformer.npz"))
    fixture = {"point": torch.from_numpy(z["points"]).to(dev), "feat": torch.from_numpy(z["feat"]).to(dev),
               "row_splits": torch.from_numpy(z["row_splits"])}
    labels = torch.from_numpy(np.random.default_rng(2).integers(0, 13, len(z["points"]))).to(dev)

    def step():
        model.zero_grad(set_to_none=True)
        with recording_grad():
            logits = model(fixture)
        F.cross_entropy(logits, labels).backward()

    res["fixture_forward_ms"] = timed(lambda: model(fixture), args.iters)
    res["fixture_step_ms"] = timed(step, args.iters)
    res["fixture_kernels_ms"] = kernel_split(lib, _lib, step, KERNELS, args.iters)
    model.zero_grad(set_to_none=True)

    rng = np.random.default_rng(0)
    point = torch.from_numpy(rng.random((args.points, 3), dtype=np.float32) * np.array([8, 6, 3], np.float32)).to(dev)
    for c in (64, 256):
        layer = Transformer(c, c, 8, 16)
        layer.load_state_dict(pt_weights.state_dict_for(layer))
        layer = layer.to(dev).eval()
        feat = torch.from_numpy(rng.standard_normal((args.points, c)).astype(np.float32)).to(dev).requires_grad_()
        g = torch.from_numpy(rng.standard_normal((args.points, c)).astype(np.float32)).to(dev)
        grads = {}

        def collect(tag):
            grads[tag] = {"feat": feat.grad, **{k: p.grad for k, p in layer.named_parameters()}}

        def fused():
            # a new plan object every step, as in the model: the inverse list is built once per step
            plan = Neighbours(index, args.points, _trusted=True)
            layer.zero_grad(set_to_none=True)
            feat.grad = None
            with recording_grad():
                out = layer([point, feat, None, plan])
            out.backward(g)
            collect("fused")

        def composed():
            layer.zero_grad(set_to_none=True)
            feat.grad = None
            composed_layer(layer, point, feat, index).backward(g)
            collect("composed")

        index = Neighbours.from_knn(point, point, 16, [0, args.points], [0, args.points]).index
        fused()
        composed()
        # two float32 runs take some ReLUs on different sides of zero: each such pair moves single
        # elements of d feat by a whole term, which the sums over all pairs in the parameter gradients average out
        a, b = grads["fused"], grads["composed"]
        dfeat = (a["feat"] - b["feat"]).abs() / b["feat"].abs().max()
        diff = {"dfeat_max": float(dfeat.max()), "dfeat_share_above_1e-4": float((dfeat > 1e-4).float().mean()),
                "dfeat_l2": float((a["feat"] - b["feat"]).norm() / b["feat"].norm()),
                "params_max": max(float((a[k] - b[k]).abs().max() / b[k].abs().max()) for k in a
                                  if k != "feat" and not k.endswith("linear_w.5.bias"))}
        tf, tc = [], []
        for _ in range(args.iters):  # alternating, the same call
            tf.append(clock(fused))
            tc.append(clock(composed))
        # the part of the fused backward that runs on torch ops: linear_p[0..2] from dh, once per op
        plan = Neighbours(index, args.points, _trusted=True)
        lp = [t.detach() for t in position_encoding(layer.linear_p)[:4]]
        dh = torch.from_numpy(rng.standard_normal((args.points, 16, 3)).astype(np.float32)).to(dev)
        first = timed(lambda: _pos_hidden_backward(plan, point, point, *lp, dh), args.iters)
        res[f"layer_c{c}"] = {"fused_ms": round(statistics.median(tf), 3),
                              "composed_torch_ms": round(statistics.median(tc), 3), "rel_diff": diff,
                              "fused_kernels_ms": kernel_split(lib, _lib, fused, LAYER_KERNELS, args.iters),
                              "pos_hidden_backward_torch_ms": first}
        del grads, feat, g
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
