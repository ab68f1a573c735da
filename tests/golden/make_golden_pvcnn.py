"""Generate tests/golden/pvcnn.npz and pvcnn_state_dict.json (build container
only; data only): one step of the reference PVCNN (ml3d/torch/models/pvcnn.py
through tools/ref_loader.py) in float32 and in float64, in train() and in
eval() with autograd on — forward, F.cross_entropy(logits, labels), backward.

ref_loader defines the two devoxelize ops as None, so the module's
``trilinear_devoxelize`` and ``avg_voxelize`` are replaced by the torch
restatements below, which follow the dtype of the features (the reference's
avg_voxelize hard-codes float32 zeros): a gather over the 8 corners with
hi = lo + (d1 > 0), differentiated by autograd, and a scatter-add mean.  The
points are passed as float32 in both runs, so the normalised coordinates and
the voxel assignment (pvcnn.py:653-662) are the float32 ones in both and the
float64 truth uses the same voxels.  The Dropout layers of the classifier are
set to p = 0 (DROPOUT_P): a random mask has no float64 truth.

Configuration (recorded in the file): width_multiplier 0.25 (166,205
parameters), voxel_resolution_multiplier VRM, 13 classes, B = 4, N = 1000 (no
multiple of 64), points U[0,1)^3 * (4, 3, 2.5) from default_rng(POINT_SEED)
with the few that land near a voxel boundary moved off it (off_boundaries),
6 extra features, random labels, torch.manual_seed(WEIGHT_SEED) weights,
stored because initialisation is not portable.

pvcnn.npz: the inputs and weights and per mode the float64 run (the truth,
rounded to float32): every 7th logit row, the loss, every parameter's
gradient norm, the full gradients of five small tensors, for train the BN
running statistics after the step; and the reference's own float32-vs-float64
relative error on each (``*_ref32_err_*``), taken before the rounding.
pvcnn_state_dict.json: state_dict names and shapes of the default PVCNN() and
of the 0.25 model.

Asserted on the reference alone (a seed that misses them is replaced, the
conditions stay).  A parameter is live when its float64 gradient norm exceeds
1e-6 of the largest; the others (biases in front of a BatchNorm in train
mode: analytically zero) must stay at or below 1e-5 of the largest in float32.
No stored relative error above 1e-2; at most 5 % of the live tensors with a
gradient-norm or full-gradient error above 5e-4; no normalised coordinate
within 1e-3 of a rounding boundary (x.5) or of an integer (the d1 > 0 test) at
either resolution; in train mode no (Leaky)ReLU input that has a gradient within
KINK_MARGIN = 1e-6 of zero relative to its layer's rms.  That margin is the
float32 noise of such an input itself (eps x sqrt(fan-in 432 .. 864)), not a
safety factor: about 3 inputs fall within every 1e-6 of zero whatever the
seed, and each carries up to 5e-3 of its layer's gradient, so a second float32
evaluation can still cross one (the margins are printed and stored as
``*_kink_margin_min``).  B = 2 misses them badly (BatchNorm1d over two samples), and
so does B = 4, N = 2048, seed 0 (conditioning of that instance): keep B >= 4."""
import copy
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

# point / feature / label seeds 1 / 2 / 3 left 8 of 53 live train-mode tensors above 5e-4; 1 / 4 / 5 left none
# (worst 1.8e-5) but has a LeakyReLU input within 1e-7 of zero in train mode (float32 runs on inputs moved by 1e-7
# differ by 2.9e-4, the GPU by 2e-3); of 52 seed triples tried 2 / 8 / 9 keeps the train-mode inputs furthest from zero
WEIGHT_SEED, POINT_SEED, FEAT_SEED, LABEL_SEED = 0, 2, 8, 9
KINK_MARGIN = 1e-6
B, N, NUM_CLASSES, WIDTH, VRM = 4, 1000, 13, 0.25, 1
DROPOUT_P = 0.0
ROW_STEP = 7
FULL = ["point_features.0.voxel_layers.0.weight", "point_features.0.point_features.layers.0.weight",
        "point_features.2.voxel_layers.3.weight", "cloud_features.1.0.weight", "classifier.4.weight"]


def avg_voxelize(feat, coords, r):
    """pvcnn.py:579-619 in the dtype of feat."""
    c = coords.to(torch.int64)
    h = (c[:, 0] * r + c[:, 1]) * r + c[:, 2]  # [B, N]
    Bn, C, _ = feat.shape
    grid = torch.zeros((Bn, C, r ** 3), dtype=feat.dtype).scatter_add(2, h[:, None, :].expand(-1, C, -1), feat)
    cnt = torch.zeros((Bn, r ** 3), dtype=feat.dtype).scatter_add(1, h, torch.ones(h.shape, dtype=feat.dtype))
    return (grid / cnt.clamp(min=1)[:, None, :]).reshape(Bn, C, r, r, r)


def trilinear_devoxelize(features, coords, r, is_training=True):
    """Gather over the 8 corners, hi = lo + (d1 > 0); autograd differentiates it."""
    dt = features.dtype
    c = coords.to(dt).clamp(0, r - 1)
    lo = torch.floor(c)
    d1 = c - lo
    d0 = 1.0 - d1
    lo = lo.to(torch.int64)
    hi = lo + (d1 > 0).to(torch.int64)
    f = features.reshape(features.shape[0], features.shape[1], -1)
    out = None
    for k in range(8):
        bits = ((k >> 2) & 1, (k >> 1) & 1, k & 1)
        ax = [hi[:, a] if bit else lo[:, a] for a, bit in enumerate(bits)]
        w = [d1[:, a] if bit else d0[:, a] for a, bit in enumerate(bits)]
        idx = (ax[0] * r + ax[1]) * r + ax[2]
        term = ((w[0] * w[1]) * w[2])[:, None, :] * f.gather(2, idx[:, None, :].expand(-1, f.shape[1], -1))
        out = term if out is None else out + term
    return out


def off_boundaries(pts, resolutions, margin=1e-3, step=4e-3, rounds=50):
    """Among 12,000 uniform coordinates some always fall within `margin` of a
    rounding boundary or an integer (about 2 % of the points per resolution),
    whatever the seed, so those are moved: by `step` grid units of the
    resolution that objects, away from the boundary, until none is left.  A
    move shifts the cloud's mean by about 1e-7 of the extent, far below the
    margin, so the loop settles in a few rounds."""
    pts = pts.copy()
    for _ in range(rounds):
        moved = 0
        for r in resolutions:
            c = torch.from_numpy(pts)
            c = c - c.mean(2, keepdim=True)
            scale = c.norm(dim=1, keepdim=True).max(dim=2, keepdim=True).values * 2.0 + 1e-6
            t = (torch.clamp((c / scale + 0.5) * r, 0, r - 1)).numpy()
            half = t * 2 - np.round(t * 2)  # signed distance to the nearest k or k + .5, times 2
            bad = np.abs(half) < 2 * 1.5 * margin
            if bad.any():
                moved += int(bad.sum())
                world = (step / r) * scale.numpy()  # [B,1,1]
                pts = np.where(bad, pts + np.where(half >= 0, 1, -1) * world, pts).astype(np.float32)
        if not moved:
            return pts
    raise AssertionError("points did not settle off the voxel boundaries")


def inputs():
    pts = np.random.default_rng(POINT_SEED).random((B, 3, N), dtype=np.float32) * \
        np.array([4, 3, 2.5], np.float32)[None, :, None]
    pts = off_boundaries(pts.astype(np.float32), sorted({int(VRM * 32), int(VRM * 16)}))
    extra = np.random.default_rng(FEAT_SEED).random((B, 6, N), dtype=np.float32)
    labels = np.random.default_rng(LABEL_SEED).integers(0, NUM_CLASSES, (B, N)).astype(np.int64)
    return pts.astype(np.float32), extra, labels


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


def layout(model):
    return [[k, list(v.shape)] for k, v in model.state_dict().items()]


def main(write=True):
    import ref_loader
    ref_loader.install()
    import ml3d.torch.models.pvcnn as ref
    ref.trilinear_devoxelize = trilinear_devoxelize
    ref.avg_voxelize = avg_voxelize
    torch.use_deterministic_algorithms(True)

    pts, extra, labels = inputs()
    out = {"points": pts, "extra": extra, "labels": labels, "row_step": np.int64(ROW_STEP),
           "width_multiplier": np.float64(WIDTH), "voxel_resolution_multiplier": np.float64(VRM),
           "num_classes": np.int64(NUM_CLASSES), "dropout_p": np.float64(DROPOUT_P),
           "full_grad_names": np.array(FULL)}

    torch.manual_seed(WEIGHT_SEED)
    model = ref.PVCNN(device="cpu", num_classes=NUM_CLASSES, width_multiplier=WIDTH,
                      voxel_resolution_multiplier=VRM)
    n_params = sum(p.numel() for p in model.parameters())
    print("parameters", n_params, "tensors", len(list(model.parameters())))
    assert n_params == 166205
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = DROPOUT_P
    start = {k: v.clone() for k, v in model.state_dict().items()}
    out["weight_names"] = np.array([k for k, _ in model.named_parameters()])
    for k, p in model.named_parameters():
        out["w:" + k] = p.detach().numpy().copy()
    model64 = copy.deepcopy(model).double()
    bn_names = [k for k in start if k.endswith("running_mean") or k.endswith("running_var")]

    # the voxel assignment of the float32 run: nothing near a rounding boundary or an integer
    resolutions = sorted({m.r for m in model.modules() if isinstance(m, ref.Voxelization)})
    print("resolutions", resolutions)
    for r in resolutions:
        vox = ref.Voxelization(r)
        ref.avg_voxelize = lambda f, c, rr: f  # noqa: E731
        _, nc = vox(torch.zeros(1), torch.from_numpy(pts))
        ref.avg_voxelize = avg_voxelize
        frac = (nc - torch.floor(nc)).numpy()
        d_half, d_int = np.abs(frac - 0.5).min(), np.minimum(frac, 1 - frac).min()
        print("r", r, "closest to x.5:", d_half, "closest to an integer:", d_int)
        assert d_half > 1e-3 and d_int > 1e-3, (r, d_half, d_int)

    # float64 model: record each (Leaky)ReLU input next to the gradient of its output
    margins = []

    def keep_input(mod, inp):
        mod._input = inp[0].detach().clone()  # the activations work in place

    def on_output(mod, inp, res_):
        x = mod._input
        if res_.requires_grad:
            res_.register_hook(lambda gr: margins.append(
                (x[gr != 0].abs() / x[gr != 0].pow(2).mean().sqrt()).numpy()))

    for mod in model64.modules():
        if isinstance(mod, (torch.nn.ReLU, torch.nn.LeakyReLU)):
            mod.register_forward_pre_hook(keep_input)
            mod.register_forward_hook(on_output)

    lab = torch.from_numpy(labels).reshape(-1)
    for mode in ("eval", "train"):
        res = {}
        margins.clear()
        for tag, mdl, dt in (("32", model, torch.float32), ("64", model64, torch.float64)):
            mdl.load_state_dict({k: v.to(dt) if v.is_floating_point() else v for k, v in start.items()})
            mdl.zero_grad()
            mdl.train(mode == "train")
            t0 = time.time()
            feat = torch.from_numpy(np.concatenate([pts, extra], 1)).to(dt)
            logits = mdl({"point": torch.from_numpy(pts), "feat": feat})
            assert logits.dtype == dt and tuple(logits.shape) == (B, N, NUM_CLASSES)
            loss = torch.nn.functional.cross_entropy(logits.reshape(-1, NUM_CLASSES), lab)
            loss.backward()
            print("pvcnn", mode, tag, round(time.time() - t0, 1), "s, loss", loss.item())
            lg = logits.detach().double().numpy().reshape(-1, NUM_CLASSES)
            r_ = res[tag] = {"rows": lg[::ROW_STEP], "loss": float(loss.item()), "names": [], "norms": [], "full": {}}
            for k, p in mdl.named_parameters():
                r_["names"].append(k)
                r_["norms"].append(float(np.linalg.norm(p.grad.double().numpy())))
                if k in FULL:
                    r_["full"][k] = p.grad.double().numpy()
            r_["bn"] = {k: v.double().numpy().copy() for k, v in mdl.state_dict().items() if k in bn_names}
        r32, r64 = res["32"], res["64"]
        assert r32["names"] == r64["names"] and sorted(r64["full"]) == sorted(FULL)
        p = f"pv_{mode}_"
        n32, n64 = np.array(r32["norms"]), np.array(r64["norms"])
        live = n64 > 1e-6 * n64.max()
        assert np.all(n32[~live] <= 1e-5 * n64.max()), n32[~live]
        out[p + "f64_logit_rows"] = r64["rows"].astype(np.float32)
        out[p + "f64_loss"] = np.float64(r64["loss"])
        out[p + "grad_names"] = np.array(r64["names"])
        out[p + "f64_grad_norms"] = n64
        out[p + "ref32_err_rows"] = np.float64(rel(r32["rows"], r64["rows"]))
        out[p + "ref32_err_loss"] = np.float64(abs(r32["loss"] - r64["loss"]) / abs(r64["loss"]))
        out[p + "ref32_err_norms"] = np.where(live, np.abs(n32 - n64) / np.maximum(n64, 1e-300), 0.0)
        errs = {"rows": float(out[p + "ref32_err_rows"]), "loss": float(out[p + "ref32_err_loss"]),
                "norms max": float(out[p + "ref32_err_norms"].max())}
        for k in FULL:
            out[p + "f64_grad:" + k] = r64["full"][k].astype(np.float32)
            out[p + "ref32_err_grad:" + k] = np.float64(rel(r32["full"][k], r64["full"][k]))
            errs[k] = float(out[p + "ref32_err_grad:" + k])
        tensor_errs = [max(float(e), errs.get(k, 0.0))
                       for k, e, lv in zip(r64["names"], out[p + "ref32_err_norms"], live) if lv]
        if mode == "train":
            out[p + "bn_names"] = np.array(bn_names)
            for k in bn_names:
                out[p + "f64_bn:" + k] = r64["bn"][k].astype(np.float32)
            out[p + "ref32_err_bn"] = np.array([rel(r32["bn"][k], r64["bn"][k]) for k in bn_names])
            errs["bn max"] = float(out[p + "ref32_err_bn"].max())
            assert all(rel(r64["bn"][k], start[k].numpy()) > 1e-4 for k in bn_names)  # the step moved them
        above = sum(e > 5e-4 for e in tensor_errs)
        print("pvcnn", mode, "ref fp32 vs fp64:", errs)
        print("   live tensors", int(live.sum()), "of", len(live), "; above 5e-4:", above, "; worst",
              max(tensor_errs), "median", float(np.median(tensor_errs)))
        assert max(errs.values()) <= 1e-2, errs
        assert above / len(tensor_errs) <= 0.05, above
        # kinks: every (Leaky)ReLU whose input changes sign between two float32
        # evaluations moves the gradients by that element's share of its layer's
        # gradient (up to 5e-3 here), far above the 1e-4 the test allows, so the
        # float64 run reports how close the inputs with a nonzero gradient come to
        # zero, relative to their layer's rms
        near = np.concatenate([m_ for m_ in margins])
        print("   (Leaky)ReLU inputs with a gradient:", near.size, "; closest to zero", near.min(), "of the rms; within",
              "1e-6 / 3e-6 / 1e-5:", int((near < 1e-6).sum()), int((near < 3e-6).sum()), int((near < 1e-5).sum()))
        out[p + "kink_margin_min"] = np.float64(near.min())
        if mode == "train":
            assert near.min() >= KINK_MARGIN, near.min()
    if not write:
        return
    path = os.path.join(HERE, "pvcnn.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    assert size < (1 << 20), size
    torch.manual_seed(0)
    layouts = {"PVCNN": layout(ref.PVCNN(device="cpu")),
               "PVCNN_w0.25": layout(ref.PVCNN(device="cpu", width_multiplier=0.25))}
    path = os.path.join(HERE, "pvcnn_state_dict.json")
    with open(path, "w") as f:
        json.dump(layouts, f, indent=0)
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
