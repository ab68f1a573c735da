"""Generate tests/golden/scn_train.npz and scn_train_grads.npz (build container
only; data only): one training step of the reference SparseConvUnet
(ml3d/torch/models/sparseconvnet.py through tools/ref_loader.py, m = 32,
residual, 20 classes, weights from randla_weights) on a batch of two small
rooms, in float32 and in float64, in train() and in eval() with autograd on —
forward, F.cross_entropy(logits, labels), backward.  The sparse convolutions
are ref_loader's autograd form of the oracle rulebook.

Rooms (built like bench.make_room, smaller; half-integer positions; roughly
every third voxel holds 2 - 3 points at the same position with different
features; the points are shuffled):
  A: floor 70 x 50, walls 24 high, two boxes — level 0 above voxel.hip's
     kDeepMax = 8192 voxels, level 1 and deeper below it, no level empty;
  B: floor 40 x 30, walls 12 high, one box.

scn_train.npz: the inputs (positions, features, labels, batch lengths, room
A's voxel count per level) and per mode the float64 run (the truth): every
7th logit row, the logit column sums, the loss, the gradient name list and
every parameter's gradient norm, for train every BN running_mean /
running_var after the step; and the reference's own float32-vs-float64
relative error on each of these (``*_ref32_err_*``).
scn_train_grads.npz: per mode the full float64 gradients of five small
tensors (full_grad_names) and the float32 reference run's logit rows.
Logit rows and full gradients of the float64 run are stored rounded to
float32 (6e-8 relative, against bounds of 1e-4 and up; the reference errors
are taken before that rounding) to keep each file under 1 MiB.

Asserted on the reference alone, so that the GPU test's bound stays tight: no
stored float32-vs-float64 error above 1e-2, and at most 5 % of the parameter
tensors with a gradient-norm error OR (for the five) a full-gradient error
above 5e-4.  Seeds that miss this are replaced, the conditions stay: feature
seed 11 gave 7 of 125 tensors in train mode, 21 gives none (worst 2.2e-5)."""
import copy
import os
import sys
import time
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)
import randla_weights  # noqa: E402

ROOM_SEED, FEAT_SEED, LABEL_SEED = 0, 21, 12  # feature seed 11 left 7 of 125 train-mode tensors above 5e-4
ROW_STEP = 7
K_DEEP_MAX = 8192  # voxel.hip kDeepMax


def room(rng, X, Y, H, boxes):
    """bench.make_room's layout at a given size: floor, four walls, hollow
    boxes with a lid; voxelize order (linear id, x fastest)."""
    vox = set()
    for x in range(X):
        for y in range(Y):
            vox.add((x, y, 0))
    for z in range(H):
        for x in range(X):
            vox.add((x, 0, z)); vox.add((x, Y - 1, z))
        for y in range(Y):
            vox.add((0, y, z)); vox.add((X - 1, y, z))
    for _ in range(boxes):
        sx, sy, sz = rng.integers(8, 16, 3)
        bx, by = rng.integers(4, X - 4 - sx), rng.integers(4, Y - 4 - sy)
        for z in range(sz):
            for x in range(bx, bx + sx):
                vox.add((x, by, z)); vox.add((x, by + sy - 1, z))
            for y in range(by, by + sy):
                vox.add((bx, y, z)); vox.add((bx + sx - 1, y, z))
        for x in range(bx, bx + sx):
            for y in range(by, by + sy):
                vox.add((x, y, sz))
    v = np.array(list(vox), np.int64)
    v = v[np.lexsort((v[:, 0], v[:, 1], v[:, 2]))]
    return v.astype(np.float32) + 0.5


def with_duplicates(rng, vpos):
    """Roughly every third voxel gets 2 - 3 points (same position); shuffled."""
    reps = np.where(rng.random(len(vpos)) < 1 / 3, rng.integers(2, 4, len(vpos)), 1)
    pos = np.repeat(vpos, reps, axis=0)
    return pos[rng.permutation(len(pos))].copy()


def inputs():
    rng = np.random.default_rng(ROOM_SEED)
    va = room(rng, 70, 50, 24, 2)
    vb = room(rng, 40, 30, 12, 1)
    pa, pb = with_duplicates(rng, va), with_duplicates(rng, vb)
    pos = np.concatenate([pa, pb])
    feat = np.random.default_rng(FEAT_SEED).random((len(pos), 3), dtype=np.float32)
    labels = np.random.default_rng(LABEL_SEED).integers(0, 20, len(pos)).astype(np.int64)
    return va, vb, pos, feat, labels, [len(pa), len(pb)]


def level_sizes(vpos):
    import oracle as O
    sizes, p = [len(vpos)], vpos
    for _ in range(6):  # the m = 32 UNet's six stride-2 Convolutions
        g = O.calculate_grid(p)
        sizes.append(len(g))
        p = g / 2
    return sizes


def stub_self_checks():
    """The autograd form of the stub against the detached float64 branch (bit
    for bit, 200 voxels) and torch.autograd.gradcheck (30 voxels, 2 -> 3)."""
    import ref_loader
    rng = np.random.default_rng(5)
    g = torch.Generator().manual_seed(5)

    def cloud(n, side):
        v = np.unique(rng.integers(0, side, (4 * n, 3)), axis=0)
        v = v[rng.permutation(len(v))[:n]]
        return torch.from_numpy(v.astype(np.float32) + 0.5)

    pos = cloud(200, 9)
    assert len(pos) == 200
    import oracle as O
    grid = torch.from_numpy(O.calculate_grid(pos.numpy()))
    cases = [(ref_loader._SparseConvStub, [3, 3, 3], 0.0, pos, pos, 16, 24, False),
             (ref_loader._SparseConvStub, [2, 2, 2], -0.5, pos, grid, 16, 24, True),
             (ref_loader._SparseConvTransposeStub, [2, 2, 2], -0.5, grid, pos, 24, 16, False)]
    for cls, ks, off, ip, op, cin, cout, norm in cases:
        layer = cls(cin, cout, ks, use_bias=True, normalize=norm, offset=torch.full((3,), off)).double()
        with torch.no_grad():
            layer.kernel.copy_(torch.randn(layer.kernel.shape, generator=g, dtype=torch.float64))
            layer.bias.copy_(torch.randn(cout, generator=g, dtype=torch.float64))
        x = torch.randn((ip.shape[0], cin), generator=g, dtype=torch.float64)
        with torch.no_grad():
            a = layer(x, ip, op, 1.0)
        b = layer(x.clone().requires_grad_(True), ip, op, 1.0)
        assert b.requires_grad and torch.equal(a, b.detach()), (cls.__name__, ks)
        assert float(a.abs().max()) > 0
        print("stub", cls.__name__, ks, "autograd forward == detached float64 branch, bit for bit;",
              int(op.shape[0]), "outputs")
    pos = cloud(30, 5)
    grid = torch.from_numpy(O.calculate_grid(pos.numpy()))
    for cls, ks, off, ip, op in [(ref_loader._SparseConvStub, [3, 3, 3], 0.0, pos, pos),
                                 (ref_loader._SparseConvStub, [2, 2, 2], -0.5, pos, grid),
                                 (ref_loader._SparseConvTransposeStub, [2, 2, 2], -0.5, grid, pos)]:
        layer = cls(2, 3, ks, use_bias=True, offset=torch.full((3,), off)).double()
        x = torch.randn((ip.shape[0], 2), generator=g, dtype=torch.float64, requires_grad=True)
        k0 = torch.randn(layer.kernel.shape, generator=g, dtype=torch.float64, requires_grad=True)
        b0 = torch.randn(3, generator=g, dtype=torch.float64, requires_grad=True)

        def f(x, k, b):
            return torch.func.functional_call(layer, {"kernel": k, "bias": b}, (x, ip, op, 1.0))
        assert torch.autograd.gradcheck(f, (x, k0, b0)), (cls.__name__, ks)
        print("stub", cls.__name__, ks, "gradcheck ok (features, kernel, bias)")


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


def full_grad_names(model):
    """First conv (cin = 3), a level-0 32 -> 32 submanifold kernel, the first
    strided Convolution (2^3, 32 -> 64), the last DeConvolution (64 -> 32),
    the classifier."""
    net = model.unet.net
    conv = [j for j, m in enumerate(net) if type(m).__name__ == "Convolution"]
    deconv = [j for j, m in enumerate(net) if type(m).__name__ == "DeConvolution"]
    return ["sub_sparse_conv.net.kernel", "unet.net.0.sub_sparse_conv1.net.kernel",
            f"unet.net.{conv[0]}.net.kernel", f"unet.net.{deconv[-1]}.net.kernel", "linear.linear.weight"]


def main(write=True):
    import ref_loader
    ref_loader.install()
    from ml3d.torch.models.sparseconvnet import SparseConvUnet
    torch.use_deterministic_algorithms(True)  # index backward sums in one order: the file is reproducible
    if write:
        stub_self_checks()
    va, vb, pos, feat, labels, lengths = inputs()
    sizes_a, sizes_b = level_sizes(va), level_sizes(vb)
    print("room A levels", sizes_a, "room B levels", sizes_b, "points", lengths)
    assert sizes_a[0] > K_DEEP_MAX >= sizes_a[1], sizes_a
    assert len(sizes_a) == 7 and min(sizes_a) > 0 and min(sizes_b) > 0
    main_out = {"pos": pos, "feat": feat, "labels": labels, "lengths": np.array(lengths, np.int64),
                "room_a_levels": np.array(sizes_a, np.int64), "row_step": np.int64(ROW_STEP)}
    grads_out = {}

    torch.manual_seed(0)
    model = SparseConvUnet(multiplier=32, residual_blocks=True, conv_block_reps=1, num_classes=20, device="cpu")
    sd = model.state_dict()
    new = randla_weights.state_dict_for([(k, tuple(v.shape)) for k, v in sd.items()], sd)
    model.load_state_dict(new)
    model64 = copy.deepcopy(model).double()
    full = full_grad_names(model)
    main_out["full_grad_names"] = np.array(full)
    bn_names = [k for k in sd if k.endswith("running_mean") or k.endswith("running_var")]
    split = np.cumsum([0] + lengths)
    lab = torch.from_numpy(labels)

    def batch(dt):
        t = lambda a: torch.from_numpy(a).to(dt)  # noqa: E731
        return types.SimpleNamespace(point=[t(pos[split[i]:split[i + 1]]) for i in range(2)],
                                     feat=[t(feat[split[i]:split[i + 1]]) for i in range(2)],
                                     batch_lengths=list(lengths))

    for mode in ("eval", "train"):
        res = {}
        for tag, mdl, dt in (("32", model, torch.float32), ("64", model64, torch.float64)):
            mdl.load_state_dict({k: v.to(dt) if v.is_floating_point() else v for k, v in new.items()})
            mdl.zero_grad()
            mdl.train(mode == "train")
            t0 = time.time()
            logits = mdl(batch(dt))
            loss = torch.nn.functional.cross_entropy(logits, lab)
            loss.backward()
            print("scn", mode, tag, round(time.time() - t0, 1), "s, loss", loss.item())
            lg = logits.detach().double().numpy()
            r = res[tag] = {"rows": lg[::ROW_STEP], "colsum": lg.sum(0), "loss": float(loss.item()), "names": [],
                            "norms": [], "full": {}}
            for k, p in mdl.named_parameters():
                if p.grad is None:
                    continue
                r["names"].append(k)
                r["norms"].append(float(np.linalg.norm(p.grad.double().numpy())))
                if k in full:
                    r["full"][k] = p.grad.double().numpy()
            r["bn"] = {k: v.double().numpy().copy() for k, v in mdl.state_dict().items() if k in bn_names}
        r32, r64 = res["32"], res["64"]
        assert r32["names"] == r64["names"] and sorted(r64["full"]) == sorted(full)
        p = f"scn_{mode}_"
        main_out[p + "f64_logit_rows"] = r64["rows"].astype(np.float32)
        main_out[p + "f64_logit_colsum"] = r64["colsum"]
        main_out[p + "f64_loss"] = np.float64(r64["loss"])
        main_out[p + "grad_names"] = np.array(r64["names"])
        main_out[p + "f64_grad_norms"] = np.array(r64["norms"], np.float64)
        grads_out[p + "logit_rows"] = r32["rows"].astype(np.float32)
        for k in full:
            grads_out[p + "f64_grad:" + k] = r64["full"][k].astype(np.float32)
        main_out[p + "ref32_err_rows"] = np.float64(rel(r32["rows"], r64["rows"]))
        main_out[p + "ref32_err_colsum"] = np.float64(rel(r32["colsum"], r64["colsum"]))
        main_out[p + "ref32_err_loss"] = np.float64(abs(r32["loss"] - r64["loss"]) / abs(r64["loss"]))
        main_out[p + "ref32_err_norms"] = np.abs(np.array(r32["norms"]) - np.array(r64["norms"])) / \
            np.maximum(np.array(r64["norms"]), 1e-300)
        for k in full:
            main_out[p + "ref32_err_grad:" + k] = np.float64(rel(r32["full"][k], r64["full"][k]))
        errs = {"rows": float(main_out[p + "ref32_err_rows"]), "loss": float(main_out[p + "ref32_err_loss"]),
                "norms max": float(main_out[p + "ref32_err_norms"].max())}
        errs.update({k: float(main_out[p + "ref32_err_grad:" + k]) for k in full})
        # per parameter tensor: the larger of its norm error and, where the
        # full gradient is stored, its full-gradient error
        tensor_errs = [max(float(e), errs.get(k, 0.0)) for k, e in zip(r64["names"], main_out[p + "ref32_err_norms"])]
        if mode == "train":
            main_out[p + "bn_names"] = np.array(bn_names)
            for k in bn_names:
                main_out[p + "f64_bn:" + k] = r64["bn"][k]
            main_out[p + "ref32_err_bn"] = np.array([rel(r32["bn"][k], r64["bn"][k]) for k in bn_names])
            errs["bn max"] = float(main_out[p + "ref32_err_bn"].max())
            # the step moved them (momentum 0.01 of the batch statistics)
            assert all(rel(r64["bn"][k], new[k].numpy()) > 1e-4 for k in bn_names)
        print("scn", mode, "ref fp32 vs fp64:", errs)
        order = np.argsort(-main_out[p + "ref32_err_norms"])[:5]
        print("   largest norm errors:", [(r64["names"][i], float(main_out[p + "ref32_err_norms"][i])) for i in order])
        # the reference alone: nothing above 1e-2, at most 5 % of the parameter
        # tensors with a stored error (gradient norm or full gradient) above
        # 5e-4, so the test's bound stays tight; seeds that miss this are
        # replaced (FEAT_SEED / LABEL_SEED), the conditions stay
        every = [v for v in errs.values()]
        above = [k for k, e in zip(r64["names"], tensor_errs) if e > 5e-4]
        frac = len(above) / len(tensor_errs)
        print("   parameter tensors with a norm or full-gradient error above 5e-4:", len(above), "of",
              len(tensor_errs), "=", round(100 * frac, 2), "%", above)
        assert max(every) <= 1e-2, errs
        assert frac <= 0.05, frac
    if not write:
        return
    for name, out in (("scn_train.npz", main_out), ("scn_train_grads.npz", grads_out)):
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
        print("wrote", path, size, "bytes")
        assert size < (1 << 20), size


if __name__ == "__main__":
    main()
