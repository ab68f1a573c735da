"""Generate tests/golden/point_transformer_grad.npz (build container only;
data only): one cross-entropy step of the reference PointTransformer
(ml3d/torch/models/point_transformer.py through tools/ref_loader.py) in
eval(), that is with every BatchNorm on its running statistics, in float32
and in float64.

Inputs, seeds, weights (pt_weights.py) and the three replaced module-level
functions are those of make_golden_point_transformer.py (knn_batch by the
oracle's knn_search on the float32 points in both runs, furthest_point_sample_v2
by the oracle's FPS per cloud, interpolation by a restatement that follows the
dtype of the features); labels default_rng(LABEL_SEED).integers(0, 13, n), loss
F.cross_entropy(logits, labels), one backward().

Stored: the float64 loss; the float64 gradient norm of every parameter tensor;
FULL gradients rounded to float32; the reference's own float32-vs-float64
error per tensor (largest element difference over the largest float64 element)
with their median and worst over the tensors that are not mathematically zero;
the names of those that are (the `linear_w.5.bias` of every Transformer: a bias
added to every neighbour's logit cancels in the softmax) and, per layer, the
ratio max|grad linear_w.5.bias| / max|grad linear_w.5.weight| of the float32
run.

Asserted on the reference alone (a label seed that misses one is replaced, the
conditions stay): loss difference at most 1e-5; over the tensors that are not
zero no error above 1e-2 and at most 5 % of them above 5e-4; no float64
gradient identically zero."""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)

from make_golden_point_transformer import BLOCKS, IN_CHANNELS, NUM_CLASSES, inputs, rel  # noqa: E402

LABEL_SEED = 2
FULL = ("encoders.0.0.linear.weight", "encoders.1.0.linear.weight", "encoders.1.1.transformer2.linear_p.0.weight",
        "encoders.1.1.transformer2.linear_p.3.weight", "encoders.2.1.transformer2.linear_w.0.weight",
        "decoders.4.0.linear2.0.weight", "cls.3.weight")
ZERO_SUFFIX = ".linear_w.5.bias"


def main(write=True):
    import oracle as O
    import ref_loader
    ref_loader.install()
    import ml3d.torch.models.point_transformer as ref
    import pt_weights

    def knn_batch(points, queries, k, points_row_splits, queries_row_splits, return_distances=True):
        p = points.detach().float().numpy()
        q = queries.detach().float().numpy()
        idx, _, dist = O.knn_search(p, q, k, np.asarray(points_row_splits, np.int64),
                                    np.asarray(queries_row_splits, np.int64), return_distances=True,
                                    index_dtype=np.int64)
        idx = torch.from_numpy(idx.reshape(-1, k))
        return (idx, torch.from_numpy(dist.reshape(-1, k))) if return_distances else idx

    def furthest_point_sample_v2(xyz, row_splits, new_row_splits):
        p = xyz.detach().float().numpy()
        rs, nrs = np.asarray(row_splits, np.int64), np.asarray(new_row_splits, np.int64)
        out = [O.furthest_point_sampling(p[rs[b]:rs[b + 1]][None], int(nrs[b + 1] - nrs[b]))[0] + rs[b]
               for b in range(len(rs) - 1)]
        return torch.from_numpy(np.concatenate(out).astype(np.int32))

    def interpolation(points, queries, feat, points_row_splits, queries_row_splits, k=3):
        idx, dist = ref.knn_batch(points, queries, k=k, points_row_splits=points_row_splits,
                                  queries_row_splits=queries_row_splits, return_distances=True)
        dist_recip = 1.0 / (dist.to(feat.dtype) + 1e-8)
        weight = dist_recip / torch.sum(dist_recip, dim=1, keepdim=True)
        new_feat = torch.zeros((queries.shape[0], feat.shape[1]), dtype=feat.dtype)
        for i in range(k):
            new_feat = new_feat + feat[idx[:, i].long(), :] * weight[:, i].unsqueeze(-1)
        return new_feat

    ref.knn_batch = knn_batch
    ref.furthest_point_sample_v2 = furthest_point_sample_v2
    ref.interpolation = interpolation

    pts, feat, row_splits = inputs()
    labels = np.random.default_rng(LABEL_SEED).integers(0, NUM_CLASSES, len(pts))
    model = ref.PointTransformer(blocks=BLOCKS, in_channels=IN_CHANNELS, num_classes=NUM_CLASSES)
    model.load_state_dict(pt_weights.state_dict_for(model), strict=True)
    model.eval()
    names = [k for k, _ in model.named_parameters()]

    loss, grads = {}, {}
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        mdl = model.double() if dt == torch.float64 else model
        mdl.zero_grad(set_to_none=True)
        batch = types.SimpleNamespace(point=torch.from_numpy(pts).to(dt), feat=torch.from_numpy(feat).to(dt),
                                      row_splits=torch.from_numpy(row_splits))
        logits = mdl(batch)
        assert logits.dtype == dt and logits.requires_grad
        ls = F.cross_entropy(logits, torch.from_numpy(labels))
        ls.backward()
        loss[tag] = float(ls.detach().double())
        grads[tag] = {k: p.grad.double().numpy().copy() for k, p in mdl.named_parameters()}
        assert not any(m.training for m in mdl.modules())

    zero = [k for k in names if k.endswith(ZERO_SUFFIX)]
    rest = [k for k in names if not k.endswith(ZERO_SUFFIX)]
    loss_diff = abs(loss["32"] - loss["64"]) / abs(loss["64"])
    err = {k: rel(grads["32"][k], grads["64"][k]) for k in names}
    rest_err = np.array([err[k] for k in rest])
    worst = max(rest, key=lambda k: err[k])
    ratios = []
    for k in zero:
        wname = k[:-len("bias")] + "weight"
        ratios.append(np.abs(grads["32"][k]).max() / np.abs(grads["32"][wname]).max())
    print("tensors", len(names), "zero", len(zero), "loss64", loss["64"], "loss diff", loss_diff)
    print("median", float(np.median(rest_err)), "worst", err[worst], worst, "share > 5e-4",
          float((rest_err > 5e-4).mean()), "share > 1e-4", float((rest_err > 1e-4).mean()))
    print("largest float32 zero gradient", max(np.abs(grads["32"][k]).max() for k in zero), "float64",
          max(np.abs(grads["64"][k]).max() for k in zero), "largest ratio", max(ratios))
    assert len(names) == 339 and len(zero) == 10 and len(rest) == 329
    assert loss_diff <= 1e-5, loss_diff
    assert rest_err.max() <= 1e-2, (worst, err[worst])
    assert (rest_err > 5e-4).mean() <= 0.05
    assert all(np.abs(grads["64"][k]).max() > 0 for k in rest)
    assert all(k in names for k in FULL)

    out = {"label_seed": np.int64(LABEL_SEED), "labels": labels.astype(np.int64), "f64_loss": np.float64(loss["64"]),
           "ref32_loss_diff": np.float64(loss_diff), "grad_names": np.array(names),
           "f64_grad_norms": np.array([np.linalg.norm(grads["64"][k]) for k in names], np.float64),
           "ref32_err": np.array([err[k] for k in names], np.float64), "ref32_err_median": np.float64(np.median(rest_err)),
           "ref32_err_worst": np.float64(rest_err.max()), "ref32_share_above_5e-4": np.float64((rest_err > 5e-4).mean()),
           "zero_grad_names": np.array(zero), "zero_grad_ratios": np.array(ratios, np.float64),
           "full_grad_names": np.array(FULL)}
    for k in FULL:
        out["f64_grad:" + k] = grads["64"][k].astype(np.float32)
    if not write:
        return
    path = os.path.join(HERE, "point_transformer_grad.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    assert size < (1 << 20), size


if __name__ == "__main__":
    main()
