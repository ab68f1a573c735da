"""Generate tests/golden/point_transformer.npz and
point_transformer_state_dict.json (build container only; data only): the
eval() forward of the reference PointTransformer
(ml3d/torch/models/point_transformer.py through tools/ref_loader.py) in
float32 and in float64.

Three module-level functions of the reference are replaced on the imported
module: ``knn_batch`` (CPU Open3D search, results moved to the GPU) by the
oracle's knn_search on the float32 points, in both runs, so the float64 truth
uses the float32 neighbours; ``furthest_point_sample_v2`` by the oracle's FPS
per cloud; ``interpolation`` by a restatement that follows the dtype of the
features (the reference accumulates into a torch.FloatTensor even in a float64
run) with the distances exactly as knn_search returns them.

Configuration (recorded in the file): blocks [2,2,2,2,2], 13 classes,
in_channels 6, two clouds of 4,500 and 6,001 points U[0,1)^3 * (4, 3, 2.5)
from default_rng(POINT_SEED) (level sizes 1125/1500, 281/375, 70/93, 17/23:
the smallest that keep 16 neighbours at the deepest level with both clouds no
multiple of 64), 3 feature columns U[0,1) from default_rng(FEAT_SEED), weights
from pt_weights.py.

point_transformer.npz: the inputs and seeds, every level's FPS rows, every 7th
logit row of the float64 run rounded to float32, and the reference's own
float32-vs-float64 relative error on those rows.
point_transformer_state_dict.json: names and shapes of the default model's
state_dict.

Asserted on the reference alone (a seed that misses one is replaced, the
conditions stay): the stored relative error is at most 1e-2; the float64
logits are finite and not collapsed (their spread over the rows is at least
1e-2 of their largest magnitude in every class column); the forward runs 13
distinct searches and in every row of each the k-th distance is strictly below
the (k+1)-th, so no neighbour set depends on tie order."""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)

POINT_SEED, FEAT_SEED = 0, 1
SIZES = (4500, 6001)
BLOCKS, NUM_CLASSES, IN_CHANNELS = [2, 2, 2, 2, 2], 13, 6
ROW_STEP = 7


def inputs():
    n = sum(SIZES)
    pts = np.random.default_rng(POINT_SEED).random((n, 3), dtype=np.float32) * np.array([4, 3, 2.5], np.float32)
    feat = np.random.default_rng(FEAT_SEED).random((n, 3), dtype=np.float32)
    return pts.astype(np.float32), feat, np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


def layout(model):
    return [[k, list(v.shape)] for k, v in model.state_dict().items()]


def main(write=True):
    import oracle as O
    import ref_loader
    ref_loader.install()
    import ml3d.torch.models.point_transformer as ref
    import pt_weights

    searches, gaps, sampled = {}, [], []

    def knn_batch(points, queries, k, points_row_splits, queries_row_splits, return_distances=True):
        p = points.detach().float().numpy()
        q = queries.detach().float().numpy()
        prs = np.asarray(points_row_splits, np.int64)
        qrs = np.asarray(queries_row_splits, np.int64)
        idx, _, dist = O.knn_search(p, q, k, prs, qrs, return_distances=True, index_dtype=np.int64)
        key = (p.tobytes(), q.tobytes(), k)
        if key not in searches:
            searches[key] = len(searches)
            _, rs1, d1 = O.knn_search(p, q, k + 1, prs, qrs, return_distances=True)
            full = np.diff(rs1) == k + 1
            last = rs1[1:][full] - 1
            gap = d1[last] - d1[last - 1]
            assert np.all(gap > 0), ("tie between the k-th and (k+1)-th neighbour", k, gap.min())
            if gap.size:
                gaps.append(float(gap.min()))
        idx = torch.from_numpy(idx.reshape(-1, k))
        return (idx, torch.from_numpy(dist.reshape(-1, k))) if return_distances else idx

    def furthest_point_sample_v2(xyz, row_splits, new_row_splits):
        p = xyz.detach().float().numpy()
        rs, nrs = np.asarray(row_splits, np.int64), np.asarray(new_row_splits, np.int64)
        out = [O.furthest_point_sampling(p[rs[b]:rs[b + 1]][None], int(nrs[b + 1] - nrs[b]))[0] + rs[b]
               for b in range(len(rs) - 1)]
        idx = np.concatenate(out).astype(np.int32)
        sampled.append(idx)
        return torch.from_numpy(idx)

    def interpolation(points, queries, feat, points_row_splits, queries_row_splits, k=3):
        idx, dist = ref.knn_batch(points, queries, k=k, points_row_splits=points_row_splits,
                                  queries_row_splits=queries_row_splits, return_distances=True)
        dist_recip = 1.0 / (dist.to(feat.dtype) + 1e-8)
        weight = dist_recip / torch.sum(dist_recip, dim=1, keepdim=True)
        new_feat = torch.zeros((queries.shape[0], feat.shape[1]), dtype=feat.dtype)
        for i in range(k):
            new_feat += feat[idx[:, i].long(), :] * weight[:, i].unsqueeze(-1)
        return new_feat

    ref.knn_batch = knn_batch
    ref.furthest_point_sample_v2 = furthest_point_sample_v2
    ref.interpolation = interpolation

    pts, feat, row_splits = inputs()
    model = ref.PointTransformer(blocks=BLOCKS, in_channels=IN_CHANNELS, num_classes=NUM_CLASSES)
    n_params = sum(p.numel() for p in model.parameters())
    print("parameters", n_params)
    model.load_state_dict(pt_weights.state_dict_for(model), strict=True)
    model.eval()

    rows = {}
    with torch.no_grad():
        for tag, dt in (("32", torch.float32), ("64", torch.float64)):
            mdl = model.double() if dt == torch.float64 else model
            sampled.clear()
            batch = types.SimpleNamespace(point=torch.from_numpy(pts).to(dt), feat=torch.from_numpy(feat).to(dt),
                                          row_splits=torch.from_numpy(row_splits))
            logits = mdl(batch)
            assert logits.dtype == dt and tuple(logits.shape) == (len(pts), NUM_CLASSES)
            rows[tag] = logits.double().numpy()[::ROW_STEP]
            rows["fps" + tag] = [s.copy() for s in sampled]
    assert len(searches) == 13, len(searches)
    assert all(np.array_equal(a, b) for a, b in zip(rows["fps32"], rows["fps64"])) and len(rows["fps64"]) == 4
    r64 = rows["64"]
    err = rel(rows["32"], r64)
    spread = (r64.max(0) - r64.min(0)) / np.abs(r64).max()
    print("ref fp32 vs fp64 on the stored rows:", err, "; logits max", np.abs(r64).max(), "; column spread min",
          spread.min(), "; smallest neighbour gap", min(gaps))
    assert np.isfinite(r64).all() and spread.min() >= 1e-2, spread
    assert err <= 1e-2, err

    out = {"points": pts, "feat": feat, "row_splits": row_splits, "point_seed": np.int64(POINT_SEED),
           "feat_seed": np.int64(FEAT_SEED), "row_step": np.int64(ROW_STEP), "blocks": np.array(BLOCKS, np.int64),
           "num_classes": np.int64(NUM_CLASSES), "in_channels": np.int64(IN_CHANNELS),
           "f64_logit_rows": r64.astype(np.float32), "ref32_err_rows": np.float64(err),
           "min_neighbour_gap": np.float64(min(gaps))}
    for lvl, s in enumerate(rows["fps64"], 1):
        out[f"fps_level{lvl}"] = s
    if not write:
        return
    path = os.path.join(HERE, "point_transformer.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    assert size < (1 << 20), size
    path = os.path.join(HERE, "point_transformer_state_dict.json")
    with open(path, "w") as f:
        json.dump({"PointTransformer": layout(ref.PointTransformer())}, f, indent=0)
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
