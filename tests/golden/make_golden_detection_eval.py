"""Generate tests/golden/detection_eval.npz (build container only, not run by
tests): the reference's detection evaluation, ml3d.metrics.mAP
(ml3d/metrics/mAP.py, imported with tools/ref_loader.py), on seeded synthetic
KITTI-like frames, with Open3D's box IoU — un-vendored — stood in for by a
float64 polygon clip written here (Sutherland-Hodgman, independent of the
library's edge-crossing / angle-sort routine, same rotation sense as
box_corners in csrc/box_iou.hpp: a corner offset (dx, dy) maps to
(dx cos ry + dy sin ry, -dx sin ry + dy cos ry)).

Frames: 8, classes 0-2 evaluated, label 3 the "similar" class of 2, label 4
ignored; difficulties 0-2 (and -1 = unrated).  Predictions are jittered
copies of the targets plus clutter.  Frame 2 has no predictions, frame 5 no
targets, frame 3 nothing of class 1.

Stored (data only): the inputs (concatenated, with row splits), the float64
BEV and 3D IoU of every prediction x target pair per frame (row-major blocks
back to back, `iou_offsets`), their nonzero masks (the BEV one is what
box_collision_test, operations.py:417-434, returns; that function itself
needs np.bool and cannot run on this numpy), the reference's mAP for bev =
True / False at two min_overlap settings and one similar_classes case, and
`iou_tol` = 4 x the worst |oracle.bev_iou - float64| over the fixture's BEV
pairs (the oracle runs the library's float32 algorithm; the margin covers the
device's sinf / cosf / atan2f against glibc's).

A seed is accepted only if (asserted, else the next seed is tried):
  * no float64 IoU lies within 1e-3 of a threshold in use;
  * no IoU lies in (0, 1e-3);
  * the nonzero IoUs of one target's column differ pairwise by > 1e-3 (so the
    best and the second-best prediction of every target, of any class subset,
    differ by more than that or are both 0);
  * every recorded mAP array has an entry strictly between 0 and 100.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

CLASSES = [0, 1, 2]
DIFFICULTIES = [0, 1, 2]
OVERLAP_A = [0.5, 0.5, 0.7]  # KITTI: pedestrian, cyclist, car
OVERLAP_B = [0.25, 0.25, 0.5]
SIMILAR = {2: 3}
THRESHOLDS = sorted(set(OVERLAP_A + OVERLAP_B))
MARGIN = 1e-3
N_FRAMES = 8
SIZES = {0: (0.6, 1.7, 0.8), 1: (0.6, 1.7, 1.8), 2: (1.6, 1.5, 3.9), 3: (1.9, 2.0, 5.0), 4: (1.0, 1.0, 1.0)}  # w, h, l


# ---- float64 IoU ------------------------------------------------------------
def _corners(cx, cy, w, l, ry):
    c, s = np.cos(ry), np.sin(ry)
    out = []
    for dx, dy in ((-w / 2, -l / 2), (w / 2, -l / 2), (w / 2, l / 2), (-w / 2, l / 2)):
        out.append((dx * c + dy * s + cx, -dx * s + dy * c + cy))
    return out


def _signed_area(poly):
    a = 0.0
    for k in range(len(poly)):
        x0, y0 = poly[k]
        x1, y1 = poly[(k + 1) % len(poly)]
        a += x0 * y1 - x1 * y0
    return 0.5 * a


def _clip(subject, clipper):
    """Sutherland-Hodgman: subject polygon clipped by a convex, counter-
    clockwise clipper."""
    out = subject
    for k in range(len(clipper)):
        if not out:
            break
        ax, ay = clipper[k]
        bx, by = clipper[(k + 1) % len(clipper)]
        side = lambda p: (bx - ax) * (p[1] - ay) - (by - ay) * (p[0] - ax)  # noqa: E731
        inp, out = out, []
        for m in range(len(inp)):
            p, q = inp[m], inp[(m + 1) % len(inp)]
            sp, sq = side(p), side(q)
            if sp >= 0:
                out.append(p)
            if (sp > 0 and sq < 0) or (sp < 0 and sq > 0):
                t = sp / (sp - sq)
                out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
    return out


def _overlap_area(a, b):
    """a, b: (cx, cy, w, l, ry) in float64."""
    pa, pb = _corners(*a), _corners(*b)
    if _signed_area(pa) < 0:
        pa = pa[::-1]
    if _signed_area(pb) < 0:
        pb = pb[::-1]
    inter = _clip(pa, pb)
    return abs(_signed_area(inter)) if len(inter) > 2 else 0.0


def iou_bev64(boxes, qboxes):
    boxes, qboxes = np.asarray(boxes, np.float64), np.asarray(qboxes, np.float64)
    out = np.zeros((len(boxes), len(qboxes)))
    for i, a in enumerate(boxes):
        for j, b in enumerate(qboxes):
            inter = _overlap_area(a, b)
            out[i, j] = inter / max(a[2] * a[3] + b[2] * b[3] - inter, 1e-8)
    return out


def iou_3d64(boxes, qboxes):
    boxes, qboxes = np.asarray(boxes, np.float64), np.asarray(qboxes, np.float64)
    out = np.zeros((len(boxes), len(qboxes)))
    for i, a in enumerate(boxes):
        for j, b in enumerate(qboxes):
            area = _overlap_area(a[[0, 2, 3, 5, 6]], b[[0, 2, 3, 5, 6]])
            height = max(min(a[1], b[1]) - max(a[1] - a[4], b[1] - b[4]), 0.0)
            ov = area * height
            out[i, j] = ov / max(a[3] * a[4] * a[5] + b[3] * b[4] * b[5] - ov, 1e-8)
    return out


# ---- inputs -----------------------------------------------------------------
def _box(rng, label, x, z):
    w, h, l = np.asarray(SIZES[label]) * rng.uniform(0.85, 1.15, 3)
    return [x, rng.uniform(1.2, 2.0), z, w, h, l, rng.uniform(-np.pi, np.pi)]


def make_frames(seed):
    rng = np.random.default_rng(seed)
    pred, target = [], []
    for f in range(N_FRAMES):
        labels = list(rng.choice([0, 1, 2, 2, 2, 3, 4], size=int(rng.integers(7, 12))))
        if f == 3:
            labels = [c for c in labels if c != 1]
        if f == 5:
            labels = []
        # targets on a jittered grid (a few of them close enough to overlap)
        cells = rng.permutation(30)[:len(labels)]
        tb = [_box(rng, c, -18 + 7.0 * (k % 6) + rng.uniform(-2, 2), 8 + 7.0 * (k // 6) + rng.uniform(-2, 2))
              for c, k in zip(labels, cells)]
        tb = np.asarray(tb, np.float32).reshape(-1, 7)
        tl = np.asarray(labels, np.int64)
        td = rng.choice([-1, 0, 0, 1, 1, 2, 2], size=len(labels)).astype(np.int64)
        pb, pl, ps, pd = [], [], [], []
        if f != 2:
            for b, c, d in zip(tb, tl, td):
                if c == 4 or rng.random() < 0.15:  # missed
                    continue
                level = rng.choice([0.3, 1.0, 2.5])  # good, fair, poor localisation
                j = b.astype(np.float64).copy()
                j[[0, 2]] += rng.normal(0, 0.12 * level, 2)
                j[1] += rng.normal(0, 0.05 * level)
                j[3:6] *= 1 + rng.normal(0, 0.04 * level, 3)
                j[6] += rng.normal(0, 0.06 * level)
                pb.append(j)
                pl.append(int(c) if c != 3 else 2)  # the similar class is predicted as the class
                ps.append(rng.uniform(0.3, 1.0))
                pd.append(int(d))
                if rng.random() < 0.2:  # a duplicate detection, lower score
                    k = j.copy()
                    k[[0, 2]] += rng.normal(0, 0.3, 2)
                    pb.append(k)
                    pl.append(pl[-1])
                    ps.append(rng.uniform(0.05, 0.5))
                    pd.append(int(d))
            for _ in range(int(rng.integers(3, 7))):  # clutter
                c = int(rng.choice([0, 1, 2, 4]))
                if f == 3 and c == 1:
                    c = 0
                pb.append(_box(rng, c, rng.uniform(-22, 22), rng.uniform(5, 45)))
                pl.append(c)
                ps.append(rng.uniform(0.05, 0.9))
                pd.append(int(rng.choice([-1, 0, 1, 2])))
        pred.append({"bbox": np.asarray(pb, np.float32).reshape(-1, 7), "label": np.asarray(pl, np.int64),
                     "score": np.asarray(ps, np.float32), "difficulty": np.asarray(pd, np.int64)})
        target.append({"bbox": tb, "label": tl, "difficulty": td})
    return pred, target


def check_margins(mats):
    for m in mats:
        assert not np.any(np.abs(m[..., None] - np.asarray(THRESHOLDS)) < MARGIN), "IoU near a threshold"
        assert not np.any((m > 0) & (m < MARGIN)), "IoU in (0, 1e-3)"
        for col in m.T:
            nz = np.sort(col[col > 0])
            assert not np.any(np.diff(nz) <= MARGIN), "two predictions tie on a target"


def main():
    import ref_loader
    ref_loader.install()
    import open3d.ml.contrib as contrib
    contrib.iou_bev_cpu = lambda a, b: iou_bev64(a, b)
    contrib.iou_3d_cpu = lambda a, b: iou_3d64(a, b)
    from ml3d.metrics import mAP
    import oracle as O

    cases = {
        "map_bev_a": dict(min_overlap=OVERLAP_A, bev=True),
        "map_3d_a": dict(min_overlap=OVERLAP_A, bev=False),
        "map_bev_b": dict(min_overlap=OVERLAP_B, bev=True),
        "map_3d_b": dict(min_overlap=OVERLAP_B, bev=False),
        "map_bev_similar": dict(min_overlap=OVERLAP_A, bev=True, similar_classes=SIMILAR),
        "map_3d_similar": dict(min_overlap=OVERLAP_A, bev=False, similar_classes=SIMILAR),
    }
    for seed in range(2024, 2024 + 200):
        pred, target = make_frames(seed)
        bev = [iou_bev64(p["bbox"][:, [0, 2, 3, 5, 6]], t["bbox"][:, [0, 2, 3, 5, 6]]) for p, t in zip(pred, target)]
        i3d = [iou_3d64(p["bbox"], t["bbox"]) for p, t in zip(pred, target)]
        try:
            check_margins(bev + i3d)
            maps = {k: mAP(pred, target, classes=CLASSES, difficulties=DIFFICULTIES, samples=41, **kw)
                    for k, kw in cases.items()}
            for k, v in maps.items():
                assert v.shape == (3, 3, 1) and np.any((v > 0) & (v < 100)), f"{k} has no entry inside (0, 100)"
        except AssertionError as e:
            print(f"seed {seed}: {e}")
            continue
        break
    else:
        raise SystemExit("no seed satisfied the margins")

    # the oracle's float32 routine against float64 on the fixture's BEV pairs
    worst = 0.0
    for p, t, m in zip(pred, target, bev):
        for i, a in enumerate(p["bbox"][:, [0, 2, 3, 5, 6]]):
            for j, b in enumerate(t["bbox"][:, [0, 2, 3, 5, 6]]):
                ra = np.array([a[0] - a[2] / 2, a[1] - a[3] / 2, a[0] + a[2] / 2, a[1] + a[3] / 2, a[4]], np.float32)
                rb = np.array([b[0] - b[2] / 2, b[1] - b[3] / 2, b[0] + b[2] / 2, b[1] + b[3] / 2, b[4]], np.float32)
                v = O.bev_iou(ra, rb)
                assert (v != 0) == (m[i, j] != 0), "oracle and float64 disagree on zero / nonzero"
                worst = max(worst, abs(v - m[i, j]))
    iou_tol = 4 * worst

    rs = lambda frames: np.concatenate([[0], np.cumsum([len(x["label"]) for x in frames])]).astype(np.int64)  # noqa: E731
    cat = lambda frames, k: np.concatenate([x[k] for x in frames])  # noqa: E731
    flat_bev, flat_3d = np.concatenate([m.ravel() for m in bev]), np.concatenate([m.ravel() for m in i3d])
    out = dict(
        seed=np.int64(seed), classes=np.asarray(CLASSES), difficulties=np.asarray(DIFFICULTIES),
        min_overlap_a=np.asarray(OVERLAP_A), min_overlap_b=np.asarray(OVERLAP_B),
        similar_from=np.asarray(list(SIMILAR.keys())), similar_to=np.asarray(list(SIMILAR.values())),
        pred_row_splits=rs(pred), pred_bbox=cat(pred, "bbox"), pred_label=cat(pred, "label"),
        pred_score=cat(pred, "score"), pred_difficulty=cat(pred, "difficulty"),
        target_row_splits=rs(target), target_bbox=cat(target, "bbox"), target_label=cat(target, "label"),
        target_difficulty=cat(target, "difficulty"),
        iou_offsets=np.concatenate([[0], np.cumsum([m.size for m in bev])]).astype(np.int64),
        iou_bev64=flat_bev, iou_3d64=flat_3d, nonzero_bev=flat_bev != 0, nonzero_3d=flat_3d != 0,
        iou_tol=np.float64(iou_tol), oracle_worst_err=np.float64(worst), **maps)
    path = os.path.join(HERE, "detection_eval.npz")
    np.savez_compressed(path, **out)
    print(f"seed {seed}: {len(flat_bev)} pairs, {int((flat_bev != 0).sum())} overlapping in BEV, "
          f"{int((flat_3d != 0).sum())} in 3D; oracle worst |err| {worst:.3e}, iou_tol {iou_tol:.3e}")
    for k, v in maps.items():
        print(k, np.round(v[..., 0], 3).tolist())
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
