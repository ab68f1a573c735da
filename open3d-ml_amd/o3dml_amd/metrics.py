"""Detection evaluation: ``precision_3d`` and ``mAP`` with the signatures and
return shapes of the reference's ``ml3d.metrics`` (metrics/mAP.py:38,164; the
validation loop object_detection.py:238-270 calls ``mAP``).

The reference computes one overlap matrix per frame, each a host -> device ->
host round trip.  ``mAP`` here filters every frame first, gets all frames'
overlap matrices from ONE batched IoU launch and one copy back
(contrib.iou_*_batch) when a GPU is visible, and from the host routine
(contrib.iou_*_cpu) otherwise — the choice ml3d.metrics makes at import —
then does the matching and the 41-point sampling on the host.

Behaviours of the reference kept on purpose:
  * a prediction is a true positive only if it is the ``argmax`` over ALL
    predictions of its class (any difficulty) for some target of the evaluated
    difficulty, and overlaps a target of that difficulty by >= min_overlap;
  * a prediction that overlaps no target of its class group (the class and its
    ``similar_classes`` partner, any difficulty) by min_overlap is a false
    positive; one that matches a target of the evaluated difficulty without
    being the best is a false positive too; one that only overlaps a similar
    class or another difficulty counts as neither;
  * difficulty d keeps boxes with 0 <= difficulty <= d (predictions too, when
    they carry a difficulty);
  * recall thresholds are sampled from the true positives' scores with the
    running ``1 / (samples - 1)`` recall step; the precision at a threshold is
    the running maximum from the right;
  * with at least ``int(samples / 4 + 1)`` entries in ``prec[::4]`` the result
    is ``sum(prec[::4]) / int(samples / 4 + 1) * 100``, otherwise the plain
    mean of ``prec``; ``samples <= 0`` gives zeros.
"""
import numpy as np
import torch

from . import contrib

_BEV_COLUMNS = [0, 2, 3, 5, 6]  # (x, z, w, l, ry) of (x, y, z, w, h, l, ry)


def _label_in(labels, wanted):
    keep = np.zeros(len(labels), bool)
    for w in wanted:
        if w is not None:
            keep |= labels == w
    return keep


def _within(data, diff):
    """Rows of difficulty 0..diff; every row when the data carry no difficulty."""
    if "difficulty" not in data:
        return np.ones(len(data["label"]), bool)
    d = np.asarray(data["difficulty"])
    return (d >= 0) & (d <= diff)


def _select(data, keep):
    return {k: np.asarray(v)[keep] for k, v in data.items()}


def _prefilter(pred, target, classes, similar_classes):
    """Predictions of the evaluated classes, targets of those and of the
    classes they are similar to."""
    pred = {k: np.asarray(v) for k, v in pred.items()}
    target = {k: np.asarray(v) for k, v in target.items()}
    p = _select(pred, _label_in(pred["label"], classes))
    t = _select(target, _label_in(target["label"], list(classes) + list(similar_classes.values())))
    return p, t


def _iou_rows(data, bev):
    box = np.asarray(data["bbox"], np.float32).reshape(-1, 7)
    return np.ascontiguousarray(box[:, _BEV_COLUMNS] if bev else box)


def _use_gpu():
    return torch.cuda.is_available() and torch.cuda.device_count() > 0


def _overlaps(frames, bev):
    """One [n_f, m_f] float32 overlap matrix per (pred, target) frame."""
    a = [_iou_rows(p, bev) for p, _ in frames]
    b = [_iou_rows(t, bev) for _, t in frames]
    if not _use_gpu():
        one = contrib.iou_bev_cpu if bev else contrib.iou_3d_cpu
        return [one(x, y) for x, y in zip(a, b)]
    width = 5 if bev else 7
    a_rs = np.concatenate([[0], np.cumsum([len(x) for x in a])]).astype(np.int64)
    b_rs = np.concatenate([[0], np.cumsum([len(x) for x in b])]).astype(np.int64)
    cat = lambda rows: np.concatenate(rows) if rows else np.zeros((0, width), np.float32)  # noqa: E731
    batch = contrib.iou_bev_batch if bev else contrib.iou_3d_batch
    return batch(cat(a), a_rs, cat(b), b_rs)


def _broadcast_overlap(min_overlap, classes):
    min_overlap = list(min_overlap)
    if len(min_overlap) != len(classes):
        assert len(min_overlap) == 1
        min_overlap = min_overlap * len(classes)
    return min_overlap


def _frame_rows(pred, target, overlap, classes, difficulties, min_overlap, similar_classes):
    """Matching of one prefiltered frame.  Returns rows[i][j], float64 [k, 3]
    (score, true positive, false positive) of the predictions of class i kept
    at difficulty j, and the false-negative counts int64 [C, D, 1]."""
    rows = [[np.zeros((0, 3)) for _ in difficulties] for _ in classes]
    fns = np.zeros((len(classes), len(difficulties), 1), np.int64)
    for i, label in enumerate(classes):
        p_of = np.flatnonzero(pred["label"] == label)
        t_of = np.flatnonzero(_label_in(target["label"], [label, similar_classes.get(label)]))
        ov = overlap[p_of][:, t_of]  # this class's predictions x its group's targets
        t_exact = target["label"][t_of] == label
        score = np.asarray(pred["score"])[p_of]
        p_data, t_data = _select(pred, p_of), _select(target, t_of)
        thr = min_overlap[i]
        for j, diff in enumerate(difficulties):
            p_idx = np.flatnonzero(_within(p_data, diff))
            t_idx = np.flatnonzero(t_exact & _within(t_data, diff))
            if len(p_idx) == 0:
                fns[i, j] = len(t_idx)
                continue
            ov_t = ov[:, t_idx]  # all predictions of the class x targets of this difficulty
            matched = (ov_t[p_idx] >= thr).any(axis=1)
            best = np.zeros(len(p_of), bool)
            best[np.argmax(ov_t, axis=0)] = True
            tp = matched & best[p_idx]
            fp = ((ov[p_idx] < thr).all(axis=1) | matched) & ~tp
            fns[i, j] = int((ov_t < thr).all(axis=0).sum())
            rows[i][j] = np.stack([score[p_idx].astype(np.float64), tp.astype(np.float64), fp.astype(np.float64)],
                                  axis=-1)
    return rows, fns


def precision_3d(pred, target, classes=[0], difficulties=[0], min_overlap=[0.5], bev=True, similar_classes={}):
    """Detection quantities of one frame.  pred / target: dicts of numpy
    arrays ('bbox' [N,7] (x,y,z,w,h,l,ry), 'label', 'difficulty'; pred also
    'score').  Returns (detection float64 [C, D, P, 3] holding (score, tp, fp)
    per prediction of the evaluated classes, rows not used by a class /
    difficulty left zero; false negatives int64 [C, D, 1])."""
    min_overlap = _broadcast_overlap(min_overlap, classes)
    p, t = _prefilter(pred, target, classes, similar_classes)
    overlap = _overlaps([(p, t)], bev)[0]
    rows, fns = _frame_rows(p, t, overlap, classes, difficulties, min_overlap, similar_classes)
    detection = np.zeros((len(classes), len(difficulties), len(p["label"]), 3))
    for i in range(len(classes)):
        for j in range(len(difficulties)):
            detection[i, j, :len(rows[i][j])] = rows[i][j]
    return detection, fns


def _sample_thresholds(scores, gt_cnt, samples):
    """Scores of the true positives at (about) equally spaced recall steps."""
    scores = np.sort(scores)[::-1]
    last = len(scores) - 1
    recall, out = 0, []
    for k, s in enumerate(scores):
        left = (k + 1) / gt_cnt
        right = (k + 2) / gt_cnt if k < last else left
        if k < last and (right - recall) < (recall - left):
            continue
        out.append(s)
        recall += 1 / (samples - 1.0)
    return out


def mAP(pred, target, classes=[0], difficulties=[0], min_overlap=[0.5], bev=True, samples=41, similar_classes={}):
    """Mean average precision over frames.  pred / target: lists (one entry
    per frame) of dicts as for precision_3d.  Returns float64 [C, D, 1], in
    percent."""
    classes, difficulties = list(classes), list(difficulties)
    min_overlap = _broadcast_overlap(min_overlap, classes)
    C, D = len(classes), len(difficulties)

    # 1. filter all frames
    frames = [_prefilter(p, t, classes, similar_classes) for p, t in zip(pred, target)]
    gt_cnt = np.zeros((C, D))
    for t in target:
        label = np.asarray(t["label"])
        for i, c in enumerate(classes):
            for j, d in enumerate(difficulties):
                gt_cnt[i, j] += np.count_nonzero((label == c) & _within(t, d))

    # 2. every frame's overlap matrix, one batched call
    overlaps = _overlaps(frames, bev)

    # 3. matching and sampling on the host
    per = [[[] for _ in range(D)] for _ in range(C)]
    for (p, t), ov in zip(frames, overlaps):
        rows, _ = _frame_rows(p, t, ov, classes, difficulties, min_overlap, similar_classes)
        for i in range(C):
            for j in range(D):
                if len(rows[i][j]):
                    per[i][j].append(rows[i][j])

    result = np.zeros((C, D, 1))
    if samples <= 0:
        return result
    want = int(samples / 4 + 1)
    for i in range(C):
        for j in range(D):
            det = np.concatenate(per[i][j]) if per[i][j] else np.zeros((0, 3))
            thresholds = _sample_thresholds(det[det[:, 1] > 0, 0], gt_cnt[i, j], samples)
            if not thresholds:
                continue
            prec = np.zeros(len(thresholds))
            for k in range(len(thresholds) - 1, -1, -1):
                at = det[:, 0] >= thresholds[k]
                tp, fp = det[at, 1].sum(), det[at, 2].sum()
                if tp + fp > 0:
                    prec[k] = tp / (tp + fp)
                if k + 1 < len(prec):
                    prec[k] = max(prec[k], prec[k + 1])
            if len(prec[::4]) < want:
                result[i, j] = np.sum(prec) / len(prec) * 100
            else:
                result[i, j] = np.sum(prec[::4]) / want * 100
    return result


__all__ = ["precision_3d", "mAP"]
