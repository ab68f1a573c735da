"""Rotated-box IoU (host routine) and detection mAP, without a GPU.

The contract is csrc/box_iou.hpp's (positional, restated from Open3D).  Pinned
by known answers, by the float64 polygon-clip matrices of
tests/golden/detection_eval.npz (make_golden_detection_eval.py: Sutherland-
Hodgman, independent of the library's routine) within the fixture's `iou_tol`
(4 x the oracle's own float32 error on those pairs), and by the oracle's
float32 orc_bev_iou.  o3dml_amd.metrics.mAP is held to the reference's
ml3d.metrics.mAP run on the float64 matrices: the fixture keeps every IoU
1e-3 away from the thresholds and from ties, so the float32 overlaps decide
every match as the float64 ones do and the results agree to rounding."""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "detection_eval.npz")
BEV_COLUMNS = [0, 2, 3, 5, 6]


@pytest.fixture(scope="module")
def G():
    return dict(np.load(GOLDEN))


def frames_of(G):
    pred, target = [], []
    prs, trs = G["pred_row_splits"], G["target_row_splits"]
    for f in range(len(prs) - 1):
        p, t = slice(prs[f], prs[f + 1]), slice(trs[f], trs[f + 1])
        pred.append({"bbox": G["pred_bbox"][p], "label": G["pred_label"][p], "score": G["pred_score"][p],
                     "difficulty": G["pred_difficulty"][p]})
        target.append({"bbox": G["target_bbox"][t], "label": G["target_label"][t],
                       "difficulty": G["target_difficulty"][t]})
    return pred, target


MAP_CASES = [("map_bev_a", "min_overlap_a", True, False), ("map_3d_a", "min_overlap_a", False, False),
             ("map_bev_b", "min_overlap_b", True, False), ("map_3d_b", "min_overlap_b", False, False),
             ("map_bev_similar", "min_overlap_a", True, True), ("map_3d_similar", "min_overlap_a", False, True)]


def check_map(G, key, overlap, bev, similar):
    from o3dml_amd import metrics
    pred, target = frames_of(G)
    sim = dict(zip(G["similar_from"].tolist(), G["similar_to"].tolist())) if similar else {}
    got = metrics.mAP(pred, target, classes=G["classes"].tolist(), difficulties=G["difficulties"].tolist(),
                      min_overlap=G[overlap].tolist(), bev=bev, samples=41, similar_classes=sim)
    assert got.shape == (3, 3, 1) and got.dtype == np.float64
    err = np.abs(got - G[key]).max()
    print(key, "max |mAP - reference| =", err)
    assert err <= 1e-9


def test_bev_known_answers():
    from o3dml_amd.contrib import iou_bev_cpu
    sq = [[0, 0, 1, 1, 0]]
    assert iou_bev_cpu(sq, sq)[0, 0] == pytest.approx(1.0, abs=1e-6)
    octagon = 2 * (np.sqrt(2) - 1)  # unit square against itself turned 45 degrees
    assert iou_bev_cpu(sq, [[0, 0, 1, 1, np.pi / 4]])[0, 0] == pytest.approx(octagon / (2 - octagon), abs=1e-6)
    far = iou_bev_cpu(sq, [[10, 10, 1, 1, 0.3], [0, 3, 1, 1, 0]])
    assert far.dtype == np.float32 and far.shape == (1, 2) and np.all(far == 0.0)


def test_3d_known_answers():
    from o3dml_amd.contrib import iou_3d_cpu
    # (x, y, z, w, h, l, ry), y the bottom face; axis-aligned, so the answer is interval arithmetic
    a = [1.0, 1.0, 2.0, 2.0, 2.0, 4.0, 0.0]   # x [0,2], y [-1,1], z [0,4]
    b = [2.0, 1.5, 3.0, 2.0, 3.0, 4.0, 0.0]   # x [1,3], y [-1.5,1.5], z [1,5]
    ov = 1.0 * 2.0 * 3.0  # x [1,2], y [-1,1], z [1,4]
    want = ov / (2 * 2 * 4 + 2 * 3 * 4 - ov)
    assert iou_3d_cpu([a], [b])[0, 0] == pytest.approx(want, abs=1e-6)
    assert iou_3d_cpu([a], [a])[0, 0] == pytest.approx(1.0, abs=1e-6)
    stacked = [1.0, 3.5, 2.0, 2.0, 2.0, 4.0, 0.0]  # same footprint, y [1.5, 3.5]
    assert iou_3d_cpu([a], [stacked])[0, 0] == 0.0
    assert iou_3d_cpu([a], [[30.0, 1.0, 2.0, 2.0, 2.0, 4.0, 0.5]])[0, 0] == 0.0


def test_fixture_iou(G):
    import oracle as O
    from o3dml_amd.contrib import iou_3d_cpu, iou_bev_cpu
    pred, target = frames_of(G)
    tol, off = float(G["iou_tol"]), G["iou_offsets"]
    assert 0 < tol < 1e-4
    worst = {"bev": 0.0, "3d": 0.0, "oracle": 0.0}
    for f, (p, t) in enumerate(zip(pred, target)):
        shape = (len(p["bbox"]), len(t["bbox"]))
        pb, tb = p["bbox"][:, BEV_COLUMNS], t["bbox"][:, BEV_COLUMNS]
        for name, got, key in (("bev", iou_bev_cpu(pb, tb), "iou_bev64"), ("3d", iou_3d_cpu(p["bbox"], t["bbox"]), "iou_3d64")):
            ref = G[key][off[f]:off[f + 1]].reshape(shape)
            assert got.shape == shape and got.dtype == np.float32
            assert np.array_equal(got != 0, ref != 0)
            assert np.array_equal(got != 0, G["nonzero_" + name][off[f]:off[f + 1]].reshape(shape))
            if ref.size:
                worst[name] = max(worst[name], np.abs(got - ref).max())
        rect = lambda b: np.stack([b[:, 0] - b[:, 2] / 2, b[:, 1] - b[:, 3] / 2, b[:, 0] + b[:, 2] / 2,  # noqa: E731
                                   b[:, 1] + b[:, 3] / 2, b[:, 4]], axis=1).astype(np.float32)
        got, ra, rb = iou_bev_cpu(pb, tb), rect(pb), rect(tb)
        for i in range(shape[0]):
            for j in range(shape[1]):
                worst["oracle"] = max(worst["oracle"], abs(float(got[i, j]) - O.bev_iou(ra[i], rb[j])))
    print("worst |host - float64|:", worst, "iou_tol", tol)
    assert worst["bev"] <= tol and worst["3d"] <= tol
    assert worst["oracle"] <= 1e-6


def test_edges():
    import torch
    from o3dml_amd import contrib
    rng = np.random.default_rng(0)
    for w, fn in ((5, contrib.iou_bev_cpu), (7, contrib.iou_3d_cpu)):
        b = rng.uniform(0.5, 2.0, (4, w)).astype(np.float32)
        for n, m in ((0, 4), (4, 0), (0, 0)):
            out = fn(b[:n], b[:m])
            assert out.shape == (n, m) and out.dtype == np.float32
        ref = fn(b, b)
        assert np.array_equal(fn(b.astype(np.float64), b.tolist()), ref)
        wide = np.zeros((4, 2 * w), np.float32)
        wide[:, ::2] = b
        view = wide[:, ::2]
        assert not view.flags.c_contiguous
        assert np.array_equal(fn(view, np.asfortranarray(b)), ref)
        for bad in (np.zeros((3, w + 1)), np.zeros((3, w - 1)), np.zeros(w), np.zeros((1, 3, w))):
            with pytest.raises(RuntimeError):
                fn(bad, b)
            with pytest.raises(RuntimeError):
                fn(b, bad)
    if not torch.cuda.is_available():
        for fn, w in ((contrib.iou_bev_cuda, 5), (contrib.iou_3d_cuda, 7)):
            with pytest.raises(RuntimeError, match="no ROCm GPU"):
                fn(np.ones((2, w), np.float32), np.ones((3, w), np.float32))
        with pytest.raises(RuntimeError, match="no ROCm GPU"):
            contrib.iou_bev_batch(np.ones((2, 5), np.float32), [0, 2], np.ones((3, 5), np.float32), [0, 3])


def test_host_routine_survives_odd_floats():
    """NaN, inf, zero and negative sizes: the call returns (bounded loops) and
    the finite rows' values are those of a call without the odd rows."""
    from o3dml_amd.contrib import iou_3d_cpu, iou_bev_cpu
    good = np.array([[0, 0, 2, 1, 0.3], [0.5, 0.2, 1, 2, -1.0]], np.float32)
    odd = np.array([[np.nan, 0, 1, 1, 0], [0, 0, np.inf, 1, 0], [0, 0, 0, 0, 0], [0, 0, -1, -2, 0.5],
                    [0, 0, 1, 1, np.inf], [np.inf, -np.inf, np.nan, 1e38, 1e38]], np.float32)
    both = np.concatenate([good, odd])
    assert np.array_equal(iou_bev_cpu(both, both)[:2, :2], iou_bev_cpu(good, good))
    pad = lambda b: np.stack([b[:, 0], b[:, 1], b[:, 1], b[:, 2], b[:, 3], b[:, 3], b[:, 4]], 1)  # noqa: E731
    assert np.array_equal(iou_3d_cpu(pad(both), pad(both))[:2, :2], iou_3d_cpu(pad(good), pad(good)))


@pytest.mark.parametrize("key,overlap,bev,similar", MAP_CASES)
def test_map_matches_reference(G, key, overlap, bev, similar, monkeypatch):
    """The host path (what a machine without a GPU takes)."""
    from o3dml_amd import metrics
    monkeypatch.setattr(metrics, "_use_gpu", lambda: False)
    check_map(G, key, overlap, bev, similar)


def test_map_quirks(G, monkeypatch):
    from o3dml_amd import metrics
    monkeypatch.setattr(metrics, "_use_gpu", lambda: False)
    pred, target = frames_of(G)
    kw = dict(classes=[0, 1, 2], difficulties=[0, 1, 2], min_overlap=[0.5])
    assert np.array_equal(metrics.mAP(pred, target, samples=0, **kw), np.zeros((3, 3, 1)))
    # a single min_overlap is used for every class
    assert np.array_equal(metrics.mAP(pred, target, **kw), metrics.mAP(pred, target, **dict(kw, min_overlap=[0.5] * 3)))
    det, fns = metrics.precision_3d(pred[0], target[0], **kw)
    n = int(np.isin(pred[0]["label"], [0, 1, 2]).sum())
    assert det.shape == (3, 3, n, 3) and fns.shape == (3, 3, 1) and fns.dtype == np.int64
    assert set(np.unique(det[..., 1:])) <= {0.0, 1.0} and not np.any((det[..., 1] == 1) & (det[..., 2] == 1))
    # a frame without predictions: every target of the class / difficulty is missed
    det, fns = metrics.precision_3d(pred[2], target[2], **kw)
    assert det.shape == (3, 3, 0, 3)
    t = target[2]
    for i in range(3):
        for j in range(3):
            assert fns[i, j, 0] == np.sum((t["label"] == i) & (t["difficulty"] >= 0) & (t["difficulty"] <= j))


def test_shim_exports_iou():
    import open3d.ml.contrib as shim
    import o3dml_amd
    for name in ("iou_bev_cpu", "iou_3d_cpu", "iou_bev_cuda", "iou_3d_cuda"):
        assert getattr(shim, name) is getattr(o3dml_amd.contrib, name) and callable(getattr(shim, name))
    assert shim.iou_bev_cpu([[0, 0, 1, 1, 0]], [[0, 0, 1, 1, 0]])[0, 0] == pytest.approx(1.0, abs=1e-6)


_REFERENCE_MAP = r"""
import sys
import numpy as np
import open3d  # OPEN3D_ML_ROOT puts the checkout's ml3d on sys.path
from ml3d.metrics import mAP, iou_bev, iou_3d
import o3dml_amd
cpu = open3d.core.cuda.device_count() == 0
assert iou_bev is (o3dml_amd.contrib.iou_bev_cpu if cpu else o3dml_amd.contrib.iou_bev_cuda)
assert iou_3d is (o3dml_amd.contrib.iou_3d_cpu if cpu else o3dml_amd.contrib.iou_3d_cuda)
G = dict(np.load(sys.argv[1]))
prs, trs = G["pred_row_splits"], G["target_row_splits"]
pred = [{"bbox": G["pred_bbox"][s:e], "label": G["pred_label"][s:e], "score": G["pred_score"][s:e],
         "difficulty": G["pred_difficulty"][s:e]} for s, e in zip(prs[:-1], prs[1:])]
target = [{"bbox": G["target_bbox"][s:e], "label": G["target_label"][s:e],
           "difficulty": G["target_difficulty"][s:e]} for s, e in zip(trs[:-1], trs[1:])]
sim = dict(zip(G["similar_from"].tolist(), G["similar_to"].tolist()))
for key, overlap, bev, similar in (("map_bev_a", "min_overlap_a", True, {}), ("map_3d_b", "min_overlap_b", False, {}),
                                   ("map_3d_similar", "min_overlap_a", False, sim)):
    got = mAP(pred, target, classes=[0, 1, 2], difficulties=[0, 1, 2], min_overlap=G[overlap].tolist(), bev=bev,
              similar_classes=similar)
    assert np.abs(got - G[key]).max() <= 1e-9, (key, got, G[key])
print("reference mAP ok")
"""


@pytest.mark.skipif(not os.path.isdir("/root/reference/ml3d"),
                    reason="the reference checkout exists only in the build container")
def test_reference_map_runs_on_the_shim():
    """An Open3D-ML checkout's own `from ml3d.metrics import mAP`, bound to
    this build's open3d.ml.contrib IoU, reproduces the recorded results (which
    the same code gave with float64 overlaps)."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    env["PYTHONPATH"] = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "open3d-ml_amd")
    env["OPEN3D_ML_ROOT"] = "/root/reference"
    r = subprocess.run([sys.executable, "-c", _REFERENCE_MAP, GOLDEN], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "reference mAP ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
