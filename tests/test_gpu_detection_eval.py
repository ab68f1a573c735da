"""Rotated-box IoU kernel (csrc/box_iou.hip) and the GPU path of
o3dml_amd.metrics.mAP on the MI355X.

The kernel and the host routine compile the same float32 routine
(csrc/box_iou.hpp); they can differ only through the device's sinf / cosf /
atan2f, which the fixture's `iou_tol` (4 x the float32 algorithm's own error
against float64 on the fixture's pairs) is sized to cover.  The seeded boxes
are drawn with KITTI-like coordinates (|x| <= 25, z <= 47, as the fixture's)
and, as in the fixture's generator, so that no IoU lies in (0, 1e-3), none
within 1e-3 of a threshold in use and no two nonzero IoUs of one column within
1e-3 of each other — a rounding difference then cannot flip a zero mask."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "detection_eval.npz")
BEV_COLUMNS = [0, 2, 3, 5, 6]
THRESHOLDS = np.array([0.25, 0.5, 0.7])
MARGIN = 1e-3
SIZES = [(1, 1), (63, 65), (64, 64), (130, 257)]


@pytest.fixture(scope="module")
def G():
    return dict(np.load(GOLDEN))


def _column_ok(col):
    nz = np.sort(col[col != 0].astype(np.float64))
    return not (np.any(nz < MARGIN) or np.any(np.abs(nz[:, None] - THRESHOLDS) < MARGIN) or np.any(np.diff(nz) <= MARGIN))


def _rand_box(rng, cx, cz):
    return [cx + rng.uniform(-0.7, 0.7), rng.uniform(0.0, 3.0), cz + rng.uniform(-0.7, 0.7), rng.uniform(0.6, 2.0),
            rng.uniform(1.0, 2.0), rng.uniform(0.8, 4.0), rng.uniform(-np.pi, np.pi)]


def make_sets(n, m, seed):
    """a [n,7], b [m,7] (x,y,z,w,h,l,ry): a's boxes sit two to a cell of a
    6 m grid (boxes of different cells are disjoint), every b box is drawn
    into a random occupied cell until its column of host IoUs, BEV and 3D,
    satisfies the margins; three b boxes in four must overlap some a box."""
    from o3dml_amd.contrib import iou_3d_cpu, iou_bev_cpu
    rng = np.random.default_rng(seed)
    cells = [(-24 + 6.0 * (k % 9), 4 + 6.0 * (k // 9)) for k in range(72)]
    a = np.asarray([_rand_box(rng, *cells[i // 2]) for i in range(n)], np.float32)
    b = np.zeros((m, 7), np.float32)
    for j in range(m):
        for _ in range(200):
            cand = np.asarray([_rand_box(rng, *cells[int(rng.integers(0, (n + 1) // 2))])], np.float32)
            bev = iou_bev_cpu(a[:, BEV_COLUMNS], cand[:, BEV_COLUMNS])[:, 0]
            if (j % 4 == 3 or bev.any()) and _column_ok(bev) and _column_ok(iou_3d_cpu(a, cand)[:, 0]):
                break
        else:
            raise AssertionError("no box satisfied the margins")
        b[j] = cand[0]
    return a, b


@pytest.fixture(scope="module")
def sets():
    """Seeded box sets and their host IoUs, computed once."""
    from o3dml_amd.contrib import iou_3d_cpu, iou_bev_cpu
    out = {}
    for k, (n, m) in enumerate(SIZES):
        a, b = make_sets(n, m, 100 + k)
        out[(n, m)] = (a, b, iou_bev_cpu(a[:, BEV_COLUMNS], b[:, BEV_COLUMNS]), iou_3d_cpu(a, b))
    return out


def _close(got, ref, tol, what):
    assert got.shape == ref.shape and got.dtype == np.float32
    assert np.array_equal(got != 0, ref != 0), what + ": zero masks differ"
    err = float(np.abs(got.astype(np.float64) - ref).max()) if ref.size else 0.0
    print(what, "max |gpu - ref| =", err, "tol", tol, "nonzero", int((ref != 0).sum()), "of", ref.size)
    assert err <= tol


@pytest.mark.parametrize("n,m", SIZES)
def test_cuda_matches_host(cuda, G, sets, n, m):
    from o3dml_amd.contrib import iou_3d_cuda, iou_bev_cuda
    a, b, ref_bev, ref_3d = sets[(n, m)]
    tol = float(G["iou_tol"])
    assert (ref_bev != 0).sum() >= max(1, 3 * m // 4)  # the sets do overlap
    _close(iou_bev_cuda(a[:, BEV_COLUMNS], b[:, BEV_COLUMNS]), ref_bev, tol, f"bev {n}x{m}")
    _close(iou_3d_cuda(a, b), ref_3d, tol, f"3d {n}x{m}")


def test_cuda_matches_fixture_float64(cuda, G):
    from o3dml_amd.contrib import iou_3d_cuda, iou_bev_cuda
    prs, trs, off, tol = G["pred_row_splits"], G["target_row_splits"], G["iou_offsets"], float(G["iou_tol"])
    for f in range(len(prs) - 1):
        p, t = G["pred_bbox"][prs[f]:prs[f + 1]], G["target_bbox"][trs[f]:trs[f + 1]]
        shape = (len(p), len(t))
        _close(iou_bev_cuda(p[:, BEV_COLUMNS], t[:, BEV_COLUMNS]), G["iou_bev64"][off[f]:off[f + 1]].reshape(shape), tol,
               f"bev frame {f}")
        _close(iou_3d_cuda(p, t), G["iou_3d64"][off[f]:off[f + 1]].reshape(shape), tol, f"3d frame {f}")


def test_batched_is_per_frame(cuda):
    """Frames 0x3, 3x0, 1x1, 70x9, 9x70, 64x64 in one launch: bit-identical to
    per-frame calls and across two runs."""
    from o3dml_amd import contrib
    rng = np.random.default_rng(7)
    shapes = [(0, 3), (3, 0), (1, 1), (70, 9), (9, 70), (64, 64)]

    def boxes(k):  # clutter in one small area: about one pair in five overlaps
        return np.asarray([_rand_box(rng, rng.uniform(-3, 3), rng.uniform(10, 16)) for _ in range(k)],
                          np.float32).reshape(-1, 7)

    a, b = [boxes(n) for n, _ in shapes], [boxes(m) for _, m in shapes]
    a_rs = np.concatenate([[0], np.cumsum([n for n, _ in shapes])])
    b_rs = np.concatenate([[0], np.cumsum([m for _, m in shapes])])
    A, B = np.concatenate(a), np.concatenate(b)
    for cols, batch, one in ((BEV_COLUMNS, contrib.iou_bev_batch, contrib.iou_bev_cuda),
                             (list(range(7)), contrib.iou_3d_batch, contrib.iou_3d_cuda)):
        first = batch(A[:, cols], a_rs, B[:, cols], b_rs)
        again = batch(A[:, cols], a_rs, B[:, cols], b_rs)
        assert len(first) == len(shapes)
        for f, shape in enumerate(shapes):
            assert first[f].shape == shape and first[f].dtype == np.float32
            assert first[f].tobytes() == again[f].tobytes()
            assert first[f].tobytes() == one(a[f][:, cols], b[f][:, cols]).tobytes()
        assert (first[5] != 0).any() and (first[5] == 0).any()  # overlapping and disjoint pairs both occur


def test_nan_rows_leave_the_rest_alone(cuda, G, sets):
    """A set with NaN / inf rows returns, and the finite rows' values are those
    of the call without them (bitwise) and the host routine's (iou_tol)."""
    from o3dml_amd.contrib import iou_3d_cuda, iou_bev_cuda
    a, b, ref_bev, ref_3d = sets[(63, 65)]
    tol = float(G["iou_tol"])
    odd = np.array([[np.nan] * 7, [0, 1, 10, np.inf, 1, 2, 0], [0, 1, 10, 1, 1, 2, np.nan], [0, 1, 10, 0, 0, 0, 0],
                    [0, 1, 10, -1, -1, -2, 0.5]], np.float32)
    a2, b2 = np.concatenate([a[:30], odd, a[30:]]), np.concatenate([odd[:2], b])
    rows = np.r_[0:30, 35:68]
    for cols, fn, ref in ((BEV_COLUMNS, iou_bev_cuda, ref_bev), (list(range(7)), iou_3d_cuda, ref_3d)):
        clean, mixed = fn(a[:, cols], b[:, cols]), fn(a2[:, cols], b2[:, cols])
        assert mixed.shape == (68, 67)
        kept = mixed[rows][:, 2:]
        assert kept.tobytes() == clean.tobytes()
        _close(kept, ref, tol, "finite rows")
        assert mixed.tobytes() == fn(a2[:, cols], b2[:, cols]).tobytes()  # deterministic, whatever the odd values


@pytest.mark.parametrize("key,overlap,bev,similar", [
    ("map_bev_a", "min_overlap_a", True, False), ("map_3d_a", "min_overlap_a", False, False),
    ("map_bev_b", "min_overlap_b", True, False), ("map_3d_b", "min_overlap_b", False, False),
    ("map_bev_similar", "min_overlap_a", True, True), ("map_3d_similar", "min_overlap_a", False, True)])
def test_map_gpu_path(cuda, G, key, overlap, bev, similar, monkeypatch):
    from o3dml_amd import contrib, metrics
    assert metrics._use_gpu()
    calls = []
    for name in ("iou_bev_batch", "iou_3d_batch"):
        real = getattr(contrib, name)
        monkeypatch.setattr(contrib, name, lambda *a, _real=real, _name=name: calls.append(_name) or _real(*a))
    prs, trs = G["pred_row_splits"], G["target_row_splits"]
    pred = [{"bbox": G["pred_bbox"][s:e], "label": G["pred_label"][s:e], "score": G["pred_score"][s:e],
             "difficulty": G["pred_difficulty"][s:e]} for s, e in zip(prs[:-1], prs[1:])]
    target = [{"bbox": G["target_bbox"][s:e], "label": G["target_label"][s:e],
               "difficulty": G["target_difficulty"][s:e]} for s, e in zip(trs[:-1], trs[1:])]
    sim = dict(zip(G["similar_from"].tolist(), G["similar_to"].tolist())) if similar else {}
    got = metrics.mAP(pred, target, classes=G["classes"].tolist(), difficulties=G["difficulties"].tolist(),
                      min_overlap=G[overlap].tolist(), bev=bev, samples=41, similar_classes=sim)
    err = np.abs(got - G[key]).max()
    print(key, "max |mAP - reference| =", err)
    assert calls == ["iou_bev_batch" if bev else "iou_3d_batch"]  # one batched call for all frames
    assert err <= 1e-9


def test_reference_import_forms_pick_the_gpu(cuda):
    """ml3d/metrics/__init__.py:3-6 with a GPU visible: device_count() > 0 and
    the `_cuda` names, which are the kernel-backed functions."""
    import open3d
    import o3dml_amd
    assert open3d.core.cuda.device_count() > 0
    from open3d.ml.contrib import iou_3d_cuda as iou_3d
    from open3d.ml.contrib import iou_bev_cuda as iou_bev
    assert iou_bev is o3dml_amd.contrib.iou_bev_cuda and iou_3d is o3dml_amd.contrib.iou_3d_cuda
    sq = np.array([[0, 0, 1, 1, 0]], np.float32)
    assert iou_bev(sq, sq)[0, 0] == pytest.approx(1.0, abs=1e-6)
    assert iou_bev(sq, sq + np.float32([10, 0, 0, 0, 0]))[0, 0] == 0.0
