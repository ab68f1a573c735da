"""PointRCNN on the GPU: one eval() forward on the fixture of the reference's
float64 run (tests/golden/point_rcnn.npz, weights from prcnn_weights.py),
checked stage by stage in the order the stages run, so a flipped discrete
choice fails where it happens.  Continuous comparisons use the project's bound:
relative error (largest difference over largest magnitude) at most
max(8 x the reference's own float32-vs-float64 error stored for that tensor,
1e-4)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def bound(G, name):
    return max(8.0 * float(G["err_" + name]), 1e-4)


def n(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def run(cuda):
    """The fixture, the model on the GPU and the results of one forward in
    each mode, shared by the tests of this file and left unchanged."""
    import prcnn_weights
    from o3dml_amd.point_rcnn import PointRCNN
    G = np.load(os.path.join(GOLDEN, "point_rcnn.npz"))
    cfg = json.loads(str(G["config"]))
    cfg = {k: cfg[k] for k in ("classes", "score_thres", "npoints", "rpn", "rcnn")}
    model = PointRCNN(**cfg)
    model.load_state_dict(prcnn_weights.state_dict_for(model), strict=True)
    model = model.to(cuda).eval()
    points = torch.from_numpy(G["points"]).to(cuda)
    model.mode = "RPN"
    rpn = model(points)
    model.mode = "RCNN"
    out = model(points)
    state = dict(fps=n(model.rpn.backbone.SA_modules[0].sampled), roi_scores=n(model.roi_scores),
                 pool_idx=n(model.rcnn.pool_index), pool_flag=n(model.rcnn.pool_empty_flag),
                 final=model.get_bboxes(out))
    return G, model, points, rpn, out, state


def test_stage1_fps_rows(run):
    G, _, _, _, _, state = run
    assert state["fps"].dtype == np.int32 and np.array_equal(state["fps"], G["fps_level1"])


def test_stage2_rpn_cls_and_reg(run):
    G, _, _, rpn, _, _ = run
    step = int(G["row_step"])
    assert tuple(rpn["cls"].shape) == (2, 2048, 1) and tuple(rpn["reg"].shape) == (2, 2048, 76)
    e_cls, e_reg = rel(n(rpn["cls"])[:, ::step, 0], G["rpn_cls_rows"]), rel(n(rpn["reg"])[:, ::step], G["rpn_reg_rows"])
    print("rpn cls", e_cls, "bound", bound(G, "cls"), "; rpn reg", e_reg, "bound", bound(G, "reg"))
    assert e_cls <= bound(G, "cls") and e_reg <= bound(G, "reg")


def test_stage3_rois_in_stored_order(run):
    G, _, _, rpn, out, state = run
    rois = n(out["rois"])
    assert rois.shape == G["rois"].shape == (2, 16, 7)
    assert torch.equal(rpn["rois"], out["rois"])  # both modes propose the same rois
    # the order: every roi is nearer to its stored roi than to any other stored roi of its cloud
    for b in range(2):
        d = np.abs(rois[b][:, None] - G["rois"][b][None]).sum(-1)
        assert np.array_equal(d.argmin(1), np.arange(16)), (b, d.argmin(1))
    e = rel(rois, G["rois"])
    e_sc = rel(state["roi_scores"], G["roi_scores"])
    print("rois", e, "bound", bound(G, "rois"), "; roi scores", e_sc, "bound", bound(G, "roi_scores"))
    assert e <= bound(G, "rois") and state["roi_scores"].shape == (2, 16) and e_sc <= bound(G, "roi_scores")


def test_stage4_roi_pool_index(run):
    G, _, _, _, _, state = run
    assert np.array_equal(state["pool_idx"], G["pool_idx"])
    assert np.array_equal(state["pool_flag"], G["pool_flag"])


def test_stage5_rcnn_cls_and_reg(run):
    G, _, _, _, out, _ = run
    assert tuple(out["cls"].shape) == (32, 1) and tuple(out["reg"].shape) == (32, 46)
    e_cls, e_reg = rel(n(out["cls"]), G["rcnn_cls"]), rel(n(out["reg"]), G["rcnn_reg"])
    print("rcnn cls", e_cls, "bound", bound(G, "rcnn_cls"), "; rcnn reg", e_reg, "bound", bound(G, "rcnn_reg"))
    assert e_cls <= bound(G, "rcnn_cls") and e_reg <= bound(G, "rcnn_reg")


def test_stage6_final_boxes(run):
    G, _, _, _, _, state = run
    assert len(state["final"]) == 2
    for b, (boxes, scores, labels) in enumerate(state["final"]):
        want = G[f"final_boxes{b}"]
        assert tuple(boxes.shape) == want.shape and labels.dtype == torch.int64
        assert np.array_equal(n(labels), G[f"final_labels{b}"])
        e_box, e_sc = rel(n(boxes), want), rel(n(scores), G[f"final_scores{b}"])
        print("cloud", b, "boxes", e_box, "bound", bound(G, "boxes"), "; scores", e_sc, "bound", bound(G, "scores"))
        assert e_box <= bound(G, "boxes") and e_sc <= bound(G, "scores")
        assert (n(scores) > 0.3).all()


def test_a_changed_rcnn_weight_breaks_stage5(run):
    """One RCNN weight tensor scaled by 1.01 must push the RCNN outputs past
    the bound (the comparison can tell a 1 % change from rounding)."""
    G, model, points, _, _, _ = run
    w = model.rcnn.merge_down_layer[0].weight
    keep = w.detach().clone()
    try:
        with torch.no_grad():
            w.mul_(1.01)
        out = model(points)
    finally:
        with torch.no_grad():
            w.copy_(keep)
    worst = max(rel(n(out["cls"]), G["rcnn_cls"]) / bound(G, "rcnn_cls"),
                rel(n(out["reg"]), G["rcnn_reg"]) / bound(G, "rcnn_reg"))
    print("relative error over its bound after the change", worst)
    assert worst > 1.0


def test_second_forward_bitwise_equal(run):
    _, model, points, _, out, state = run
    again = model(points)
    for k in ("rois", "cls", "reg"):
        assert torch.equal(again[k].view(torch.int32), out[k].view(torch.int32)), k
    assert np.array_equal(n(model.rcnn.pool_index), state["pool_idx"])


def test_rpn_mode_and_empty_second_range(run):
    """mode "RPN" returns rois, cls, reg; cloud 1 has every z below 40, so its
    rois come through the "second range is empty" branch: all 16 rows are
    filled from the first range."""
    G, _, points, rpn, _, _ = run
    assert set(rpn) == {"rois", "cls", "reg"} and tuple(rpn["rois"].shape) == (2, 16, 7)
    assert float(points[1, :, 2].max()) < 40 < float(points[0, :, 2].max())
    rois = n(rpn["rois"])
    assert (rois[0, :, 2] <= 40).sum() == 11 and (rois[0, :, 2] > 40).sum() == 5  # 70 % / 30 % of 16
    assert (rois[1, :, 2] <= 40).all() and (np.abs(rois[1]).sum(1) > 0).all()
