"""PointRCNN without a GPU: the state_dict layout against the reference's
(tests/golden/point_rcnn_state_dict.json), the box helpers on CPU tensors
against values of the reference's float64 run (tests/golden/point_rcnn.npz),
the roi_pool restatement against an independent brute-force membership, and
the failure modes (training, no GPU)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from roi_pool_ref import membership_margin, roi_pool_ref  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixture():
    return np.load(os.path.join(GOLDEN, "point_rcnn.npz"))


def model_config(G):
    cfg = json.loads(str(G["config"]))
    return {k: cfg[k] for k in ("classes", "score_thres", "npoints", "rpn", "rcnn")}


def test_state_dict_layout_is_the_references():
    from o3dml_amd.point_rcnn import PointRCNN
    want = json.load(open(os.path.join(GOLDEN, "point_rcnn_state_dict.json")))["PointRCNN"]
    got = [[k, list(v.shape)] for k, v in PointRCNN(**model_config(fixture())).state_dict().items()]
    assert got == want
    assert len(want) == 244 and sum(int(np.prod(s)) for _, s in want) == 3901774


def test_weights_load_strict():
    sys.path.insert(0, GOLDEN)
    import prcnn_weights
    from o3dml_amd.point_rcnn import PointRCNN
    m = PointRCNN(**model_config(fixture()))
    sd = prcnn_weights.state_dict_for(m)
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m.rcnn.reg_blocks[4].weight, sd["rcnn.reg_blocks.4.weight"])
    assert "rpn.proposal_layer.mean_size" not in sd  # a plain attribute in the reference too


def test_decode_bbox_target_on_cpu():
    """The RCNN decoding (rois [n,7], get_ry_fine) of the reference's float64
    run, recomputed from its stored rois and regressions in float64 and in
    float32."""
    from o3dml_amd.point_rcnn import decode_bbox_target
    G = fixture()
    rois = torch.from_numpy(G["rois"]).view(-1, 7)
    reg = torch.from_numpy(G["rcnn_reg"])
    anchor = torch.tensor([1.52563191462, 1.62856739989, 3.88311640418])
    kw = dict(loc_scope=1.5, loc_bin_size=0.5, num_head_bin=9, get_xz_fine=True, get_y_by_bin=False, get_ry_fine=True)
    got = decode_bbox_target(rois, reg, anchor_size=anchor, **kw).numpy()
    scale = np.abs(G["decoded"]).max()
    # the reference keeps the bin centre plus residual in float32 even in its float64 run (an in-place add
    # into `x_bin.float()`): offsets of up to 3 m rounded to 2.4e-7, so 1e-7 of the 59 m scale, not 1e-12
    assert got.dtype == np.float64 and np.abs(got - G["decoded"]).max() <= 1e-7 * scale
    got32 = decode_bbox_target(rois.float(), reg.float(), anchor_size=anchor, **kw).numpy()
    assert got32.dtype == np.float32 and np.abs(got32 - G["decoded"]).max() <= 1e-5 * scale
    assert torch.equal(rois, torch.from_numpy(G["rois"]).view(-1, 7))  # inputs untouched


def test_decode_bbox_target_points_form():
    """The RPN form: roi_box3d [n,3], 12 heading bins over 2 pi wrapped to
    (-pi, pi]; one hand-written row."""
    from o3dml_amd.point_rcnn import decode_bbox_target
    reg = torch.zeros(1, 76)
    reg[0, 3], reg[0, 12 + 8] = 5.0, 5.0  # x bin 3 -> -1.25, z bin 8 -> 1.25
    reg[0, 24 + 3], reg[0, 36 + 8] = 0.5, -0.5  # residuals +-0.25
    reg[0, 48] = 0.75  # y offset
    reg[0, 49 + 7], reg[0, 61 + 7] = 5.0, 0.5  # heading bin 7 of 12: 210 deg + 7.5 deg -> wraps
    reg[0, 73:] = torch.tensor([0.0, 1.0, -0.5])
    box = decode_bbox_target(torch.tensor([[10.0, 1.0, 20.0]]), reg, anchor_size=torch.tensor([1.0, 2.0, 4.0]),
                             loc_scope=3.0, loc_bin_size=0.5, num_head_bin=12)[0]
    want = [10 - 1.25 + 0.25, 1.75, 20 + 1.25 - 0.25, 1.0, 4.0, 2.0, np.deg2rad(217.5) - 2 * np.pi]
    assert np.allclose(box.numpy(), want, atol=1e-5)


def test_enlarge_box3d():
    from o3dml_amd.point_rcnn import enlarge_box3d
    G = fixture()
    rois = torch.from_numpy(G["rois"]).view(-1, 7)
    keep = rois.clone()
    got = enlarge_box3d(rois, 1.0)
    assert torch.equal(rois, keep)
    assert np.abs(got.view(G["pooled_boxes"].shape).numpy() - G["pooled_boxes"]).max() <= 1e-12 * 80
    assert np.array_equal(enlarge_box3d(rois.numpy(), 1.0), got.numpy())
    # the centre of the box (y - h / 2) stays where it was
    assert torch.allclose(got[:, 1] - got[:, 3] / 2, rois[:, 1] - rois[:, 3] / 2, atol=1e-12)


def test_canonical_transform():
    from o3dml_amd.point_rcnn import canonical_transform, rotate_pc_along_y_torch
    G = fixture()
    before, after = torch.from_numpy(G["canon_before"]), G["canon_after"]
    rois = torch.from_numpy(G["rois"])[:, :before.shape[1]]
    keep = before.clone()
    got = canonical_transform(before, rois).numpy()
    assert torch.equal(before, keep)
    assert np.abs(got - after).max() <= 1e-12 * np.abs(after).max()
    a = torch.tensor([np.pi / 2], dtype=torch.float64)
    out = rotate_pc_along_y_torch(torch.tensor([[[1.0, 7.0, 0.0, 9.0]]], dtype=torch.float64), a)
    assert np.allclose(out.numpy(), [[[0.0, 7.0, 1.0, 9.0]]], atol=1e-12)  # x -> z, y and the feature untouched


def test_roi_pool_ref_against_brute_force():
    """The float32 restatement against an independent float64 point-in-box
    test (box frame, per-point loop) on the fixture's rois, whose margins the
    generator checked."""
    G = fixture()
    xyz, boxes = G["points"], G["pooled_boxes"]
    S = 512
    _, flag, idx = roi_pool_ref(xyz, boxes, np.zeros(xyz.shape[:2] + (1,), np.float32), S)
    assert np.array_equal(idx, G["pool_idx"]) and np.array_equal(flag, G["pool_flag"])
    for b in range(xyz.shape[0]):
        for k in range(boxes.shape[1]):
            x, y, z, h, w, l, ry = (float(v) for v in boxes[b, k])
            R = np.array([[np.cos(ry), -np.sin(ry)], [np.sin(ry), np.cos(ry)]])
            mem = []
            for i, p in enumerate(xyz[b].astype(np.float64)):
                d = p - [x, y - h / 2, z]
                loc = R @ d[[0, 2]]
                if max(abs(d[0]), abs(d[2])) <= 10 and abs(d[1]) <= h / 2 and abs(loc[0]) <= l / 2 and \
                        abs(loc[1]) <= w / 2:
                    mem.append(i)
            want = np.full(S, -1) if not mem else np.array(mem[:S] if len(mem) >= S else
                                                            [mem[s % len(mem)] for s in range(S)])
            assert np.array_equal(idx[b, k], want), (b, k)
            assert flag[b, k] == (not mem)
            assert np.array_equal(membership_margin(xyz[b], boxes[b, k])[0].nonzero()[0], np.array(mem, np.int64))
    assert np.array_equal(np.array([len(np.unique(i[i >= 0])) for i in idx.reshape(-1, S)]),
                          np.minimum(G["roi_counts"], S))


def test_fixture_margins():
    """The fixture's discrete choices keep the margin its generator asserts:
    per kind, the smallest margin over the float32-vs-float64 difference of
    the compared quantity is at least `margin` (100).  The order of all
    consecutive candidate scores is recorded only (the generator says why)."""
    G = fixture()
    ratios = dict(zip(G["margin_names"].tolist(), G["margin_ratios"].tolist()))
    assert float(G["margin"]) == 100.0 and len(ratios) == 14
    recorded_only = "score order among the top nms_pre"
    assert recorded_only in ratios
    low = {k: v for k, v in ratios.items() if v < float(G["margin"]) and k != recorded_only}
    assert not low, low
    assert np.allclose(G["margin_ratios"], G["margin_values"] / G["margin_differences"])


def test_train_mode_raises():
    from o3dml_amd.point_rcnn import PointRCNN, PointnetSAModule
    m = PointRCNN(**model_config(fixture())).train()
    with pytest.raises(NotImplementedError, match="PointRCNN: training is not built yet"):
        m(torch.zeros(1, 64, 3))
    with pytest.raises(NotImplementedError, match="training is not built yet"):
        sa = PointnetSAModule(mlp=[4, 8], npoint=2, radius=1.0, nsample=2).train()
        sa(torch.zeros(1, 8, 3), torch.zeros(1, 8, 4))


def test_no_gpu_raises():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from o3dml_amd import ops
    from o3dml_amd.point_rcnn import PointRCNN
    with pytest.raises(RuntimeError, match="no ROCm GPU"):
        ops.roi_pool(torch.zeros(1, 4, 3), torch.ones(1, 1, 7), torch.zeros(1, 4, 2), 4)
    with pytest.raises(RuntimeError, match="no ROCm GPU"):
        PointRCNN(**model_config(fixture())).eval()(torch.zeros(1, 64, 3))


def test_roi_pool_is_an_open3d_name():
    import o3dml_amd
    from o3dml_amd import ops, torch_ops
    assert "roi_pool" in ops.__all__ and "roi_pool_indexed" not in ops.__all__
    assert "roi_pool" in torch_ops.OPS
    o3dml_amd.register_torch_ops()
    s = str(torch.ops.open3d.roi_pool.default._schema)
    assert "Tensor xyz, Tensor boxes3d, Tensor pts_feature" in s and "sampled_pts_num" in s
