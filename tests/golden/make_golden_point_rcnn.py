"""Generate tests/golden/point_rcnn.npz and point_rcnn_state_dict.json (build
container only; data only): the eval() forward of the reference PointRCNN
(ml3d/torch/models/point_rcnn.py through tools/ref_loader.py), mode "RCNN",
in float32 and in float64.

The Open3D ops the reference binds are replaced on the imported modules:
furthest_point_sampling, ball_query, three_nn and nms by the CPU oracle (on the
float32 cast of their arguments, in both runs: inside the RPN these depend on
the input xyz only, so the float64 run uses the float32 run's indices by
construction); three_interpolate by the oracle in float32 and by the same sum
in float64; three_nn's distances are recomputed in float64 for the float64
run; roi_pool by the numpy restatement of this project's contract
(tests/roi_pool_ref.py) for the indices, the rows gathered in the run's dtype.

Configuration (recorded in the file): ml3d/configs/pointrcnn_kitti.yml with
npoint 2048, RPN SA npoints [512, 128, 32, 8], nms_pre 512, nms_post_val 16;
widths and the RCNN part as in the yml; B = 2; weights from prcnn_weights.py.
The scene (default_rng(SCENE_SEED), camera frame): per cloud a uniform
background of 16 x 2 x 20 m and two car-sized blobs of 600 points, dense
enough that a roi can hold 512; cloud 0 has z in [30, 50], on both sides of
40 m, cloud 1 z in [12, 32], so its "second range is empty" branch runs.

Asserted on the reference alone (a seed that misses one is replaced, the
conditions stay): both runs make the same discrete choice everywhere (every
FPS row, ball-query index, NMS keep list, roi_pool index and label); the
output is not degenerate (rois differ, at least 4 final boxes, at least one
dropped by the score threshold); some roi has fewer than S members, some has
at least S; cloud 1 takes the "second range is empty" branch; and the margins:

Every discrete choice that depends on computed values and reaches the output
has a margin of at least MARGIN = 100 times the float32-vs-float64 difference
of the quantity it compares.  The difference is that of the compared quantity
itself (this logit, this score, this distance, this slack), taken between the
two runs and never below half a float32 step at the quantity's size
(`own_err`): a difference of exactly 0 is luck, not margin.  torch runs on one
thread, so the float32 run and its differences do not depend on the machine's
core count.  The kinds:
the 0 / 40 / 80 m range masks of every point; the scores on both sides of each
pre-NMS cut; the x / z / ry bin argmaxes of every NMS candidate of the RPN and
of every roi of the RCNN (gap of the two largest logits against their two
differences); in all six NMS calls, for the kept boxes that leave the proposal
layer and the next one: their BEV IoU with every other candidate against the
threshold, their score against every box they suppress, and the scores of
consecutive kept boxes (the stored order); roi_pool membership of every point
in every enlarged roi (the smallest of the slacks to the six faces and the
10 m prefilter, `min_slack`: membership flips only where it crosses 0; the same
float64 arithmetic as tests/roi_pool_ref.membership_margin, which is checked to
give the same members); every FPS pick inside the RCNN's set-abstraction levels
(gap to the best point at other coordinates: cyclic duplicates tie exactly and
resolve by index in both runs); every ball-query pair of those levels against
the squared radius; the final scores against score_thres.

Recorded with its real gap and difference but not asserted: `score order among
the top nms_pre`, every consecutive pair of the ~500 candidates of a cloud.
Its smallest gap is about 1e-6 for any seed (2,048 scores in a spread of a few
units), below one float32 difference; two neighbours in that order that are
neither at a cut, nor overlapping above the threshold, nor both kept can swap
without changing anything downstream, and the three cases where the order
decides are asserted above.

The fixture stores per kind the smallest ratio, its margin and its difference
(`margin_names`, `margin_ratios`, `margin_values`, `margin_differences`).
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

SCENE_SEED = 506  # the first of seeds 300.. that meets every margin condition (about 1 in 240 does)
B, NPOINT = 2, 2048
ROW_STEP = 8
MARGIN = 100.0
RECORDED_ONLY = "score order among the top nms_pre"  # see the docstring
RATIOS, MISSED = [], []  # (condition, margin / difference) of the run, and the conditions below MARGIN
YML = "ml3d/configs/pointrcnn_kitti.yml"  # in the reference checkout (tools/ref_loader.py REFERENCE)


def config():
    import ref_loader
    import yaml
    cfg = yaml.safe_load(open(os.path.join(ref_loader.REFERENCE, YML)))["model"]
    cfg = {k: cfg[k] for k in ("classes", "score_thres", "augment", "rpn", "rcnn")}
    cfg["npoints"] = NPOINT
    cfg["rpn"]["backbone"]["SA_config"]["npoints"] = [512, 128, 32, 8]
    cfg["rpn"]["head"]["nms_pre"] = 512
    cfg["rpn"]["head"]["nms_post_val"] = 16
    return cfg


def scene(seed=SCENE_SEED):
    rng = np.random.default_rng(seed)
    clouds = []
    for z0 in (30.0, 12.0):  # cloud 0: z in [30, 50], cloud 1: z in [12, 32]
        n_blob = 600
        blobs = []
        for _ in range(2):
            c = rng.random(3) * [10, 0.4, 14] + [-5, 0.6, z0 + 3]
            blobs.append(c + (rng.random((n_blob, 3)) - 0.5) * [3.2, 1.4, 1.7])
        bg = rng.random((NPOINT - 2 * n_blob, 3)) * [16, 2, 20] + [-8, -0.5, z0]
        pts = np.concatenate(blobs + [bg])
        clouds.append(pts[rng.permutation(NPOINT)])
    return np.stack(clouds).astype(np.float32)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


def layout(model):
    return [[k, list(v.shape)] for k, v in model.state_dict().items()]


def own_err(q64, q32):
    """The float32-vs-float64 difference of each compared quantity itself, not
    below half a float32 step at its size (a difference of 0 is luck)."""
    q64, q32 = np.asarray(q64, np.float64), np.asarray(q32, np.float64)
    return np.maximum(np.abs(q64 - q32), 0.5 * np.spacing(np.abs(q64).astype(np.float32)).astype(np.float64))


def need(margin, err, what):
    """Record the smallest margin / difference over the choices of one kind."""
    margin, err = np.atleast_1d(np.asarray(margin, np.float64)), np.atleast_1d(np.asarray(err, np.float64))
    if margin.size == 0:
        return
    r = margin / err
    k = int(np.argmin(r))
    RATIOS.append((what, float(r.flat[k]), float(margin.flat[k]), float(err.flat[k])))
    if r.flat[k] < MARGIN:
        MISSED.append(what)


def merge():
    """One entry per kind: the worst of the records with the same name."""
    out = {}
    for what, r, m, e in RATIOS:
        if what not in out or r < out[what][0]:
            out[what] = (r, m, e)
    return out


def top2(l64, l32):
    """Per row: the gap of the two largest logits and the differences of the two."""
    o = np.argsort(l64, axis=1)
    i, j = o[:, -1:], o[:, -2:-1]
    e = own_err(l64, l32)
    g = np.take_along_axis
    return (g(l64, i, 1) - g(l64, j, 1))[:, 0], (g(e, i, 1) + g(e, j, 1))[:, 0]


def min_slack(xyz, box):
    """float64: the smallest of the slacks to the eight bounds of roi_pool
    membership; a point is a member iff it is >= 0, and membership flips only
    where it crosses 0."""
    p = np.asarray(xyz, np.float64)
    x, y, z, h, w, l, ry = (float(v) for v in box)
    dx, dy, dz = p[:, 0] - x, p[:, 1] - (y - h / 2), p[:, 2] - z
    xr = dx * np.cos(ry) - dz * np.sin(ry)
    zr = dx * np.sin(ry) + dz * np.cos(ry)
    return np.min([10.0 - np.abs(dx), h / 2 - np.abs(dy), 10.0 - np.abs(dz), l / 2 - np.abs(xr), w / 2 - np.abs(zr)],
                  axis=0)


def fps_gaps(x64, x32, npoint):
    """float64 FPS of x64 [b,n,3] -> (rows [b,npoint], per pick the gap
    between its distance and the best distance of a point at other
    coordinates, and the float32-vs-float64 difference of those two distances:
    the same picks followed on x32, the float32 run's coordinates)."""
    b, n, _ = x64.shape
    m64, m32 = np.full((b, n), 1e10), np.full((b, n), 1e10)
    last = np.zeros(b, np.int64)
    rows, gaps, errs = [last.copy()], [], []
    ar = np.arange(b)
    for _ in range(1, npoint):
        m64 = np.minimum(m64, ((x64 - x64[ar, last][:, None]) ** 2).sum(-1))
        m32 = np.minimum(m32, ((x32 - x32[ar, last][:, None]) ** 2).sum(-1))
        last = m64.argmax(1)
        other = np.any(x64 != x64[ar, last][:, None], axis=2)
        second = np.where(other, m64, -np.inf).argmax(1)
        live = (m64[ar, last] > 0) & other.any(1)  # else all left at distance 0: exact ties, by index in both runs
        e = own_err(m64, m32)
        gaps.append((m64[ar, last] - m64[ar, second])[live])
        errs.append((e[ar, last] + e[ar, second])[live])
        rows.append(last.copy())
    return np.stack(rows, 1), np.concatenate(gaps), np.concatenate(errs)


def main(write=True, seed=SCENE_SEED):
    import oracle as O
    import ref_loader
    ref_loader.install()
    import open3d
    open3d.core.cuda.device_count = lambda: 1  # the reference imports and calls the GPU ops only then
    open3d.ml.contrib.iou_bev_cuda = open3d.ml.contrib.iou_3d_cuda = None
    import ml3d.torch.models.point_rcnn as ref
    import ml3d.torch.utils.pointnet.pointnet2_utils as pu
    import ml3d.torch.utils.roipool3d.roipool3d_utils as ru
    import prcnn_weights
    from roi_pool_ref import membership_margin, roi_pool_ref

    torch.set_num_threads(1)  # one reduction order: the float32 run, and with it every difference, is reproducible
    log = {}

    def f32(t):
        return np.ascontiguousarray(t.detach().float().numpy())

    def furthest_point_sampling(xyz, npoint):
        idx = O.furthest_point_sampling(f32(xyz), int(npoint))
        log.setdefault("fps", []).append((xyz.detach().double().numpy().copy(), idx))
        return torch.from_numpy(idx)

    def ball_query(xyz, center, radius, nsample):
        idx = O.ball_query(f32(xyz), f32(center), float(radius), int(nsample))
        log.setdefault("ball", []).append((xyz.detach().double().numpy().copy(),
                                           center.detach().double().numpy().copy(), float(radius), idx))
        return torch.from_numpy(idx)

    def three_nn(query, data):
        d2, idx = O.three_nn(f32(query), f32(data))
        if query.dtype == torch.float64:
            nb = torch.gather(data.unsqueeze(1).expand(-1, query.shape[1], -1, -1), 2,
                              torch.from_numpy(idx).long().unsqueeze(-1).expand(-1, -1, -1, 3))
            return ((query.unsqueeze(2) - nb) ** 2).sum(-1), torch.from_numpy(idx)
        return torch.from_numpy(d2), torch.from_numpy(idx)

    def three_interpolate(feats, idx, weight):
        if feats.dtype == torch.float32:
            return torch.from_numpy(O.three_interpolate(f32(feats), idx.numpy(), f32(weight)))
        out = 0
        for k in range(3):
            g = torch.gather(feats, 2, idx[:, None, :, k].long().expand(-1, feats.shape[1], -1))
            out = out + g * weight[:, None, :, k]
        return out

    def nms(bev, scores, thresh):
        keep = O.nms(f32(bev), f32(scores).reshape(-1), float(thresh))
        log.setdefault("nms", []).append((bev.detach().double().numpy().copy(),
                                          scores.detach().double().numpy().reshape(-1).copy(), float(thresh), keep))
        return torch.from_numpy(keep)

    def roi_pool(xyz, boxes, feat, S):
        _, flag, idx = roi_pool_ref(f32(xyz), f32(boxes), np.zeros(feat.shape[:2] + (0,), np.float32), S)
        rows = torch.cat([xyz, feat], dim=2)
        ii = torch.from_numpy(np.maximum(idx, 0)).long()
        pooled = torch.stack([rows[b][ii[b]] for b in range(xyz.shape[0])])
        pooled = pooled * torch.from_numpy(1 - flag).to(pooled.dtype)[:, :, None, None]
        log["pool"] = dict(xyz=xyz.double().numpy().copy(), boxes=boxes.double().numpy().copy(), idx=idx, flag=flag,
                           before=pooled.clone(), after=pooled)  # the reference transforms `pooled` in place
        return pooled, torch.from_numpy(flag)

    pu.furthest_point_sampling, pu.ball_query = furthest_point_sampling, ball_query
    pu.three_nn, pu.three_interpolate = three_nn, three_interpolate
    ref.nms = nms
    ru.roi_pool = roi_pool

    cfg = config()
    pts = scene(seed)
    assert pts[0, :, 2].min() < 40 < pts[0, :, 2].max() and pts[1, :, 2].max() < 34
    model = ref.PointRCNN(device="cpu", **cfg)
    model.load_state_dict(prcnn_weights.state_dict_for(model), strict=True)
    model.eval()
    thres = cfg["score_thres"]

    runs = {}
    with torch.no_grad():
        for tag, dt in (("32", torch.float32), ("64", torch.float64)):
            m = model.double() if dt == torch.float64 else model
            log.clear()
            points = torch.from_numpy(pts).to(dt)
            # PointRCNN.forward (point_rcnn.py:115-140), its stages kept apart
            cls, reg, xyz, feats = m.rpn(points)
            raw = cls[:, :, 0]
            proposals = ref.decode_bbox_target(
                xyz.view(-1, 3), reg.view(-1, reg.shape[-1]), anchor_size=m.rpn.proposal_layer.mean_size,
                loc_scope=3.0, loc_bin_size=0.5, num_head_bin=12, get_xz_fine=True).view(B, -1, 7)
            rois, roi_scores = m.rpn.proposal_layer(raw, reg, xyz)
            n_rpn_nms = len(log["nms"])
            seg = (torch.sigmoid(raw) > thres).float()
            out = m.rcnn(rois, [None], xyz, feats.permute(0, 2, 1), seg, torch.norm(xyz, p=2, dim=2))
            # inference_end (point_rcnn.py:379-402) up to the BEVBox3D objects
            rc, rr = out["cls"].view(B, -1, out["cls"].shape[1]), out["reg"].view(B, -1, out["reg"].shape[1])
            decoded = ref.decode_bbox_target(
                rois.view(-1, 7), out["reg"], anchor_size=m.rcnn.proposal_layer.mean_size, loc_scope=1.5,
                loc_bin_size=0.5, num_head_bin=9, get_xz_fine=True, get_y_by_bin=False, get_ry_fine=True)
            boxes, scores = m.rcnn.proposal_layer(rc, rr, rois)
            final = []
            for bb, sc in zip(boxes, scores):
                sc = torch.sigmoid(sc)
                keep = torch.flatten(sc > thres)
                final.append((bb[keep].double().numpy(), sc[keep].double().numpy().reshape(-1),
                              (sc < thres).long()[keep].numpy().reshape(-1), sc.double().numpy().reshape(-1)))
            runs[tag] = dict(cls=cls.double().numpy(), reg=reg.double().numpy(), proposals=proposals.double().numpy(),
                             rois=rois.double().numpy(), roi_scores=roi_scores.double().numpy(),
                             rcnn_cls=out["cls"].double().numpy(), rcnn_reg=out["reg"].double().numpy(),
                             decoded=decoded.double().numpy(), final=final, n_rpn_nms=n_rpn_nms,
                             log={k: v for k, v in log.items()})
    r32, r64 = runs["32"], runs["64"]

    differ = []  # discrete choices that differ between the two runs (asserted empty at the end)

    def same(what, x, y):
        if not np.array_equal(x, y):
            differ.append(what)
            print("  DIFFERS between float32 and float64:", what)

    for lvl, ((_, x), (_, y)) in enumerate(zip(r32["log"]["fps"], r64["log"]["fps"])):
        same(f"FPS call {lvl}", x, y)
    for lvl, (x, y) in enumerate(zip(r32["log"]["ball"], r64["log"]["ball"])):
        same(f"ball query call {lvl}", x[3], y[3])
    assert len(r32["log"]["nms"]) == len(r64["log"]["nms"]) == 6 and r64["n_rpn_nms"] == 4
    for lvl, (x, y) in enumerate(zip(r32["log"]["nms"], r64["log"]["nms"])):
        same(f"NMS call {lvl}", x[3], y[3])
    same("roi_pool idx", r32["log"]["pool"]["idx"], r64["log"]["pool"]["idx"])
    for lvl, (x, y) in enumerate(zip(r32["final"], r64["final"])):
        same(f"final labels of cloud {lvl}", x[2], y[2])

    print("margins")
    pl = model.rpn.proposal_layer
    pre = [0, int(pl.nms_pre * 0.7), pl.nms_pre - int(pl.nms_pre * 0.7)]
    post = [0, int(pl.nms_post_val * 0.7), pl.nms_post_val - int(pl.nms_post_val * 0.7)]
    s64, s32 = r64["cls"][:, :, 0], r32["cls"][:, :, 0]
    se = own_err(s64, s32)
    z, z32 = r64["proposals"][:, :, 2], r32["proposals"][:, :, 2]
    need(np.min([np.abs(z - v) for v in (0.0, 40.0, 80.0)], axis=0), own_err(z, z32), "range masks")
    cand, second_empty = [], []
    for b in range(B):
        order = np.argsort(-s64[b], kind="stable")
        zo = z[b][order]
        first = order[(zo > 0) & (zo <= 40)]
        second = order[(zo > 40) & (zo <= 80)]
        second_empty.append(len(second) == 0)
        parts = [(first, pre[1]), (second, pre[2])] if len(second) else [(first, pre[1]), (first[pre[1]:], pre[2])]
        for rows, k in parts:
            cand.append((b, rows[:k]))
            if len(rows) > k:
                i, j = rows[k - 1], rows[k]
                need(s64[b][i] - s64[b][j], se[b][i] + se[b][j], "scores at the pre-NMS cuts")
        top = np.concatenate([c for bb, c in cand if bb == b])
        top = top[np.argsort(-s64[b][top], kind="stable")]
        need(-np.diff(s64[b][top]), se[b][top][:-1] + se[b][top][1:], "score order among the top nms_pre")
    assert second_empty == [False, True], second_empty
    rows64 = np.concatenate([r64["reg"][b][c] for b, c in cand])
    rows32 = np.concatenate([r32["reg"][b][c] for b, c in cand])
    for lo, hi in ((0, 12), (12, 24), (49, 61)):
        need(*top2(rows64[:, lo:hi], rows32[:, lo:hi]), "RPN bin argmaxes of the candidates")
    for lo, hi in ((0, 6), (6, 12), (25, 34)):
        need(*top2(r64["rcnn_reg"][:, lo:hi], r32["rcnn_reg"][:, lo:hi]), "RCNN bin argmaxes")

    for call, ((b64, sc64, thr, keep), (b32, sc32, _, _)) in enumerate(zip(r64["log"]["nms"], r32["log"]["nms"])):
        c = (b64[:, :2] + b64[:, 2:4]) / 2
        near = np.argwhere(np.triu(np.abs(c[:, None] - c[None]).max(-1) < 12, 1))
        twin = np.abs(b64[:, None] - b32[None]).sum(-1).argmin(1)  # the same candidate in the float32 run
        e = own_err(sc64, sc32[twin])
        if call < r64["n_rpn_nms"]:  # only the first post-NMS boxes leave the proposal layer, and the next one bounds them
            keep = keep[:post[1 + call % 2] + 1]
        kept = set(keep.tolist())
        iou_m, iou_e, ord_m, ord_e = [], [], [], []
        for i, j in near:
            if i not in kept and j not in kept:  # only a kept box suppresses
                continue
            u64 = O.bev_iou(b64[i].astype(np.float32), b64[j].astype(np.float32))
            u32 = O.bev_iou(b32[twin[i]].astype(np.float32), b32[twin[j]].astype(np.float32))
            iou_m.append(abs(u64 - thr))
            iou_e.append(max(abs(u64 - u32), 2.0 ** -24))
            if u64 > thr:  # a kept box must outrank what it suppresses
                ord_m.append(abs(sc64[i] - sc64[j]))
                ord_e.append(e[i] + e[j])
        need(iou_m, iou_e, "BEV IoU against the NMS threshold")
        need(ord_m, ord_e, "score order: a kept box against a box it suppresses")
        need(np.abs(np.diff(sc64[keep])), e[keep][:-1] + e[keep][1:], "score order of the kept boxes")

    pool, pool32 = r64["log"]["pool"], r32["log"]["pool"]
    cnts = []
    for b in range(B):
        for k in range(pool["boxes"].shape[1]):
            ins, _ = membership_margin(pool["xyz"][b], pool["boxes"][b, k])
            sl = min_slack(pool["xyz"][b], pool["boxes"][b, k])
            assert np.array_equal(ins, sl >= 0)
            cnts.append(int(ins.sum()))
            got = np.unique(pool["idx"][b, k][pool["idx"][b, k] >= 0])
            assert np.array_equal(got, np.nonzero(ins)[0][:512]), (b, k)
            sl32 = min_slack(pool32["xyz"][b], pool32["boxes"][b, k])
            # a slack is a difference of coordinates of up to 50 m: not below half a float32 step there
            need(np.abs(sl), np.maximum(np.abs(sl - sl32), 0.5 * np.spacing(np.float32(np.abs(pool["xyz"][b]).max()))),
                 "roi_pool membership (faces and prefilter)")
    cnts = np.array(cnts)
    print("  roi member counts", cnts.tolist())
    assert (cnts < 512).any() and (cnts >= 512).any()

    fps = [c for c in r64["log"]["fps"] if c[0].shape[0] == cnts.size]
    fps32 = [c for c in r32["log"]["fps"] if c[0].shape[0] == cnts.size]
    assert len(fps) == 2
    for lvl, ((x64, idx), (x32, _)) in enumerate(zip(fps, fps32)):
        rows, gaps, errs = fps_gaps(x64, x32, idx.shape[1])
        assert np.array_equal(rows, idx), f"float64 FPS of RCNN level {lvl} picks other rows"
        need(gaps, errs, f"FPS pick gaps, RCNN level {lvl}")
    balls = [c for c in r64["log"]["ball"] if c[0].shape[0] == cnts.size]
    balls32 = [c for c in r32["log"]["ball"] if c[0].shape[0] == cnts.size]
    assert len(balls) == 2
    for lvl, ((x64, c64, radius, _), (x32, c32, _, _)) in enumerate(zip(balls, balls32)):
        d64 = ((c64[:, :, None] - x64[:, None]) ** 2).sum(-1)
        d32 = ((c32[:, :, None] - x32[:, None]) ** 2).sum(-1)
        r2 = float(np.float32(radius)) ** 2
        need(np.abs(d64 - r2).ravel(), own_err(d64, d32).ravel(), f"ball-query radius, RCNN level {lvl}")
    all_sc = np.concatenate([f[3] for f in r64["final"]])
    all_sc32 = np.concatenate([f[3] for f in r32["final"]])
    need(np.abs(all_sc - thres), own_err(all_sc, all_sc32), "final score threshold")
    kinds = merge()
    for k, (r, m, e) in kinds.items():
        print(f"  {k}: smallest margin / difference {r:.1f} (margin {m:.3e}, float32-vs-float64 difference {e:.3e})")
    missed = sorted(k for k, v in kinds.items() if v[0] < MARGIN)

    assert not differ, differ
    missed = [k for k in missed if k != RECORDED_ONLY]
    assert not missed, ("margins below %g x the float32-vs-float64 difference" % MARGIN, missed)
    print("not degenerate; rcnn scores", np.round(np.sort(r64["rcnn_cls"].reshape(-1)), 2).tolist())
    n_final = sum(len(f[1]) for f in r64["final"])
    assert n_final >= 4 and n_final < len(all_sc), (n_final, len(all_sc))
    assert np.ptp(r64["rois"][:, :, :3], axis=1).min() > 1.0 and np.isfinite(r64["rcnn_reg"]).all()

    errs = {k: rel(r32[k], r64[k]) for k in ("cls", "reg", "rois", "roi_scores", "rcnn_cls", "rcnn_reg", "decoded")}
    errs["boxes"] = max(rel(a[0], b[0]) for a, b in zip(r32["final"], r64["final"]) if len(b[0]))
    errs["scores"] = max(rel(a[1], b[1]) for a, b in zip(r32["final"], r64["final"]) if len(b[0]))
    print("reference float32 vs float64:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= 1e-3, errs

    before, after = pool["before"].double().numpy(), pool["after"].double().numpy()
    out = {"points": pts, "scene_seed": np.int64(seed), "row_step": np.int64(ROW_STEP), "margin": np.float64(MARGIN),
           "config": np.array(json.dumps(cfg)), "fps_level1": r64["log"]["fps"][0][1],
           "rpn_cls_rows": s64[:, ::ROW_STEP], "rpn_reg_rows": r64["reg"][:, ::ROW_STEP], "rois": r64["rois"],
           "roi_scores": r64["roi_scores"], "pooled_boxes": pool["boxes"], "pool_idx": pool["idx"],
           "pool_flag": pool["flag"], "rcnn_cls": r64["rcnn_cls"], "rcnn_reg": r64["rcnn_reg"],
           "decoded": r64["decoded"], "canon_before": before[:, :4, :6, :3], "canon_after": after[:, :4, :6, :3],
           "roi_counts": cnts.astype(np.int64), "margin_names": np.array(list(kinds)),
           "margin_ratios": np.array([v[0] for v in kinds.values()], np.float64),
           "margin_values": np.array([v[1] for v in kinds.values()], np.float64),
           "margin_differences": np.array([v[2] for v in kinds.values()], np.float64)}
    for b, f in enumerate(r64["final"]):
        out[f"final_boxes{b}"], out[f"final_scores{b}"], out[f"final_labels{b}"] = f[0], f[1], f[2].astype(np.int64)
    for k, v in errs.items():
        out["err_" + k] = np.float64(v)
    if not write:
        return out
    path = os.path.join(HERE, "point_rcnn.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    assert size < (1 << 20), size
    path = os.path.join(HERE, "point_rcnn_state_dict.json")
    with open(path, "w") as f:
        json.dump({"PointRCNN": layout(ref.PointRCNN(device="cpu", **config()))}, f, indent=0)
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")
    return out


if __name__ == "__main__":
    main(write="--dry" not in sys.argv[2:], seed=int(sys.argv[1]) if len(sys.argv) > 1 else SCENE_SEED)
