"""PointRCNN inference (ml3d/torch/models/point_rcnn.py, ml3d/torch/modules/
pointnet.py): the module tree and state_dict of the reference, and its eval()
forward for mode "RPN" and mode "RCNN".

Through this library's HIP kernels run the farthest-point sampling, the ball
queries, three_nn / three_interpolate of the feature propagation, the rotated
BEV NMS of both proposal layers and roi_pool (csrc/roi_pool.hip).  The grouping
of a set-abstraction level is a plain torch row gather of [xyz | feature] rows
by the ball-query index (one index_select per scale); the pooled rows of
roi_pool arrive channels-last already.

Activations are kept channels-last ([B, n, C], [B, n, nsample, C]) from the
input to the heads, so every 1x1 Conv1d / Conv2d of the reference is a Linear
over the same weight tensor (viewed [out, in]) and the BatchNorm behind it is
folded into that Linear in eval form on every call, from the module's current
tensors.  The Conv modules themselves are kept, so a reference state_dict
loads with strict=True, key for key and shape for shape.

Proposal selection (ProposalLayer) is tensor code: the only host reads are the
reference's own per-range "is this range empty" branch and the NMS keep count.
Training is not built: forward() in train() mode raises NotImplementedError;
ProposalTargetLayer, the losses, preprocess / transform and augmentation are
not part of this module.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from ._util import require_gpu
from .point_transformer import fold_bn

_TRAINING = "PointRCNN: training is not built yet"


def gen_CNN(channels, conv=nn.Conv1d, bias=True, activation=nn.ReLU, batch_norm=None):
    """Sequential of 1x1 conv [, batch norm], activation per channel step
    (ml3d/torch/utils/torch_utils.py gen_CNN)."""
    layers = []
    for cin, cout in zip(channels[:-1], channels[1:]):
        layers.append(conv(cin, cout, 1, bias=bias))
        if batch_norm is not None:
            layers.append(batch_norm(cout))
        if activation is not None:
            layers.append(activation(inplace=True))
    return nn.Sequential(*layers)


def run_channels_last(seq, x):
    """Apply a Sequential of 1x1 convs, batch norms (eval form, folded into the
    conv before them), ReLUs and Dropouts (identity in eval) to x [..., C]."""
    mods = list(seq)
    i = 0
    while i < len(mods):
        m = mods[i]
        if isinstance(m, (nn.Conv1d, nn.Conv2d)):
            w, b = m.weight.view(m.out_channels, m.in_channels), m.bias
            if i + 1 < len(mods) and isinstance(mods[i + 1], (nn.BatchNorm1d, nn.BatchNorm2d)):
                scale, shift = fold_bn(mods[i + 1])
                w = w * scale[:, None]
                b = shift if b is None else b * scale + shift
                i += 1
            x = F.linear(x, w, b)
        elif isinstance(m, nn.ReLU):
            x = F.relu_(x)
        elif not isinstance(m, nn.Dropout):
            raise RuntimeError(f"PointRCNN: no channels-last form of {type(m).__name__}")
        i += 1
    return x


# ---------------------------------------------------------------------------
# PointNet++ modules (pointnet.py, pointnet2_utils.py)
# ---------------------------------------------------------------------------
class QueryAndGroup(nn.Module):
    """Rows [xyz - centre | feature] of the first nsample points inside the
    ball of every centre (pointnet2_utils.py:223-278), channels-last."""

    def __init__(self, radius, nsample, use_xyz=True):
        super().__init__()
        self.radius, self.nsample, self.use_xyz = radius, nsample, use_xyz

    def forward(self, xyz, new_xyz, features=None):
        B, N, _ = xyz.shape
        idx = ops.ball_query(xyz, new_xyz, self.radius, self.nsample)  # [B, npoint, nsample], rows of the cloud
        rows = (idx.long() + (torch.arange(B, device=idx.device) * N).view(B, 1, 1)).view(-1)
        shape = (B, new_xyz.shape[1], self.nsample, -1)
        grouped_xyz = xyz.reshape(B * N, 3)[rows].view(shape) - new_xyz.unsqueeze(2)
        if features is None:
            if not self.use_xyz:
                raise RuntimeError("QueryAndGroup: no features and use_xyz is off")
            return grouped_xyz
        grouped = features.reshape(B * N, features.shape[2])[rows].view(shape)
        return torch.cat([grouped_xyz, grouped], dim=3) if self.use_xyz else grouped


class GroupAll(nn.Module):
    """One group of all points (pointnet2_utils.py:281-313): [B, 1, N, 3 + C]."""

    def __init__(self, use_xyz=True):
        super().__init__()
        self.use_xyz = use_xyz

    def forward(self, xyz, new_xyz, features=None):
        if features is None:
            return xyz.unsqueeze(1)
        return (torch.cat([xyz, features], dim=2) if self.use_xyz else features).unsqueeze(1)


class PointnetSAModuleMSG(nn.Module):
    """Set abstraction with multi-scale grouping (pointnet.py:110-211).
    forward(xyz [B,N,3], features [B,N,C] or None) -> (new_xyz [B,npoint,3] or
    None, new_features [B, npoint or 1, sum of the scales' widths]); `sampled`
    holds the FPS rows of the last forward."""

    def __init__(self, *, npoint, radii, nsamples, mlps, batch_norm=None, use_xyz=True, bias=False):
        super().__init__()
        assert len(radii) == len(nsamples) == len(mlps)
        self.npoint = npoint
        self.groupers = nn.ModuleList()
        self.mlps = nn.ModuleList()
        for radius, nsample, spec in zip(radii, nsamples, mlps):
            self.groupers.append(QueryAndGroup(radius, nsample, use_xyz) if npoint is not None else GroupAll(use_xyz))
            spec = list(spec)
            if use_xyz:
                spec[0] += 3
            self.mlps.append(gen_CNN(spec, conv=nn.Conv2d, batch_norm=batch_norm, bias=bias))
        self.sampled = None

    def forward(self, xyz, features=None):
        if self.training:
            raise NotImplementedError(_TRAINING)
        new_xyz = None
        if self.npoint is not None:
            self.sampled = ops.furthest_point_sampling(xyz, self.npoint)
            new_xyz = torch.gather(xyz, 1, self.sampled.long().unsqueeze(2).expand(-1, -1, 3))
        out = [run_channels_last(mlp, grouper(xyz, new_xyz, features)).max(dim=2).values
               for grouper, mlp in zip(self.groupers, self.mlps)]
        return new_xyz, torch.cat(out, dim=2)


class PointnetSAModule(PointnetSAModuleMSG):
    """Single-scale set abstraction (pointnet.py:214-246)."""

    def __init__(self, *, mlp, npoint=None, radius=None, nsample=None, batch_norm=None, use_xyz=True, bias=False):
        super().__init__(mlps=[mlp], npoint=npoint, radii=[radius], nsamples=[nsample], batch_norm=batch_norm,
                         use_xyz=use_xyz, bias=bias)


class PointnetFPModule(nn.Module):
    """Feature propagation (pointnet.py:252-298): the known features are
    interpolated over the three nearest known points with inverse-distance
    weights, concatenated with the unknown points' own and passed through the
    MLP.  Channels-last in and out."""

    def __init__(self, *, mlp, batch_norm=None, bias=False):
        super().__init__()
        self.mlp = gen_CNN(mlp, conv=nn.Conv2d, batch_norm=batch_norm, bias=bias)

    def forward(self, unknown, known, unknown_feats, known_feats):
        if self.training:
            raise NotImplementedError(_TRAINING)
        dist2, idx = ops.three_nn(unknown, known)
        recip = 1.0 / (torch.sqrt(dist2) + 1e-8)
        weight = recip / torch.sum(recip, dim=2, keepdim=True)
        interpolated = ops.three_interpolate(known_feats.transpose(1, 2).contiguous(), idx, weight).transpose(1, 2)
        feats = interpolated if unknown_feats is None else torch.cat([interpolated, unknown_feats], dim=2)
        return run_channels_last(self.mlp, feats)


class Pointnet2MSG(nn.Module):
    """PointNet++ encoder / decoder (pointnet.py:40-104).  forward(pointcloud
    [B,N,3+c]) -> (xyz [B,N,3], features [B,N,fp_mlps[0][-1]])."""

    def __init__(self, in_channels=6, use_xyz=True, SA_config=None, fp_mlps=()):
        super().__init__()
        SA_config = SA_config or {"npoints": [128, 32, -1], "radius": [0.2, 0.4, 100], "nsample": [64, 64, 64],
                                  "mlps": [[128, 128, 128], [128, 128, 256], [256, 256, 512]]}
        self.SA_modules = nn.ModuleList()
        skip = [in_channels]
        out_channels = in_channels
        for i in range(len(SA_config["npoints"])):
            mlps = [[in_channels] + list(m) for m in SA_config["mlps"][i]]
            out_channels = sum(m[-1] for m in mlps)
            self.SA_modules.append(PointnetSAModuleMSG(npoint=SA_config["npoints"][i], radii=SA_config["radius"][i],
                                                       nsamples=SA_config["nsample"][i], mlps=mlps, use_xyz=use_xyz,
                                                       batch_norm=nn.BatchNorm2d))
            in_channels = out_channels
            skip.append(out_channels)
        self.FP_modules = nn.ModuleList()
        for i in range(len(fp_mlps)):
            pre = fp_mlps[i + 1][-1] if i + 1 < len(fp_mlps) else out_channels
            self.FP_modules.append(PointnetFPModule(mlp=[pre + skip[i]] + list(fp_mlps[i]), batch_norm=nn.BatchNorm2d))

    def forward(self, pointcloud):
        xyz = pointcloud[..., 0:3].contiguous()
        features = pointcloud[..., 3:].contiguous() if pointcloud.shape[-1] > 3 else None
        l_xyz, l_features = [xyz], [features]
        for sa in self.SA_modules:
            new_xyz, new_features = sa(l_xyz[-1], l_features[-1])
            l_xyz.append(new_xyz)
            l_features.append(new_features)
        for i in range(-1, -(len(self.FP_modules) + 1), -1):
            l_features[i - 1] = self.FP_modules[i](l_xyz[i - 1], l_xyz[i], l_features[i - 1], l_features[i])
        return l_xyz[0], l_features[0]


# ---------------------------------------------------------------------------
# boxes
# ---------------------------------------------------------------------------
def rotate_pc_along_y_torch(pc, rot_angle):
    """pc [n, ..., 3 + c] with x, z (columns 0 and 2) rotated about the y axis
    by rot_angle [n] (point_rcnn.py:1275-1295): x' = x cos a - z sin a,
    z' = x sin a + z cos a.  Returns a new tensor."""
    a = rot_angle.view((-1,) + (1,) * (pc.dim() - 2))
    cosa, sina = torch.cos(a), torch.sin(a)
    x, z = pc[..., 0], pc[..., 2]
    out = pc.clone()
    out[..., 0] = x * cosa - z * sina
    out[..., 2] = x * sina + z * cosa
    return out


def enlarge_box3d(boxes3d, extra_width):
    """boxes [n,7] (x, y, z, h, w, l, ry) grown by extra_width on every side;
    y stays the bottom face (roipool3d_utils.py:8-21)."""
    large = boxes3d.copy() if isinstance(boxes3d, np.ndarray) else boxes3d.clone()
    large[:, 3:6] += extra_width * 2
    large[:, 1] += extra_width
    return large


def canonical_transform(pooled, rois):
    """pooled [B,M,S,3+C], rois [B,M,7]: the pooled xyz moved to the roi's
    origin (x, y, z of the roi) and rotated by its ry (point_rcnn.py:878-884).
    Returns a new tensor."""
    B, M = rois.shape[:2]
    out = pooled.clone()
    out[..., 0:3] -= rois[:, :, None, 0:3]
    return rotate_pc_along_y_torch(out.view(B * M, pooled.shape[2], -1), rois[..., 6].reshape(-1)).view(pooled.shape)


def xywhr_to_xyxyr(boxes):
    """BEV boxes (x, y, w, h, r) -> (x1, y1, x2, y2, r) (objdet_helper.py:69)."""
    half_w, half_h = boxes[:, 2] / 2, boxes[:, 3] / 2
    return torch.stack([boxes[:, 0] - half_w, boxes[:, 1] - half_h, boxes[:, 0] + half_w, boxes[:, 1] + half_h,
                        boxes[:, 4]], dim=1)


def decode_bbox_target(roi_box3d, pred_reg, loc_scope, loc_bin_size, num_head_bin, anchor_size, get_xz_fine=True,
                       get_y_by_bin=False, loc_y_scope=0.5, loc_y_bin_size=0.25, get_ry_fine=False):
    """Bin-based box decoding (point_rcnn.py:1153-1272): roi_box3d [n,3]
    (points) or [n,7] (rois), pred_reg [n,C] -> boxes [n,7] (x, y, z, h, w, l,
    ry).  Works on CPU and GPU tensors."""
    anchor_size = anchor_size.to(roi_box3d.device)
    nbin = int(loc_scope / loc_bin_size) * 2
    ny = int(loc_y_scope / loc_y_bin_size) * 2

    def pick(lo, n, index):
        return torch.gather(pred_reg[:, lo:lo + n], 1, index.unsqueeze(1)).squeeze(1)

    x_bin = torch.argmax(pred_reg[:, 0:nbin], dim=1)
    z_bin = torch.argmax(pred_reg[:, nbin:2 * nbin], dim=1)
    pos_x = x_bin.float() * loc_bin_size + loc_bin_size / 2 - loc_scope
    pos_z = z_bin.float() * loc_bin_size + loc_bin_size / 2 - loc_scope
    start = 2 * nbin
    if get_xz_fine:
        pos_x = pos_x + pick(2 * nbin, nbin, x_bin) * loc_bin_size
        pos_z = pos_z + pick(3 * nbin, nbin, z_bin) * loc_bin_size
        start = 4 * nbin
    if get_y_by_bin:
        y_bin = torch.argmax(pred_reg[:, start:start + ny], dim=1)
        y_res = pick(start + ny, ny, y_bin) * loc_y_bin_size
        pos_y = y_bin.float() * loc_y_bin_size + loc_y_bin_size / 2 - loc_y_scope + y_res
        pos_y = pos_y + roi_box3d[:, 1]
        start += 2 * ny
    else:
        pos_y = roi_box3d[:, 1] + pred_reg[:, start]
        start += 1
    ry_bin = torch.argmax(pred_reg[:, start:start + num_head_bin], dim=1)
    ry_res_norm = pick(start + num_head_bin, num_head_bin, ry_bin)
    if get_ry_fine:  # pi / 2 split into bins
        per = (np.pi / 2) / num_head_bin
        ry = (ry_bin.float() * per + per / 2) + ry_res_norm * (per / 2) - np.pi / 4
    else:
        per = (2 * np.pi) / num_head_bin
        ry = (ry_bin.float() * per + ry_res_norm * (per / 2)) % (2 * np.pi)
        ry = torch.where(ry > np.pi, ry - 2 * np.pi, ry)
    start += 2 * num_head_bin
    assert start + 3 == pred_reg.shape[1], (start, pred_reg.shape)
    hwl = pred_reg[:, start:start + 3] * anchor_size + anchor_size
    box = torch.cat((pos_x.view(-1, 1), pos_y.view(-1, 1), pos_z.view(-1, 1), hwl, ry.view(-1, 1)), dim=1)
    if roi_box3d.shape[1] == 7:
        roi_ry = roi_box3d[:, 6]
        box = rotate_pc_along_y_torch(box, -roi_ry)
        box[:, 6] += roi_ry
    box[:, [0, 2]] += roi_box3d[:, [0, 2]]
    return box


class ProposalLayer(nn.Module):
    """Boxes from per-point (RPN) or per-roi (RCNN) regressions
    (point_rcnn.py:984-1150).  post_process: y moved to the bottom face, then
    per cloud the distance-based top-k and rotated NMS, zero-padded to
    nms_post rows; else NMS only, one ragged list entry per cloud."""

    def __init__(self, device=None, nms_pre=9000, nms_post=512, nms_thres=0.85, nms_post_val=None,
                 nms_thres_val=None, mean_size=(1.0,), loc_xz_fine=True, loc_scope=3.0, loc_bin_size=0.5,
                 num_head_bin=12, get_y_by_bin=False, get_ry_fine=False, loc_y_scope=0.5, loc_y_bin_size=0.25,
                 post_process=True):
        super().__init__()
        self.nms_pre, self.nms_post, self.nms_thres = nms_pre, nms_post, nms_thres
        self.nms_post_val, self.nms_thres_val = nms_post_val, nms_thres_val
        self.mean_size = torch.tensor(list(mean_size), dtype=torch.float32)  # not a buffer: not in the state_dict
        self.loc_scope, self.loc_bin_size, self.num_head_bin = loc_scope, loc_bin_size, num_head_bin
        self.loc_xz_fine, self.get_y_by_bin, self.get_ry_fine = loc_xz_fine, get_y_by_bin, get_ry_fine
        self.loc_y_scope, self.loc_y_bin_size = loc_y_scope, loc_y_bin_size
        self.post_process = post_process

    def _eval_nms(self):
        post = self.nms_post if self.training or self.nms_post_val is None else self.nms_post_val
        thres = self.nms_thres if self.training or self.nms_thres_val is None else self.nms_thres_val
        return post, thres

    def decode(self, rpn_reg, xyz):
        return decode_bbox_target(xyz.reshape(-1, xyz.shape[-1]), rpn_reg.reshape(-1, rpn_reg.shape[-1]),
                                  anchor_size=self.mean_size, loc_scope=self.loc_scope,
                                  loc_bin_size=self.loc_bin_size, num_head_bin=self.num_head_bin,
                                  get_xz_fine=self.loc_xz_fine, get_y_by_bin=self.get_y_by_bin,
                                  get_ry_fine=self.get_ry_fine, loc_y_scope=self.loc_y_scope,
                                  loc_y_bin_size=self.loc_y_bin_size).view(xyz.shape[0], -1, 7)

    def forward(self, rpn_scores, rpn_reg, xyz):
        B = xyz.shape[0]
        proposals = self.decode(rpn_reg, xyz)
        nms_post, nms_thres = self._eval_nms()
        if not self.post_process:
            boxes, scores = [], []
            for k in range(B):
                keep = ops.nms(xywhr_to_xyxyr(proposals[k][:, [0, 2, 3, 5, 6]]), rpn_scores[k].reshape(-1), nms_thres)
                boxes.append(proposals[k, keep])
                scores.append(rpn_scores[k, keep])
            return boxes, scores
        proposals[..., 1] += proposals[..., 3] / 2  # y: the centre of the bottom face
        order = torch.sort(rpn_scores, dim=1, descending=True)[1]
        ret_boxes = rpn_scores.new_zeros(B, nms_post, 7)
        ret_scores = rpn_scores.new_zeros(B, nms_post)
        for k in range(B):
            s, p = self.distance_based_proposal(rpn_scores[k], proposals[k], order[k])
            ret_boxes[k, :p.shape[0]] = p
            ret_scores[k, :p.shape[0]] = s
        return ret_boxes, ret_scores

    def distance_based_proposal(self, scores, proposals, order):
        """scores [N], proposals [N,7], order [N] (descending score): 70 % of
        the budget from z in (0, 40], the rest from (40, 80]; when the second
        range is empty its budget goes to the next boxes of the first."""
        nms_post, nms_thres = self._eval_nms()
        ranges = [0, 40.0, 80.0]
        pre = [0, int(self.nms_pre * 0.7), self.nms_pre - int(self.nms_pre * 0.7)]
        post = [0, int(nms_post * 0.7), nms_post - int(nms_post * 0.7)]
        scores, proposals = scores[order], proposals[order]
        dist = proposals[:, 2]
        first = (dist > ranges[0]) & (dist <= ranges[1])
        out_s, out_p = [], []
        for i in (1, 2):
            mask = (dist > ranges[i - 1]) & (dist <= ranges[i])
            if mask.sum() != 0:  # one host read per range, as in the reference
                cur_s, cur_p = scores[mask][:pre[i]], proposals[mask][:pre[i]]
            else:
                assert i == 2, i
                cur_s, cur_p = scores[first][pre[1]:][:pre[2]], proposals[first][pre[1]:][:pre[2]]
            keep = ops.nms(xywhr_to_xyxyr(cur_p[:, [0, 2, 3, 5, 6]]), cur_s, nms_thres)[:post[i]]
            out_s.append(cur_s[keep])
            out_p.append(cur_p[keep])
        return torch.cat(out_s, dim=0), torch.cat(out_p, dim=0)


# ---------------------------------------------------------------------------
# the two stages
# ---------------------------------------------------------------------------
def _head(in_ch, widths, out_ch, batch_norm, db_ratio):
    layers, chans = [], [in_ch, *widths]
    for cin, cout in zip(chans[:-1], chans[1:]):
        if batch_norm:
            layers += [nn.Conv1d(cin, cout, 1, bias=False), nn.BatchNorm1d(cout), nn.ReLU(inplace=True),
                       nn.Dropout(db_ratio)]
        else:
            layers += [nn.Conv1d(cin, cout, 1, bias=True), nn.ReLU(inplace=True)]
    layers.append(nn.Conv1d(chans[-1], out_ch, 1, bias=True))
    return nn.Sequential(*layers)


def _reg_channels(pl):
    nbin = int(pl.loc_scope / pl.loc_bin_size) * 2
    ny = int(pl.loc_y_scope / pl.loc_y_bin_size) * 2
    return nbin * (4 if pl.loc_xz_fine else 2) + pl.num_head_bin * 2 + 3 + (2 * ny if pl.get_y_by_bin else 1)


class RPN(nn.Module):
    """Stage 1 (point_rcnn.py:616-692): backbone, per-point foreground score
    and box regression.  forward(points [B,N,3+c]) -> (cls [B,N,1], reg
    [B,N,C], xyz [B,N,3], features [B,N,128] channels-last)."""

    def __init__(self, device=None, backbone=None, cls_in_ch=128, cls_out_ch=(128,), reg_in_ch=128,
                 reg_out_ch=(128,), db_ratio=0.5, head=None, focal_loss=None, loss_weight=(1.0, 1.0), **kwargs):
        super().__init__()
        self.backbone = Pointnet2MSG(**(backbone or {}))
        self.proposal_layer = ProposalLayer(device=device, **(head or {}))
        self.cls_blocks = _head(cls_in_ch, cls_out_ch, 1, True, db_ratio)
        self.reg_blocks = _head(reg_in_ch, reg_out_ch, _reg_channels(self.proposal_layer), True, db_ratio)

    def forward(self, x):
        if self.training:
            raise NotImplementedError(_TRAINING)
        xyz, features = self.backbone(x)
        return run_channels_last(self.cls_blocks, features), run_channels_last(self.reg_blocks, features), xyz, features


class RCNN(nn.Module):
    """Stage 2 (point_rcnn.py:743-916): roi_pool, canonical transform, three
    set-abstraction levels over each roi's points, classification and box
    refinement per roi.  `pool_index` / `pool_empty_flag` hold roi_pool's
    point index per slot and its flags of the last forward."""

    def __init__(self, num_classes, device=None, in_channels=128, SA_config=None, cls_out_ch=(256, 256),
                 reg_out_ch=(256, 256), db_ratio=0.5, use_xyz=True, xyz_up_layer=(128, 128), head=None,
                 target_head=None, loss=None):
        super().__init__()
        SA_config = SA_config or {"npoints": [128, 32, -1], "radius": [0.2, 0.4, 100], "nsample": [64, 64, 64],
                                  "mlps": [[128, 128, 128], [128, 128, 256], [256, 256, 512]]}
        target_head = target_head or {}
        self.rcnn_input_channel = 5
        self.pool_extra_width = target_head.get("pool_extra_width", 1.0)
        self.num_points = target_head.get("num_points", 512)
        self.proposal_layer = ProposalLayer(device=device, **(head or {}))
        self.SA_modules = nn.ModuleList()
        for i, npoint in enumerate(SA_config["npoints"]):
            mlp = [in_channels] + list(SA_config["mlps"][i])
            self.SA_modules.append(PointnetSAModule(npoint=None if npoint == -1 else npoint,
                                                    radius=SA_config["radius"][i], nsample=SA_config["nsample"][i],
                                                    mlp=mlp, use_xyz=use_xyz, bias=True))
            in_channels = mlp[-1]
        self.xyz_up_layer = gen_CNN([self.rcnn_input_channel] + list(xyz_up_layer), conv=nn.Conv2d)
        c_out = xyz_up_layer[-1]
        self.merge_down_layer = gen_CNN([c_out * 2, c_out], conv=nn.Conv2d)
        self.cls_blocks = _head(in_channels, cls_out_ch, 1 if num_classes == 2 else num_classes, False, db_ratio)
        self.reg_blocks = _head(in_channels, reg_out_ch, _reg_channels(self.proposal_layer), False, db_ratio)
        self.pool_index = self.pool_empty_flag = None

    def forward(self, roi_boxes3d, rpn_xyz, rpn_features, seg_mask, pts_depth):
        """rois [B,M,7], rpn_xyz [B,N,3], rpn_features [B,N,C] channels-last,
        seg_mask, pts_depth [B,N] -> {"rois", "cls" [B*M, 1 or classes],
        "reg" [B*M, C]}."""
        if self.training:
            raise NotImplementedError(_TRAINING)
        B = roi_boxes3d.shape[0]
        pts_feature = torch.cat((seg_mask.unsqueeze(2), (pts_depth / 70.0 - 0.5).unsqueeze(2), rpn_features), dim=2)
        pooled_boxes = enlarge_box3d(roi_boxes3d.reshape(-1, 7), self.pool_extra_width).view(B, -1, 7)
        pooled, self.pool_empty_flag, self.pool_index = ops.roi_pool_indexed(
            rpn_xyz.contiguous(), pooled_boxes.contiguous(), pts_feature.contiguous(), self.num_points)
        pooled = canonical_transform(pooled, roi_boxes3d)
        pts_input = pooled.view(-1, pooled.shape[2], pooled.shape[3])
        xyz = pts_input[..., 0:3].contiguous()
        xyz_feature = run_channels_last(self.xyz_up_layer, pts_input[..., 0:self.rcnn_input_channel])
        merged = torch.cat((xyz_feature, pts_input[..., self.rcnn_input_channel:]), dim=2)
        features = run_channels_last(self.merge_down_layer, merged)
        for sa in self.SA_modules:
            xyz, features = sa(xyz, features)
        rcnn_cls = run_channels_last(self.cls_blocks, features).squeeze(1)
        rcnn_reg = run_channels_last(self.reg_blocks, features).squeeze(1)
        return {"rois": roi_boxes3d, "cls": rcnn_cls, "reg": rcnn_reg}


def _points(inputs):
    p = inputs if isinstance(inputs, torch.Tensor) else (
        inputs["point"] if isinstance(inputs, dict) else getattr(inputs, "point"))
    return p if isinstance(p, torch.Tensor) else torch.stack(list(p))


class PointRCNN(nn.Module):
    """Module tree and state_dict of ml3d PointRCNN (point_rcnn.py:55-140),
    eval() forward only.  forward takes the clouds as a tensor [B,N,3+c], or a
    batch whose `point` (attribute or key) is that tensor or a list of B
    [N,3+c] tensors, and returns {"rois", "cls", "reg"}: of the RPN for mode
    "RPN" (rois [B,M,7], cls [B,N,1], reg [B,N,C]), of the RCNN for mode
    "RCNN" (cls [B*M,1], reg [B*M,C]).  `roi_scores` [B,M] holds the RPN scores
    of the rois of the last forward (the reference drops them)."""

    def __init__(self, name="PointRCNN", device="cuda", classes=("Car",), score_thres=0.3, npoints=16384, rpn=None,
                 rcnn=None, mode="RCNN", **kwargs):
        super().__init__()
        assert mode in ("RPN", "RCNN")
        self.name, self.mode = name, mode
        self.npoints, self.classes, self.score_thres = npoints, list(classes), score_thres
        self.lbl2name = dict(enumerate(self.classes))
        self.rpn = RPN(device=device, **(rpn or {}))
        self.rcnn = RCNN(device=device, num_classes=len(self.classes), **(rcnn or {}))
        self.roi_scores = None

    def forward(self, inputs):
        if self.training:
            raise NotImplementedError(_TRAINING)
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            require_gpu()
            raise RuntimeError("PointRCNN: the model must be on the GPU (there is no CPU path)")
        points = _points(inputs)
        if points.dim() != 3 or points.shape[2] < 3 or points.dtype != torch.float32:
            raise RuntimeError(f"PointRCNN: points must be float32 [B, N, 3 + c], got {points.dtype} "
                               f"{list(points.shape)}")
        with torch.no_grad():
            points = points.detach().to(dev).contiguous()
            cls_score, reg_score, xyz, features = self.rpn(points)
            scores_raw = cls_score[:, :, 0]
            rois, self.roi_scores = self.rpn.proposal_layer(scores_raw, reg_score, xyz)
            if self.mode == "RPN":
                return {"rois": rois, "cls": cls_score, "reg": reg_score}
            seg_mask = (torch.sigmoid(scores_raw) > self.score_thres).float()
            pts_depth = torch.norm(xyz, p=2, dim=2)
            return self.rcnn(rois, xyz, features, seg_mask, pts_depth)

    def get_bboxes(self, results):
        """The reference's inference_end (point_rcnn.py:375-402) up to, and
        not including, its BEVBox3D objects: per cloud (boxes [k,7] camera
        frame (x, y, z, h, w, l, ry), scores [k], labels int64 [k]) of the
        refined boxes that survive the RCNN's NMS and the score threshold."""
        rois = results["rois"]
        B = rois.shape[0]
        with torch.no_grad():
            cls = results["cls"].view(B, -1, results["cls"].shape[1])
            reg = results["reg"].view(B, -1, results["reg"].shape[1])
            boxes, scores = self.rcnn.proposal_layer(cls, reg, rois)
            out = []
            for bb, sc in zip(boxes, scores):
                if sc.shape[-1] == 1:
                    sc = torch.sigmoid(sc).reshape(-1)
                    labels = (sc < self.score_thres).long()
                else:
                    labels = torch.argmax(sc, dim=-1)
                    sc = torch.gather(F.softmax(sc, dim=-1), 1, labels.unsqueeze(1)).squeeze(1)
                keep = sc > self.score_thres
                out.append((bb[keep], sc[keep], labels[keep]))
            return out


__all__ = ["PointRCNN", "RPN", "RCNN", "ProposalLayer", "Pointnet2MSG", "PointnetSAModuleMSG", "PointnetSAModule",
           "PointnetFPModule", "QueryAndGroup", "GroupAll", "decode_bbox_target", "enlarge_box3d",
           "canonical_transform", "rotate_pc_along_y_torch", "xywhr_to_xyxyr", "gen_CNN", "run_channels_last"]
