"""PVCNN (ml3d/torch/models/pvcnn.py): the module tree and state_dict of the
reference, with the point <-> voxel transfers on the HIP kernels of
csrc/pvcnn.hip.

Per PVConv block the reference (a) normalises the coordinates, (b) builds the
voxel assignment and scatter-adds every channel on its own (avg_voxelize,
pvcnn.py:579-619), (c) runs Conv3d / BatchNorm3d and (d) devoxelizes
trilinearly.  Here (a), the voxel plan of (b) and the corner indices and
weights of (d) depend on the coordinates and the resolution only, so the
model computes them once per distinct resolution per forward (the default net
has r = 32 once and r = 16 three times) and every block of that resolution
shares them; the per-voxel lists the devoxelize backward sums over are built
once per resolution on the first backward.  (a) stays in torch exactly as the
reference writes it: one ulp there moves points across voxel boundaries.
Conv3d and BatchNorm3d stay torch / MIOpen.

Every sum in the HIP ops runs in one fixed order (no float atomics): the
point <-> voxel transfers are bitwise reproducible, forward and backward.
Worst case: with every point in one voxel that voxel is summed by a single
lane (N terms per channel); accepted.
"""
import functools

import torch
import torch.nn as nn
from torch.autograd import Function

from . import _lib
from ._util import gpu_device, ptr, stream_handle, to_dev, workspace


# ---------------------------------------------------------------------------
# voxel plan + mean voxelize
# ---------------------------------------------------------------------------
class VoxelPlan:
    """The points of every voxel in ascending index (opaque workspace) and the
    per-voxel counts, built once per (vox int32 [B,3,N], r)."""

    def __init__(self, vox, resolution):
        dev = gpu_device(vox)
        if not isinstance(vox, torch.Tensor) or vox.dtype != torch.int32 or vox.dim() != 3 or vox.shape[1] != 3:
            raise RuntimeError("vox must be int32 [B, 3, N], got "
                               f"{getattr(vox, 'dtype', type(vox))} {list(getattr(vox, 'shape', []))}")
        self.r = int(resolution)
        if self.r < 1:
            raise RuntimeError(f"resolution must be >= 1, got {self.r}")
        self.vox = to_dev(vox, dev)
        self.B, _, self.N = vox.shape
        self.cnt = torch.empty((self.B, self.r ** 3), dtype=torch.int32, device=dev)
        self.ws = workspace(_lib.load().o3dml_avg_voxelize_plan_workspace_size(self.B, self.N, self.r), dev)
        _lib.call("o3dml_avg_voxelize_plan", ptr(self.vox), self.B, self.N, self.r, ptr(self.cnt), ptr(self.ws),
                  self.ws.numel(), stream_handle(dev))


def _check_feat(name, t, B, last):
    if t.dtype != torch.float32 or t.dim() != 3 or t.shape[0] != B or t.shape[2] != last:
        raise RuntimeError(f"{name} must be float32 [{B}, C, {last}], got {t.dtype} {list(t.shape)}")


class AvgVoxelization(Function):
    """feat [B,C,N], VoxelPlan -> grid [B,C,r,r,r]: the mean of the features
    of each voxel's points, summed in ascending point index, 0 where empty."""

    @staticmethod
    def forward(ctx, feat, plan):
        _check_feat("feat", feat, plan.B, plan.N)
        dev = plan.cnt.device
        f = to_dev(feat.detach(), dev)
        C, r = f.shape[1], plan.r
        grid = torch.empty((plan.B, C, r, r, r), dtype=torch.float32, device=dev)
        _lib.call("o3dml_avg_voxelize_forward", ptr(f), ptr(plan.ws), ptr(plan.cnt), plan.B, C, plan.N, r, ptr(grid),
                  stream_handle(dev))
        ctx.plan = plan
        return grid

    @staticmethod
    def backward(ctx, grad_grid):
        plan = ctx.plan
        dev = plan.cnt.device
        g = to_dev(grad_grid, dev, torch.float32)
        C = g.shape[1]
        out = torch.empty((plan.B, C, plan.N), dtype=torch.float32, device=dev)
        _lib.call("o3dml_avg_voxelize_backward", ptr(g), ptr(plan.vox), ptr(plan.cnt), plan.B, C, plan.N, plan.r,
                  ptr(out), stream_handle(dev))
        return out, None


def avg_voxelize(feat, vox_or_plan, r=None):
    """Mean voxelize (pvcnn.py:579-619): feat [B,C,N] and either int32 voxel
    coordinates [B,3,N] with the resolution, or a VoxelPlan built from them."""
    plan = vox_or_plan if isinstance(vox_or_plan, VoxelPlan) else VoxelPlan(vox_or_plan, r)
    return AvgVoxelization.apply(feat, plan)


# ---------------------------------------------------------------------------
# trilinear devoxelize
# ---------------------------------------------------------------------------
class DevoxelizePlan:
    """Corner indices and weights of coords [B,3,N] at one resolution, written
    by the first devoxelize that uses the plan, and the per-voxel entry lists
    the backward sums over, built by the first backward."""

    def __init__(self, coords, resolution):
        self.coords = coords.detach().contiguous()
        self.r = int(resolution)
        self.inds = self.wgts = self.ws = None

    def backward_lists(self):
        if self.ws is None:
            dev = self.inds.device
            B, _, N = self.inds.shape
            self.ws = workspace(_lib.load().o3dml_trilinear_devoxelize_backward_workspace_size(B, N, self.r), dev)
            _lib.call("o3dml_trilinear_devoxelize_backward_plan", ptr(self.inds), B, N, self.r, ptr(self.ws),
                      self.ws.numel(), stream_handle(dev))
        return self.ws


class TrilinearDevoxelization(Function):
    """features [B,C,r,r,r], coords [B,3,N] (grid units) -> [B,C,N]
    (pvcnn.py:17-63).  `plan` (a DevoxelizePlan of the same coords and
    resolution) shares the indices, weights and backward lists between calls;
    without one the call makes its own."""

    @staticmethod
    def forward(ctx, features, coords, resolution, is_training=True, plan=None):
        if plan is None:
            plan = DevoxelizePlan(coords, resolution)
        dev = gpu_device(features, plan.coords)
        r = plan.r
        B, _, N = plan.coords.shape
        if (features.dtype != torch.float32 or features.dim() != 5 or features.shape[0] != B
                or tuple(features.shape[2:]) != (r, r, r)):
            raise RuntimeError(f"features must be float32 [{B}, C, {r}, {r}, {r}], got {features.dtype} "
                               f"{list(features.shape)}")
        f = to_dev(features.detach(), dev)
        c = to_dev(plan.coords, dev, torch.float32)
        C = f.shape[1]
        outs = torch.empty((B, C, N), dtype=torch.float32, device=dev)
        first = is_training and plan.inds is None
        if first:  # later calls of this plan recompute them in registers and store nothing
            plan.inds = torch.empty((B, 8, N), dtype=torch.int32, device=dev)
            plan.wgts = torch.empty((B, 8, N), dtype=torch.float32, device=dev)
        _lib.call("o3dml_trilinear_devoxelize_forward", ptr(c), ptr(f), B, C, N, r, int(first), ptr(outs),
                  ptr(plan.inds) if first else None, ptr(plan.wgts) if first else None, stream_handle(dev))
        if is_training:
            ctx.plan = plan
        return outs

    @staticmethod
    def backward(ctx, grad_output):
        plan = ctx.plan
        dev = plan.inds.device
        g = to_dev(grad_output, dev, torch.float32)
        B, C, N = g.shape
        r = plan.r
        out = torch.empty((B, C, r, r, r), dtype=torch.float32, device=dev)
        _lib.call("o3dml_trilinear_devoxelize_backward_planned", ptr(g), ptr(plan.wgts), ptr(plan.backward_lists()),
                  B, C, N, r, ptr(out), stream_handle(dev))
        return out, None, None, None, None


trilinear_devoxelize = TrilinearDevoxelization.apply


# ---------------------------------------------------------------------------
# modules (names as the reference's state_dict requires)
# ---------------------------------------------------------------------------
class _Shared:
    """What the blocks of one forward share per resolution."""

    def __init__(self):
        self.by_resolution = {}


class Voxelization(nn.Module):
    """Normalised coordinates -> voxel grid of mean features (pvcnn.py:622-670)."""

    def __init__(self, resolution, normalize=True, eps=1e-6):
        super().__init__()
        self.r = int(resolution)
        self.normalize = normalize
        self.eps = eps

    def assign(self, coords):
        """(norm_coords [B,3,N] in [0, r-1], VoxelPlan) — pvcnn.py:653-662."""
        coords = coords.detach()
        norm_coords = coords - coords.mean(2, keepdim=True)
        if self.normalize:
            norm_coords = norm_coords / (norm_coords.norm(dim=1, keepdim=True).max(dim=2, keepdim=True).values * 2.0 +
                                         self.eps) + 0.5
        else:
            norm_coords = (norm_coords + 1) / 2.0
        norm_coords = torch.clamp(norm_coords * self.r, 0, self.r - 1)
        vox_coords = torch.round(norm_coords).to(torch.int32)
        return norm_coords, VoxelPlan(vox_coords, self.r)

    def forward(self, features, coords, shared=None):
        key = (self.r, self.normalize, self.eps)
        hit = None if shared is None else shared.by_resolution.get(key)
        if hit is None:
            norm_coords, plan = self.assign(coords)
            hit = (norm_coords, plan, DevoxelizePlan(norm_coords, self.r))
            if shared is not None:
                shared.by_resolution[key] = hit
        return AvgVoxelization.apply(features, hit[1]), hit[0], hit[2]

    def extra_repr(self):
        return "resolution={}{}".format(self.r, ", normalized eps = {}".format(self.eps) if self.normalize else "")


class SE3d(nn.Module):
    def __init__(self, channel, reduction=8):
        super().__init__()
        self.fc = nn.Sequential(nn.Linear(channel, channel // reduction, bias=False), nn.ReLU(inplace=True),
                                nn.Linear(channel // reduction, channel, bias=False), nn.Sigmoid())

    def forward(self, inputs):
        return inputs * self.fc(inputs.mean(-1).mean(-1).mean(-1)).view(inputs.shape[0], inputs.shape[1], 1, 1, 1)


class SharedMLP(nn.Module):
    """1x1 convolution + BatchNorm + ReLU per output width (pvcnn.py:455-501)."""

    def __init__(self, in_channels, out_channels, dim=1):
        super().__init__()
        if dim not in (1, 2):
            raise ValueError(dim)
        conv, bn = (nn.Conv1d, nn.BatchNorm1d) if dim == 1 else (nn.Conv2d, nn.BatchNorm2d)
        if not isinstance(out_channels, (list, tuple)):
            out_channels = [out_channels]
        layers = []
        for oc in out_channels:
            layers += [conv(in_channels, oc, 1), bn(oc), nn.ReLU(True)]
            in_channels = oc
        self.layers = nn.Sequential(*layers)

    def forward(self, inputs):
        if isinstance(inputs, (list, tuple)):
            return (self.layers(inputs[0]), *inputs[1:])
        return self.layers(inputs)


class PVConv(nn.Module):
    """Voxel branch (voxelize, two Conv3d + BN + LeakyReLU, devoxelize) plus
    point branch (SharedMLP), summed (pvcnn.py:504-576).  Inputs (features,
    coords) or (features, coords, shared)."""

    def __init__(self, in_channels, out_channels, kernel_size, resolution, with_se=False, normalize=True, eps=1e-6):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.resolution = kernel_size, resolution
        self.voxelization = Voxelization(resolution, normalize=normalize, eps=eps)
        voxel_layers = []
        for cin in (in_channels, out_channels):
            voxel_layers += [nn.Conv3d(cin, out_channels, kernel_size, stride=1, padding=kernel_size // 2),
                             nn.BatchNorm3d(out_channels, eps=1e-4), nn.LeakyReLU(0.1, True)]
        if with_se:
            voxel_layers.append(SE3d(out_channels))
        self.voxel_layers = nn.Sequential(*voxel_layers)
        self.point_features = SharedMLP(in_channels, out_channels)

    def forward(self, inputs):
        features, coords = inputs[0], inputs[1]
        shared = inputs[2] if len(inputs) > 2 else None
        grid, _, devox = self.voxelization(features, coords, shared)
        grid = self.voxel_layers(grid)
        keep = self.training or (torch.is_grad_enabled() and grid.requires_grad)
        voxel_features = trilinear_devoxelize(grid, devox.coords, self.resolution, keep, devox)
        return (voxel_features + self.point_features(features), *inputs[1:])


def _linear_bn_relu(in_channels, out_channels):
    return nn.Sequential(nn.Linear(in_channels, out_channels), nn.BatchNorm1d(out_channels), nn.ReLU(True))


def create_mlp_components(in_channels, out_channels, classifier=False, dim=2, width_multiplier=1):
    """Layers of an MLP head (pvcnn.py:358-408): widths below 1 are Dropout
    rates; the last entry is a plain Linear / Conv1d when classifier."""
    r = width_multiplier
    block = _linear_bn_relu if dim == 1 else SharedMLP
    if not isinstance(out_channels, (list, tuple)):
        out_channels = [out_channels]
    if len(out_channels) == 0 or (len(out_channels) == 1 and out_channels[0] is None):
        return nn.Sequential(), in_channels, in_channels
    layers = []
    for oc in out_channels[:-1]:
        if oc < 1:
            layers.append(nn.Dropout(oc))
        else:
            oc = int(r * oc)
            layers.append(block(in_channels, oc))
            in_channels = oc
    last = out_channels[-1]
    if classifier:
        layers.append(nn.Linear(in_channels, last) if dim == 1 else nn.Conv1d(in_channels, last, 1))
        return layers, last
    layers.append(block(in_channels, int(r * last)))
    return layers, int(r * last)


def create_pointnet_components(blocks, in_channels, with_se=False, normalize=True, eps=1e-6, width_multiplier=1,
                               voxel_resolution_multiplier=1):
    """PVConv / SharedMLP stack from (out_channels, num_blocks, resolution)
    rows (pvcnn.py:411-452) -> (layers, out channels, concatenated channels)."""
    r, vr = width_multiplier, voxel_resolution_multiplier
    layers, concat_channels = [], 0
    for out_channels, num_blocks, voxel_resolution in blocks:
        out_channels = int(r * out_channels)
        if voxel_resolution is None:
            block = SharedMLP
        else:
            block = functools.partial(PVConv, kernel_size=3, resolution=int(vr * voxel_resolution), with_se=with_se,
                                      normalize=normalize, eps=eps)
        for _ in range(num_blocks):
            layers.append(block(in_channels, out_channels))
            in_channels = out_channels
            concat_channels += out_channels
    return layers, in_channels, concat_channels


class PVCNN(nn.Module):
    """Module tree and state_dict of ml3d PVCNN (pvcnn.py:66-160): forward
    takes {'point': [B,3,N], 'feat': [B,9,N]} and returns [B,N,num_classes]."""

    blocks = ((64, 1, 32), (64, 2, 16), (128, 1, 16), (1024, 1, None))

    def __init__(self, name="PVCNN", device="cuda", num_classes=13, num_points=40960, extra_feature_channels=6,
                 width_multiplier=1, voxel_resolution_multiplier=1, batcher="DefaultBatcher", augment=None,
                 ignored_label_inds=(), **kwargs):
        super().__init__()
        self.cfg = dict(name=name, num_classes=num_classes, num_points=num_points,
                        extra_feature_channels=extra_feature_channels, width_multiplier=width_multiplier,
                        voxel_resolution_multiplier=voxel_resolution_multiplier, batcher=batcher, augment=augment,
                        ignored_label_inds=list(ignored_label_inds), **kwargs)
        self.device = device
        self.in_channels = extra_feature_channels + 3
        layers, channels_point, concat_channels_point = create_pointnet_components(
            blocks=self.blocks, in_channels=self.in_channels, with_se=False, width_multiplier=width_multiplier,
            voxel_resolution_multiplier=voxel_resolution_multiplier)
        self.point_features = nn.ModuleList(layers)
        layers, channels_cloud = create_mlp_components(in_channels=channels_point, out_channels=[256, 128],
                                                       classifier=False, dim=1, width_multiplier=width_multiplier)
        self.cloud_features = nn.Sequential(*layers)
        layers, _ = create_mlp_components(in_channels=concat_channels_point + channels_cloud,
                                          out_channels=[512, 0.3, 256, 0.3, num_classes], classifier=True, dim=2,
                                          width_multiplier=width_multiplier)
        self.classifier = nn.Sequential(*layers)

    def forward(self, inputs):
        dev = next(self.parameters()).device
        coords = inputs["point"].to(dev)
        feat = inputs["feat"].to(dev)
        shared = _Shared()
        outs = []
        for block in self.point_features:
            feat = block((feat, coords, shared))[0]
            outs.append(feat)
        cloud = self.cloud_features(feat.max(dim=-1, keepdim=False).values)
        outs.append(cloud.unsqueeze(-1).repeat([1, 1, coords.size(-1)]))
        return self.classifier(torch.cat(outs, dim=1)).transpose(1, 2)

    def get_loss(self, sem_seg_loss, results, inputs, device):
        """(loss, labels, scores) over the labels not in ignored_label_inds,
        remapped to the logit columns (pvcnn.py:284-305)."""
        num_classes = self.cfg["num_classes"]
        ignored = [int(i) for i in self.cfg["ignored_label_inds"]]
        labels = inputs["data"]["label"].reshape(-1).to(device)
        scores = results.reshape(-1, results.shape[-1]).to(device)
        keep = torch.ones_like(labels, dtype=torch.bool)
        for ign in ignored:
            keep &= labels != ign
        scores, labels = scores[keep], labels[keep].long()
        remap = list(range(num_classes))
        for ign in ignored:
            if ign >= 0:
                remap = remap[:ign] + [0] + remap[ign:]
        labels = torch.tensor(remap, dtype=torch.int64, device=labels.device)[labels]
        return sem_seg_loss.weighted_CrossEntropyLoss(scores, labels), labels, scores


__all__ = ["PVCNN", "PVConv", "SharedMLP", "SE3d", "Voxelization", "VoxelPlan", "DevoxelizePlan", "AvgVoxelization",
           "TrilinearDevoxelization", "avg_voxelize", "trilinear_devoxelize", "create_mlp_components",
           "create_pointnet_components"]
