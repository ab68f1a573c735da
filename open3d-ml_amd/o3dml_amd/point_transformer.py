"""PointTransformer (ml3d/torch/models/point_transformer.py): the module tree
and state_dict of the reference, its eval() forward on the HIP kernels of
csrc/point_transformer.hip and the ragged FPS of csrc/pointnet2.hip, and the
gradients of that forward (csrc/point_transformer_grad.hip) with the
BatchNorms frozen on their running statistics.

The reference searches neighbours on the CPU in every layer (knn_batch
:700-734, twice per Transformer layer), loops over the clouds for the
farthest-point sampling and materialises four (n, nsample, c) tensors per
Transformer layer.  Here a search is a `Neighbours` plan (an index [m, k] and,
where asked, the distances) built on the GPU by ops.knn_search, and what
depends on the points only is shared: every block of a level, in encoder and
decoder, searches the same points with the same nsample, so the model builds
one self-kNN plan per level (5), one per TransitionDown (4) and one k = 3 plan
with distances per TransitionUp (4): 13 per forward where the reference runs
28 searches.  The sampling of a level is one launch for all clouds.  A
Transformer layer keeps one (n, nsample, c) tensor, the input of
Linear(c, c/8): `relation` gathers k, subtracts q, adds the positional
encoding and applies the first BatchNorm and ReLU of linear_w in one pass, and
`aggregate` gathers v, recomputes the positional encoding, and does the
softmax over the neighbours and the weighted sum in registers.  The dense
Linears stay on torch / rocBLAS.

BatchNorms are used in eval form, folded to scale and shift on every call
from the module's current tensors: nothing folded is kept between forwards.
After `level_row_splits` (host arithmetic on a host copy of row_splits) the
forward reads nothing back from the device.  Batch-statistics training is not
built: forward() in train() mode raises NotImplementedError.

Gradients.  The four ops (relation, aggregate, knn_interpolate, group) are
differentiable in their feature tensors, in weight, scale_w / shift_w and the
six pos tensors, never in coordinates (a coordinate tensor that requires grad
raises): with grad mode on and such an input requiring grad they record a
torch.autograd.Function whose backward runs the HIP kernels; otherwise they
launch what they always did and return a detached result.  A scatter-add of
the backward (d feat_k, d feat_v, d feat) is a sum per source row over the
plan's inverse neighbour list (Neighbours.inverse(), built once per plan and
kept on it) in ascending pair order.  The backward saves the forward's inputs
and relation's output; softmax and positional encoding are recomputed.  The
first positional Linear, BatchNorm and ReLU (three floats per pair) are
finished with a handful of torch ops from the kernels' dh.
A plain model(batch) never records: inside `with recording_grad():` (thread
local, nests) and with grad mode on, the eval() forwards of the modules below
record autograd, BatchNorms folded from the modules' weight and bias with
differentiable torch ops and the running statistics as constants (frozen-BN
fine-tuning, saliency); the dense Linears, ReLUs, the maximum over nsample,
the head's per-cloud mean and the residual adds run under torch autograd.

Every sum in the HIP ops runs in one fixed order (no float atomics): a second
forward, and a second backward, is bitwise equal to the first.
"""
import contextlib
import threading

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib, ops
from ._util import gpu_device, ptr, require_gpu, row_splits_host, stream_handle, to_dev, workspace

MAX_NSAMPLE = 64
MAX_INTERPOLATE_K = 8

# ---------------------------------------------------------------------------
# the gradient switch
# ---------------------------------------------------------------------------
_switch = threading.local()


@contextlib.contextmanager
def recording_grad():
    """Inside this context (per thread, nests), with grad mode on, the eval()
    forwards of the modules below record autograd; BatchNorms stay frozen."""
    depth = getattr(_switch, "depth", 0)
    _switch.depth = depth + 1
    try:
        yield
    finally:
        _switch.depth = depth


def _recording():
    return getattr(_switch, "depth", 0) > 0 and torch.is_grad_enabled()


def _graph():
    """The context a module forward runs in: autograd inside the switch, else none."""
    return contextlib.nullcontext() if _recording() else torch.no_grad()


def _relu(x):
    return F.relu(x) if _recording() else F.relu_(x)


def _param(t):
    return t if _recording() else t.detach()


def _f32(name, t, shape):
    """t as a detached contiguous float32 tensor of `shape` (None: any size)."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != len(shape) or any(
            s is not None and int(d) != int(s) for d, s in zip(t.shape, shape)):
        want = ", ".join("*" if s is None else str(int(s)) for s in shape)
        raise RuntimeError(f"{name} must be float32 [{want}], got {getattr(t, 'dtype', type(t))} "
                           f"{list(getattr(t, 'shape', []))}")
    return t.detach()


# ---------------------------------------------------------------------------
# neighbour plans
# ---------------------------------------------------------------------------
class Neighbours:
    """For m queries the rows of their k neighbours among n_src source rows:
    index int32 [m, k] on the GPU and, where asked, distance float32 [m, k]
    (as knn_search returns it: squared for L2).  The kernels trust a plan, so
    this constructor, given an explicit index, checks its range once (one host
    read); `from_knn` builds one from ops.knn_search, whose rows are in range
    by construction."""

    def __init__(self, index, n_src, distance=None, _trusted=False):
        dev = gpu_device(index)
        if not isinstance(index, torch.Tensor) or index.dim() != 2 or index.dtype not in (torch.int32, torch.int64):
            raise RuntimeError("index must be an int32 or int64 tensor [m, k], got "
                               f"{getattr(index, 'dtype', type(index))} {list(getattr(index, 'shape', []))}")
        self.m, self.k = int(index.shape[0]), int(index.shape[1])
        self.n_src = int(n_src)
        if self.k < 1:
            raise RuntimeError("index must have at least one column")
        if not _trusted and self.m > 0:
            lo, hi = int(index.min()), int(index.max())
            if lo < 0 or hi >= self.n_src:
                raise RuntimeError(f"index entries must lie in [0, {self.n_src}), got {lo}..{hi}")
        self.index = to_dev(index.detach(), dev, torch.int32)
        self.distance = None
        if distance is not None:
            self.distance = to_dev(_f32("distance", distance, (self.m, self.k)), dev)
        self._inverse = None

    def inverse(self):
        """(inv_splits int64 [n_src + 1], inv_pairs int32 [m * k]): row s holds
        the flat pair ids t = i * k + j with index[i, j] == s in ascending t (a
        stable argsort of the index).  Built on first use, kept on the plan."""
        if self._inverse is None:
            dev = self.index.device
            if self.m * self.k >= 1 << 31:
                raise RuntimeError(f"Neighbours.inverse: m * k = {self.m} * {self.k} must be below 2^31")
            splits = torch.empty(self.n_src + 1, dtype=torch.int64, device=dev)
            pairs = torch.empty(self.m * self.k, dtype=torch.int32, device=dev)
            ws = workspace(_lib.load().o3dml_pt_invert_plan_workspace_size(self.m, self.k, self.n_src), dev)
            _lib.call("o3dml_pt_invert_plan", ptr(self.index), self.m, self.k, self.n_src, ptr(splits), ptr(pairs),
                      ptr(ws), ws.numel(), stream_handle(dev))
            self._inverse = (splits, pairs)
        return self._inverse

    @classmethod
    def from_knn(cls, points, queries, k, points_row_splits=None, queries_row_splits=None, distances=False):
        """The k nearest points of each query inside its cloud (ops.knn_search:
        ascending (distance, index), bit-exact against the oracle).  Row
        splits are host arrays (a device tensor costs a read back); every
        cloud that has queries must have at least k points."""
        k = int(k)
        prs = row_splits_host(points_row_splits, points.shape[0])
        qrs = row_splits_host(queries_row_splits, queries.shape[0])
        if len(prs) != len(qrs):
            raise RuntimeError("points_row_splits and queries_row_splits must have the same length")
        for b in range(len(prs) - 1):
            if qrs[b + 1] > qrs[b] and prs[b + 1] - prs[b] < k:
                raise RuntimeError(f"cloud {b} has {prs[b + 1] - prs[b]} points, fewer than k = {k}")
        res = ops.knn_search(points, queries, k, prs, qrs, return_distances=bool(distances))
        dev = gpu_device(points, queries)
        m = queries.shape[0]
        idx = to_dev(res.neighbors_index, dev).view(m, k)
        dist = to_dev(res.neighbors_distance, dev).view(m, k) if distances else None
        return cls(idx, points.shape[0], dist, _trusted=True)


# ---------------------------------------------------------------------------
# the ops
# ---------------------------------------------------------------------------
def furthest_point_sample_ragged(xyz, row_splits, new_row_splits):
    """furthest_point_sample_v2 (pointnet2_utils.py:89-99) in one launch: xyz
    [n, 3], cloud b = rows row_splits[b]..row_splits[b+1], sampled to
    new_row_splits[b+1] - new_row_splits[b] points -> int32 [new_row_splits[-1]]
    of global rows (int32 as in the reference: an int32 tensor plus a 0-dim
    int64 stays int32).  Per cloud the result of ops.furthest_point_sampling
    on that cloud alone, plus its offset."""
    dev = gpu_device(xyz)
    x = to_dev(_f32("xyz", xyz, (None, 3)), dev)
    n = x.shape[0]
    rs = row_splits_host(row_splits, n)
    nrs = np.ascontiguousarray(np.asarray(
        new_row_splits.detach().cpu() if isinstance(new_row_splits, torch.Tensor) else new_row_splits, dtype=np.int64))
    if nrs.ndim != 1 or len(nrs) != len(rs) or nrs[0] != 0 or np.any(np.diff(nrs) < 0):
        raise RuntimeError(f"new_row_splits must start at 0, be non-decreasing and have {len(rs)} entries")
    sizes, want = np.diff(rs), np.diff(nrs)
    for b in np.nonzero((sizes == 0) & (want > 0))[0]:
        raise RuntimeError(f"furthest_point_sample_ragged: cloud {int(b)} is empty but {int(want[b])} samples are "
                           "asked of it")
    B, m_total = len(rs) - 1, int(nrs[-1])
    max_n = int(sizes.max()) if B else 0
    out = torch.empty(m_total, dtype=torch.int32, device=dev)
    ws = workspace(_lib.load().o3dml_furthest_point_sampling_ragged_workspace_size(n, max_n), dev)
    _lib.call("o3dml_furthest_point_sampling_ragged", ptr(x), n, B, ptr(to_dev(rs, dev)), ptr(to_dev(nrs, dev)),
              max_n, m_total, ptr(out), ptr(ws), ws.numel(), stream_handle(dev))
    return out


def fold_bn(bn):
    """(scale, shift) of a BatchNorm in eval form, from its current tensors.
    Inside recording_grad() the fold is differentiable in weight and bias; the
    running statistics are constants either way."""
    scale = _param(bn.weight) * torch.rsqrt(bn.running_var + bn.eps)
    return scale, _param(bn.bias) - bn.running_mean * scale


def position_encoding(linear_p):
    """The six tensors of a Transformer's linear_p (Linear(3,3), BatchNorm1d(3),
    ReLU, Linear(3,c)) the kernels take: (w1, b1, scale_p, shift_p, w2, b2)."""
    scale, shift = fold_bn(linear_p[1])
    return (_param(linear_p[0].weight), _param(linear_p[0].bias), scale, shift, _param(linear_p[3].weight),
            _param(linear_p[3].bias))


def _records(coords, diff):
    """True when the op has to record autograd: grad mode on and one of the
    differentiable inputs requires grad.  Coordinates are never differentiated."""
    if not torch.is_grad_enabled():
        return False
    for name, t in coords:
        if isinstance(t, torch.Tensor) and t.requires_grad:
            raise RuntimeError(f"PointTransformer ops are not differentiated with respect to coordinates: {name} "
                               "requires grad (detach it)")
    return any(isinstance(t, torch.Tensor) and t.requires_grad for t in diff)


def _gather_sum(plan, rows, ld, col0, c, div=1, dist=None):
    """out[s] = sum over row s of plan.inverse(), ascending, of rows[t // div, col0:col0 + c]
    (weighted by the interpolation's weights when dist is given) -> [n_src, c]."""
    dev = plan.index.device
    splits, pairs = plan.inverse()
    out = torch.empty((plan.n_src, c), dtype=torch.float32, device=dev)
    _lib.call("o3dml_pt_gather_sum", ptr(rows), ld, col0, div, None, ptr(dist), plan.k, ptr(splits), ptr(pairs),
              plan.n_src, c, ptr(out), stream_handle(dev))
    return out


def _pos_hidden_backward(plan, q, s, w1, b1, sc, sh, dh):
    """Gradients of linear_p[0..2] from dh [m, k, 3] = d loss / d h, h =
    relu(sc * (w1 d + b1) + sh): three floats per pair, recomputed with torch
    ops over [m * k, 3] rows (torch.sum over the rows: a fixed order) ->
    (d w1, d b1, d sc, d sh)."""
    d = (s[plan.index.reshape(-1).long()].view(plan.m, plan.k, 3) - q.unsqueeze(1)).view(-1, 3)
    lin = torch.addmm(b1, d, w1.T)
    du = dh.view(-1, 3) * (sc * lin + sh > 0)
    dl = du * sc
    return (dl.unsqueeze(2) * d.unsqueeze(1)).sum(0), dl.sum(0), (du * lin).sum(0), du.sum(0)


def _grad_ws(c, dev):
    return workspace(_lib.load().o3dml_pt_backward_workspace_size(c), dev)


def _plan_inputs(plan, xyz_q, xyz_src, feat, c=None):
    require_gpu()
    if not isinstance(plan, Neighbours):
        raise RuntimeError(f"plan must be a Neighbours, got {type(plan)}")
    dev = plan.index.device
    if not 1 <= plan.k <= MAX_NSAMPLE:
        raise RuntimeError(f"nsample must be in 1..{MAX_NSAMPLE}, got {plan.k}")
    q = to_dev(_f32("xyz_q", xyz_q, (plan.m, 3)), dev)
    s = to_dev(_f32("xyz_src", xyz_src, (plan.n_src, 3)), dev)
    f = to_dev(_f32("feat", feat, (plan.n_src, c)), dev)
    if f.shape[1] < 1:
        raise RuntimeError("feat must have at least one channel")
    return dev, q, s, f


def _pos_inputs(pos, c, dev):
    shapes = ((3, 3), (3,), (3,), (3,), (c, 3), (c,))
    names = ("w1", "b1", "scale_p", "shift_p", "w2", "b2")
    if len(pos) != 6:
        raise RuntimeError("pos must be (w1, b1, scale_p, shift_p, w2, b2)")
    return [to_dev(_f32(nm, t, sh), dev) for nm, t, sh in zip(names, pos, shapes)]


def relation(plan, xyz_q, xyz_src, feat_k, feat_q, pos, scale_w, shift_w):
    """relu(scale_w * (feat_k[idx] - feat_q[:, None] + p_r) + shift_w) ->
    [m, nsample, c] (point_transformer.py:430-453 and the first BatchNorm and
    ReLU of linear_w); pos as position_encoding() returns it.  Differentiable
    in feat_k, feat_q, pos, scale_w and shift_w."""
    require_gpu()
    if _records((("xyz_q", xyz_q), ("xyz_src", xyz_src)), (feat_k, feat_q, *pos, scale_w, shift_w)):
        if len(pos) != 6:
            raise RuntimeError("pos must be (w1, b1, scale_p, shift_p, w2, b2)")
        return _Relation.apply(plan, xyz_q, xyz_src, feat_k, feat_q, *pos, scale_w, shift_w)
    return _relation(plan, xyz_q, xyz_src, feat_k, feat_q, pos, scale_w, shift_w)[0]


def _relation(plan, xyz_q, xyz_src, feat_k, feat_q, pos, scale_w, shift_w):
    """(out, the checked device tensors the kernel read)."""
    dev, q, s, fk = _plan_inputs(plan, xyz_q, xyz_src, feat_k)
    c = fk.shape[1]
    fq = to_dev(_f32("feat_q", feat_q, (plan.m, c)), dev)
    p = _pos_inputs(pos, c, dev)
    sw = to_dev(_f32("scale_w", scale_w, (c,)), dev)
    tw = to_dev(_f32("shift_w", shift_w, (c,)), dev)
    out = torch.empty((plan.m, plan.k, c), dtype=torch.float32, device=dev)
    _lib.call("o3dml_pt_relation", ptr(q), ptr(s), ptr(plan.index), ptr(fk), ptr(fq), *[ptr(t) for t in p], ptr(sw),
              ptr(tw), plan.m, plan.k, c, ptr(out), stream_handle(dev))
    return out, (q, s, fk, fq, *p, sw, tw)


class _Relation(torch.autograd.Function):
    """Saves the forward's inputs and its output (whose sign is the ReLU mask)."""

    @staticmethod
    def forward(ctx, plan, xyz_q, xyz_src, feat_k, feat_q, w1, b1, sc, sh, w2, b2, scale_w, shift_w):
        out, saved = _relation(plan, xyz_q, xyz_src, feat_k, feat_q, (w1, b1, sc, sh, w2, b2), scale_w, shift_w)
        ctx.plan = plan
        ctx.save_for_backward(*saved, out)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        plan = ctx.plan
        q, s, fk, fq, w1, b1, sc, sh, w2, b2, sw, tw, out = ctx.saved_tensors
        dev, (m, k, c) = out.device, out.shape
        g = to_dev(g, dev, torch.float32)
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
        gr, dq, dh = new(m, k, c), new(m, c), new(m, k, 3)
        dsw, dtw, dw2, db2 = new(c), new(c), new(c, 3), new(c)
        ws = _grad_ws(c, dev)
        _lib.call("o3dml_pt_relation_backward", ptr(q), ptr(s), ptr(plan.index), ptr(fk), ptr(fq), ptr(w1), ptr(b1),
                  ptr(sc), ptr(sh), ptr(w2), ptr(b2), ptr(sw), ptr(tw), ptr(out), ptr(g), m, k, c, ptr(gr), ptr(dq),
                  ptr(dh), ptr(dsw), ptr(dtw), ptr(dw2), ptr(db2), ptr(ws), ws.numel(), stream_handle(dev))
        dfk = _gather_sum(plan, gr, c, 0, c) if ctx.needs_input_grad[3] else None
        first = _pos_hidden_backward(plan, q, s, w1, b1, sc, sh, dh) if any(ctx.needs_input_grad[5:9]) else (None,) * 4
        return (None, None, None, dfk, dq, *first, dw2, db2, dsw, dtw)


def aggregate(plan, xyz_q, xyz_src, feat_v, weight, pos, share_planes):
    """sum_j softmax_j(weight)[.., ch mod (c/s)] * (feat_v[idx] + p_r) -> [m, c]
    (point_transformer.py:461-465); weight [m, nsample, c / share_planes].
    Differentiable in feat_v, weight and pos."""
    require_gpu()
    if _records((("xyz_q", xyz_q), ("xyz_src", xyz_src)), (feat_v, weight, *pos)):
        if len(pos) != 6:
            raise RuntimeError("pos must be (w1, b1, scale_p, shift_p, w2, b2)")
        return _Aggregate.apply(plan, xyz_q, xyz_src, feat_v, weight, *pos, share_planes)
    return _aggregate(plan, xyz_q, xyz_src, feat_v, weight, pos, share_planes)[0]


def _aggregate(plan, xyz_q, xyz_src, feat_v, weight, pos, share_planes):
    dev, q, s, fv = _plan_inputs(plan, xyz_q, xyz_src, feat_v)
    c, sp = fv.shape[1], int(share_planes)
    if sp < 1 or c % sp:
        raise RuntimeError(f"c = {c} must be a multiple of share_planes = {sp}")
    w = to_dev(_f32("weight", weight, (plan.m, plan.k, c // sp)), dev)
    p = _pos_inputs(pos, c, dev)
    out = torch.empty((plan.m, c), dtype=torch.float32, device=dev)
    _lib.call("o3dml_pt_aggregate", ptr(q), ptr(s), ptr(plan.index), ptr(fv), ptr(w), *[ptr(t) for t in p], plan.m,
              plan.k, c, sp, ptr(out), stream_handle(dev))
    return out, (q, s, fv, w, *p)


class _Aggregate(torch.autograd.Function):
    """Saves the forward's inputs only: the softmax is recomputed."""

    @staticmethod
    def forward(ctx, plan, xyz_q, xyz_src, feat_v, weight, w1, b1, sc, sh, w2, b2, share_planes):
        out, saved = _aggregate(plan, xyz_q, xyz_src, feat_v, weight, (w1, b1, sc, sh, w2, b2), share_planes)
        ctx.plan, ctx.share_planes = plan, int(share_planes)
        ctx.save_for_backward(*saved)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        plan, sp = ctx.plan, ctx.share_planes
        q, s, fv, w, w1, b1, sc, sh, w2, b2 = ctx.saved_tensors
        dev, m, k, c = fv.device, plan.m, plan.k, fv.shape[1]
        g = to_dev(g, dev, torch.float32)
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
        dval, dwt, dh, dw2, db2 = new(m, k, c), new(m, k, c // sp), new(m, k, 3), new(c, 3), new(c)
        ws = _grad_ws(c, dev)
        _lib.call("o3dml_pt_aggregate_backward", ptr(q), ptr(s), ptr(plan.index), ptr(fv), ptr(w), ptr(w1), ptr(b1),
                  ptr(sc), ptr(sh), ptr(w2), ptr(b2), ptr(g), m, k, c, sp, ptr(dval), ptr(dwt), ptr(dh), ptr(dw2),
                  ptr(db2), ptr(ws), ws.numel(), stream_handle(dev))
        dfv = _gather_sum(plan, dval, c, 0, c) if ctx.needs_input_grad[3] else None
        first = _pos_hidden_backward(plan, q, s, w1, b1, sc, sh, dh) if any(ctx.needs_input_grad[5:9]) else (None,) * 4
        return (None, None, None, dfv, dwt, *first, dw2, db2, None)


def knn_interpolate(plan, feat):
    """Inverse-distance interpolation (point_transformer.py:737-776): feat
    [n_src, c] -> [m, c] with weights r / sum r, r = 1 / (distance + 1e-8).
    Differentiable in feat."""
    require_gpu()
    if _records((), (feat,)):
        return _Interpolate.apply(plan, feat)
    return _knn_interpolate(plan, feat)


class _Interpolate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, feat):
        ctx.plan = plan
        return _knn_interpolate(plan, feat)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        plan = ctx.plan
        g = to_dev(g, plan.index.device, torch.float32)
        c = g.shape[1]
        return None, _gather_sum(plan, g, c, 0, c, div=plan.k, dist=plan.distance)


def _knn_interpolate(plan, feat):
    if not isinstance(plan, Neighbours):
        raise RuntimeError(f"plan must be a Neighbours, got {type(plan)}")
    if plan.distance is None:
        raise RuntimeError("knn_interpolate needs a plan with distances")
    if not 1 <= plan.k <= MAX_INTERPOLATE_K:
        raise RuntimeError(f"k must be in 1..{MAX_INTERPOLATE_K}, got {plan.k}")
    dev = plan.index.device
    f = to_dev(_f32("feat", feat, (plan.n_src, None)), dev)
    c = f.shape[1]
    if c < 1:
        raise RuntimeError("feat must have at least one channel")
    out = torch.empty((plan.m, c), dtype=torch.float32, device=dev)
    _lib.call("o3dml_pt_knn_interpolate", ptr(f), ptr(plan.index), ptr(plan.distance), plan.m, plan.k, c, ptr(out),
              stream_handle(dev))
    return out


def group(plan, xyz_q, xyz_src, feat):
    """[xyz_src[idx] - xyz_q[:, None] | feat[idx]] -> [m, nsample, 3 + c]
    (queryandgroup with use_xyz, point_transformer.py:650-697).
    Differentiable in feat."""
    require_gpu()
    if _records((("xyz_q", xyz_q), ("xyz_src", xyz_src)), (feat,)):
        return _Group.apply(plan, xyz_q, xyz_src, feat)
    return _group(plan, xyz_q, xyz_src, feat)


class _Group(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, xyz_q, xyz_src, feat):
        ctx.plan = plan
        return _group(plan, xyz_q, xyz_src, feat)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        plan = ctx.plan
        g = to_dev(g, plan.index.device, torch.float32)
        c = g.shape[2] - 3
        return None, None, None, _gather_sum(plan, g, 3 + c, 3, c)


def _group(plan, xyz_q, xyz_src, feat):
    dev, q, s, f = _plan_inputs(plan, xyz_q, xyz_src, feat)
    c = f.shape[1]
    out = torch.empty((plan.m, plan.k, 3 + c), dtype=torch.float32, device=dev)
    _lib.call("o3dml_pt_group", ptr(q), ptr(s), ptr(plan.index), ptr(f), plan.m, plan.k, c, ptr(out),
              stream_handle(dev))
    return out


def level_row_splits(row_splits, strides=(1, 4, 4, 4, 4), nsample=(8, 16, 16, 16, 16)):
    """Row splits of every level (point_transformer.py:509-514: n_b // stride
    per cloud), as int64 numpy arrays; pure host arithmetic.  Raises when a
    cloud of a level has fewer points than the level's nsample (the reference
    then fails in a reshape): with the default strides the smallest usable
    cloud has 16 * 256 = 4096 points."""
    rs = np.asarray(row_splits.detach().cpu() if isinstance(row_splits, torch.Tensor) else row_splits, dtype=np.int64)
    if rs.ndim != 1 or len(rs) < 2 or rs[0] != 0 or np.any(np.diff(rs) < 0):
        raise RuntimeError("row_splits must be 1-D, start at 0 and be non-decreasing")
    if len(strides) != len(nsample):
        raise RuntimeError("strides and nsample must have one entry per level")
    out, sizes = [], np.diff(rs)
    for level, (stride, ns) in enumerate(zip(strides, nsample)):
        sizes = sizes // int(stride)
        for b, nb in enumerate(sizes):
            if nb < ns:
                raise RuntimeError(f"PointTransformer: level {level}: cloud {b} has {int(nb)} points, fewer than "
                                   f"nsample = {int(ns)}")
        out.append(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))
    return out


# ---------------------------------------------------------------------------
# modules (names as the reference's state_dict requires)
# ---------------------------------------------------------------------------
_TRAINING = "PointTransformer: training is not built yet"


def _self_plan(pxo):
    """The self-kNN plan a block was handed (4th entry), else None."""
    return pxo[3] if len(pxo) > 3 else None


class Transformer(nn.Module):
    """Vector self-attention over the nsample nearest points
    (point_transformer.py:377-467).  pxo: [point, feat, row_splits] or
    [point, feat, row_splits, Neighbours]; without a plan the layer searches."""

    def __init__(self, in_planes, out_planes, share_planes=8, nsample=16):
        super().__init__()
        self.mid_planes = mid_planes = out_planes // 1
        self.out_planes = out_planes
        self.share_planes = share_planes
        self.nsample = nsample
        self.linear_q = nn.Linear(in_planes, mid_planes)
        self.linear_k = nn.Linear(in_planes, mid_planes)
        self.linear_v = nn.Linear(in_planes, out_planes)
        self.linear_p = nn.Sequential(nn.Linear(3, 3), nn.BatchNorm1d(3), nn.ReLU(inplace=True),
                                      nn.Linear(3, out_planes))
        self.linear_w = nn.Sequential(nn.BatchNorm1d(mid_planes), nn.ReLU(inplace=True),
                                      nn.Linear(mid_planes, mid_planes // share_planes),
                                      nn.BatchNorm1d(mid_planes // share_planes), nn.ReLU(inplace=True),
                                      nn.Linear(out_planes // share_planes, out_planes // share_planes))
        self.softmax = nn.Softmax(dim=1)

    def forward(self, pxo):
        if self.training:
            raise NotImplementedError(_TRAINING)
        point, feat, row_splits = pxo[0], pxo[1], pxo[2]
        plan = _self_plan(pxo)
        if plan is None:
            plan = Neighbours.from_knn(point, point, self.nsample, row_splits, row_splits)
        with _graph():
            feat_q, feat_k, feat_v = self.linear_q(feat), self.linear_k(feat), self.linear_v(feat)
            pos = position_encoding(self.linear_p)
            w = relation(plan, point, point, feat_k, feat_q, pos, *fold_bn(self.linear_w[0]))
            # Linear(c, c/s) with the BatchNorm behind it folded in, ReLU, Linear(c/s, c/s)
            scale, shift = fold_bn(self.linear_w[3])
            lin = self.linear_w[2]
            w = _relu(F.linear(w, lin.weight * scale[:, None], lin.bias * scale + shift))
            w = self.linear_w[5](w)
            return aggregate(plan, point, point, feat_v, w, pos, self.share_planes)


class TransitionDown(nn.Module):
    """Farthest-point sampling to n_b // stride points per cloud, then
    Linear + BatchNorm + ReLU over each sample's nsample nearest source rows
    [relative xyz | feat] and their maximum (point_transformer.py:470-536).
    Returns [point, feat, row_splits]; `sampled` holds the sampled rows of the
    last forward of a stride != 1 layer."""

    def __init__(self, in_planes, out_planes, stride=1, nsample=16):
        super().__init__()
        self.stride, self.nsample = stride, nsample
        if stride != 1:
            self.linear = nn.Linear(3 + in_planes, out_planes, bias=False)
            self.pool = nn.MaxPool1d(nsample)
        else:
            self.linear = nn.Linear(in_planes, out_planes, bias=False)
        self.bn = nn.BatchNorm1d(out_planes)
        self.relu = nn.ReLU(inplace=True)
        self.sampled = None

    def forward(self, pxo):
        if self.training:
            raise NotImplementedError(_TRAINING)
        point, feat, row_splits = pxo[0], pxo[1], pxo[2]
        with _graph():
            scale, shift = fold_bn(self.bn)
            weight = self.linear.weight * scale[:, None]
            if self.stride == 1:
                return [point, _relu(F.linear(feat, weight, shift)), row_splits]
            rs = row_splits_host(row_splits, point.shape[0])
            new_rs = np.concatenate([[0], np.cumsum(np.diff(rs) // self.stride)]).astype(np.int64)
            idx = furthest_point_sample_ragged(point, rs, new_rs)
            self.sampled = idx
            new_point = point[idx.long(), :]
            plan = Neighbours.from_knn(point, new_point, self.nsample, rs, new_rs)
            rows = group(plan, new_point, point, feat)  # (m, nsample, 3 + c)
            feat = _relu(F.linear(rows, weight, shift)).max(dim=1).values
            return [new_point, feat, new_rs]


class TransitionUp(nn.Module):
    """Decoder layer (point_transformer.py:539-600): the head concatenates
    each cloud's mean feature; the others add the features of the coarser
    level interpolated over the 3 nearest coarse points."""

    def __init__(self, in_planes, out_planes=None):
        super().__init__()
        if out_planes is None:
            self.linear1 = nn.Sequential(nn.Linear(2 * in_planes, in_planes), nn.BatchNorm1d(in_planes),
                                         nn.ReLU(inplace=True))
            self.linear2 = nn.Sequential(nn.Linear(in_planes, in_planes), nn.ReLU(inplace=True))
        else:
            self.linear1 = nn.Sequential(nn.Linear(out_planes, out_planes), nn.BatchNorm1d(out_planes),
                                         nn.ReLU(inplace=True))
            self.linear2 = nn.Sequential(nn.Linear(in_planes, out_planes), nn.BatchNorm1d(out_planes),
                                         nn.ReLU(inplace=True))

    def forward(self, pxo1, pxo2=None):
        if self.training:
            raise NotImplementedError(_TRAINING)
        with _graph():
            if pxo2 is None:
                point, feat, row_splits = pxo1[0], pxo1[1], pxo1[2]
                rs = row_splits_host(row_splits, feat.shape[0])
                parts = []
                for b in range(len(rs) - 1):
                    start, count = int(rs[b]), int(rs[b + 1] - rs[b])
                    feat_b = feat[start:start + count, :]
                    parts.append(torch.cat((feat_b, self.linear2(feat_b.sum(0, True) / count).repeat(count, 1)), 1))
                return self.linear1(torch.cat(parts, 0))
            point_1, feat_1, row_splits_1 = pxo1[0], pxo1[1], pxo1[2]
            point_2, feat_2, row_splits_2 = pxo2[0], pxo2[1], pxo2[2]
            plan = Neighbours.from_knn(point_2, point_1, 3, row_splits_2, row_splits_1, distances=True)
            return self.linear1(feat_1) + knn_interpolate(plan, self.linear2(feat_2))


class Bottleneck(nn.Module):
    """Linear, Transformer, Linear with BatchNorms and a residual
    (point_transformer.py:603-647); passes a plan in pxo[3] on."""
    expansion = 1

    def __init__(self, in_planes, planes, share_planes=8, nsample=16):
        super().__init__()
        self.linear1 = nn.Linear(in_planes, planes, bias=False)
        self.bn1 = nn.BatchNorm1d(planes)
        self.transformer2 = Transformer(planes, planes, share_planes, nsample)
        self.bn2 = nn.BatchNorm1d(planes)
        self.linear3 = nn.Linear(planes, planes * self.expansion, bias=False)
        self.bn3 = nn.BatchNorm1d(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)

    def forward(self, pxo):
        if self.training:
            raise NotImplementedError(_TRAINING)
        point, feat, row_splits = pxo[0], pxo[1], pxo[2]
        with _graph():
            identity = feat
            feat = self.relu(self.bn1(self.linear1(feat)))
            feat = self.relu(self.bn2(self.transformer2([point, feat, *pxo[2:]])))
            feat = self.bn3(self.linear3(feat))
            feat = self.relu(feat + identity)
        return [point, feat, *pxo[2:]]


def _field(batch, name):
    return batch[name] if isinstance(batch, dict) else getattr(batch, name)


class PointTransformer(nn.Module):
    """Module tree and state_dict of ml3d PointTransformer
    (point_transformer.py:18-196), eval() forward only.  forward takes a batch
    with point [n, 3], feat [n, in_channels - 3] and row_splits [B + 1]
    (attributes or keys) and returns logits [n, num_classes]."""

    planes = (32, 64, 128, 256, 512)
    strides = (1, 4, 4, 4, 4)
    nsamples = (8, 16, 16, 16, 16)
    share_planes = 8

    def __init__(self, name="PointTransformer", blocks=(2, 2, 2, 2, 2), in_channels=6, num_classes=13,
                 voxel_size=0.04, max_voxels=80000, batcher="ConcatBatcher", augment=None, **kwargs):
        super().__init__()
        self.cfg = dict(name=name, blocks=list(blocks), in_channels=in_channels, num_classes=num_classes,
                        voxel_size=voxel_size, max_voxels=max_voxels, batcher=batcher, augment=augment, **kwargs)
        self.in_channels = in_channels
        self.in_planes = in_channels
        planes = self.planes
        self.encoders = nn.ModuleList(
            self._make_enc(planes[i], blocks[i], self.share_planes, self.strides[i], self.nsamples[i])
            for i in range(5))
        self.decoders = nn.ModuleList(
            self._make_dec(planes[i], 2, self.share_planes, self.nsamples[i], is_head=i == 4)
            for i in range(4, -1, -1))
        self.cls = nn.Sequential(nn.Linear(planes[0], planes[0]), nn.BatchNorm1d(planes[0]), nn.ReLU(inplace=True),
                                 nn.Linear(planes[0], num_classes))

    def _make_enc(self, planes, blocks, share_planes=8, stride=1, nsample=16):
        layers = [TransitionDown(self.in_planes, planes * Bottleneck.expansion, stride, nsample)]
        self.in_planes = planes * Bottleneck.expansion
        for _ in range(1, blocks):
            layers.append(Bottleneck(self.in_planes, self.in_planes, share_planes, nsample=nsample))
        return nn.Sequential(*layers)

    def _make_dec(self, planes, blocks, share_planes=8, nsample=16, is_head=False):
        layers = [TransitionUp(self.in_planes, None if is_head else planes * Bottleneck.expansion)]
        self.in_planes = planes * Bottleneck.expansion
        for _ in range(1, blocks):
            layers.append(Bottleneck(self.in_planes, self.in_planes, share_planes, nsample=nsample))
        return nn.Sequential(*layers)

    def forward(self, batch):
        if self.training:
            raise NotImplementedError(_TRAINING)
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            require_gpu()
            raise RuntimeError("PointTransformer: the model must be on the GPU (there is no CPU path)")
        point = to_dev(_f32("point", _field(batch, "point"), (None, 3)), dev)
        feat = _field(batch, "feat")
        levels = level_row_splits(_field(batch, "row_splits"), self.strides, self.nsamples)
        if levels[0][-1] != point.shape[0]:
            raise RuntimeError(f"row_splits ends at {int(levels[0][-1])}, point has {point.shape[0]} rows")
        with _graph():
            if self.in_channels == 3:
                feat = point
            else:
                feat = torch.cat((point, to_dev(_f32("feat", feat, (point.shape[0], self.in_channels - 3)), dev)), 1)
            # level i: points[i + 1], feats[i + 1], levels[i] and one self-kNN plan for all of its blocks
            points, feats, plans = [point], [feat], []
            for i in range(5):
                p, f, _ = self.encoders[i][0]([points[i], feats[i], levels[max(i - 1, 0)]])
                plan = Neighbours.from_knn(p, p, self.nsamples[i], levels[i], levels[i])
                f = self.encoders[i][1:]([p, f, levels[i], plan])[1]
                points.append(p)
                feats.append(f)
                plans.append(plan)
            for i in range(4, -1, -1):
                dec = self.decoders[4 - i]
                here = [points[i + 1], feats[i + 1], levels[i]]
                f = dec[0](here) if i == 4 else dec[0](here, [points[i + 2], feats[i + 2], levels[i + 1]])
                feats[i + 1] = dec[1:]([points[i + 1], f, levels[i], plans[i]])[1]
            return self.cls(feats[1])

    def sampled_indices(self):
        """The rows each of the four strided TransitionDown layers sampled in
        the last forward (int32, rows of the level above)."""
        return [enc[0].sampled for enc in self.encoders if enc[0].stride != 1]


__all__ = ["PointTransformer", "Transformer", "TransitionDown", "TransitionUp", "Bottleneck", "Neighbours",
           "furthest_point_sample_ragged", "relation", "aggregate", "knn_interpolate", "group", "level_row_splits",
           "fold_bn", "position_encoding", "recording_grad"]
