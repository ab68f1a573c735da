"""ops.sa_mlp_max on the GPU against the composition it replaces (gather,
centre subtraction, concatenate, Linear + ReLU per layer, max over the group)
in float64 torch on the CPU.  The bound is the project's: largest absolute
difference over largest magnitude <= 1e-4; the float32 composition on the CPU
has to keep it too, so the bound is one float32 arithmetic can meet."""
import pytest
import torch

pytestmark = pytest.mark.gpu
BOUND = 1e-4


def make(widths, B, M, N, S, use_xyz=True, group_all=False, seed=0):
    g = torch.Generator().manual_seed(seed)
    C = widths[0] - (3 if use_xyz else 0)
    xyz = torch.rand(B, N, 3, generator=g)
    feat = torch.randn(B, N, C, generator=g) if C else None
    weights = [torch.randn(o, i, generator=g) / i ** 0.5 for i, o in zip(widths[:-1], widths[1:])]
    biases = [0.1 * torch.randn(o, generator=g) for o in widths[1:]]
    if group_all:
        return xyz, None, feat, None, weights, biases
    new_xyz = torch.rand(B, M, 3, generator=g)
    # as ball_query pads: h hits ascending, then the first hit repeated; no hit: a row of zeros
    idx = torch.zeros(B, M, S, dtype=torch.int32)
    for b in range(B):
        for m in range(M):
            h = int(torch.randint(0, S + 1, (1,), generator=g))
            if h:
                hits = torch.randperm(N, generator=g)[:h].sort().values.int()
                idx[b, m] = hits[0]
                idx[b, m, :len(hits)] = hits
    return xyz, new_xyz, feat, idx, weights, biases


def composed(xyz, new_xyz, feat, idx, weights, biases, use_xyz, dtype):
    c = lambda t: None if t is None else t.to(dtype)  # noqa: E731
    xyz, new_xyz, feat = c(xyz), c(new_xyz), c(feat)
    B, N, _ = xyz.shape
    idx = torch.arange(N).expand(B, 1, N) if idx is None else idx.long()
    pick = lambda t: torch.stack([t[b][idx[b]] for b in range(B)])  # noqa: E731
    rows = pick(xyz) - (0 if new_xyz is None else new_xyz[:, :, None])
    h = rows if feat is None else (torch.cat([rows, pick(feat)], -1) if use_xyz else pick(feat))
    for w, b in zip(weights, biases):
        h = torch.relu(h @ w.to(dtype).T + b.to(dtype))
    return h.max(dim=2).values


def err(a, ref):
    return float((a.double() - ref).abs().max() / ref.abs().max())


def check(cuda, widths, B, M, N, S, use_xyz=True, group_all=False):
    from o3dml_amd import ops
    args = make(widths, B, M, N, S, use_xyz, group_all)
    ref = composed(*args, use_xyz, torch.float64)
    e32 = err(composed(*args, use_xyz, torch.float32), ref)
    assert e32 <= BOUND, e32
    dev = [None if t is None else t.to(cuda) for t in args[:4]]
    wb = [[t.to(cuda) for t in ts] for ts in args[4:]]
    out = ops.sa_mlp_max(*dev, *wb, use_xyz=use_xyz)
    again = ops.sa_mlp_max(*dev, *wb, use_xyz=use_xyz)
    e = err(out.cpu(), ref)
    print(f"widths {widths} B {B} M {M} N {N} S {S}: {e:.3g} (float32 composition {e32:.3g}), bound {BOUND}")
    assert tuple(out.shape) == tuple(ref.shape) and e <= BOUND
    assert torch.equal(out, again)  # run to run bitwise


@pytest.mark.parametrize("widths, use_xyz", [
    ([3, 16, 16, 32], True), ([67, 64, 96, 128], True), ([259, 128, 196, 256], True), ([515, 256, 384, 512], True),
    ([24, 32, 48], False), ([7, 33], True), ([7, 5, 33], True), ([7, 5, 33, 16, 40], True)])
def test_widths(cuda, widths, use_xyz):
    check(cuda, widths, B=2, M=5, N=70, S=40, use_xyz=use_xyz)  # S > 32: 64-row tiles where the widths allow them


# (16, 511): enough groups that S <= 32 takes 64-row tiles of four groups, the last tile holding two
@pytest.mark.parametrize("S, M", [(1, 5), (3, 5), (16, 5), (32, 5), (33, 5), (64, 5), (100, 5), (1, 1), (3, 1),
                                  (16, 511)])
def test_group_sizes(cuda, S, M):
    check(cuda, [19, 32, 64], B=2, M=M, N=70, S=S)


def test_group_all(cuda):
    check(cuda, [11, 16, 32], B=2, M=1, N=37, S=37, group_all=True)


def test_width_above_the_limit_raises(cuda):
    from o3dml_amd import ops
    xyz, new_xyz, feat, idx, weights, biases = [
        t if t is None or isinstance(t, list) else t.to(cuda) for t in make([7, 513], 1, 2, 10, 4)]
    with pytest.raises(RuntimeError, match="513"):
        ops.sa_mlp_max(xyz, new_xyz, feat, idx, weights, biases)


def test_module_switch(cuda):
    """Two scales with BatchNorm: the same result fused and composed, and the
    kernel's timing counter counts the fused launches only."""
    from o3dml_amd import _lib
    from o3dml_amd.point_rcnn import PointnetSAModuleMSG
    torch.manual_seed(0)
    sa = PointnetSAModuleMSG(npoint=6, radii=[0.3, 0.6], nsamples=[8, 16], mlps=[[4, 16, 32], [4, 16, 16, 24]],
                             batch_norm=torch.nn.BatchNorm2d)
    for m in sa.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0, 0.1)
    sa = sa.to(cuda).eval()
    xyz, feat = torch.rand(2, 50, 3, device=cuda), torch.randn(2, 50, 4, device=cuda)
    lib = _lib.load()
    lib.o3dml_timing_enable(1)
    try:
        res, launches = [], []
        for fused in (True, False):
            sa.fused = fused
            lib.o3dml_timing_reset()
            with torch.no_grad():
                res.append(sa(xyz, feat)[1])
            torch.cuda.synchronize()
            launches.append(_lib.kernel_times(["sa_mlp_max"])["sa_mlp_max"][1])
    finally:
        lib.o3dml_timing_enable(0)
    e = err(res[0].cpu(), res[1].cpu().double())
    print("fused against composed", e, "bound", BOUND)
    assert tuple(res[0].shape) == (2, 6, 56) and e <= BOUND and launches == [2, 0]
