"""ops.fp_mlp on the GPU against the composition it replaces (weights from
dist2, gather of the three rows, weighted sum, concatenate, Linear + ReLU per
layer) in float64 torch on the CPU.  The bound is the project's: largest
absolute difference over largest magnitude <= 1e-4; the float32 composition on
the CPU has to keep it too, so the bound is one float32 arithmetic can meet."""
import pytest
import torch

pytestmark = pytest.mark.gpu
BOUND = 1e-4


def make(C2, C1, mlp, B, n, m, seed=0):
    g = torch.Generator().manual_seed(seed)
    unknown, known = torch.rand(B, n, 3, generator=g), torch.rand(B, m, 3, generator=g)
    unknown[0, 0] = known[0, 0]  # a coincident point: dist2 = 0
    d = ((unknown[:, :, None] - known[:, None]) ** 2).sum(-1)
    dist2, idx = d.topk(min(3, m), dim=2, largest=False)  # the exact three nearest
    pad = (0, 3 - min(3, m))  # as three_nn leaves a slot it did not fill
    dist2 = torch.nn.functional.pad(dist2, pad, value=float("inf")).contiguous()
    idx = torch.nn.functional.pad(idx, pad, value=0).int().contiguous()
    kf = torch.randn(B, m, C2, generator=g)
    uf = torch.randn(B, n, C1, generator=g) if C1 else None
    widths = [C2 + C1] + list(mlp)
    weights = [torch.randn(o, i, generator=g) / i ** 0.5 for i, o in zip(widths[:-1], widths[1:])]
    biases = [0.1 * torch.randn(o, generator=g) for o in widths[1:]]
    return uf, kf, dist2, idx, weights, biases


def composed(uf, kf, dist2, idx, weights, biases, dtype):
    recip = 1.0 / (dist2.to(dtype).sqrt() + 1e-8)
    w = recip / recip.sum(2, keepdim=True)
    rows = torch.stack([kf[b].to(dtype)[idx[b].long()] for b in range(kf.shape[0])])  # [B, n, 3, C2]
    h = (rows * w[..., None]).sum(2)
    if uf is not None:
        h = torch.cat([h, uf.to(dtype)], -1)
    for wt, b in zip(weights, biases):
        h = torch.relu(h @ wt.to(dtype).T + b.to(dtype))
    return h


def err(a, ref):
    return float((a.double() - ref).abs().max() / ref.abs().max())


def check(cuda, C2, C1, mlp, B, n, m):
    from o3dml_amd import ops
    args = make(C2, C1, mlp, B, n, m)
    ref = composed(*args, torch.float64)
    e32 = err(composed(*args, torch.float32), ref)
    assert e32 <= BOUND, e32
    dev = [None if t is None else t.to(cuda) for t in args[:4]]
    wb = [[t.to(cuda) for t in ts] for ts in args[4:]]
    out = ops.fp_mlp(*dev, *wb)
    again = ops.fp_mlp(*dev, *wb)
    e = err(out.cpu(), ref)
    print(f"C2 {C2} C1 {C1} mlp {mlp} B {B} n {n} m {m}: {e:.3g} (float32 composition {e32:.3g}), bound {BOUND}")
    assert tuple(out.shape) == tuple(ref.shape) and e <= BOUND
    assert torch.equal(out, again)  # run to run bitwise


@pytest.mark.parametrize("C2, C1, mlp", [
    (1024, 512, [512, 512]), (512, 256, [512, 512]), (512, 96, [256, 256]), (256, 1, [128, 128]),
    (7, 5, [33, 3]),             # odd widths, the one chunk straddles C2, c_L < 32
    (7, 0, [5, 33, 16, 40]),     # unknown_feats=None, L = 4
    (70, 3, [33])])              # L = 1; the second chunk straddles C2, which is no multiple of 8
def test_widths(cuda, C2, C1, mlp):
    check(cuda, C2, C1, mlp, B=2, n=70, m=50)


# Tiles are 32 rows whatever the shape: B * n = 2 .. 400 is 1 .. 13 tiles, one workgroup each, the
# last one partial but for n = 32, 64.  Past 1024 tiles the workgroups walk the tiles with that
# stride: n = 20000 is 1250 tiles, so 226 workgroups take a second one.
@pytest.mark.parametrize("n, m", [(1, 50), (31, 50), (32, 50), (33, 50), (64, 50), (65, 50), (200, 50),
                                  (33, 1), (33, 2), (33, 3), (20000, 50)])
def test_rows(cuda, n, m):
    check(cuda, 16, 3, [32, 64], B=2, n=n, m=m)


@pytest.mark.parametrize("C2, C1, mlp, number", [(2000, 49, [8], "2049"), (7, 5, [513], "513")])
def test_above_a_limit_raises(cuda, C2, C1, mlp, number):
    from o3dml_amd import ops
    uf, kf, dist2, idx, weights, biases = [
        t if t is None or isinstance(t, list) else t.to(cuda) for t in make(C2, C1, mlp, 1, 4, 5)]
    with pytest.raises(RuntimeError, match=number):
        ops.fp_mlp(uf, kf, dist2, idx, weights, biases)


def test_module_switch(cuda):
    """A module with BatchNorm: the same result fused and composed, the
    kernel's timing counter counts the fused launch only, and a forward without
    unknown features runs fused."""
    from o3dml_amd import _lib
    from o3dml_amd.point_rcnn import PointnetFPModule
    torch.manual_seed(0)
    fp = PointnetFPModule(mlp=[24 + 5, 48, 40], batch_norm=torch.nn.BatchNorm2d)
    bare = PointnetFPModule(mlp=[24, 16], batch_norm=torch.nn.BatchNorm2d)
    for m in list(fp.modules()) + list(bare.modules()):
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0, 0.1)
    fp, bare = fp.to(cuda).eval(), bare.to(cuda).eval()
    unknown, known = torch.rand(2, 50, 3, device=cuda), torch.rand(2, 20, 3, device=cuda)
    uf, kf = torch.randn(2, 50, 5, device=cuda), torch.randn(2, 20, 24, device=cuda)
    lib = _lib.load()
    lib.o3dml_timing_enable(1)
    try:
        res, launches = [], []
        for mod, feats, fused in ((fp, uf, True), (fp, uf, False), (bare, None, True), (bare, None, False)):
            mod.fused = fused
            lib.o3dml_timing_reset()
            with torch.no_grad():
                res.append(mod(unknown, known, feats, kf))
            torch.cuda.synchronize()
            launches.append(_lib.kernel_times(["fp_mlp"])["fp_mlp"][1])
    finally:
        lib.o3dml_timing_enable(0)
    e = [err(res[k].cpu(), res[k + 1].cpu().double()) for k in (0, 2)]
    print("fused against composed", e, "bound", BOUND)
    assert tuple(res[0].shape) == (2, 50, 40) and tuple(res[2].shape) == (2, 50, 16)
    assert max(e) <= BOUND and launches == [1, 0, 1, 0]
