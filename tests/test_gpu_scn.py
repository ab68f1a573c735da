"""SparseConvUnet forward on the HIP layers vs the reference model's logits
(tests/golden/scn.npz: the reference SparseConvUnet with oracle-backed
SparseConv layers, deterministic weights from randla_weights.fill), residual
and plain; tolerance 1e-4 of the logit range.  Also: the rulebook cache of one
forward changes nothing, and the InputLayer voxel map matches the reference's
(every point maps to the voxel holding its floor cell).

One training step against float64 (tests/golden/scn_train.npz and
scn_train_grads.npz, made by make_golden_scn_train.py: the reference
SparseConvUnet m = 32, residual, 20 classes, sparse convolutions as the
oracle rulebook in torch ops under autograd) on a batch of two rooms — room A
9,920 voxels at level 0 (above voxel.hip's kDeepMax = 8192), then 2,393, 581,
128, 34, 6, 2; room B 3,463; a third of the voxels hold 2 - 3 points — in
eval() with autograd on and in train(): every 7th logit row, the loss, every
parameter's gradient norm, five full gradients and (train) every BN running
statistic, by C3's rule: loss within 1e-5 relative, everything else within
max(1e-4, 2 x the reference's own fp32-vs-fp64 error on that quantity),
gradients also allowed the reference's worst fp32 tensor error of the mode.
The reference's own fp32 errors (read from the fixture by the test):
  eval:  rows 2.8e-7, loss 1.9e-8, gradient norms <= 2.4e-7, full gradients
         <= 2.5e-7;
  train: rows 1.1e-6, loss 5.2e-8, BN running statistics <= 9.7e-8, gradient
         norms median 3.5e-7, worst 1.8e-5 (unet.net.30.batch_norm2.bn.bias),
         full gradients 1.4e-5 (first conv kernel), 1.4e-5 (level-0 32 -> 32
         kernel), 2.2e-5 (first strided Convolution), 1.3e-6 (last
         DeConvolution), 9.4e-7 (linear.linear.weight).
So with this fixture every bound, in both modes, gradients included, is the
1e-4 floor: the rule's two allowances (2 x the reference's error, its worst
tensor error of the mode: 2.5e-7 / 2.2e-5) never exceed it, and a per-mille
error in a backward path fails in train mode as in eval mode.  The generator
keeps it so: it asserts that no reference error exceeds 1e-2 and that at most
5 % of the 125 parameter tensors have a gradient-norm error OR a
full-gradient error above 5e-4 (here none; feature seed 11 gave 7 of 125 in
train mode, first-layer kernel gradients 3e-3 .. 5e-3 off, and was replaced).

The graph modes (O3DML_SCN_GRAPH 1: one captured body per size signature; 3,
the default: the one-call plan and a body captured on its buffers) are also
held to the eager forward (mode 0) bit for bit on room A (its level 0 runs the
multi-workgroup plan levels), with feature rows wider than the three columns
the InputLayer averages, after parameters or buffers were replaced by other
tensors (load_state_dict(assign=True), a new nn.Parameter, a fresh buffer at
version 0), and on a batch of two, which mode 3 hands to mode 1's path."""
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import randla_weights  # noqa: E402

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(HERE, "golden", "scn.npz"))
T = np.load(os.path.join(HERE, "golden", "scn_train.npz"))
TG = np.load(os.path.join(HERE, "golden", "scn_train_grads.npz"))


def _model(residual, dev):
    from o3dml_amd.sparseconvnet import SparseConvUnet
    m = SparseConvUnet(multiplier=8, residual_blocks=residual, conv_block_reps=1, num_classes=5)
    sd = m.state_dict()
    m.load_state_dict(randla_weights.state_dict_for([(k, tuple(v.shape)) for k, v in sd.items()], sd))
    return m.to(dev).eval()


def _inputs(dev):
    pos = torch.from_numpy(G["pos"]).to(dev)
    feat = torch.from_numpy(G["feat"]).to(dev)
    return types.SimpleNamespace(point=[pos], feat=[feat], batch_lengths=[pos.shape[0]])


K_DEEP_MAX = 8192  # voxel.hip: more level-0 voxels than this run the multi-workgroup plan levels


def _room_a(dev):
    """Room A of the training fixture (9,920 voxels, duplicates) as one frame."""
    n = int(T["lengths"][0])
    pos = torch.from_numpy(T["pos"][:n]).to(dev)
    feat = torch.from_numpy(T["feat"][:n]).to(dev)
    return types.SimpleNamespace(point=[pos], feat=[feat], batch_lengths=[n])


def _n_voxels(x):
    return torch.unique(torch.floor(x.point[0]), dim=0).shape[0]


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


@pytest.mark.parametrize("tag,residual", [("res", True), ("plain", False)])
def test_scn_logits_match_reference(cuda, tag, residual):
    m = _model(residual, cuda)
    with torch.no_grad():
        out = m(_inputs(cuda)).cpu().numpy()
    ref = G[f"{tag}_logits"]
    assert out.shape == ref.shape
    err = np.abs(out - ref).max() / np.abs(ref).max()
    assert err < 1e-4, err


def test_scn_search_rulebook_equals_lattice(cuda):
    from o3dml_amd import layers
    m = _model(True, cuda)
    inp = _inputs(cuda)
    a = m(inp).detach()  # autograd on: unfused layers, so only the rulebook differs
    for mod in m.modules():
        if isinstance(mod, layers.SparseConv):
            mod.lattice_rulebook = False
    b = m(inp).detach()
    assert torch.equal(a, b)


def test_input_layer_voxel_map(cuda):
    from o3dml_amd.sparseconvnet import InputLayer
    g = torch.Generator().manual_seed(0)
    pos = (torch.rand((3000, 3), generator=g) * 20).to(cuda)
    feat = torch.rand((3000, 3), generator=g).to(cuda)
    avg, vpos, imap = InputLayer()(feat, pos)
    cell_of_voxel = torch.floor(vpos).long()
    assert torch.equal(cell_of_voxel[imap], torch.floor(pos).long())
    # voxel mean
    ref = torch.zeros_like(avg).index_add_(0, imap, feat) / torch.bincount(imap, minlength=avg.shape[0])[:, None]
    assert torch.allclose(avg, ref, atol=1e-6)


def test_scn_off_lattice_input_recomputes(cuda):
    """Positions off the half-integer lattice: the deferred lattice check fails,
    the forward is recomputed with per-layer checks (search rulebook), and the
    result equals a forward with the lattice rulebook disabled."""
    from o3dml_amd import layers
    m = _model(False, cuda)
    inp = _inputs(cuda)
    inp.point = [inp.point[0] - 0.1 * (torch.arange(inp.point[0].shape[0], device=cuda) % 2)[:, None]]
    a = m(inp).detach()
    for mod in m.modules():
        if isinstance(mod, layers.SparseConv):
            mod.lattice_rulebook = False
    b = m(inp).detach()
    assert torch.equal(a, b)
    with torch.no_grad():  # fused eval form, same fallback
        c = m(inp)
    assert ((c - b).abs().max() / b.abs().max()).item() < 1e-5


@pytest.mark.parametrize("residual", [True, False])
def test_scn_fused_eval_matches_unfused(cuda, residual):
    """Eval without autograd folds BN + ReLU into the next convolution's gather
    and the residual add into its epilogue; with autograd enabled the layers
    run unfused.  Same logits within fp32 rounding."""
    m = _model(residual, cuda)
    inp = _inputs(cuda)
    with torch.no_grad():
        a = m(inp)
    b = m(inp).detach()
    err = ((a - b).abs().max() / b.abs().max()).item()
    assert err < 1e-5, err


@pytest.mark.parametrize("mode", ["1", "3", "3-inline-maps"])
@pytest.mark.parametrize("residual", [True, False])
def test_scn_graph_replay_equals_eager(cuda, residual, mode, monkeypatch):
    """The eval body replayed from HIP graphs gives the eager forward's logits
    bit for bit — mode "1": one graph per size signature
    (sparseconvnet._ScnBody); mode "3": the InputLayer and every level
    grid as one library call (o3dml_scn_plan) into persistent buffers the
    captured body reads in place — on the first sighting of a size signature
    (eager, nothing captured), on the capture frame, on replays
    with new features, after a second room (second signature) was captured in
    between, and after the weights change (a new capture keyed on the
    parameter versions).  Mode 3 builds the kernel maps on a second stream
    (O3DML_SCN_MAP_STREAM, default on; "3-inline-maps": off)."""
    _graph_replay_equals_eager(cuda, residual, mode, monkeypatch, _inputs(cuda), (2, 3))


@pytest.mark.parametrize("mode", ["1", "3", "3-inline-maps"])
@pytest.mark.parametrize("residual", [True, False])
def test_scn_graph_replay_equals_eager_room_a(cuda, residual, mode, monkeypatch):
    """test_scn_graph_replay_equals_eager on the training fixture's room A
    (the same parametrisation; a second test so the first one's ids stay):
    9,920 level-0 voxels and 9/10 of its points as the second room (two
    thirds of them would leave fewer than 8,193 voxels), so both signatures
    are above kDeepMax and the captured frames are the ones whose plan runs
    the multi-workgroup levels, not the single-workgroup scn_deep_levels
    kernel the 5,000-point room takes."""
    _graph_replay_equals_eager(cuda, residual, mode, monkeypatch, _room_a(cuda), (9, 10), above=K_DEEP_MAX)


def _graph_replay_equals_eager(cuda, residual, mode, monkeypatch, inp, part, above=None):
    from o3dml_amd import sparseconvnet as S
    if mode == "3-inline-maps":
        monkeypatch.setenv("O3DML_SCN_MAP_STREAM", "0")
        mode = "3"
    m = _model(residual, cuda)
    g = torch.Generator(device="cpu").manual_seed(1)
    n = inp.point[0].shape[0]
    keep = torch.randperm(n, generator=g)[: n * part[0] // part[1]].to(cuda)
    room2 = types.SimpleNamespace(point=[inp.point[0][keep].contiguous()], feat=[inp.feat[0][keep].contiguous()],
                                  batch_lengths=[keep.shape[0]])
    if above is not None:
        assert min(_n_voxels(inp), _n_voxels(room2)) > above

    def run(x, graph):
        monkeypatch.setenv("O3DML_SCN_GRAPH", mode if graph else "0")
        with torch.no_grad():
            out = m(x).clone()
        if graph and mode == "3" and above is not None:  # the plan's own level-0 row count of this frame
            assert int(m.__dict__["_o3dml_scn_plan"][1].sizes[0]) > above
        return out

    name = {"1": "_o3dml_scn_single", "3": "_o3dml_scn_plan_bodies"}[mode]
    assert torch.equal(run(inp, True), run(inp, False))
    assert len(m.__dict__.get(name, {})) == 0  # captured on the second sighting of a size signature
    frames = [types.SimpleNamespace(point=inp.point, feat=[torch.rand_like(inp.feat[0])], batch_lengths=[n]),
              room2, room2, inp]
    for x in frames:
        assert torch.equal(run(x, True), run(x, False))
    cache = m.__dict__[name]
    assert len(cache) == 2 and all(b.graph is not None for b in cache.values())
    if mode == "3":
        assert all(isinstance(b, S._ScnPlanBody) for b in cache.values())
    else:
        assert all(isinstance(b, S._ScnBody) for b in cache.values())
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(0.5)
    for _ in range(2):
        assert torch.equal(run(inp, True), run(inp, False))
    assert len(cache) == 3


def test_scn_default_mode_batched_falls_back_to_single_graph(cuda, monkeypatch):
    """The default mode (O3DML_SCN_GRAPH unset: 3) on a batch of two — the
    frame and two thirds of its points: the plan takes one batch element, so
    the forward goes through mode 1's path (one _ScnBody over both elements,
    nothing captured by the plan) and equals the eager forward bit for bit on
    the first sighting, the capture and the replay."""
    from o3dml_amd import sparseconvnet as S
    m = _model(True, cuda)
    inp = _inputs(cuda)
    n = inp.point[0].shape[0]
    keep = torch.randperm(n, generator=torch.Generator(device="cpu").manual_seed(1))[: n * 2 // 3].to(cuda)
    batch = types.SimpleNamespace(point=[inp.point[0], inp.point[0][keep].contiguous()],
                                  feat=[inp.feat[0], inp.feat[0][keep].contiguous()],
                                  batch_lengths=[n, keep.shape[0]])
    for frame in ("first sighting", "capture", "replay"):
        monkeypatch.delenv("O3DML_SCN_GRAPH", raising=False)
        with torch.no_grad():
            out = m(batch).clone()
        monkeypatch.setenv("O3DML_SCN_GRAPH", "0")
        with torch.no_grad():
            assert torch.equal(out, m(batch)), frame
    single = m.__dict__["_o3dml_scn_single"]
    assert len(single) == 1 and all(isinstance(b, S._ScnBody) and b.graph is not None for b in single.values())
    assert not m.__dict__.get("_o3dml_scn_plan_bodies")


def test_scn_plan_matches_input_layer_and_grids(cuda):
    """o3dml_scn_plan (one call) gives the InputLayer's voxel positions, mean
    features and point -> voxel map and every level's calculate_grid bit for
    bit (the eager path's torch / ops composition)."""
    from o3dml_amd import ops
    from o3dml_amd.sparseconvnet import InputLayer, _ScnPlan
    inp = _inputs(cuda)
    pts, feat = inp.point[0], inp.feat[0]
    plan = _ScnPlan(8192 * (1 + pts.shape[0] // 8192), 3, 6, cuda)
    n, pos, vf, imap, (outs, halves) = plan.run(pts, feat)
    avg, vpos, m = InputLayer()(feat, pts)
    assert n == pts.shape[0] and torch.equal(pos, vpos) and torch.equal(vf, avg) and torch.equal(imap, m)
    p = vpos
    for lvl, half in zip(outs, halves):
        ref = ops.calculate_grid(p)
        assert torch.equal(lvl, ref)
        p = ref / 2
        assert torch.equal(half, p)


@pytest.mark.parametrize("mode", ["1", "3"])
@pytest.mark.parametrize("cols", [6, 70])
def test_scn_extra_feature_columns(cuda, cols, mode, monkeypatch):
    """Feature rows wider than three columns: the InputLayer averages columns
    0 - 2 only (the reference's sparseconvnet.py:318-326 and the eager path),
    so in every graph mode the first-sighting, capture and replay frames equal
    the eager forward of feats[:, :3] bit for bit — 6 columns (the first
    convolution's cin check used to raise in mode 3) and 70 (above the plan's
    64-column limit)."""
    m = _model(True, cuda)
    inp = _room_a(cuda)
    n = inp.batch_lengths[0]
    extra = torch.rand((n, cols - 3), generator=torch.Generator().manual_seed(cols)).to(cuda)
    wide = types.SimpleNamespace(point=inp.point, feat=[torch.cat([inp.feat[0], extra], 1)], batch_lengths=[n])
    assert wide.feat[0].shape == (n, cols)
    monkeypatch.setenv("O3DML_SCN_GRAPH", "0")
    with torch.no_grad():
        ref = m(inp).clone()
    monkeypatch.setenv("O3DML_SCN_GRAPH", mode)
    for frame in ("first sighting", "capture", "replay"):
        with torch.no_grad():
            assert torch.equal(m(wide), ref), frame
    name = {"1": "_o3dml_scn_single", "3": "_o3dml_scn_plan_bodies"}[mode]
    assert all(b.graph is not None for b in m.__dict__[name].values()) and len(m.__dict__[name]) == 1


@pytest.mark.parametrize("mode", ["1", "3"])
def test_scn_replaced_weights_invalidate_graph(cuda, mode, monkeypatch):
    """Parameters / buffers replaced by OTHER tensors (not modified in place)
    after a graph was captured and replayed: load_state_dict(assign=True), a
    fresh nn.Parameter on one convolution kernel, a fresh running_var at
    version 0 (the folded BatchNorm's version key alone cannot see it).  The
    next two forwards of the graph mode equal the eager forward on the new
    weights bit for bit and differ from the output before the change."""
    m = _model(True, cuda)
    inp = _inputs(cuda)

    def run(graph):
        monkeypatch.setenv("O3DML_SCN_GRAPH", mode if graph else "0")
        with torch.no_grad():
            return m(inp).clone()

    def load_assign():
        new = {k: (v.detach() * 0.75 if v.is_floating_point() and not k.endswith("offset") else v.detach().clone())
               for k, v in m.state_dict().items()}
        m.load_state_dict(new, assign=True)

    def new_parameter():
        conv = m.unet.net[0].sub_sparse_conv1.net
        conv.kernel = torch.nn.Parameter(conv.kernel.detach() * 1.5)

    def new_buffer():
        bn = m.batch_norm.bn
        fresh = bn.running_var * 2.0 + 0.25
        assert fresh._version == 0 and bn.running_var._version == 0
        bn.running_var = fresh

    name = {"1": "_o3dml_scn_single", "3": "_o3dml_scn_plan_bodies"}[mode]
    for change in (load_assign, new_parameter, new_buffer):
        before = [run(True) for _ in range(3)][-1]  # first sighting, capture, replay
        assert all(b.graph is not None for b in m.__dict__[name].values()) and len(m.__dict__[name]) == 1
        change()
        after = [run(True), run(True)]  # the graph mode first: nothing else has refreshed a cache for it
        ref = run(False)
        assert not torch.equal(ref, before), change.__name__
        for a in after:
            assert torch.equal(a, ref), change.__name__


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_scn_step_matches_reference(cuda, mode):
    """Forward, cross entropy and backward of the HIP SparseConvUnet on the
    two-room batch against the float64 run of the reference model (module
    docstring): strided / transposed convolutions' dIn and dW, the derived
    transpose maps under autograd, BN batch statistics over the concatenated
    batch, the OutputLayer gather's backward with several points per voxel,
    split-K dIn."""
    from o3dml_amd.sparseconvnet import SparseConvUnet
    m = SparseConvUnet(multiplier=32, residual_blocks=True, conv_block_reps=1, num_classes=20)
    sd = m.state_dict()
    m.load_state_dict(randla_weights.state_dict_for([(k, tuple(v.shape)) for k, v in sd.items()], sd))
    m = m.to(cuda).train(mode == "train")
    split = np.cumsum([0] + T["lengths"].tolist())
    pos, feat = torch.from_numpy(T["pos"]).to(cuda), torch.from_numpy(T["feat"]).to(cuda)
    inp = types.SimpleNamespace(point=[pos[split[i]:split[i + 1]] for i in range(2)],
                                feat=[feat[split[i]:split[i + 1]] for i in range(2)],
                                batch_lengths=T["lengths"].tolist())
    assert int(T["room_a_levels"][0]) > K_DEEP_MAX >= int(T["room_a_levels"][1])
    logits = m(inp)
    loss = torch.nn.functional.cross_entropy(logits, torch.from_numpy(T["labels"]).to(cuda))
    loss.backward()
    lg = logits.detach().cpu().numpy()
    p = f"scn_{mode}_"
    step = int(T["row_step"])
    # C3's rule (test_gpu_full.test_c3_step_matches_reference): against the
    # float64 run within 1e-4, or twice the reference's own float32 error where
    # that is larger; gradients also the reference's worst fp32 tensor error
    worst32 = max([float(T[k]) for k in T.files if k.startswith(p + "ref32_err_grad:")] +
                  [float(T[p + "ref32_err_norms"].max())])
    bound = lambda ref32_err: max(1e-4, 2.0 * float(ref32_err))  # noqa: E731
    gbound = lambda ref32_err: max(bound(ref32_err), worst32)  # noqa: E731
    ref_rows = T[p + "f64_logit_rows"]
    assert lg.shape == (len(pos), 20) and lg[::step].shape == ref_rows.shape
    err = _rel(lg[::step], ref_rows)
    print(f"{mode}: rows {err:.3g} (bound {bound(T[p + 'ref32_err_rows']):.3g})")
    assert err < bound(T[p + "ref32_err_rows"]), err
    assert _rel(lg[::step], TG[p + "logit_rows"]) < 1e-4  # and the fp32 reference itself
    np.testing.assert_allclose(lg.astype(np.float64).sum(0), T[p + "f64_logit_colsum"], rtol=0,
                               atol=1e-5 * len(lg) * np.abs(ref_rows).max())
    ref_loss = float(T[p + "f64_loss"])
    print(f"{mode}: loss {abs(loss.item() - ref_loss) / abs(ref_loss):.3g}")
    assert abs(loss.item() - ref_loss) < 1e-5 * abs(ref_loss)
    params = dict(m.named_parameters())
    names = [str(s) for s in T[p + "grad_names"]]
    missing = [k for k in names if k not in params or params[k].grad is None]
    assert not missing, missing
    bad, top = [], (0.0, None)
    for k, ref_norm, err32 in zip(names, T[p + "f64_grad_norms"], T[p + "ref32_err_norms"]):
        g = params[k].grad.detach().double().norm().item()
        err = abs(g - ref_norm) / (ref_norm + 1e-30)
        top = max(top, (err, k))
        if err > gbound(err32):
            bad.append((k, err, float(err32)))
    print(f"{mode}: worst gradient norm {top[0]:.3g} ({top[1]}), worst32 {worst32:.3g}")
    assert not bad, sorted(bad, key=lambda b: -b[1])[:8]
    full = [str(s) for s in T["full_grad_names"]]
    assert len(full) == 5
    for k in full:
        err = _rel(params[k].grad.cpu().numpy(), TG[p + "f64_grad:" + k])
        print(f"{mode}: full gradient {k} {err:.3g} (reference fp32 {float(T[p + 'ref32_err_grad:' + k]):.3g})")
        assert err < gbound(T[p + "ref32_err_grad:" + k]), (k, err)
    if mode == "train":
        state = m.state_dict()
        bn_names = [str(s) for s in T[p + "bn_names"]]
        assert len(bn_names) == sum(k.endswith(("running_mean", "running_var")) for k in state)
        for k, err32 in zip(bn_names, T[p + "ref32_err_bn"]):
            err = _rel(state[k].cpu().numpy(), T[p + "f64_bn:" + k])
            assert err < bound(err32), (k, err)


def test_scn_too_few_feature_columns_raise(cuda, monkeypatch):
    """Fewer than the three feature columns the InputLayer averages: the plan
    mode does not hand the short rows to o3dml_scn_plan (which would read
    three per point) but fails as the eager InputLayer does."""
    m = _model(True, cuda)
    inp = _inputs(cuda)
    narrow = types.SimpleNamespace(point=inp.point, feat=[inp.feat[0][:, :2].contiguous()],
                                   batch_lengths=inp.batch_lengths)
    for mode in ("0", "3"):
        monkeypatch.setenv("O3DML_SCN_GRAPH", mode)
        with torch.no_grad(), pytest.raises(IndexError):
            m(narrow)
