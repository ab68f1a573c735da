"""Parity at the FULL sizes the bench times (tests/golden/full.npz, made by
tests/golden/make_golden_full.py from the reference imported in the build
container).

C2 — SemanticKITTI-shaped 120,000-point scan (bench.make_scan(0)):
  * the GPU grid subsampling reproduces the reference sub-cloud bit for bit
    (sha256 of the oracle's contrib.subsample);
  * A2: the k = 45,056 patch crops and the 1-NN projection of every raw point
    against sklearn's float64 KDTree (randlanet.py:141-152,
    semseg_spatially_regular.py:94-95): sets / indices equal except entries
    tagged as float64 near-ties (within 1e-6 relative);
  * the fused GPU RandLANet on one full 45,056-point patch (GPU kNN levels)
    against the reference model: logits within 2e-4 abs, column sums within
    1e-5 per row.
C3 — KPFCNN (kpconv_s3dis.yml, first_features_dim 128) on bench.make_c3(0),
  40,000 points: every collate array sha-identical to the reference collate;
  eval and training mode against the reference model run in float64: logits
  within 1e-4 of their range (also vs the fp32 reference), loss within 1e-5
  relative, every parameter-gradient norm and three full gradients within
  max(1e-4, 2x the reference's own fp32-vs-fp64 error on that tensor, the
  reference's worst fp32 tensor error in that mode) — at this depth the
  reference's fp32 first-layer gradient is itself 4.4e-4 (eval) / 2.7e-3
  (training) off the fp64 one.
C4 — SparseConvUnet m=32 on the 88,006-voxel room (bench.make_room(0)):
  logits within 1e-4 of their range, column sums within 1e-5 per row, per
  element |a - b| <= 1e-4 |b| + 1e-5 max|b| against the float64 run (the
  reference's own fp32 logits sit within 2.8e-7 of it) — on the three frames
  of the default graph mode, i.e. the path bench.py times: the first sighting
  of the size signature (eager body on the plan's buffers), the capture frame
  and the replay (bit-equal to the first); a fourth frame with other features
  replays the captured body and equals the O3DML_SCN_GRAPH=0 forward bit for
  bit.  (The training step of the same model against float64:
  test_gpu_scn.test_scn_step_matches_reference.)"""
import hashlib
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.dirname(HERE))
import randla_weights  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.load(os.path.join(HERE, "golden", "full.npz"))
C2_K = 45056
C2_CENTERS = (1000, 40000, 77777)
C2_PERM_SEED = 5
C3_CFG = dict(lbl_values=list(range(13)), num_classes=13, ignored_label_inds=[], first_subsampling_dl=0.04,
              in_features_dim=5, first_features_dim=128, batch_norm_momentum=0.98, conv_radius=2.5,
              KP_extent=1.2, num_kernel_points=15)


def sha(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(a.dtype.str.encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


@pytest.fixture(scope="module")
def c2(cuda):
    import bench
    from o3dml_amd import ops
    scan, _ = bench.make_scan(0)
    scan_t = torch.from_numpy(scan).to(cuda)
    sub_t = ops.grid_subsample(scan_t, [len(scan)], 0.06).points
    return scan, scan_t, sub_t


def test_c2_grid_subsample_is_reference_subcloud(c2):
    sub = c2[2].cpu().numpy()
    assert len(sub) == int(F["c2_sub_n"]) and sha(sub) == str(F["c2_sub_sha"])


def test_c2_patch_crops_vs_sklearn(c2):
    from o3dml_amd import ops
    sub_t = c2[2]
    for j, c in enumerate(C2_CENTERS):
        got = ops.knn_search(sub_t, sub_t[c:c + 1].contiguous(), C2_K).neighbors_index.cpu().numpy()
        ref = F[f"c2_crop{j}"]
        amb = set(F[f"c2_crop{j}_amb"].tolist())
        assert len(got) == len(ref) == C2_K and len(np.unique(got)) == C2_K
        assert set(got.tolist()) - amb == set(ref.tolist()) - amb, j


def test_c2_projection_vs_sklearn(c2):
    from o3dml_amd import ops
    scan, scan_t, sub_t = c2
    proj = ops.knn_search(sub_t, scan_t, 1).neighbors_index.cpu().numpy()
    keep = np.ones(len(scan), bool)
    keep[F["c2_proj_amb"]] = False
    assert keep.sum() > 0.99 * len(scan)
    assert np.array_equal(proj[keep], F["c2_proj"][keep])


def test_c2_randla_full_patch_vs_reference(c2):
    from o3dml_amd import ops
    from o3dml_amd.randlanet import RandLANet
    sub_t = c2[2]
    c = C2_CENTERS[0]
    crop = ops.knn_search(sub_t, sub_t[c:c + 1].contiguous(), C2_K).neighbors_index.cpu().numpy()
    sub = sub_t.cpu().numpy()
    perm = np.random.default_rng(C2_PERM_SEED).permutation(C2_K)
    pc = sub[crop.astype(np.int64)][perm].copy()
    pc[:, :2] -= pc[:, :2].mean(0, dtype=np.float64).astype(np.float32)
    dev = sub_t.device
    inputs = {"features": torch.from_numpy(pc)[None].to(dev)}
    cs, nb, sb, up = [], [], [], []
    cur = torch.from_numpy(pc).to(dev)
    for _ in range(4):
        n = ops.knn_search(cur, cur, 16).neighbors_index.view(-1, 16).long()
        sub_l = cur[: cur.shape[0] // 4].contiguous()
        u = ops.knn_search(sub_l, cur, 1).neighbors_index.view(-1, 1).long()
        cs.append(cur[None])
        nb.append(n[None])
        sb.append(n[: cur.shape[0] // 4][None])
        up.append(u[None])
        cur = sub_l
    inputs.update(coords=cs, neighbor_indices=nb, sub_idx=sb, interp_idx=up)
    m = RandLANet(num_points=C2_K)
    sd = m.state_dict()
    m.load_state_dict(randla_weights.state_dict_for([(k, tuple(v.shape)) for k, v in sd.items()]))
    m = m.to(dev).eval()
    with torch.no_grad():
        out = m(inputs)[0].cpu().numpy()
    np.testing.assert_allclose(out[::11], F["c2_logit_rows"], rtol=0, atol=2e-4)
    np.testing.assert_allclose(out.astype(np.float64).sum(0), F["c2_logit_colsum"], rtol=0, atol=1e-5 * C2_K)
    # per element against the float64 run of the reference model (same
    # neighbours and weights; make_golden_full.py): |a - b| <= 1e-4 |b| + a
    # floor, the floor = 10x the reference's OWN fp32 error (max over the
    # patch of |ref32 - ref64| / max |row|, ~1.1e-6) times the row's max |b| —
    # it only matters where the logit is small against its row (the
    # reference's own fp32 logits reach 0.3 relative error there)
    b = F["c2_f64_logit_rows"]
    a = out[::11].astype(np.float64)
    floor = 10.0 * float(F["c2_ref32_err_vs_rowmax"]) * np.abs(b).max(1, keepdims=True)
    excess = np.abs(a - b) - (1e-4 * np.abs(b) + floor)
    worst = np.unravel_index(np.argmax(excess), excess.shape)
    assert excess.max() <= 0, (f"element {worst}: |a-b| {abs(a[worst] - b[worst]):.3g} vs bound "
                               f"{1e-4 * abs(b[worst]) + floor[worst[0], 0]:.3g} (b {b[worst]:.4g})")
    np.testing.assert_allclose(out.astype(np.float64).sum(0), F["c2_f64_logit_colsum"], rtol=1e-5,
                               atol=1e-6 * C2_K)


@pytest.fixture(scope="module")
def c3(cuda):
    import bench
    from o3dml_amd.kpfcnn import Config, DEFAULTS, segmentation_inputs
    pts, feats, labels, lengths = bench.make_c3(0)
    cfg = Config(DEFAULTS)
    cfg.update(C3_CFG)
    b = segmentation_inputs(cfg, torch.from_numpy(pts).to(cuda), torch.from_numpy(feats).to(cuda), labels, lengths,
                            rotations=list(F["c3_rotations"]))
    return b


def test_c3_collate_matches_reference(c3):
    b = c3
    for l in range(5):
        arrays = {"layer_points": b.points[l].cpu().numpy().astype(np.float32),
                  "neighbors": b.neighbors[l].cpu().numpy().astype(np.int32),
                  "pools": b.pools[l].cpu().numpy().astype(np.int32),
                  "upsamples": b.upsamples[l].cpu().numpy().astype(np.int32),
                  "layer_lengths": np.asarray(b.lengths[l]).astype(np.int32)}
        for name, a in arrays.items():
            shape = tuple(F[f"c3_shape_{name}_{l}"].tolist())
            if shape[0] == 0:
                assert a.shape[0] == 0, (name, l)
                continue
            assert a.shape == shape, (name, l, a.shape, shape)
            assert sha(a) == str(F[f"c3_sha_{name}_{l}"]), (name, l)


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_c3_step_matches_reference(c3, mode):
    from o3dml_amd.kpfcnn import KPFCNN
    dev = c3.features.device
    m = KPFCNN(**C3_CFG)
    sd = m.state_dict()
    new = randla_weights.state_dict_for([(k, tuple(v.shape)) for k, v in sd.items()], sd)
    for k in sd:
        if k.endswith("kernel_points"):
            new[k] = torch.from_numpy(F["c3_kp:" + k])
    m.load_state_dict(new)
    m = m.to(dev).train(mode == "train")
    logits = m(c3)
    loss = torch.nn.functional.cross_entropy(logits, c3.labels)
    loss.backward()
    lg = logits.detach().cpu().numpy()
    # against the float64 run of the reference model (the truth): within 1e-4,
    # or within twice the reference's own float32 error where that is larger
    # (deep gradients: the reference's fp32 drifts 4e-4 .. 3e-3 from fp64)
    # every gradient is also allowed the reference's own worst fp32 tensor
    # error in this mode (training: 2.7e-3 on the first KPConv weights — batch
    # statistics through five BN levels amplify fp32 rounding in both)
    worst32 = max(float(F[k]) for k in F.files if k.startswith(f"c3_{mode}_ref32_err_grad:"))
    bound = lambda ref32_err: max(1e-4, 2.0 * float(ref32_err))  # noqa: E731
    gbound = lambda ref32_err: max(bound(ref32_err), worst32)  # noqa: E731
    assert _rel(lg[::10], F[f"c3_{mode}_f64_logit_rows"]) < bound(F[f"c3_{mode}_ref32_err_rows"])
    assert _rel(lg[::10], F[f"c3_{mode}_logit_rows"]) < 1e-4  # and the fp32 reference itself
    ref_rows = F[f"c3_{mode}_logit_rows"]
    np.testing.assert_allclose(lg.astype(np.float64).sum(0), F[f"c3_{mode}_logit_colsum"], rtol=0,
                               atol=1e-5 * len(lg) * np.abs(ref_rows).max())
    ref_loss = float(F[f"c3_{mode}_f64_loss"])
    assert abs(loss.item() - ref_loss) < 1e-5 * abs(ref_loss)
    params = dict(m.named_parameters())
    names = [str(s) for s in F[f"c3_{mode}_grad_names"]]
    bad = []
    for k, ref_norm, err32 in zip(names, F[f"c3_{mode}_f64_grad_norms"], F[f"c3_{mode}_ref32_err_norms"]):
        g = params[k].grad.detach().double().norm().item()
        err = abs(g - ref_norm) / (ref_norm + 1e-30)
        if err > gbound(err32):
            bad.append((k, err, float(err32)))
    assert not bad, sorted(bad, key=lambda b: -b[1])[:8]
    for key in F.files:
        if key.startswith(f"c3_{mode}_f64_grad:"):
            k = key.split(":", 1)[1]
            err = _rel(params[k].grad.cpu().numpy(), F[key])
            assert err < gbound(F[f"c3_{mode}_ref32_err_grad:{k}"]), (k, err)


def test_c4_scn_full_room_vs_reference(cuda, monkeypatch):
    import bench
    monkeypatch.delenv("O3DML_SCN_GRAPH", raising=False)  # the default mode: what bench.py times
    from o3dml_amd.sparseconvnet import SparseConvUnet
    pos, _ = bench.make_room(0)
    assert len(pos) == int(F["c4_n"])
    feat = np.random.default_rng(3).random((len(pos), 3), dtype=np.float32)
    m = SparseConvUnet(multiplier=32, residual_blocks=True, conv_block_reps=1, num_classes=20)
    sd = m.state_dict()
    m.load_state_dict(randla_weights.state_dict_for([(k, tuple(v.shape)) for k, v in sd.items()], sd))
    m = m.to(cuda).eval()
    inp = types.SimpleNamespace(point=[torch.from_numpy(pos).to(cuda)], feat=[torch.from_numpy(feat).to(cuda)],
                                batch_lengths=[len(pos)])
    # three frames of the same room: the first sighting of its size signature
    # (the eager body on the plan's buffers), the capture frame, the replay —
    # the path behind unet.ms_per_frame
    frames = []
    with torch.no_grad():
        for j in range(3):
            frames.append(m(inp).clone())
            bodies = m.__dict__.get("_o3dml_scn_plan_bodies", {})
            if j == 0:
                assert len(bodies) == 0
            else:
                assert len(bodies) == 1 and all(b.graph is not None for b in bodies.values())
    out = frames[0].cpu().numpy()
    ref = F["c4_logit_rows"]
    assert _rel(out[::11], ref) < 1e-4
    # per element against the float64 run of the same reference model:
    # |a - b| <= 1e-4 |b| + floor, floor = 1e-5 max|b| (the reference's own
    # fp32 logits sit within c4_ref32_abs_err = 2.8e-7 of it)
    b64 = F["c4_f64_logit_rows"]
    err = np.abs(out[::11].astype(np.float64) - b64)
    bound = 1e-4 * np.abs(b64) + 1e-5 * np.abs(b64).max()
    assert (err <= bound).all(), (float((err / bound).max()), float(err.max()))
    np.testing.assert_allclose(out.astype(np.float64).sum(0), F["c4_logit_colsum"], rtol=0,
                               atol=1e-5 * len(out) * np.abs(ref).max())
    for j, frame in enumerate(frames[1:], 1):  # the capture frame and the replay, to the same bounds
        o = frame.cpu().numpy()
        err = np.abs(o[::11].astype(np.float64) - b64)
        assert (err <= bound).all(), (j, float((err / bound).max()), float(err.max()))
        np.testing.assert_allclose(o.astype(np.float64).sum(0), F["c4_logit_colsum"], rtol=0,
                                   atol=1e-5 * len(o) * np.abs(ref).max())
    assert torch.equal(frames[2], frames[0])
    # a fourth frame with other features replays the captured body: the eager
    # forward (O3DML_SCN_GRAPH=0) of the same input, bit for bit
    feat2 = np.random.default_rng(4).random((len(pos), 3), dtype=np.float32)
    inp2 = types.SimpleNamespace(point=inp.point, feat=[torch.from_numpy(feat2).to(cuda)], batch_lengths=[len(pos)])
    with torch.no_grad():
        replayed = m(inp2).clone()
        assert len(m.__dict__["_o3dml_scn_plan_bodies"]) == 1  # no new capture
        monkeypatch.setenv("O3DML_SCN_GRAPH", "0")
        eager = m(inp2)
    assert not torch.equal(replayed, frames[0]) and torch.equal(replayed, eager)
