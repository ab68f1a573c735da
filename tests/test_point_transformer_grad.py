"""PointTransformer gradients without a GPU: the numpy restatement of the
inverse neighbour list that tests/test_gpu_point_transformer_grad.py holds the
HIP kernel to, the conditions recorded in tests/golden/point_transformer_grad.npz,
the recording_grad() switch and the loud failures."""
import os

import numpy as np
import pytest
import torch

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def inverse_ref(idx, n_src):
    """(inv_splits int64 [n_src + 1], inv_pairs int32 [m * k]): row s holds the
    flat pair ids t with idx.ravel()[t] == s in ascending t."""
    flat = np.asarray(idx).ravel()
    pairs = np.argsort(flat, kind="stable").astype(np.int32)
    splits = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=n_src))]).astype(np.int64)
    return splits, pairs


def test_inverse_restatement_against_a_loop():
    rng = np.random.default_rng(0)
    for m, k, n_src in ((1, 1, 1), (7, 3, 5), (20, 4, 50)):
        idx = rng.integers(0, n_src, (m, k))
        splits, pairs = inverse_ref(idx, n_src)
        assert splits.dtype == np.int64 and pairs.dtype == np.int32 and splits[-1] == m * k
        for s in range(n_src):
            want = [i * k + j for i in range(m) for j in range(k) if idx[i, j] == s]
            assert pairs[splits[s]:splits[s + 1]].tolist() == want


def test_fixture_conditions():
    z = np.load(os.path.join(G, "point_transformer_grad.npz"))
    names = [str(s) for s in z["grad_names"]]
    zero = [str(s) for s in z["zero_grad_names"]]
    assert len(names) == 339 and len(set(names)) == 339
    assert zero == [k for k in names if k.endswith(".linear_w.5.bias")] and len(zero) == 10
    err = {k: float(e) for k, e in zip(names, z["ref32_err"])}
    rest = np.array([err[k] for k in names if k not in zero])
    assert len(rest) == 329
    assert float(z["ref32_loss_diff"]) <= 1e-5
    assert rest.max() <= 1e-2 and rest.max() == float(z["ref32_err_worst"])
    assert (rest > 5e-4).mean() <= 0.05 and (rest > 5e-4).mean() == float(z["ref32_share_above_5e-4"])
    assert np.median(rest) == float(z["ref32_err_median"])
    assert (z["f64_grad_norms"][[k not in zero for k in names]] > 0).all()
    assert len(z["zero_grad_ratios"]) == 10 and z["zero_grad_ratios"].max() < 1e-4
    full = [str(s) for s in z["full_grad_names"]]
    assert len(full) == 7
    from o3dml_amd.point_transformer import PointTransformer
    shapes = {k: tuple(p.shape) for k, p in PointTransformer().named_parameters()}
    assert list(shapes) == names
    for k in full:
        assert z["f64_grad:" + k].dtype == np.float32 and z["f64_grad:" + k].shape == shapes[k]
    labels = np.random.default_rng(int(z["label_seed"])).integers(0, 13, len(z["labels"]))
    assert np.array_equal(labels, z["labels"])
    assert os.path.getsize(os.path.join(G, "point_transformer_grad.npz")) < (1 << 20)


def test_recording_grad_exists_and_nests():
    from o3dml_amd import point_transformer as pt
    assert "recording_grad" in pt.__all__
    assert not pt._recording()
    with pt.recording_grad():
        assert pt._recording()
        with pt.recording_grad():
            assert pt._recording()
        assert pt._recording()
        with torch.no_grad():
            assert not pt._recording()
    assert not pt._recording()
    # a fold inside the switch is differentiable in weight and bias only
    bn = torch.nn.BatchNorm1d(4).eval()
    assert not pt.fold_bn(bn)[0].requires_grad
    with pt.recording_grad():
        scale, shift = pt.fold_bn(bn)
    assert scale.requires_grad and shift.requires_grad
    (scale.sum() + shift.sum()).backward()
    assert bn.weight.grad is not None and bn.bias.grad is not None


def test_switch_is_thread_local():
    import threading
    from o3dml_amd import point_transformer as pt
    seen = []
    with pt.recording_grad():
        t = threading.Thread(target=lambda: seen.append(pt._recording()))
        t.start()
        t.join()
    assert seen == [False]


def test_ops_requiring_grad_fail_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from o3dml_amd import point_transformer as pt
    xyz = torch.zeros(8, 3)
    feat = torch.zeros(8, 8, requires_grad=True)
    pos = (torch.zeros(3, 3), torch.zeros(3), torch.zeros(3), torch.zeros(3), torch.zeros(8, 3), torch.zeros(8))
    with pytest.raises(RuntimeError, match="no ROCm GPU"):
        pt.relation(None, xyz, xyz, feat, feat, pos, torch.ones(8), torch.zeros(8))
    with pytest.raises(RuntimeError, match="no ROCm GPU"):
        pt.aggregate(None, xyz, xyz, feat, torch.zeros(8, 2, 1, requires_grad=True), pos, 8)
    with pytest.raises(RuntimeError, match="no ROCm GPU"):
        pt.knn_interpolate(None, feat)
    with pytest.raises(RuntimeError, match="no ROCm GPU"):
        pt.group(None, xyz, xyz, feat)


def test_train_mode_raises_inside_the_switch():
    from o3dml_amd import point_transformer as pt
    batch = {"point": torch.zeros(8, 3), "feat": torch.zeros(8, 3), "row_splits": torch.tensor([0, 8])}
    with pt.recording_grad():
        with pytest.raises(NotImplementedError, match="PointTransformer: training is not built yet"):
            pt.PointTransformer().train()(batch)
        with pytest.raises(NotImplementedError, match="training is not built yet"):
            pt.Transformer(8, 8).train()([torch.zeros(8, 3), torch.zeros(8, 8), np.array([0, 8])])
