"""ops.roi_pool on the GPU against the numpy restatement of its contract
(tests/roi_pool_ref.py).  Every comparison is exact: the exact cases use
ry = 0 and dyadic coordinates, so float32 rounds nothing; the rotated case
first asserts in float64 that no point is within 1e-4 of a bound, far beyond
any float32 or cosf / sinf rounding."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from roi_pool_ref import membership_margin, roi_pool_ref  # noqa: E402

pytestmark = pytest.mark.gpu

TILE = 4096  # kRpTile of csrc/roi_pool.hip: points scanned per workgroup step
FAR = 500.0  # a coordinate outside every box and every prefilter of these tests


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def pool(cuda, xyz, boxes, feat, S):
    from o3dml_amd import ops
    out = ops.roi_pool_indexed(*(torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(cuda)
                                 for a in (xyz, boxes, feat)), S)
    pooled, flag, idx = (t.cpu().numpy() for t in out)
    assert pooled.dtype == np.float32 and flag.dtype == np.int32 and idx.dtype == np.int32
    return pooled, flag, idx


def check(cuda, xyz, boxes, feat, S):
    """GPU == restatement: index, flag and the rows bit for bit."""
    pooled, flag, idx = pool(cuda, xyz, boxes, feat, S)
    rp, rf, ri = roi_pool_ref(xyz, boxes, feat, S)
    assert np.array_equal(idx, ri)
    assert np.array_equal(flag, rf)
    assert pooled.shape == rp.shape and np.array_equal(bits(pooled), bits(rp))
    return pooled, flag, idx


def index_feature(B, N, C=1):
    """Feature channel 0 is the point index, the others a dyadic pattern."""
    f = np.zeros((B, N, C), np.float32)
    f[:, :, 0] = np.arange(N)
    for c in range(1, C):
        f[:, :, c] = (np.arange(N) * 3 + c) % 64 / 8
    return f


# ------------------------------------------------------------------ exact cases
STEP = 2.0 ** -10
BOX = (1.0, 2.0, 3.0, 2.0, 4.0, 8.0, 0.0)  # centre (1, 1, 3), half sizes l/2 = 4 (x), h/2 = 1 (y), w/2 = 2 (z)


def face_points():
    """Six points on the faces (py = y is the bottom, py = y - h the top), six
    one step beyond them, three with a NaN coordinate; all dyadic."""
    on = [(5, 1, 3), (-3, 1, 3), (1, 2, 3), (1, 0, 3), (1, 1, 5), (1, 1, 1)]
    off = [(5 + STEP, 1, 3), (-3 - STEP, 1, 3), (1, 2 + STEP, 3), (1, -STEP, 3), (1, 1, 5 + STEP), (1, 1, 1 - STEP)]
    for q in on + off:
        assert all(float(np.float32(v)) == v for v in q)  # float32 holds them exactly
    return np.array(on + off + [(np.nan, 1, 3), (1, np.nan, 3), (1, 1, np.nan)], np.float32)


def test_exact_faces(cuda):
    pts = face_points()[None]
    _, flag, idx = check(cuda, pts, np.array([[BOX]], np.float32), index_feature(1, pts.shape[1], 2), 8)
    assert flag[0, 0] == 0
    assert idx[0, 0].tolist() == [0, 1, 2, 3, 4, 5, 0, 1]  # the six face points, cyclic; nothing beyond, no NaN


def test_exact_prefilter(cuda):
    """l = w = 32: half sizes of 16 m, yet nothing beyond 10 m of the centre
    in x or z is a member; exactly 10 m is."""
    box = (0.0, 1.0, 0.0, 2.0, 32.0, 32.0, 0.0)
    pts = np.array([(10, 0, 0), (10.5, 0, 0), (-10, 0, 0), (-10.5, 0, 0), (0, 0, 10), (0, 0, 10.5), (0, 0, -10),
                    (0, 0, -10.5), (10 + STEP, 0, 0), (0, 0, -10 - STEP)], np.float32)[None]
    _, flag, idx = check(cuda, pts, np.array([[box]], np.float32), index_feature(1, pts.shape[1]), 4)
    assert flag[0, 0] == 0 and idx[0, 0].tolist() == [0, 2, 4, 6]


def test_nan_box_is_empty(cuda):
    pts = np.array([(1, 1, 3)] * 5, np.float32)[None]
    boxes = np.array([[BOX] * 8], np.float32)
    for k in range(7):
        boxes[0, k, k] = np.nan
    pooled, flag, idx = check(cuda, pts, boxes, index_feature(1, 5, 3), 4)
    assert flag[0].tolist() == [1] * 7 + [0]
    assert np.all(idx[0, :7] == -1) and np.all(bits(pooled[0, :7]) == 0)
    assert idx[0, 7].tolist() == [0, 1, 2, 3]


# ------------------------------------------------------------------ counts
def cloud_with_members(N, members_per_box):
    """N points far away, except that box k (centre x = 40 k) holds the points
    listed for it; boxes 2 x 2 x 2, ry = 0."""
    xyz = np.full((1, N, 3), FAR, np.float32)
    boxes = []
    assert len({i for mem in members_per_box for i in mem}) == sum(len(mem) for mem in members_per_box)
    for k, mem in enumerate(members_per_box):
        boxes.append((40.0 * k, 1.0, 0.0, 2.0, 2.0, 2.0, 0.0))
        for j, i in enumerate(mem):
            xyz[0, i] = (40.0 * k + (j % 5) / 4 - 0.5, (j % 3) / 2 - 0.5, (j % 7) / 8)
    return xyz, np.array([boxes], np.float32)


def test_counts_at_s8(cuda):
    mem = {0: [], 1: [17], 3: [4, 90, 91], 7: list(range(100, 107)), 8: list(range(200, 216, 2)),
           9: list(range(300, 309))}
    xyz, boxes = cloud_with_members(400, list(mem.values()))
    _, flag, idx = check(cuda, xyz, boxes, index_feature(1, 400, 2), 8)
    assert flag[0].tolist() == [1, 0, 0, 0, 0, 0]
    assert idx[0, 0].tolist() == [-1] * 8
    assert idx[0, 1].tolist() == [17] * 8
    assert idx[0, 2].tolist() == [4, 90, 91, 4, 90, 91, 4, 90]
    assert idx[0, 3].tolist() == list(range(100, 107)) + [100]
    assert idx[0, 4].tolist() == mem[8]
    assert idx[0, 5].tolist() == mem[9][:8]


def test_every_point_a_member_n_below_s(cuda):
    xyz, boxes = cloud_with_members(5, [list(range(5))])
    _, _, idx = check(cuda, xyz, boxes, index_feature(1, 5), 8)
    assert idx[0, 0].tolist() == [0, 1, 2, 3, 4, 0, 1, 2]


@pytest.mark.parametrize("N", [TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE + 10])
def test_tile_edges(cuda, N):
    """Members at the ends of the scan tiles and of the cloud; the S-th member
    of box 1 lies in a later tile than its first where the cloud has one."""
    last = [0, 63, 64, 255, 256, N - 4, N - 2]
    spread = sorted(({5, N - 1} | {i for i in (TILE - 1, TILE, TILE + 3, TILE + 700) if i < N} |
                     set(range(N // 2, N // 2 + 6))) - set(last))
    xyz, boxes = cloud_with_members(N, [last, spread, [N - 3]])
    _, flag, idx = check(cuda, xyz, boxes, index_feature(1, N, 2), 8)
    assert idx[0, 0].tolist() == last + [0] and idx[0, 1].tolist() == spread[:8] and idx[0, 2].tolist() == [N - 3] * 8
    assert flag[0].tolist() == [0, 0, 0]
    assert N < 2 * TILE or spread[0] < TILE <= spread[7]


def test_empty_box_overwrites_a_nan_filled_output(cuda):
    """Through the C entry, on outputs pre-filled with NaN / garbage and no
    memset: an empty box's block must come back as zeros."""
    from o3dml_amd import _lib
    from o3dml_amd._util import ptr, stream_handle
    xyz, boxes = cloud_with_members(300, [[], [7, 8]])
    C, S = 5, 8
    x, b = torch.from_numpy(xyz).to(cuda), torch.from_numpy(boxes).to(cuda)
    f = torch.from_numpy(index_feature(1, 300, C)).to(cuda)
    pooled = torch.full((1, 2, S, 3 + C), float("nan"), device=cuda)
    flag = torch.full((1, 2), 77, dtype=torch.int32, device=cuda)
    idx = torch.full((1, 2, S), 77, dtype=torch.int32, device=cuda)
    _lib.call("o3dml_roi_pool", ptr(x), ptr(b), ptr(f), 1, 300, 2, C, S, ptr(pooled), ptr(flag), ptr(idx),
              stream_handle(cuda))
    assert np.all(bits(pooled[0, 0].cpu().numpy()) == 0)
    assert flag.cpu().tolist() == [[1, 0]] and idx[0, 0].cpu().tolist() == [-1] * S
    rp, _, ri = roi_pool_ref(xyz, boxes, f.cpu().numpy(), S)
    assert np.array_equal(bits(pooled.cpu().numpy()), bits(rp)) and np.array_equal(idx.cpu().numpy(), ri)
    # idx_out may be null
    pooled2 = torch.full_like(pooled, float("nan"))
    _lib.call("o3dml_roi_pool", ptr(x), ptr(b), ptr(f), 1, 300, 2, C, S, ptr(pooled2), ptr(flag), None,
              stream_handle(cuda))
    assert np.array_equal(bits(pooled2.cpu().numpy()), bits(rp))


# ------------------------------------------------------------------ shapes
@pytest.mark.parametrize("M,C,S", [(1, 1, 1), (3, 2, 7), (65, 130, 512), (1, 130, 7), (65, 1, 512), (3, 2, 512)])
def test_shapes(cuda, M, C, S):
    """B = 2 with different boxes per batch item; points on a 1/8 grid, boxes
    with dyadic sizes and ry = 0, so float32 is exact on both sides."""
    rng = np.random.default_rng(100 * M + C + S)
    N = 1500
    xyz = (rng.integers(0, 8 * 24, (2, N, 3)) / 8).astype(np.float32)
    boxes = np.zeros((2, M, 7), np.float32)
    boxes[:, :, :3] = rng.integers(0, 4 * 24, (2, M, 3)) / 4
    boxes[:, :, 3:6] = rng.integers(1, 8 * 14, (2, M, 3)) / 4  # up to 28 m: the prefilter cuts some
    feat = (rng.integers(-512, 512, (2, N, C)) / 16).astype(np.float32)
    feat[:, :, 0] = np.arange(N)
    _, flag, idx = check(cuda, xyz, boxes, feat, S)
    assert not np.array_equal(idx[0], idx[1])
    if M == 65:  # empty, partly filled and (for S = 512, C = 1 or 130) cyclic boxes are all present
        cnt = np.array([[len(np.unique(i[i >= 0])) for i in idx[b]] for b in range(2)])
        assert (cnt == 0).any() and ((cnt > 0) & (cnt < S)).any()


# ------------------------------------------------------------------ rotated
def rotated_case():
    rng = np.random.default_rng(26)  # a seed whose margins pass test_rotated_random's assertion
    B, N, M = 2, 1000, 9
    xyz = (rng.random((B, N, 3)) * [30, 4, 30] + [-15, -1, 0]).astype(np.float32)
    boxes = np.zeros((B, M, 7), np.float32)
    boxes[:, :, :3] = rng.random((B, M, 3)) * [20, 2, 20] + [-10, 1, 5]
    boxes[:, :, 3:6] = rng.random((B, M, 3)) * [3, 10, 22] + [1, 2, 2]
    boxes[:, :, 6] = rng.random((B, M)) * 2 * np.pi - np.pi
    feat = index_feature(B, N, 4)
    return xyz, boxes, feat


def test_rotated_random(cuda):
    xyz, boxes, feat = rotated_case()
    inside = 0
    for b in range(2):
        for m in range(9):
            ins, margin = membership_margin(xyz[b], boxes[b, m])
            assert margin.min() > 1e-4, (b, m, margin.min())
            inside += int(ins.sum())
    assert inside > 500  # not a vacuous case
    pooled, flag, idx = check(cuda, xyz, boxes, feat, 64)
    assert np.array_equal(pooled[..., 3][idx >= 0], idx[idx >= 0].astype(np.float32))  # channel 0 is the index
    cnt = np.array([[len(np.unique(i[i >= 0])) for i in idx[b]] for b in range(2)])
    assert ((cnt > 0) & (cnt < 64)).any() and (cnt == 64).any()


def test_two_runs_bitwise_equal(cuda):
    xyz, boxes, feat = rotated_case()
    a, b = pool(cuda, xyz, boxes, feat, 64), pool(cuda, xyz, boxes, feat, 64)
    for u, v in zip(a, b):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32))


# ------------------------------------------------------------------ surface
def test_status_paths(cuda):
    from o3dml_amd import ops
    xyz = torch.zeros(2, 10, 3, device=cuda)
    boxes = torch.ones(2, 4, 7, device=cuda)
    feat = torch.zeros(2, 10, 5, device=cuda)
    with pytest.raises(RuntimeError, match="float32"):
        ops.roi_pool(xyz.double(), boxes, feat, 4)
    with pytest.raises(RuntimeError, match="float32"):
        ops.roi_pool(xyz, boxes, feat.half(), 4)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.roi_pool(xyz, boxes, torch.zeros(2, 5, 10, device=cuda).transpose(1, 2), 4)
    with pytest.raises(RuntimeError, match="share B"):
        ops.roi_pool(xyz, boxes[:1], feat, 4)
    with pytest.raises(RuntimeError, match="share B"):
        ops.roi_pool(xyz, boxes, feat[:, :9].contiguous(), 4)
    with pytest.raises(RuntimeError, match="xyz must be float32"):
        ops.roi_pool(torch.zeros(2, 10, 4, device=cuda), boxes, feat, 4)
    with pytest.raises(RuntimeError, match="boxes3d must be float32"):
        ops.roi_pool(xyz, torch.zeros(2, 4, 5, device=cuda), feat, 4)
    with pytest.raises(RuntimeError, match="sampled_pts_num"):
        ops.roi_pool(xyz, boxes, feat, 0)
    pooled, flag = ops.roi_pool(xyz, boxes[:, :0], feat, 4)  # M = 0
    assert tuple(pooled.shape) == (2, 0, 4, 8) and tuple(flag.shape) == (2, 0) and flag.dtype == torch.int32
    pooled, flag = ops.roi_pool(xyz[:, :0], boxes, feat[:, :0], 4)  # N = 0
    assert tuple(pooled.shape) == (2, 4, 4, 8) and not pooled.any() and flag.cpu().tolist() == [[1] * 4] * 2


def test_registered_torch_op(cuda):
    import o3dml_amd
    from o3dml_amd import ops
    o3dml_amd.register_torch_ops()
    xyz, boxes, feat = (torch.from_numpy(a).to(cuda) for a in rotated_case())
    a = torch.ops.open3d.roi_pool(xyz, boxes, feat, 16)
    b = ops.roi_pool(xyz, boxes, feat, 16)
    assert len(a) == 2 and a[1].dtype == torch.int32
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
