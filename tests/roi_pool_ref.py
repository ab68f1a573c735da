"""numpy restatement of the roi_pool contract (csrc/roi_pool.hip, DESIGN §5
"PointRCNN inference"), shared by the tests and by the fixture generator
tests/golden/make_golden_point_rcnn.py.

roi_pool_ref follows the kernel's float32 arithmetic step by step (products
rounded before they are added); numpy's float32 cos / sin may differ from the
device's in the last bit, so bit-exact comparisons use ry = 0 or inputs whose
margins (`membership_margin`, float64) are far larger than that."""
import numpy as np

PREFILTER = 10.0


def members_f32(xyz, box):
    """bool [N]: the contract's membership of every point of one cloud in one
    box (x, y, z, h, w, l, ry), in float32."""
    f = np.float32
    p = np.asarray(xyz, f)
    x, y, z, h, w, l, ry = (f(v) for v in box)
    hh, hw, hl = h * f(0.5), w * f(0.5), l * f(0.5)
    cy = y - hh
    cs, sn = np.cos(ry, dtype=f), np.sin(ry, dtype=f)
    with np.errstate(invalid="ignore"):
        dx, dy, dz = p[:, 0] - x, p[:, 1] - cy, p[:, 2] - z
        xr = dx * cs - dz * sn
        zr = dx * sn + dz * cs
        return ((np.abs(dx) <= f(PREFILTER)) & (np.abs(dy) <= hh) & (np.abs(dz) <= f(PREFILTER)) & (xr >= -hl) &
                (xr <= hl) & (zr >= -hw) & (zr <= hw))


def roi_pool_ref(xyz, boxes3d, pts_feature, sampled_pts_num):
    """-> (pooled f32 [B,M,S,3+C], empty_flag i32 [B,M], idx i32 [B,M,S])."""
    xyz = np.asarray(xyz, np.float32)
    boxes3d = np.asarray(boxes3d, np.float32)
    feat = np.asarray(pts_feature, np.float32)
    B, N, _ = xyz.shape
    M, C, S = boxes3d.shape[1], feat.shape[2], int(sampled_pts_num)
    pooled = np.zeros((B, M, S, 3 + C), np.float32)
    flag = np.zeros((B, M), np.int32)
    idx = np.full((B, M, S), -1, np.int32)
    for b in range(B):
        rows = np.concatenate([xyz[b], feat[b]], axis=1)
        for m in range(M):
            mem = np.nonzero(members_f32(xyz[b], boxes3d[b, m]))[0]
            if len(mem) == 0:
                flag[b, m] = 1
                continue
            pick = mem[:S] if len(mem) >= S else mem[np.arange(S) % len(mem)]
            idx[b, m] = pick
            pooled[b, m] = rows[pick]
    return pooled, flag, idx


def membership_margin(xyz, box):
    """float64: (inside bool [N], margin [N]) with margin the distance of each
    point to the nearest of the eight bounds that decide its membership (the
    six faces and the prefilter in x and z)."""
    p = np.asarray(xyz, np.float64)
    x, y, z, h, w, l, ry = (float(v) for v in box)
    dx, dy, dz = p[:, 0] - x, p[:, 1] - (y - h / 2), p[:, 2] - z
    xr = dx * np.cos(ry) - dz * np.sin(ry)
    zr = dx * np.sin(ry) + dz * np.cos(ry)
    slack = np.stack([PREFILTER - np.abs(dx), h / 2 - np.abs(dy), PREFILTER - np.abs(dz), l / 2 - np.abs(xr),
                      w / 2 - np.abs(zr)])
    return np.all(slack >= 0, axis=0), np.min(np.abs(slack), axis=0)
