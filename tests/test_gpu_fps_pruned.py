"""Bucket-pruned farthest-point sampling (csrc/fps_pruned.hip): the bits of the
float64 reference on the exact cases, of the oracle and the direct kernels on
general floats with a bucket of two wave passes, a ragged batch against its
clouds alone, and the count of visited buckets where the algorithm fixes it."""
import numpy as np
import pytest
import torch

import exact_cases as X
import oracle as O

pytestmark = pytest.mark.gpu

EXACT = [f"lattice-{k}" for k in (1, 63, 65, 1025, 4097, 32769)] + [
    "short-40", "m1-65", "perm-1025", "identical-1025", "two-clusters-2049", "scaled-1025"]


def _splits(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


@pytest.mark.parametrize("name", EXACT)
def test_pruned_exact(cuda, name):
    """Ties, duplicates, m > n, m = 1, a box of zero extent, a tail bucket and
    distances beyond the 1e10 start value: a wrong tie direction or an unsound
    skip shows here."""
    from o3dml_amd import ops
    c = X.fps_cases()[name]
    got = ops.furthest_point_sampling(torch.tensor(c["xyz"]).to(cuda), c["m"], method="pruned").cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, c["ref"])


def test_pruned_planes_two_passes(cuda):
    """131,073 points, the smallest cloud whose buckets hold 128 points (two
    passes of a wave), on five planes plus noise so that most buckets are
    skipped; m = 500 keeps the direct kernel's rounds within a second."""
    from o3dml_amd import ops
    n, m = 2048 * 64 + 1, 500
    rng = np.random.default_rng(77)
    pts = rng.random((n, 3), dtype=np.float32) * np.array([8, 6, 3], np.float32)
    plane = rng.integers(0, 5, n)
    pts[plane < 2, 2] = (plane[plane < 2] * 3).astype(np.float32)  # floor and ceiling
    pts[plane == 2, 0] = 0
    pts[plane == 3, 0] = 8
    pts[plane == 4, 1] = 6
    pts += rng.normal(0, 0.01, (n, 3)).astype(np.float32)
    x = torch.from_numpy(pts[None]).to(cuda)
    got = ops.furthest_point_sampling(x, m, method="pruned")
    assert torch.equal(got, ops.furthest_point_sampling(x, m, method="pruned"))
    assert torch.equal(got, ops.furthest_point_sampling(x, m, method="direct"))
    assert np.array_equal(got.cpu().numpy(), O.furthest_point_sampling(pts[None], m))


def test_pruned_ragged_batch(cuda):
    """Clouds around the bucket size and above the register limit, two of
    them asked for no sample: each equals itself sampled alone by the direct
    kernels, plus its offset."""
    from o3dml_amd import ops
    from o3dml_amd.point_transformer import furthest_point_sample_ragged
    sizes = [1, 3, 63, 64, 65, 4100, 33000]
    rng = np.random.default_rng(78)
    xyz = torch.from_numpy(rng.random((sum(sizes), 3), dtype=np.float32) * np.array([4, 3, 2.5], np.float32)).to(cuda)
    rs, nrs = _splits(sizes), _splits([k // 4 for k in sizes])
    got = furthest_point_sample_ragged(xyz, rs, nrs, method="pruned")
    assert got.dtype == torch.int32 and tuple(got.shape) == (int(nrs[-1]),)
    for b, k in enumerate(sizes):
        alone = ops.furthest_point_sampling(xyz[rs[b]:rs[b + 1]][None], k // 4, method="direct")[0] + int(rs[b])
        assert torch.equal(got[nrs[b]:nrs[b + 1]], alone), b


def test_pruned_visits_each_bucket_once_on_identical_points(cuda):
    """Every point of a cloud equal: round 1 visits each bucket, after it
    every bucket's maximum and every bound are 0 and nothing is visited again,
    so the counter is the number of 64-point buckets."""
    from o3dml_amd.point_transformer import furthest_point_sample_ragged
    c = X.fps_cases()["identical-1025"]
    B, k, _ = c["xyz"].shape
    xyz = torch.tensor(c["xyz"]).to(cuda).reshape(B * k, 3)
    rs, nrs = _splits([k] * B), _splits([c["m"]] * B)
    got, visited = furthest_point_sample_ragged(xyz, rs, nrs, method="pruned", return_visited=True)
    assert np.array_equal(got.cpu().numpy().reshape(B, -1) - rs[:-1, None], c["ref"])
    assert int(visited.item()) == B * -(-k // 64)
