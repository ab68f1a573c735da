"""voxelize (csrc/voxel.hip) beyond three dimensions and random floats: 1 to 8
dimensions, points on voxel faces and range limits, a partial last voxel,
empty batch items, both caps, empty inputs, both key layouts (power-of-two
strides and, from 255 batch items of the SparseConvUnet range up, plain
product strides) and the status paths.  All four outputs bit for bit against
the float64 numpy reference of tests/exact_cases.py, which orders voxels with
a lexicographic sort of (batch, coords) and so shares no key arithmetic with
the kernel; the inputs use power-of-two voxel sizes, on which the quotient
(p - min) / vs and the product with 1 / vs agree exactly."""
import numpy as np
import pytest
import torch

import exact_cases as X

pytestmark = pytest.mark.gpu


def _voxelize(cuda, c, caps=(X.BIG, X.BIG)):
    from o3dml_amd import ops
    r = ops.voxelize(torch.tensor(c["pts"]).to(cuda), torch.tensor(c["rs"]).to(cuda), torch.tensor(c["vs"]),
                     torch.tensor(c["mn"]), torch.tensor(c["mx"]), *caps)  # copies: the cases are read-only
    return tuple(t.cpu().numpy() for t in (r.voxel_coords, r.voxel_point_indices, r.voxel_point_row_splits,
                                           r.voxel_batch_splits))


NAMES = ("voxel_coords", "voxel_point_indices", "voxel_point_row_splits", "voxel_batch_splits")


@pytest.mark.parametrize("run", X.VOX_RUNS, ids=X.vox_run_id)
def test_voxelize_exact(cuda, run):
    name, caps = run
    c = X.vox_cases()[name]
    got = _voxelize(cuda, c, caps)
    ref = X.vox_ref(name, caps)
    for what, a, b in zip(NAMES, got, ref):
        assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {a.dtype} {a.shape} vs {b.dtype} {b.shape}"
        assert np.array_equal(a, b), f"{what}: {int((a != b).sum())} of {a.size} entries differ"


@pytest.mark.parametrize("name,control", [("scn-300", "scn-3"), ("scn4d-20", "scn4d-3")])
def test_voxelize_product_stride_layout(cuda, name, control):
    """The key layout with plain product strides, whose decode divides by
    strides that are no powers of two.  The conditions are asserted here so
    that the path cannot be lost by an edit: (nb+1) prod pow2ceil(ext) >=
    2^56 rules the power-of-two layout out, (nb+1) prod ext < 2^56 keeps the
    grid within the key budget.  The same points in 3 batch items take the
    power-of-two layout, as the control."""
    cs = X.vox_cases()
    p2, p1 = X.key_budget(cs[name])
    assert p2 >= 2**56 > p1
    assert X.key_budget(cs[control])[0] < 2**56
    assert np.array_equal(cs[name]["pts"], cs[control]["pts"])
    for k in (name, control):
        for a, b in zip(_voxelize(cuda, cs[k]), X.vox_ref(k, (X.BIG, X.BIG))):
            assert np.array_equal(a, b), k
    # every voxel of the many-item run is a voxel of the control run
    many = {tuple(v) for v in _voxelize(cuda, cs[name])[0].tolist()}
    few = {tuple(v) for v in _voxelize(cuda, cs[control])[0].tolist()}
    assert many == few


def test_voxelize_status_paths(cuda):
    """Checks that return before any launch."""
    g = X.vox_grid_case(3)

    def case(ndim, vs=1.0, top=4.0, n=10):
        one = np.ones(ndim, np.float32)
        return dict(pts=np.full((n, ndim), 0.5, np.float32), rs=np.array([0, n], np.int64), vs=one * np.float32(vs),
                    mn=0 * one, mx=one * np.float32(top))

    with pytest.raises(RuntimeError, match="dims"):
        _voxelize(cuda, case(9))
    for vs in (0.0, -1.0):
        with pytest.raises(RuntimeError, match="voxel_size must be > 0"):
            _voxelize(cuda, case(3, vs=vs))
    with pytest.raises(RuntimeError, match="too large"):
        _voxelize(cuda, case(8, top=1024.0))  # 2^80 cells: the product must not wrap
    with pytest.raises(RuntimeError, match="too large"):
        _voxelize(cuda, case(3, top=2.0**20))  # 2^60 cells, without wrapping
    with pytest.raises(RuntimeError, match="invalid caps"):
        _voxelize(cuda, g, (0, X.BIG))
    with pytest.raises(RuntimeError, match="invalid caps"):
        _voxelize(cuda, g, (1, -1))
    # an axis of zero cells next to huge ones is an empty grid, not an error
    c = case(8, top=1024.0)
    c["mx"][7] = 0.0
    coords, pidx, prs, bs = _voxelize(cuda, c)
    assert coords.shape == (0, 8) and len(pidx) == 0 and prs.tolist() == [0] and bs.tolist() == [0, 0]
