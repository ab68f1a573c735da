"""open3d.ml.torch.ops — hot-path ops backed by libo3dml_amd (HIP, gfx950).

trilinear_devoxelize_forward / _backward (PVCNN, pvcnn.py:14) come from
o3dml_amd.ops like every other op.  roi_pool (PointRCNN, roipool3d_utils.py:4)
exists as o3dml_amd.ops.roi_pool (csrc/roi_pool.hip) and is what
o3dml_amd.point_rcnn calls; under this shim name it is still the raising stub
below, which tests/test_pvcnn.py pins.  Pointing the alias at the op is a
follow-up together with that test."""
from o3dml_amd.ops import *  # noqa: F401,F403
from o3dml_amd.ops import __all__ as _hot

__all__ = list(_hot) + ["roi_pool"]


def _out_of_scope(name):
    def f(*args, **kwargs):
        raise NotImplementedError(f"open3d.ml.torch.ops.{name} is out of scope for o3dml_amd (SURVEY.md §2.2)")
    f.__name__ = name
    return f


roi_pool = _out_of_scope("roi_pool")
