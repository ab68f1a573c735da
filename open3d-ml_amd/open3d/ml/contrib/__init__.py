"""open3d.ml.contrib: grid subsampling (KPConv) on the GPU and the pairwise
rotated-box IoU the reference's evaluation and augmentation use
(metrics/__init__.py:5-9 -> metrics/mAP.py:85-89; datasets/utils/
operations.py:7,430): ``iou_*_cuda`` run the HIP kernel, ``iou_*_cpu`` the
library's host routine (no GPU needed)."""
from o3dml_amd.contrib import (iou_3d_cpu, iou_3d_cuda, iou_bev_cpu, iou_bev_cuda,  # noqa: F401
                               subsample, subsample_batch)
