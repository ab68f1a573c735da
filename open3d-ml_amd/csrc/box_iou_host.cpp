// box_iou_host.cpp — host pairwise rotated-box IoU, replacing
// open3d.ml.contrib.iou_bev_cpu / iou_3d_cpu: the ground-truth-sampling
// augmentation's collision test (ml3d/datasets/utils/operations.py:430, from
// forked data-loader workers) and ml3d.metrics on a machine without a GPU
// (metrics/__init__.py:8-9, metrics/mAP.py:85-89).  The same box_iou.hpp
// routine as the kernel, compiled for the host; no HIP runtime call is made
// here, so it is safe after fork() and without a device.
#include "box_iou.hpp"
#include "common.hpp"

namespace o3dml {

// out[i*m + j] = IoU(boxes_a row i, boxes_b row j), rows in `mode`'s layout.
void box_iou_host(const float* boxes_a, int64_t n, const float* boxes_b, int64_t m, int mode, float* out) {
    const int w = box_iou_row_width(mode);
    for (int64_t i = 0; i < n; ++i)
        for (int64_t j = 0; j < m; ++j) out[i * m + j] = box_iou_pair(boxes_a + i * w, boxes_b + j * w, mode);
}

}  // namespace o3dml

O3DML_API int o3dml_box_iou_host(const float* boxes_a_host, int64_t n, const float* boxes_b_host, int64_t m, int mode,
                                 float* out_host) {
    O3DML_GUARD_BEGIN
    O3DML_REQUIRE(mode == o3dml::kIouBev || mode == o3dml::kIou3d, "box_iou: mode %d is neither 0 (BEV) nor 1 (3D)",
                  mode);
    O3DML_REQUIRE(n >= 0 && m >= 0, "box_iou: negative size (n %lld, m %lld)", (long long)n, (long long)m);
    if (n == 0 || m == 0) return 0;
    O3DML_REQUIRE(boxes_a_host && boxes_b_host && out_host, "box_iou: null pointer with %lld x %lld pairs to compute",
                  (long long)n, (long long)m);
    o3dml::box_iou_host(boxes_a_host, n, boxes_b_host, m, mode, out_host);
    O3DML_GUARD_END
}
