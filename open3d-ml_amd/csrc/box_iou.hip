// box_iou.hip — pairwise rotated-box IoU (BEV and 3D), replacing
// open3d.ml.contrib.iou_bev_cuda / iou_3d_cuda as bound by
// ml3d/metrics/__init__.py:5-6 and called from precision_3d
// (metrics/mAP.py:85-89) and PointRCNN's proposal target layer
// (torch/models/point_rcnn.py:1423).  The geometry and the row layouts are
// box_iou.hpp's († Open3D IoUImpl, restated).
//
// One ragged, batched launch: frame f holds rows [a_splits[f], a_splits[f+1])
// of boxes_a and [b_splits[f], b_splits[f+1]) of boxes_b, and its row-major
// [n_f, m_f] block of the output starts at out_offsets[f] (prefix sums of
// n_f*m_f).  A single pair of box sets is a batch of one.  One lane per
// (i, j) pair, pairs dealt to lanes in output order: the IoU is ~200
// dependent ALU operations with a small private polygon array, and it is the
// number of independent waves that hides it (as in nms_mask_kernel), so the
// grid is one thread per pair up to a cap, then grid-stride.
#include "box_iou.hpp"
#include "common.hpp"

namespace o3dml {

constexpr int kIouBlock = 256;
constexpr int64_t kIouMaxBlocks = 1 << 20;

template <int MODE>
__global__ void __launch_bounds__(kIouBlock)
        box_iou_ragged_kernel(const float* __restrict__ boxes_a, int64_t n_a, const int64_t* __restrict__ a_splits,
                              const float* __restrict__ boxes_b, int64_t n_b, const int64_t* __restrict__ b_splits,
                              const int64_t* __restrict__ out_offsets, int n_batch, int64_t n_pairs,
                              float* __restrict__ out) {
    constexpr int W = MODE == kIou3d ? 7 : 5;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kIouBlock;
    for (int64_t p = static_cast<int64_t>(blockIdx.x) * kIouBlock + threadIdx.x; p < n_pairs; p += stride) {
        // frame of pair p: the last f with out_offsets[f] <= p (empty frames
        // repeat an offset and are skipped by the search)
        const int f = batch_of(p, out_offsets, n_batch);
        const int64_t a0 = a_splits[f], b0 = b_splits[f];
        const int64_t nf = a_splits[f + 1] - a0, mf = b_splits[f + 1] - b0;
        const int64_t local = p - out_offsets[f];
        float v = 0.f;
        // splits that do not describe the offsets (a caller's mistake) read
        // nothing out of range: the pair is written as 0
        if (mf > 0 && local >= 0 && local < nf * mf) {
            const int64_t ia = a0 + local / mf, ib = b0 + local % mf;
            if (ia >= 0 && ia < n_a && ib >= 0 && ib < n_b) {
                float a[W], b[W];
#pragma unroll
                for (int k = 0; k < W; ++k) {
                    a[k] = boxes_a[ia * W + k];
                    b[k] = boxes_b[ib * W + k];
                }
                v = box_iou_pair(a, b, MODE);
            }
        }
        out[p] = v;
    }
}

}  // namespace o3dml

using namespace o3dml;

O3DML_API int o3dml_box_iou_ragged(const float* boxes_a, int64_t n_a, const int64_t* a_row_splits,
                                   const float* boxes_b, int64_t n_b, const int64_t* b_row_splits,
                                   const int64_t* out_offsets, int64_t n_batch, int64_t n_pairs, int mode, float* out,
                                   void* stream) {
    O3DML_GUARD_BEGIN
    O3DML_REQUIRE(mode == kIouBev || mode == kIou3d, "box_iou: mode %d is neither 0 (BEV) nor 1 (3D)", mode);
    O3DML_REQUIRE(n_a >= 0 && n_b >= 0 && n_pairs >= 0, "box_iou: negative size (n_a %lld, n_b %lld, n_pairs %lld)",
                  (long long)n_a, (long long)n_b, (long long)n_pairs);
    O3DML_REQUIRE(n_batch >= 1 && n_batch <= INT32_MAX - 1, "box_iou: n_batch %lld outside [1, 2^31-2]",
                  (long long)n_batch);
    if (n_pairs == 0) return 0;
    O3DML_REQUIRE(boxes_a && boxes_b && a_row_splits && b_row_splits && out_offsets && out,
                  "box_iou: null pointer with %lld pairs to compute", (long long)n_pairs);
    hipStream_t st = as_stream(stream);
    int64_t blocks = ceil_div(n_pairs, kIouBlock);
    if (blocks > kIouMaxBlocks) blocks = kIouMaxBlocks;
    TimedRegion tr("box_iou", st);
    if (mode == kIou3d)
        box_iou_ragged_kernel<kIou3d><<<static_cast<unsigned>(blocks), kIouBlock, 0, st>>>(
                boxes_a, n_a, a_row_splits, boxes_b, n_b, b_row_splits, out_offsets, static_cast<int>(n_batch),
                n_pairs, out);
    else
        box_iou_ragged_kernel<kIouBev><<<static_cast<unsigned>(blocks), kIouBlock, 0, st>>>(
                boxes_a, n_a, a_row_splits, boxes_b, n_b, b_row_splits, out_offsets, static_cast<int>(n_batch),
                n_pairs, out);
    O3DML_LAUNCH_CHECK();
    O3DML_GUARD_END
}
