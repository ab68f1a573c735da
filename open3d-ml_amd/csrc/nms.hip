// nms.hip — rotated bird's-eye-view NMS, replacing open3d.ml.torch.ops.nms as
// bound by ml3d/torch/utils/objdet_helper.py:27 and called from
// multiclass_nms (objdet_helper.py:346) inside PointPillars.get_bboxes_single
// (point_pillars.py:1005).  Boxes are (x_min, y_min, x_max, y_max, yaw) rotated
// about their centre; overlap is the area of the convex intersection polygon
// (edge crossings + contained corners, ordered by angle, shoelace area) and a
// lower-scored box is dropped when IoU > threshold († Open3D IoUImpl /
// NmsImpl, restated in oracle/o3d_oracle.c orc_nms).  The overlap geometry
// (bev_iou) lives in box_iou.hpp, shared with the pairwise IoU kernel.
//
// Three launches, all on the caller's stream:
//   1. rank kernel: stable descending score order (rank = #{higher score} +
//      #{equal score with lower index}), O(N^2) compares over an LDS-staged
//      score tile — N is a few hundred per class (nms_pre = 100 upstream);
//   2. mask kernel: one 64-lane wavefront per (row, column block) of the upper
//      triangle; lane l tests column block*64+l and the wave ballot is the
//      64-bit suppression word (bit l: box block*64+l overlaps box row);
//   3. sweep kernel: one wavefront walks the sorted boxes in order, keeping
//      the running "removed" bitmap (and, up to 64 KiB, the mask) in LDS and
//      OR-ing in each kept box's row.
#include "box_iou.hpp"
#include "common.hpp"

namespace o3dml {

constexpr int kNmsBlock = 64;  // one wavefront == one 64-bit mask word

// Total-order sort key of a score: ascending floats map to ascending keys,
// -0 and +0 share a key (they compare equal), every NaN maps to 0, below -inf.
// With the index tie-break the ranks are a permutation for any input, so
// order[] is always fully written.
__device__ __forceinline__ uint32_t score_key(float s) {
    if (s != s) return 0u;
    const uint32_t u = __float_as_uint(s + 0.0f);  // -0 -> +0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// order[rank(i)] = i, stable descending by score_key.
__global__ void __launch_bounds__(256) nms_rank_kernel(const float* __restrict__ scores, int n,
                                                        int32_t* __restrict__ order) {
    __shared__ uint32_t tile[256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const uint32_t ki = i < n ? score_key(scores[i]) : 0u;
    int rank = 0;
    for (int base = 0; base < n; base += 256) {
        const int j = base + threadIdx.x;
        tile[threadIdx.x] = j < n ? score_key(scores[j]) : 0u;
        __syncthreads();
        const int lim = min(256, n - base);
        for (int t = 0; t < lim; ++t) {
            const uint32_t kj = tile[t];
            rank += (kj > ki) || (kj == ki && base + t < i);
        }
        __syncthreads();
    }
    if (i < n) order[rank] = i;
}

// mask[i * words + cb] bit l: sorted box (cb*64 + l) > i overlaps sorted box i.
// One wavefront per (row i, column block cb): lane l evaluates column cb*64+l
// and the 64-bit word is the wave ballot, so the n*words words come from
// n*words independent waves (the IoU is ~200 dependent ALU ops with a small
// private polygon array; wave-level parallelism is what hides it).
constexpr int kNmsRowsPerBlock = 4;
__global__ void __launch_bounds__(kNmsBlock* kNmsRowsPerBlock)
        nms_mask_kernel(const float* __restrict__ boxes, const int32_t* __restrict__ order, int n, int words,
                        float thresh, uint64_t* __restrict__ mask) {
    const int lane = threadIdx.x & (kNmsBlock - 1);
    const int i = blockIdx.y * kNmsRowsPerBlock + (threadIdx.x >> 6);
    const int cb = blockIdx.x;
    if (i >= n || cb < (i >> 6)) return;  // wave-uniform
    const int j = cb * kNmsBlock + lane;
    float me[5], other[5];
    const float* src = boxes + static_cast<int64_t>(order[i]) * 5;
#pragma unroll
    for (int k = 0; k < 5; ++k) me[k] = src[k];
    bool hit = false;
    if (j > i && j < n) {
        const float* o = boxes + static_cast<int64_t>(order[j]) * 5;
#pragma unroll
        for (int k = 0; k < 5; ++k) other[k] = o[k];
        hit = bev_iou(me, other) > thresh;
    }
    const uint64_t bits = __ballot(hit);
    if (lane == 0) mask[static_cast<int64_t>(i) * words + cb] = bits;
}

// One wavefront: greedy sweep in score order.  keep[] gets original indices.
// STAGE: the whole upper-triangular mask is first copied into LDS (coalesced),
// so the sequential loop touches no global memory; otherwise each kept row is
// read from global memory.
template <bool STAGE>
__global__ void __launch_bounds__(kNmsBlock) nms_sweep_kernel(const uint64_t* __restrict__ mask,
                                                              const int32_t* __restrict__ order, int n, int words,
                                                              int64_t* __restrict__ keep,
                                                              int64_t* __restrict__ keep_count) {
    extern __shared__ uint64_t lds[];
    uint64_t* removed = lds;
    uint64_t* rows = lds + words;
    const int t = threadIdx.x;
    for (int w = t; w < words; w += kNmsBlock) removed[w] = 0;
    if (STAGE) {
        const int64_t total = static_cast<int64_t>(n) * words;
        for (int64_t e = t; e < total; e += kNmsBlock) {
            const int r = static_cast<int>(e / words), w = static_cast<int>(e - static_cast<int64_t>(r) * words);
            if (w >= (r >> 6)) rows[e] = mask[e];
        }
    }
    __syncthreads();
    int64_t cnt = 0;
    for (int i = 0; i < n; ++i) {
        const bool gone = (removed[i >> 6] >> (i & 63)) & 1ull;
        __syncthreads();
        if (gone) continue;
        if (t == 0) keep[cnt] = order[i];
        ++cnt;
        const uint64_t* row = (STAGE ? rows : mask) + static_cast<int64_t>(i) * words;
        for (int w = (i >> 6) + t; w < words; w += kNmsBlock) removed[w] |= row[w];
        __syncthreads();
    }
    if (t == 0) *keep_count = cnt;
}

}  // namespace o3dml

using namespace o3dml;

namespace {
constexpr int64_t kNmsMaxBoxes = 1 << 16;  // mask = N^2/8 bytes (512 MiB at the cap)
constexpr size_t kNmsStageBytes = 64 * 1024;  // mask staged in LDS up to ~700 boxes
inline int64_t nms_words(int64_t n) { return ceil_div(n, kNmsBlock); }
}  // namespace

O3DML_API size_t o3dml_nms_workspace_size(int64_t n) {
    if (n <= 0) return 0;
    return ws_bytes<int32_t>(n) + ws_bytes<uint64_t>(n * nms_words(n));
}

// boxes f32 [N,5] (x1,y1,x2,y2,yaw), scores f32 [N] -> keep int64 [<=N]
// (original indices in descending-score order), *keep_count (device int64).
O3DML_API int o3dml_nms(const float* boxes, const float* scores, int64_t n, float nms_overlap_thresh, int64_t* keep,
                        int64_t* keep_count, void* workspace, size_t workspace_bytes, void* stream) {
    O3DML_GUARD_BEGIN
    O3DML_REQUIRE(n >= 0 && n <= kNmsMaxBoxes, "nms: number of boxes %lld outside [0, %lld]", (long long)n,
                  (long long)kNmsMaxBoxes);
    hipStream_t st = as_stream(stream);
    if (n == 0) {
        fill_async(keep_count, 0, sizeof(int64_t), st);
        return 0;
    }
    const int ni = static_cast<int>(n), words = static_cast<int>(nms_words(n));
    Workspace ws(workspace, workspace_bytes);
    int32_t* order = ws.take<int32_t>(n);
    uint64_t* mask = ws.take<uint64_t>(n * words);
    nms_rank_kernel<<<static_cast<unsigned>(ceil_div(n, 256)), 256, 0, st>>>(scores, ni, order);
    O3DML_LAUNCH_CHECK();
    nms_mask_kernel<<<dim3(words, static_cast<unsigned>(ceil_div(n, kNmsRowsPerBlock))), kNmsBlock * kNmsRowsPerBlock,
                      0, st>>>(boxes, order, ni, words, nms_overlap_thresh, mask);
    O3DML_LAUNCH_CHECK();
    const size_t staged = sizeof(uint64_t) * (static_cast<size_t>(words) + static_cast<size_t>(n) * words);
    if (staged <= kNmsStageBytes)
        nms_sweep_kernel<true><<<1, kNmsBlock, staged, st>>>(mask, order, ni, words, keep, keep_count);
    else
        nms_sweep_kernel<false><<<1, kNmsBlock, sizeof(uint64_t) * words, st>>>(mask, order, ni, words, keep,
                                                                                keep_count);
    O3DML_LAUNCH_CHECK();
    O3DML_GUARD_END
}
