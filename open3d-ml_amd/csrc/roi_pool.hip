// roi_pool.hip — PointRCNN's RoI point pooling (ml3d/torch/utils/roipool3d/
// roipool3d_utils.py:24 calls open3d.ml.torch.ops.roi_pool): for every box the
// first S points inside it, in ascending point index, as rows [xyz | feature].
//
// The contract (DESIGN §5 "PointRCNN inference"; the upstream native kernel
// was not available to compare against).  Layouts, contiguous float32: xyz
// [B,N,3], boxes3d [B,M,7] = (x, y, z, h, w, l, ry) in the camera frame with
// y the bottom face and the y axis pointing down, so the centre is
// cy = y - h/2; pts_feature [B,N,C]; pooled [B,M,S,3+C]; empty_flag int32
// [B,M]; idx_out int32 [B,M,S] (nullable).  Point p is a member of a box iff
//   |px-x| <= 10, |py-cy| <= h/2, |pz-z| <= 10                (10 m prefilter)
//   xr = (px-x) cos ry - (pz-z) sin ry,  -l/2 <= xr <= l/2
//   zr = (px-x) sin ry + (pz-z) cos ry,  -w/2 <= zr <= w/2
// in float32 with every product rounded before it is added (cosf / sinf of the
// device); the bounds are closed and a NaN anywhere gives no member.  With cnt
// members: cnt == 0 -> flag 1, the box's [S,3+C] block zeros, idx -1;
// 0 < cnt < S -> slot s holds member s % cnt; cnt >= S -> the first S members.
// Rows are copied bit for bit.
//
// Mapping: a workgroup of 4 waves scans the cloud in tiles of kRpTile points
// (kRpPer per thread, so the loads of a tile are in flight together and a
// 16,384-point cloud takes four barriers); a ballot per wave and sub-tile, the
// 64 popcounts exchanged through LDS (two buffers, one barrier per tile) and
// prefix-summed by every wave with shuffles, the popcount of the lanes below
// gives a member its position, and positions < S go to an index list in LDS.
// The scan stops at the first tile that brings cnt to S.  Then lanes run along
// the (slot, channel) elements of the block: rows of 3+C floats are not
// 16-byte aligned, so one element per lane, stores coalesced, with eight
// loads of a lane in flight before their stores (the gather is bound by
// latency, not by issue).  A box's slots are split over G <= 8 workgroups
// (each repeats the scan, which reads at most 12 N bytes from L2) so that a
// call with few boxes still fills the chip.  Every output element
// is written, nothing is accumulated and there are no atomics: run-to-run
// bitwise equal, and correct on an output that was not cleared.
#include <cmath>

#include "common.hpp"

namespace o3dml {

constexpr int kRpBlock = 256;
constexpr int kRpWaves = kRpBlock / 64;
constexpr int kRpPer = 16;
constexpr int kRpTile = kRpBlock * kRpPer;
static_assert(kRpPer * kRpWaves == 64, "one popcount per lane of the prefix wave");
constexpr int kRpMaxSlots = 8192;  // the index list of a box lives in LDS
constexpr int kRpBatch = 8;        // gathered elements per lane between two rounds of stores
constexpr int kRpMaxSplit = 8;     // workgroups per box at most: each repeats the scan (16 measured slower)

__global__ void __launch_bounds__(kRpBlock)
roi_pool_kernel(const float* __restrict__ xyz, const float* __restrict__ boxes, const float* __restrict__ feat,
                int64_t N, int64_t M, int C, int S, int G, int per, float* __restrict__ pooled,
                int32_t* __restrict__ flag, int32_t* __restrict__ idx_out) {
    extern __shared__ int rp_lds[];
    int* sel = rp_lds;     // [S] members by position
    int* wc = rp_lds + S;  // [2][kRpPer][kRpWaves] popcounts of a tile, two buffers
    const int64_t bm = blockIdx.x / G;
    const int g = static_cast<int>(blockIdx.x % G);
    const int64_t b = bm / M;
    const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();

    const float* bx = boxes + bm * 7;
    const float x = bx[0], y = bx[1], z = bx[2], hh = bx[3] * 0.5f, hw = bx[4] * 0.5f, hl = bx[5] * 0.5f;
    const float cy = y - hh, cs = cosf(bx[6]), sn = sinf(bx[6]);
    const float* px = xyz + b * N * 3;

    int cnt = 0, buf = 0;
    for (int64_t t0 = 0; t0 < N && cnt < S; t0 += kRpTile, buf ^= 1) {
        bool in[kRpPer];
        uint64_t bal[kRpPer];
#pragma unroll
        for (int j = 0; j < kRpPer; ++j) {
            const int64_t i = t0 + j * kRpBlock + tid;
            in[j] = false;
            if (i < N) {
                const float dx = px[3 * i] - x, dy = px[3 * i + 1] - cy, dz = px[3 * i + 2] - z;
                const float xr = dx * cs - dz * sn, zr = dx * sn + dz * cs;
                // positive form: a NaN fails every comparison
                in[j] = fabsf(dx) <= 10.f && fabsf(dy) <= hh && fabsf(dz) <= 10.f && xr >= -hl && xr <= hl &&
                        zr >= -hw && zr <= hw;
            }
        }
#pragma unroll
        for (int j = 0; j < kRpPer; ++j) {
            bal[j] = __ballot(in[j]);
            if (lane == 0) wc[(buf * kRpPer + j) * kRpWaves + wave] = __popcll(bal[j]);
        }
        __syncthreads();
        // every wave scans the 64 popcounts of the tile itself: lane = sub-tile * kRpWaves + wave
        const int c = wc[buf * 64 + lane];
        const int inc = wave_inclusive_scan(c);
#pragma unroll
        for (int j = 0; j < kRpPer; ++j) {
            const int pos = cnt + __shfl(inc - c, j * kRpWaves + wave, 64) + __popcll(bal[j] & lanemask_lt());
            if (in[j] && pos < S) sel[pos] = static_cast<int>(t0 + j * kRpBlock + tid);
        }
        cnt += __shfl(inc, 63, 64);  // the same in every thread
    }
    __syncthreads();

    const int cu = cnt < S ? cnt : S;
    const int s0 = g * per, s1 = s0 + per < S ? s0 + per : S;
    if (g == 0 && tid == 0) flag[bm] = cu == 0;
    if (s0 >= s1) return;
    if (idx_out) {
        for (int s = s0 + tid; s < s1; s += kRpBlock) idx_out[bm * S + s] = cu == 0 ? -1 : sel[cu < S ? s % cu : s];
    }
    const int W = C + 3;
    const int total = (s1 - s0) * W;
    float* out = pooled + (bm * S + s0) * W;
    if (cu == 0) {
        for (int e = tid; e < total; e += kRpBlock) out[e] = 0.f;
        return;
    }
    const float* pf = feat + b * N * C;
    // element e = row * W + col, stepped without a division; kRpBatch loads in flight per lane
    const int dq = kRpBlock / W, dr = kRpBlock % W;
    int row = tid / W, col = tid % W;
    for (int e0 = tid; e0 < total; e0 += kRpBlock * kRpBatch) {
        float v[kRpBatch];
#pragma unroll
        for (int u = 0; u < kRpBatch; ++u) {
            if (e0 + u * kRpBlock < total) {
                const int s = s0 + row;
                const int64_t i = sel[cu < S ? s % cu : s];
                v[u] = col < 3 ? px[3 * i + col] : pf[i * C + (col - 3)];
            }
            row += dq;
            col += dr;
            if (col >= W) {
                col -= W;
                ++row;
            }
        }
#pragma unroll
        for (int u = 0; u < kRpBatch; ++u)
            if (e0 + u * kRpBlock < total) out[e0 + u * kRpBlock] = v[u];
    }
}

}  // namespace o3dml

using namespace o3dml;

O3DML_API int o3dml_roi_pool(const float* xyz, const float* boxes3d, const float* pts_feature, int64_t B, int64_t N,
                             int64_t M, int64_t C, int64_t S, float* pooled, int32_t* empty_flag, int32_t* idx_out,
                             void* stream) {
    O3DML_GUARD_BEGIN
    O3DML_REQUIRE(B >= 0 && M >= 0, "roi_pool: B = %lld, M = %lld must not be negative", (long long)B, (long long)M);
    O3DML_REQUIRE(N >= 0 && N < (int64_t(1) << 31), "roi_pool: N = %lld out of range", (long long)N);
    O3DML_REQUIRE(C >= 0 && C <= 65536, "roi_pool: C must be in 0..65536, got %lld", (long long)C);
    O3DML_REQUIRE(S >= 1 && S <= kRpMaxSlots, "roi_pool: sampled_pts_num must be in 1..%d, got %lld", kRpMaxSlots,
                  (long long)S);
    const int64_t boxes = B * M;
    if (boxes == 0) return 0;
    // split a box's slots until about four workgroups per CU are in the grid
    int64_t G = ceil_div(1024, boxes);
    if (G > kRpMaxSplit) G = kRpMaxSplit;
    if (G > S) G = S;
    const int64_t per = ceil_div(S, G);
    G = ceil_div(S, per);
    O3DML_REQUIRE(boxes * G < (int64_t(1) << 31), "roi_pool: B * M = %lld boxes exceed the grid", (long long)boxes);
    hipStream_t st = as_stream(stream);
    TimedRegion tr("roi_pool", st);
    const size_t lds = (static_cast<size_t>(S) + 2 * kRpPer * kRpWaves) * sizeof(int);
    roi_pool_kernel<<<static_cast<unsigned>(boxes * G), kRpBlock, lds, st>>>(
            xyz, boxes3d, pts_feature, N, M, static_cast<int>(C), static_cast<int>(S), static_cast<int>(G),
            static_cast<int>(per), pooled, empty_flag, idx_out);
    O3DML_LAUNCH_CHECK();
    O3DML_GUARD_END
}
