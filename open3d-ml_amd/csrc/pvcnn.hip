// pvcnn.hip — PVCNN's point <-> voxel ops (ml3d/torch/models/pvcnn.py:14, 37,
// 57, 579-619): trilinear devoxelize forward / backward and mean voxelize
// forward / backward over a dense r^3 grid per batch item.
//
// Layouts (contiguous float32 unless noted, r3 = r*r*r):
//   coords [B,3,N] (grid units), feat/grid [B,C,r3], outs [B,C,N],
//   inds int32 [B,8,N], wgts [B,8,N], vox int32 [B,3,N], cnt int32 [B,r3].
// Mapping: one lane per point (devoxelize forward, voxelize backward) or per
// voxel (the two sums), looping over a group of channels, so a point's corner
// indices and weights and a voxel's entry list are read once per group and the
// stores along N / r3 are coalesced; the gathers stay inside one channel plane
// (128 KB at r = 32).
// Order of sums: every scatter-add is turned into a per-destination list
// (prim::build_inverse: stable sort, ascending source position) that one lane
// sums front to back, every product rounded before it is added
// (-ffp-contract=off).  No float atomics, no memset: run-to-run bitwise equal.
// Known worst case: all points in one voxel leave one lane summing B*N (or
// 8*N) terms; accepted.
#include "common.hpp"
#include "primitives.hpp"

namespace o3dml {

constexpr int kPvBlock = 256;
constexpr int kPvChan = 16;  // channels per block of the per-point kernels
constexpr int kPvAcc = 8;    // accumulators per lane of the per-voxel sums

__device__ __forceinline__ float clamp_grid(float a, float top) { return fminf(fmaxf(a, 0.f), top); }

__global__ void __launch_bounds__(kPvBlock)
devox_forward_kernel(const float* __restrict__ coords, const float* __restrict__ feat, int C, int N, int r,
                     int write_iw, float* __restrict__ outs, int32_t* __restrict__ inds,
                     float* __restrict__ wgts) {
    const int64_t i = blockIdx.x * static_cast<int64_t>(kPvBlock) + threadIdx.x;
    if (i >= N) return;
    const int64_t b = blockIdx.z;
    const int64_t r3 = static_cast<int64_t>(r) * r * r;
    const float top = static_cast<float>(r - 1);
    const float* cp = coords + b * 3 * N;
    int lo[3], hi[3];
    float d0[3], d1[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float x = clamp_grid(cp[static_cast<int64_t>(a) * N + i], top);
        const float f = floorf(x);
        d1[a] = x - f;
        d0[a] = 1.0f - d1[a];
        lo[a] = static_cast<int>(f);
        hi[a] = lo[a] + (d1[a] > 0.f ? 1 : 0);
    }
    int idx[8];
    float w[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int bx = (k >> 2) & 1, by = (k >> 1) & 1, bz = k & 1;
        idx[k] = ((bx ? hi[0] : lo[0]) * r + (by ? hi[1] : lo[1])) * r + (bz ? hi[2] : lo[2]);
        w[k] = ((bx ? d1[0] : d0[0]) * (by ? d1[1] : d0[1])) * (bz ? d1[2] : d0[2]);
    }
    if (write_iw && blockIdx.y == 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            inds[(b * 8 + k) * N + i] = idx[k];
            wgts[(b * 8 + k) * N + i] = w[k];
        }
    }
    const int c0 = blockIdx.y * kPvChan;
    const int c1 = min(C, c0 + kPvChan);
    for (int c = c0; c < c1; ++c) {
        const float* f = feat + (b * C + c) * r3;
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = f[idx[k]];
        float acc = w[0] * v[0];
#pragma unroll
        for (int k = 1; k < 8; ++k) acc += w[k] * v[k];
        outs[(b * C + c) * N + i] = acc;
    }
}

// key of entry e of inds [B,8,N]: b * r3 + inds[e]; an index outside [0, r3)
// gets the key B * r3, which build_inverse drops
__global__ void devox_keys_kernel(const int32_t* __restrict__ inds, int64_t B, int64_t per_batch, int64_t r3,
                                  uint32_t* __restrict__ keys) {
    const int64_t total = B * per_batch;
    for (int64_t e = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; e < total;
         e += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int64_t b = e / per_batch;
        const int64_t v = inds[e];
        keys[e] = static_cast<uint32_t>(v >= 0 && v < r3 ? b * r3 + v : B * r3);
    }
}

// grad_feat[b,c,v] = sum over the entries of voxel (b,v), ascending flat
// position e = k*N + i, of wgts.flat[e] * grad_out[b,c,i]
__global__ void __launch_bounds__(kPvBlock)
devox_backward_kernel(const float* __restrict__ grad_out, const float* __restrict__ wgts,
                      const uint32_t* __restrict__ pairs, const int64_t* __restrict__ off, int C, int64_t N,
                      int64_t r3, float* __restrict__ grad_feat) {
    const int64_t v = blockIdx.x * static_cast<int64_t>(kPvBlock) + threadIdx.x;
    if (v >= r3) return;
    const int64_t b = blockIdx.z;
    const int c0 = blockIdx.y * kPvAcc;
    const int nc = min(kPvAcc, C - c0);
    const float* g = grad_out + (b * C + c0) * N;
    const int64_t base = b * 8 * N;
    float acc[kPvAcc];
#pragma unroll
    for (int j = 0; j < kPvAcc; ++j) acc[j] = 0.f;
    const int64_t p1 = off[b * r3 + v + 1];
    for (int64_t p = off[b * r3 + v]; p < p1; ++p) {
        const uint32_t e = pairs[p];
        const float w = wgts[e];
        const int64_t i = (static_cast<int64_t>(e) - base) % N;
#pragma unroll
        for (int j = 0; j < kPvAcc; ++j)
            if (j < nc) acc[j] += w * g[j * N + i];
    }
#pragma unroll
    for (int j = 0; j < kPvAcc; ++j)
        if (j < nc) grad_feat[(b * C + c0 + j) * r3 + v] = acc[j];
}

__device__ __forceinline__ int clamp_vox(int v, int r) { return min(max(v, 0), r - 1); }

__device__ __forceinline__ int64_t vox_hash(const int32_t* __restrict__ vb, int64_t N, int64_t i, int r) {
    const int64_t x = clamp_vox(vb[i], r), y = clamp_vox(vb[N + i], r), z = clamp_vox(vb[2 * N + i], r);
    return (x * r + y) * r + z;
}

__global__ void vox_keys_kernel(const int32_t* __restrict__ vox, int64_t B, int64_t N, int r, int64_t r3,
                                uint32_t* __restrict__ keys) {
    const int64_t total = B * N;
    for (int64_t e = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; e < total;
         e += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int64_t b = e / N;
        keys[e] = static_cast<uint32_t>(b * r3 + vox_hash(vox + b * 3 * N, N, e - b * N, r));
    }
}

__global__ void vox_count_kernel(const int64_t* __restrict__ off, int64_t nseg, int32_t* __restrict__ cnt) {
    for (int64_t s = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; s < nseg;
         s += static_cast<int64_t>(gridDim.x) * blockDim.x)
        cnt[s] = static_cast<int32_t>(off[s + 1] - off[s]);
}

// grid[b,c,v] = (sum of feat[b,c,i] over the voxel's points, ascending i) / max(cnt, 1)
__global__ void __launch_bounds__(kPvBlock)
vox_forward_kernel(const float* __restrict__ feat, const uint32_t* __restrict__ pairs,
                   const int64_t* __restrict__ off, int C, int64_t N, int64_t r3, float* __restrict__ grid) {
    const int64_t v = blockIdx.x * static_cast<int64_t>(kPvBlock) + threadIdx.x;
    if (v >= r3) return;
    const int64_t b = blockIdx.z;
    const int c0 = blockIdx.y * kPvAcc;
    const int nc = min(kPvAcc, C - c0);
    const float* f = feat + (b * C + c0) * N;
    float acc[kPvAcc];
#pragma unroll
    for (int j = 0; j < kPvAcc; ++j) acc[j] = 0.f;
    const int64_t p0 = off[b * r3 + v], p1 = off[b * r3 + v + 1];
    for (int64_t p = p0; p < p1; ++p) {
        const int64_t i = static_cast<int64_t>(pairs[p]) - b * N;
#pragma unroll
        for (int j = 0; j < kPvAcc; ++j)
            if (j < nc) acc[j] += f[j * N + i];
    }
    const float den = static_cast<float>(p1 > p0 ? p1 - p0 : 1);
#pragma unroll
    for (int j = 0; j < kPvAcc; ++j)
        if (j < nc) grid[(b * C + c0 + j) * r3 + v] = acc[j] / den;
}

// grad_feat[b,c,i] = grad_grid[b,c,h_i] / cnt[b,h_i]
__global__ void __launch_bounds__(kPvBlock)
vox_backward_kernel(const float* __restrict__ grad_grid, const int32_t* __restrict__ vox,
                    const int32_t* __restrict__ cnt, int C, int64_t N, int r, int64_t r3,
                    float* __restrict__ grad_feat) {
    const int64_t i = blockIdx.x * static_cast<int64_t>(kPvBlock) + threadIdx.x;
    if (i >= N) return;
    const int64_t b = blockIdx.z;
    const int64_t h = vox_hash(vox + b * 3 * N, N, i, r);
    const int32_t n = cnt[b * r3 + h];
    const float den = static_cast<float>(n > 1 ? n : 1);
    const int c0 = blockIdx.y * kPvChan;
    const int c1 = min(C, c0 + kPvChan);
    for (int c = c0; c < c1; ++c) grad_feat[(b * C + c) * N + i] = grad_grid[(b * C + c) * r3 + h] / den;
}

namespace {

int64_t checked_r3(const char* what, int64_t B, int64_t per_batch, int64_t r) {
    O3DML_REQUIRE(r >= 1, "%s: resolution must be >= 1, got %lld", what, (long long)r);
    O3DML_REQUIRE(r <= 1290, "%s: resolution %lld: r^3 exceeds 2^31 - 1", what, (long long)r);
    const int64_t r3 = r * r * r;
    O3DML_REQUIRE(r3 <= 2147483647LL, "%s: resolution %lld: r^3 exceeds 2^31 - 1", what, (long long)r);
    O3DML_REQUIRE(B >= 0 && per_batch >= 0, "%s: negative size", what);
    const unsigned __int128 lim = static_cast<unsigned __int128>(1) << 32;
    const unsigned __int128 ub = static_cast<unsigned __int128>(B);
    O3DML_REQUIRE(ub * static_cast<unsigned __int128>(per_batch) < lim, "%s: %lld x %lld entries exceed 32-bit ids",
                  what, (long long)B, (long long)per_batch);
    O3DML_REQUIRE(ub * static_cast<unsigned __int128>(r3) < lim - 1, "%s: %lld x %lld voxels exceed 32-bit ids", what,
                  (long long)B, (long long)r3);
    return r3;
}

// grid of a kernel with one lane per element of n, a channel group per
// blockIdx.y and a batch item per blockIdx.z
dim3 pv_grid(const char* what, int64_t n, int64_t C, int group, int64_t B) {
    const int64_t gx = ceil_div(n, kPvBlock), gy = ceil_div(C, group);
    O3DML_REQUIRE(gx < (int64_t(1) << 31) && gy <= 65535 && B <= 65535,
                  "%s: launch grid %lld x %lld x %lld too large", what, (long long)gx, (long long)gy, (long long)B);
    return dim3(static_cast<unsigned>(gx), static_cast<unsigned>(gy), static_cast<unsigned>(B));
}

// A plan is the workspace of one build_inverse call: [keys | sorted keys |
// pairs | off | sort scratch].  The views below restate where build_inverse
// put pairs and off; the builders check them against what it returned.
struct PlanView {
    const uint32_t* pairs;
    const int64_t* off;
};

PlanView plan_view(const void* plan_ws, int64_t total) {
    const char* base = static_cast<const char*>(plan_ws);
    const size_t slab = ws_bytes<uint32_t>(total);
    return PlanView{reinterpret_cast<const uint32_t*>(base + 2 * slab),
                    reinterpret_cast<const int64_t*>(base + 3 * slab)};
}

size_t plan_bytes(int64_t total, int64_t nseg) { return ws_bytes<uint32_t>(total) + prim::inverse_workspace_bytes(total, nseg); }

void check_plan(const prim::Inverse& inv, const void* plan_ws, int64_t total) {
    const PlanView pv = plan_view(plan_ws, total);
    O3DML_REQUIRE(pv.pairs == inv.pairs && pv.off == inv.off, "pvcnn: plan layout does not match build_inverse");
}

}  // namespace
}  // namespace o3dml

using namespace o3dml;

// coords [B,3,N], feat [B,C,r3] -> outs [B,C,N]; inds int32 / wgts [B,8,N]
// written when is_training, zero-filled otherwise
O3DML_API int o3dml_trilinear_devoxelize_forward(const float* coords, const float* feat, int64_t B, int64_t C,
                                                 int64_t N, int64_t r, int is_training, float* outs, int32_t* inds,
                                                 float* wgts, void* stream) {
    O3DML_GUARD_BEGIN
    checked_r3("trilinear_devoxelize_forward", B, 8 * N, r);
    O3DML_REQUIRE(C >= 0 && N < (int64_t(1) << 31), "trilinear_devoxelize_forward: bad C or N");
    if (B == 0 || N == 0) return 0;
    hipStream_t st = as_stream(stream);
    if (!is_training) {
        if (inds) fill_async(inds, 0, sizeof(int32_t) * B * 8 * N, st);
        if (wgts) fill_async(wgts, 0, sizeof(float) * B * 8 * N, st);
    }
    const int write_iw = is_training && inds && wgts;
    if (C == 0 && !write_iw) return 0;
    const dim3 g = pv_grid("trilinear_devoxelize_forward", N, C > 0 ? C : 1, kPvChan, B);
    devox_forward_kernel<<<g, kPvBlock, 0, st>>>(coords, feat, static_cast<int>(C), static_cast<int>(N),
                                                 static_cast<int>(r), write_iw, outs, inds, wgts);
    O3DML_LAUNCH_CHECK();
    O3DML_GUARD_END
}

O3DML_API size_t o3dml_trilinear_devoxelize_backward_workspace_size(int64_t B, int64_t N, int64_t r) {
    return plan_bytes(B * 8 * N, B * r * r * r);
}

// The per-voxel entry lists of inds [B,8,N], built once and reused by every
// backward that shares inds (plan_ws: *_backward_workspace_size bytes).
O3DML_API int o3dml_trilinear_devoxelize_backward_plan(const int32_t* inds, int64_t B, int64_t N, int64_t r,
                                                       void* plan_ws, size_t ws_bytes_, void* stream) {
    O3DML_GUARD_BEGIN
    const int64_t r3 = checked_r3("trilinear_devoxelize_backward", B, 8 * N, r);
    if (B == 0) return 0;
    hipStream_t st = as_stream(stream);
    const int64_t total = B * 8 * N;
    Workspace ws(plan_ws, ws_bytes_);
    uint32_t* keys = ws.take<uint32_t>(total);
    if (total > 0) {
        devox_keys_kernel<<<stream_grid(total, 256), 256, 0, st>>>(inds, B, 8 * N, r3, keys);
        O3DML_LAUNCH_CHECK();
    }
    check_plan(prim::build_inverse(keys, total, B * r3, ws, st), plan_ws, total);
    O3DML_GUARD_END
}

// grad_out [B,C,N], wgts [B,8,N], plan -> grad_feat [B,C,r3], fully written
O3DML_API int o3dml_trilinear_devoxelize_backward_planned(const float* grad_out, const float* wgts,
                                                          const void* plan_ws, int64_t B, int64_t C, int64_t N,
                                                          int64_t r, float* grad_feat, void* stream) {
    O3DML_GUARD_BEGIN
    const int64_t r3 = checked_r3("trilinear_devoxelize_backward", B, 8 * N, r);
    if (B == 0 || C <= 0) return 0;
    const PlanView pv = plan_view(plan_ws, B * 8 * N);
    const dim3 g = pv_grid("trilinear_devoxelize_backward", r3, C, kPvAcc, B);
    devox_backward_kernel<<<g, kPvBlock, 0, as_stream(stream)>>>(grad_out, wgts, pv.pairs, pv.off,
                                                                static_cast<int>(C), N, r3, grad_feat);
    O3DML_LAUNCH_CHECK();
    O3DML_GUARD_END
}

O3DML_API int o3dml_trilinear_devoxelize_backward(const float* grad_out, const int32_t* inds, const float* wgts,
                                                  int64_t B, int64_t C, int64_t N, int64_t r, float* grad_feat,
                                                  void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = o3dml_trilinear_devoxelize_backward_plan(inds, B, N, r, workspace, workspace_bytes, stream);
    if (rc != 0) return rc;
    return o3dml_trilinear_devoxelize_backward_planned(grad_out, wgts, workspace, B, C, N, r, grad_feat, stream);
}

O3DML_API size_t o3dml_avg_voxelize_plan_workspace_size(int64_t B, int64_t N, int64_t r) {
    return plan_bytes(B * N, B * r * r * r);
}

// vox int32 [B,3,N] -> cnt int32 [B,r3] and the voxel plan (the points of
// every voxel in ascending index), reused by every forward of this (vox, r)
O3DML_API int o3dml_avg_voxelize_plan(const int32_t* vox, int64_t B, int64_t N, int64_t r, int32_t* cnt,
                                      void* plan_ws, size_t ws_bytes_, void* stream) {
    O3DML_GUARD_BEGIN
    const int64_t r3 = checked_r3("avg_voxelize_plan", B, N, r);
    O3DML_REQUIRE(N < (int64_t(1) << 31), "avg_voxelize_plan: N too large");
    if (B == 0) return 0;
    hipStream_t st = as_stream(stream);
    const int64_t total = B * N;
    Workspace ws(plan_ws, ws_bytes_);
    uint32_t* keys = ws.take<uint32_t>(total);
    if (total > 0) {
        vox_keys_kernel<<<stream_grid(total, 256), 256, 0, st>>>(vox, B, N, static_cast<int>(r), r3, keys);
        O3DML_LAUNCH_CHECK();
    }
    const prim::Inverse inv = prim::build_inverse(keys, total, B * r3, ws, st);
    check_plan(inv, plan_ws, total);
    vox_count_kernel<<<stream_grid(B * r3, 256), 256, 0, st>>>(inv.off, B * r3, cnt);
    O3DML_LAUNCH_CHECK();
    O3DML_GUARD_END
}

// feat [B,C,N], plan -> grid [B,C,r3], fully written (cnt is the plan's; the
// kernel reads the list lengths, which are the same numbers)
O3DML_API int o3dml_avg_voxelize_forward(const float* feat, const void* plan_ws, const int32_t* cnt, int64_t B,
                                         int64_t C, int64_t N, int64_t r, float* grid, void* stream) {
    O3DML_GUARD_BEGIN
    (void)cnt;
    const int64_t r3 = checked_r3("avg_voxelize_forward", B, N, r);
    if (B == 0 || C <= 0) return 0;
    const PlanView pv = plan_view(plan_ws, B * N);
    const dim3 g = pv_grid("avg_voxelize_forward", r3, C, kPvAcc, B);
    vox_forward_kernel<<<g, kPvBlock, 0, as_stream(stream)>>>(feat, pv.pairs, pv.off, static_cast<int>(C), N, r3,
                                                             grid);
    O3DML_LAUNCH_CHECK();
    O3DML_GUARD_END
}

// grad_grid [B,C,r3] -> grad_feat [B,C,N] (a gather)
O3DML_API int o3dml_avg_voxelize_backward(const float* grad_grid, const int32_t* vox, const int32_t* cnt, int64_t B,
                                          int64_t C, int64_t N, int64_t r, float* grad_feat, void* stream) {
    O3DML_GUARD_BEGIN
    const int64_t r3 = checked_r3("avg_voxelize_backward", B, N, r);
    if (B == 0 || C <= 0 || N == 0) return 0;
    const dim3 g = pv_grid("avg_voxelize_backward", N, C, kPvChan, B);
    vox_backward_kernel<<<g, kPvBlock, 0, as_stream(stream)>>>(grad_grid, vox, cnt, static_cast<int>(C), N,
                                                              static_cast<int>(r), r3, grad_feat);
    O3DML_LAUNCH_CHECK();
    O3DML_GUARD_END
}
