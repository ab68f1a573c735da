// fps_pruned.hip — exact bucket-pruned farthest-point sampling for large
// clouds (ml3d/torch/utils/pointnet/pointnet2_utils.py:55, 89-99).
//
// The same greedy as pointnet2.hip (from index 0, squared L2 by dist_l2,
// min-distances from 1e10, ties -> smallest original index), bit for bit, but
// a round touches only the spatial buckets whose points can still change:
//
//   set-up   per-cloud box -> 30-bit Morton key under the cloud id -> one
//            radix sort of the batch -> gather into 16-byte records
//            {x, y, z, md} + int32 original index, cut into buckets of S
//            points (S a multiple of 64, at most kMaxBuckets per cloud);
//   kernel   one 1024-lane workgroup per cloud.  Each lane owns kPer buckets:
//            their boxes in registers, (mx, index, coordinates of the point
//            holding mx) in an LDS table.  In a round with new sample s a
//            bucket is skipped when lb = dist_l2(clamp(s, box), s) >= mx:
//            |c - s| <= |p - s| per axis for every p of the box, and fp32
//            subtraction, squaring and the two fmaf of dist_l2 are monotone,
//            so lb <= dist_l2(p, s) in fp32 and no md of the bucket changes.
//            Written as !(lb >= mx), a NaN bound visits the bucket.  Visited
//            buckets go to an LDS list; wave w walks entries w, w + 16, ...
//            with 16-byte loads and recomputes the table entry exactly.  The
//            round's winner is the argmax over the table (original indices
//            compared on ties) and its coordinates come from the table: no
//            global read sits between two rounds but the visited records.
//
// Three barriers per round: list complete -> table complete -> wave partials
// complete.  No workgroup waits on another, no global atomics in the loop.
#include "common.hpp"
#include "primitives.hpp"

namespace o3dml {
namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
// 2048 buckets: 2 per lane (12 box registers), a 40 KB table + 8 KB list in
// LDS (static, below 64 KB); S stays 64 up to 131,072 points per cloud.
constexpr int kMaxBuckets = 2048;
constexpr int kPer = kMaxBuckets / kThreads;
constexpr int kUnroll = 4;  // buckets a wave has in flight in step (b)
constexpr int kNoIndex = 0x7fffffff;
constexpr int kMortonBits = 30;
constexpr float kInf = __builtin_huge_valf();

inline int bucket_size(int64_t max_n) {
    const int64_t q = ceil_div(max_n, int64_t(64) * kMaxBuckets);
    return static_cast<int>(64 * (q < 1 ? 1 : q));
}

// First record slot of cloud b (rows from r0): every cloud starts on a bucket
// boundary and has room for its tail bucket's padding, in closed form.
__host__ __device__ inline int64_t cloud_slot(int64_t r0, int64_t b, int S) { return (r0 / S + b) * S; }

__device__ __forceinline__ void merge(float& v, int& i, float v2, int i2) {
    if (v2 > v || (v2 == v && i2 < i)) {
        v = v2;
        i = i2;
    }
}

__device__ __forceinline__ void wave_argmax(float& v, int& i) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float v2 = __shfl_xor(v, off, 64);
        const int i2 = __shfl_xor(i, off, 64);
        merge(v, i, v2, i2);
    }
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fminf(v, __shfl_xor(v, off, 64));
    return v;
}

__device__ __forceinline__ float wave_maxf(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

// box[b] = {lo x y z, 1024 / extent x y z} over the cloud's finite
// coordinates (0 where the extent is 0, infinite or there is none).
__global__ void __launch_bounds__(kThreads) fpsp_box_kernel(const float* __restrict__ xyz,
                                                            const int64_t* __restrict__ row_splits,
                                                            float* __restrict__ box,
                                                            unsigned long long* __restrict__ visited) {
    __shared__ float red[6][kWaves];
    const int b = blockIdx.x, t = threadIdx.x;
    if (b == 0 && t == 0 && visited) *visited = 0ull;
    const int64_t r0 = row_splits[b], r1 = row_splits[b + 1];
    float lo[3] = {kInf, kInf, kInf}, hi[3] = {-kInf, -kInf, -kInf};
    for (int64_t k = r0 + t; k < r1; k += kThreads) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const float v = xyz[3 * k + d];
            if (fabsf(v) < kInf) {  // false for NaN
                lo[d] = fminf(lo[d], v);
                hi[d] = fmaxf(hi[d], v);
            }
        }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        lo[d] = wave_min(lo[d]);
        hi[d] = wave_maxf(hi[d]);
        if (lane_id() == 0) {
            red[d][wave_id()] = lo[d];
            red[3 + d][wave_id()] = hi[d];
        }
    }
    __syncthreads();
    if (t < 3) {
        float l = kInf, h = -kInf;
        for (int w = 0; w < kWaves; ++w) {
            l = fminf(l, red[t][w]);
            h = fmaxf(h, red[3 + t][w]);
        }
        const float ext = h - l;
        box[6 * b + t] = l < kInf ? l : 0.f;
        box[6 * b + 3 + t] = (ext > 0.f && ext < kInf) ? 1024.f / ext : 0.f;
    }
}

__device__ __forceinline__ uint32_t spread10(uint32_t v) {  // bit i -> bit 3 i
    v = (v | (v << 16)) & 0x030000ffu;
    v = (v | (v << 8)) & 0x0300f00fu;
    v = (v | (v << 4)) & 0x030c30c3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

// key = cloud id above a 30-bit Morton code, 10 bits per axis inside the
// cloud's box.  The key only orders the points: any value is a correct one,
// so non-finite coordinates are clamped like the rest (NaN -> cell 0).
__global__ void fpsp_keys_kernel(const float* __restrict__ xyz, const int64_t* __restrict__ row_splits, int B,
                                 int64_t n, const float* __restrict__ box, uint64_t* __restrict__ keys) {
    for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n;
         i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        int lo = 0, hi = B;  // the cloud with row_splits[b] <= i < row_splits[b + 1]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (row_splits[mid] <= i) lo = mid;
            else hi = mid;
        }
        uint32_t code = 0;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const float q = (xyz[3 * i + d] - box[6 * lo + d]) * box[6 * lo + 3 + d];
            const uint32_t c = !(q >= 0.f) ? 0u : (q >= 1023.f ? 1023u : static_cast<uint32_t>(q));
            code |= spread10(c) << d;
        }
        keys[i] = (static_cast<uint64_t>(lo) << kMortonBits) | code;
    }
}

// Sorted position i of cloud b (the clouds keep their row ranges: the cloud id
// is the key's top) -> record slot; orig holds the index inside the cloud.
__global__ void fpsp_gather_kernel(const float* __restrict__ xyz, const int64_t* __restrict__ row_splits, int64_t n,
                                   const uint64_t* __restrict__ skeys, const uint32_t* __restrict__ srows, int S,
                                   float4* __restrict__ recs, int32_t* __restrict__ orig) {
    for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n;
         i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int64_t b = static_cast<int64_t>(skeys[i] >> kMortonBits);
        const int64_t r0 = row_splits[b], row = srows[i];
        const int64_t slot = cloud_slot(r0, b, S) + (i - r0);
        recs[slot] = make_float4(xyz[3 * row], xyz[3 * row + 1], xyz[3 * row + 2], 1e10f);
        orig[slot] = static_cast<int32_t>(row - r0);
    }
}

__global__ void __launch_bounds__(kThreads)
fps_pruned_kernel(const float* __restrict__ xyz, const int64_t* __restrict__ row_splits,
                  const int64_t* __restrict__ new_row_splits, float4* __restrict__ recs, int32_t* __restrict__ orig,
                  float* __restrict__ boxes, int S, int32_t* __restrict__ out,
                  unsigned long long* __restrict__ visited) {
    // the bucket table: max of the bucket's min-distances, the original index
    // holding it (smallest on ties) and that point's coordinates
    __shared__ float t_mx[kMaxBuckets];
    __shared__ int t_idx[kMaxBuckets];
    __shared__ float t_x[kMaxBuckets], t_y[kMaxBuckets], t_z[kMaxBuckets];
    __shared__ int s_list[kMaxBuckets];
    __shared__ float sv[kWaves];
    __shared__ int si[kWaves], sg[kWaves];
    __shared__ int s_cnt;

    const int b = blockIdx.x, t = threadIdx.x, w = wave_id(), lane = lane_id();
    const int64_t r0 = row_splits[b], o0 = new_row_splits[b];
    const int n = static_cast<int>(row_splits[b + 1] - r0), m = static_cast<int>(new_row_splits[b + 1] - o0);
    if (n <= 0 || m <= 0) return;
    int32_t* __restrict__ o = out + o0;
    const int add = static_cast<int>(r0);
    if (t == 0) o[0] = add;
    if (m == 1) return;

    const int nb = (n + S - 1) / S;
    if (nb > kMaxBuckets) return;  // a cloud larger than the max_n the caller gave
    const int64_t base = cloud_slot(r0, b, S);
    float4* __restrict__ rec = recs + base;
    int32_t* __restrict__ oi = orig + base;
    float* __restrict__ bx = boxes + (base / S) * 6;

    // the tail bucket's padding: md = -1 never wins and never changes
    for (int k = n + t; k < nb * S; k += kThreads) {
        rec[k] = make_float4(0.f, 0.f, 0.f, -1.f);
        oi[k] = kNoIndex;
    }
    if (t == 0) s_cnt = 0;
    __syncthreads();

    // prologue: each bucket's box and its table entry (all md are 1e10: the
    // entry is the bucket's smallest original index)
    for (int g = w; g < nb; g += kWaves) {
        float lo[3] = {kInf, kInf, kInf}, hi[3] = {-kInf, -kInf, -kInf};
        float best = -2.f, px = 0.f, py = 0.f, pz = 0.f;
        int besti = kNoIndex;
        for (int k = g * S + lane; k < (g + 1) * S; k += 64) {
            const float4 r = rec[k];
            const int i = oi[k];
            if (r.w >= 0.f) {  // fminf / fmaxf drop a NaN coordinate: such a point never changes
                lo[0] = fminf(lo[0], r.x), hi[0] = fmaxf(hi[0], r.x);
                lo[1] = fminf(lo[1], r.y), hi[1] = fmaxf(hi[1], r.y);
                lo[2] = fminf(lo[2], r.z), hi[2] = fmaxf(hi[2], r.z);
            }
            if (r.w > best || (r.w == best && i < besti)) best = r.w, besti = i, px = r.x, py = r.y, pz = r.z;
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            lo[d] = wave_min(lo[d]);
            hi[d] = wave_maxf(hi[d]);
        }
        float v = best;
        int i = besti;
        wave_argmax(v, i);
        if (besti == i) t_mx[g] = v, t_idx[g] = i, t_x[g] = px, t_y[g] = py, t_z[g] = pz;
        if (lane < 3) bx[6 * g + lane] = lane == 0 ? lo[0] : (lane == 1 ? lo[1] : lo[2]);
        else if (lane < 6) bx[6 * g + lane] = lane == 3 ? hi[0] : (lane == 4 ? hi[1] : hi[2]);
    }
    __syncthreads();

    float blo[kPer][3], bhi[kPer][3], cmx[kPer];
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
        const int k = t + r * kThreads;
        const bool ok = k < nb;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            blo[r][d] = ok ? bx[6 * k + d] : 0.f;
            bhi[r][d] = ok ? bx[6 * k + 3 + d] : 0.f;
        }
        cmx[r] = ok ? t_mx[k] : -1.f;
    }

    float sx = xyz[3 * r0], sy = xyz[3 * r0 + 1], sz = xyz[3 * r0 + 2];
    unsigned long long vis = 0;
    for (int j = 1; j < m; ++j) {
        // (a) which of this lane's buckets can change: dist_l2 with the
        // update's argument order (point, sample), the point being the sample
        // clamped into the box
        bool dirty[kPer];
        uint64_t mask[kPer];
        int tot = 0;
#pragma unroll
        for (int r = 0; r < kPer; ++r) {
            const float cx = fminf(fmaxf(sx, blo[r][0]), bhi[r][0]);
            const float cy = fminf(fmaxf(sy, blo[r][1]), bhi[r][1]);
            const float cz = fminf(fmaxf(sz, blo[r][2]), bhi[r][2]);
            const float lb = dist_l2(cx, cy, cz, sx, sy, sz);
            dirty[r] = t + r * kThreads < nb && !(lb >= cmx[r]);
            mask[r] = __ballot(dirty[r]);
            tot += __popcll(mask[r]);
        }
        if (tot) {
            int at = 0;
            if (lane == 0) at = atomicAdd(&s_cnt, tot);
            at = __shfl(at, 0, 64);
#pragma unroll
            for (int r = 0; r < kPer; ++r) {
                if (dirty[r]) s_list[at + __popcll(mask[r] & lanemask_lt())] = t + r * kThreads;
                at += __popcll(mask[r]);
            }
        }
        __syncthreads();
        const int cnt = s_cnt;
        if (t == 0) vis += static_cast<unsigned long long>(cnt);

        // (b) the listed buckets: update md, recompute the table entry
        for (int e = w; e < cnt; e += kWaves * kUnroll) {
            int g[kUnroll], besti[kUnroll];
            float best[kUnroll], px[kUnroll], py[kUnroll], pz[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const int ee = e + u * kWaves;
                g[u] = ee < cnt ? s_list[ee] : -1;
                best[u] = -2.f, besti[u] = kNoIndex, px[u] = py[u] = pz[u] = 0.f;
            }
            for (int p = lane; p < S; p += 64) {
                float4 r[kUnroll];
                int i[kUnroll];
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) {
                    if (g[u] >= 0) {
                        r[u] = rec[g[u] * S + p];
                        i[u] = oi[g[u] * S + p];
                    }
                }
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) {
                    if (g[u] >= 0) {
                        const float d = dist_l2(r[u].x, r[u].y, r[u].z, sx, sy, sz);
                        float md = r[u].w;
                        if (d < md) {
                            md = d;
                            reinterpret_cast<float*>(rec + (g[u] * S + p))[3] = d;
                        }
                        if (md > best[u] || (md == best[u] && i[u] < besti[u]))
                            best[u] = md, besti[u] = i[u], px[u] = r[u].x, py[u] = r[u].y, pz[u] = r[u].z;
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                if (g[u] >= 0) {
                    float v = best[u];
                    int i = besti[u];
                    wave_argmax(v, i);
                    if (besti[u] == i)
                        t_mx[g[u]] = v, t_idx[g[u]] = i, t_x[g[u]] = px[u], t_y[g[u]] = py[u], t_z[g[u]] = pz[u];
                }
            }
        }
        __syncthreads();
        if (t == 0) s_cnt = 0;

        // (c) argmax over the table; the bucket rides along for the coordinates
        float v = -2.f;
        int i = kNoIndex, gw = 0;
#pragma unroll
        for (int r = 0; r < kPer; ++r) {
            const int k = t + r * kThreads;
            if (k < nb) {
                cmx[r] = t_mx[k];
                const int i2 = t_idx[k];
                if (cmx[r] > v || (cmx[r] == v && i2 < i)) v = cmx[r], i = i2, gw = k;
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float v2 = __shfl_xor(v, off, 64);
            const int i2 = __shfl_xor(i, off, 64);
            const int g2 = __shfl_xor(gw, off, 64);
            if (v2 > v || (v2 == v && i2 < i)) v = v2, i = i2, gw = g2;
        }
        if (lane == 0) sv[w] = v, si[w] = i, sg[w] = gw;
        __syncthreads();
        v = lane < kWaves ? sv[lane] : -2.f;
        i = lane < kWaves ? si[lane] : kNoIndex;
        gw = lane < kWaves ? sg[lane] : 0;
#pragma unroll
        for (int off = kWaves / 2; off >= 1; off >>= 1) {
            const float v2 = __shfl_xor(v, off, 64);
            const int i2 = __shfl_xor(i, off, 64);
            const int g2 = __shfl_xor(gw, off, 64);
            if (v2 > v || (v2 == v && i2 < i)) v = v2, i = i2, gw = g2;
        }
        i = __shfl(i, 0, 64);
        gw = __shfl(gw, 0, 64);
        sx = t_x[gw], sy = t_y[gw], sz = t_z[gw];
        if (t == 0) o[j] = i + add;
    }
    if (t == 0 && visited) atomicAdd(visited, vis);
}

}  // namespace
}  // namespace o3dml

using namespace o3dml;

O3DML_API size_t o3dml_fps_pruned_workspace_size(int64_t n, int64_t B, int64_t max_n) {
    const int S = bucket_size(max_n);
    const int64_t slots = cloud_slot(n, B, S);
    return ws_bytes<float>(6 * B) + 2 * ws_bytes<uint64_t>(n) + ws_bytes<uint32_t>(n) +
           prim::radix_sort_workspace_bytes<uint64_t>(n) + ws_bytes<float4>(slots) + ws_bytes<int32_t>(slots) +
           ws_bytes<float>(6 * (slots / S));
}

// xyz f32 [n,3], device row_splits / new_row_splits int64 [B+1] -> out int32
// [m_total] (global rows); visited: nullable device u64, buckets passed in (b)
O3DML_API int o3dml_fps_pruned(const float* xyz, int64_t n, int64_t B, const int64_t* row_splits,
                               const int64_t* new_row_splits, int64_t max_n, int64_t m_total, int32_t* out,
                               uint64_t* visited, void* workspace, size_t workspace_bytes, void* stream) {
    O3DML_GUARD_BEGIN
    O3DML_REQUIRE(max_n > 0 || m_total == 0, "fps_pruned: empty cloud");
    const int S = bucket_size(max_n);
    const int64_t slots = cloud_slot(n, B, S);
    O3DML_REQUIRE(n >= 0 && B >= 0 && max_n <= n && slots < (int64_t(1) << 31) && m_total < (int64_t(1) << 31) &&
                          B < (int64_t(1) << 31),
                  "fps_pruned: too large");
    hipStream_t st = as_stream(stream);
    auto* vis = reinterpret_cast<unsigned long long*>(visited);
    if (B == 0 || m_total == 0) {
        if (vis) fill_async(vis, 0, sizeof(*vis), st);
        return 0;
    }
    TimedRegion tr("fps_ragged", st);
    TimedRegion setup("fps_pruned_setup", st);
    Workspace ws(workspace, workspace_bytes);
    float* box = ws.take<float>(6 * B);
    uint64_t* keys = ws.take<uint64_t>(n);
    uint64_t* skeys = ws.take<uint64_t>(n);
    uint32_t* srows = ws.take<uint32_t>(n);
    float4* recs = ws.take<float4>(slots);
    int32_t* orig = ws.take<int32_t>(slots);
    float* boxes = ws.take<float>(6 * (slots / S));
    const unsigned g = static_cast<unsigned>(B);
    fpsp_box_kernel<<<g, kThreads, 0, st>>>(xyz, row_splits, box, vis);
    O3DML_LAUNCH_CHECK();
    fpsp_keys_kernel<<<stream_grid(n, 256), 256, 0, st>>>(xyz, row_splits, static_cast<int>(B), n, box, keys);
    O3DML_LAUNCH_CHECK();
    prim::radix_sort_pairs<uint64_t>(keys, nullptr, skeys, srows, n,
                                     kMortonBits + prim::bits_needed(static_cast<uint64_t>(B - 1)), ws, st);
    fpsp_gather_kernel<<<stream_grid(n, 256), 256, 0, st>>>(xyz, row_splits, n, skeys, srows, S, recs, orig);
    O3DML_LAUNCH_CHECK();
    setup.end();
    fps_pruned_kernel<<<g, kThreads, 0, st>>>(xyz, row_splits, new_row_splits, recs, orig, boxes, S, out, vis);
    O3DML_LAUNCH_CHECK();
    O3DML_GUARD_END
}
