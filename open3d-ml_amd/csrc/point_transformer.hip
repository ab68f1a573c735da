// point_transformer.hip — the gather ops of PointTransformer's eval() forward
// (ml3d/torch/models/point_transformer.py): the relation tensor and the
// softmax aggregation of a Transformer layer (:427-467), the inverse-distance
// kNN interpolation of TransitionUp (:737-776) and the grouped rows of
// TransitionDown (:521-532, queryandgroup :650-697).
//
// Layouts (contiguous float32 unless noted): xyz [*,3], feature rows [*,c]
// row-major, idx int32 [n, nsample] of source rows (a Neighbours plan of
// o3dml_amd/point_transformer.py: every entry in [0, n_src), checked there).
// Mapping: lanes run along the channels, one lane per (query, 4 channels)
// with 16-byte loads and stores when c is a multiple of 4 and the rows are
// 16-byte aligned, else one channel per lane; a lane walks its query's
// neighbours in index order, so what depends on the query and the channels
// only (q, the second positional Linear, the BatchNorm affine, the softmax
// maxima) stays in registers across the nsample gathers.
// The positional encoding p_r = W2 relu(bn_p(W1 d + b1)) + b2 of a pair is
// three numbers and a 3 -> c map: every lane recomputes it (pos_hidden,
// pos_channel, shared by relation and aggregate so both see the same bits)
// and it is never stored.  BatchNorms arrive folded to scale / shift.
// Order of sums: over the neighbours in index order, in one lane; products
// are rounded before they are added except where fmaf is spelled out.  No
// atomics: run-to-run bitwise equal.
#include "point_transformer.hpp"

namespace o3dml {

// R[i,j,:] = relu(sw * ((k[idx[i,j],:] - q[i,:]) + p_r(i,j)) + tw)
template <int VEC>
__global__ void __launch_bounds__(kPtBlock)
pt_relation_kernel(PtPos pos, const float* __restrict__ xyz_q, const float* __restrict__ xyz_s,
                   const int32_t* __restrict__ idx, const float* __restrict__ fk, const float* __restrict__ fq,
                   const float* __restrict__ sw, const float* __restrict__ tw, int64_t n, int ns, int c,
                   float* __restrict__ out) {
    const int lpr = c / VEC;
    const int64_t t = blockIdx.x * static_cast<int64_t>(kPtBlock) + threadIdx.x;
    if (t >= n * lpr) return;
    const int64_t i = t / lpr;
    const int ch = static_cast<int>(t % lpr) * VEC;
    PtLane<VEC> lane;
    lane.init(pos, xyz_q, i, ch);
    float q[VEC], s_[VEC], t_[VEC];
    load_vec<VEC>(fq + i * c + ch, q);
    load_vec<VEC>(sw + ch, s_);
    load_vec<VEC>(tw + ch, t_);
    const int32_t* ii = idx + i * ns;
    float* o = out + i * ns * c + ch;
#pragma unroll 4
    for (int j = 0; j < ns; ++j) {
        const int64_t s = ii[j];
        float kv[VEC], p[VEC], r[VEC];
        load_vec<VEC>(fk + s * c + ch, kv);
        lane.encode(xyz_s, s, p);
#pragma unroll
        for (int e = 0; e < VEC; ++e) r[e] = fmaxf(s_[e] * ((kv[e] - q[e]) + p[e]) + t_[e], 0.f);
        store_vec<VEC>(o + static_cast<int64_t>(j) * c, r);
    }
}

// out[i,ch] = sum_j softmax_j(w[i,:,ch % cs])_j * (v[idx[i,j],ch] + p_r(i,j)[ch]),
// the softmax with the maximum over j subtracted, the quotient taken last
template <int VEC>
__global__ void __launch_bounds__(kPtBlock)
pt_aggregate_kernel(PtPos pos, const float* __restrict__ xyz_q, const float* __restrict__ xyz_s,
                    const int32_t* __restrict__ idx, const float* __restrict__ fv, const float* __restrict__ w,
                    int64_t n, int ns, int c, int cs, float* __restrict__ out) {
    const int lpr = c / VEC;
    const int64_t t = blockIdx.x * static_cast<int64_t>(kPtBlock) + threadIdx.x;
    if (t >= n * lpr) return;
    const int64_t i = t / lpr;
    const int ch = static_cast<int>(t % lpr) * VEC;
    PtLane<VEC> lane;
    lane.init(pos, xyz_q, i, ch);
    const int32_t* ii = idx + i * ns;
    const float* wi = w + i * ns * cs;
    int wc[VEC];
    float mx[VEC], den[VEC], acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        wc[e] = (ch + e) % cs;
        mx[e] = wi[wc[e]];
        den[e] = 0.f;
        acc[e] = 0.f;
    }
    for (int j = 1; j < ns; ++j) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) mx[e] = fmaxf(mx[e], wi[static_cast<int64_t>(j) * cs + wc[e]]);
    }
#pragma unroll 4
    for (int j = 0; j < ns; ++j) {
        const int64_t s = ii[j];
        float v[VEC], p[VEC];
        load_vec<VEC>(fv + s * c + ch, v);
        lane.encode(xyz_s, s, p);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const float ex = expf(wi[static_cast<int64_t>(j) * cs + wc[e]] - mx[e]);
            den[e] += ex;
            acc[e] += ex * (v[e] + p[e]);
        }
    }
    float r[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) r[e] = acc[e] / den[e];
    store_vec<VEC>(out + i * c + ch, r);
}

constexpr int kPtMaxInterp = 8;

// out[i,:] = sum_t (r_t / sum_t r_t) * feat[idx[i,t],:], r_t = 1 / (d_t + 1e-8)
template <int VEC>
__global__ void __launch_bounds__(kPtBlock)
pt_interpolate_kernel(const float* __restrict__ feat, const int32_t* __restrict__ idx, const float* __restrict__ dist,
                      int64_t n, int k, int c, float* __restrict__ out) {
    const int lpr = c / VEC;
    const int64_t t = blockIdx.x * static_cast<int64_t>(kPtBlock) + threadIdx.x;
    if (t >= n * lpr) return;
    const int64_t i = t / lpr;
    const int ch = static_cast<int>(t % lpr) * VEC;
    float r[kPtMaxInterp];
    float norm = 0.f;
#pragma unroll
    for (int u = 0; u < kPtMaxInterp; ++u) {
        r[u] = 0.f;
        if (u < k) {
            r[u] = 1.0f / (dist[i * k + u] + 1e-8f);
            norm += r[u];
        }
    }
    float acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
#pragma unroll
    for (int u = 0; u < kPtMaxInterp; ++u) {
        if (u < k) {
            const float wgt = r[u] / norm;
            float f[VEC];
            load_vec<VEC>(feat + static_cast<int64_t>(idx[i * k + u]) * c + ch, f);
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[e] += f[e] * wgt;
        }
    }
    store_vec<VEC>(out + i * c + ch, acc);
}

// out[i,j,:] = [xyz_s[idx[i,j]] - xyz_q[i] | feat[idx[i,j],:]]: rows of 3 + c
// floats are not 16-byte aligned, so one element per lane, stores coalesced
__global__ void __launch_bounds__(kPtBlock)
pt_group_kernel(const float* __restrict__ xyz_q, const float* __restrict__ xyz_s, const int32_t* __restrict__ idx,
                const float* __restrict__ feat, int64_t rows, int ns, int c, float* __restrict__ out) {
    const int wdt = c + 3;
    const int64_t total = rows * wdt;
    for (int64_t e = blockIdx.x * static_cast<int64_t>(kPtBlock) + threadIdx.x; e < total;
         e += static_cast<int64_t>(gridDim.x) * kPtBlock) {
        const int64_t row = e / wdt;
        const int col = static_cast<int>(e % wdt);
        const int64_t s = idx[row];
        out[e] = col < 3 ? xyz_s[3 * s + col] - xyz_q[3 * (row / ns) + col] : feat[s * c + (col - 3)];
    }
}

}  // namespace o3dml

using namespace o3dml;

O3DML_API int o3dml_pt_relation(const float* xyz_q, const float* xyz_src, const int32_t* idx, const float* feat_k,
                                const float* feat_q, const float* w1, const float* b1, const float* scale_p,
                                const float* shift_p, const float* w2, const float* b2, const float* scale_w,
                                const float* shift_w, int64_t n, int64_t nsample, int64_t c, float* out,
                                void* stream) {
    O3DML_GUARD_BEGIN
    pt_check_layer("pt_relation", n, nsample, c);
    if (n == 0) return 0;
    hipStream_t st = as_stream(stream);
    TimedRegion tr("pt_relation", st);
    const PtPos pos{w1, b1, scale_p, shift_p, w2, b2};
    const int ns = static_cast<int>(nsample), ci = static_cast<int>(c);
    if (c % 4 == 0 && aligned16({feat_k, feat_q, scale_w, shift_w, out}))
        pt_relation_kernel<4><<<pt_grid(n * (c / 4)), kPtBlock, 0, st>>>(pos, xyz_q, xyz_src, idx, feat_k, feat_q,
                                                                          scale_w, shift_w, n, ns, ci, out);
    else
        pt_relation_kernel<1><<<pt_grid(n * c), kPtBlock, 0, st>>>(pos, xyz_q, xyz_src, idx, feat_k, feat_q, scale_w,
                                                                    shift_w, n, ns, ci, out);
    O3DML_LAUNCH_CHECK();
    O3DML_GUARD_END
}

O3DML_API int o3dml_pt_aggregate(const float* xyz_q, const float* xyz_src, const int32_t* idx, const float* feat_v,
                                 const float* weight, const float* w1, const float* b1, const float* scale_p,
                                 const float* shift_p, const float* w2, const float* b2, int64_t n, int64_t nsample,
                                 int64_t c, int64_t share_planes, float* out, void* stream) {
    O3DML_GUARD_BEGIN
    pt_check_layer("pt_aggregate", n, nsample, c);
    O3DML_REQUIRE(share_planes >= 1 && c % share_planes == 0,
                  "pt_aggregate: c = %lld is not a multiple of share_planes = %lld", (long long)c,
                  (long long)share_planes);
    if (n == 0) return 0;
    hipStream_t st = as_stream(stream);
    TimedRegion tr("pt_aggregate", st);
    const PtPos pos{w1, b1, scale_p, shift_p, w2, b2};
    const int ns = static_cast<int>(nsample), ci = static_cast<int>(c), cs = static_cast<int>(c / share_planes);
    if (c % 4 == 0 && aligned16({feat_v, out}))
        pt_aggregate_kernel<4><<<pt_grid(n * (c / 4)), kPtBlock, 0, st>>>(pos, xyz_q, xyz_src, idx, feat_v, weight, n,
                                                                           ns, ci, cs, out);
    else
        pt_aggregate_kernel<1><<<pt_grid(n * c), kPtBlock, 0, st>>>(pos, xyz_q, xyz_src, idx, feat_v, weight, n, ns,
                                                                     ci, cs, out);
    O3DML_LAUNCH_CHECK();
    O3DML_GUARD_END
}

O3DML_API int o3dml_pt_knn_interpolate(const float* feat, const int32_t* idx, const float* dist, int64_t n, int64_t k,
                                       int64_t c, float* out, void* stream) {
    O3DML_GUARD_BEGIN
    O3DML_REQUIRE(n >= 0 && n < (int64_t(1) << 31), "pt_knn_interpolate: n = %lld out of range", (long long)n);
    O3DML_REQUIRE(k >= 1 && k <= kPtMaxInterp, "pt_knn_interpolate: k must be in 1..%d, got %lld", kPtMaxInterp,
                  (long long)k);
    O3DML_REQUIRE(c >= 1 && c <= 65536, "pt_knn_interpolate: c must be in 1..65536, got %lld", (long long)c);
    if (n == 0) return 0;
    hipStream_t st = as_stream(stream);
    TimedRegion tr("pt_knn_interpolate", st);
    const int ki = static_cast<int>(k), ci = static_cast<int>(c);
    if (c % 4 == 0 && aligned16({feat, out}))
        pt_interpolate_kernel<4><<<pt_grid(n * (c / 4)), kPtBlock, 0, st>>>(feat, idx, dist, n, ki, ci, out);
    else
        pt_interpolate_kernel<1><<<pt_grid(n * c), kPtBlock, 0, st>>>(feat, idx, dist, n, ki, ci, out);
    O3DML_LAUNCH_CHECK();
    O3DML_GUARD_END
}

O3DML_API int o3dml_pt_group(const float* xyz_q, const float* xyz_src, const int32_t* idx, const float* feat,
                             int64_t n, int64_t nsample, int64_t c, float* out, void* stream) {
    O3DML_GUARD_BEGIN
    pt_check_layer("pt_group", n, nsample, c);
    if (n == 0) return 0;
    hipStream_t st = as_stream(stream);
    TimedRegion tr("pt_group", st);
    const int64_t rows = n * nsample;
    pt_group_kernel<<<stream_grid(rows * (c + 3), kPtBlock, 256 * 32), kPtBlock, 0, st>>>(
            xyz_q, xyz_src, idx, feat, rows, static_cast<int>(nsample), static_cast<int>(c), out);
    O3DML_LAUNCH_CHECK();
    O3DML_GUARD_END
}
