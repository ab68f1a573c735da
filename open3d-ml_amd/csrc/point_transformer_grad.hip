// point_transformer_grad.hip — the backward of PointTransformer's four gather
// ops (point_transformer.hip): the inverse of a neighbour list, the gather-sum
// over it that turns every scatter-add of the backward into a fixed-order sum
// per source row, and the backward of `relation` and `aggregate`.
//
// Inverse list: row s holds the flat pair ids t = i * k + j with idx[i,j] == s
// in ascending t (stable LSD radix sort of the index, then one binary search
// per row boundary): the bits of a stable argsort, no host read.
// Gather-sum: one lane per (source row, 4 channels | 1 channel) walks its row
// of the inverse list in order; a row of any length is one serial sum.
// relation / aggregate backward: a workgroup owns R = 256 / L whole queries, L
// = lanes of one query (c / 4 or c; rows wider than 256 lanes are walked in
// chunks of 256 lanes, the chunk loop outermost), so the sums across the
// channels of one pair (dh = W2^T gr, dsm) are reductions inside the
// workgroup: lanes put their terms in LDS, dh goes down a fixed binary tree
// over the lanes of the row, dsm is summed by one lane per softmax column in
// ascending channel.  The lanes recompute the positional encoding with the
// forward's device functions (point_transformer.hpp).  Sums over all pairs
// (d scale_w, d shift_w, d W2, d b2) stay in registers over the workgroup's
// queries (grid-stride), are summed over the R rows in LDS in row order and
// written as one partial per workgroup; a second kernel adds the partials in
// workgroup order.  No atomics anywhere: run-to-run bitwise equal.
#include "point_transformer.hpp"
#include "primitives.hpp"

namespace o3dml {

constexpr int kPtGradBlocks = 1024;  // most workgroups (and partials) of a backward kernel
constexpr int kPtJB = 4;             // neighbours per LDS reduction round

struct PtGradGeom {
    int L, R, P, chunks;
    unsigned grid;
};

inline PtGradGeom pt_grad_geom(int64_t n, int c, int vec) {
    PtGradGeom g;
    const int lpr = c / vec;
    g.L = lpr < kPtBlock ? lpr : kPtBlock;
    g.R = kPtBlock / g.L;
    g.chunks = static_cast<int>(ceil_div(lpr, g.L));
    g.P = 1;
    while (g.P < g.L) g.P <<= 1;
    int64_t groups = ceil_div(n, g.R);
    if (groups > kPtGradBlocks) groups = kPtGradBlocks;
    g.grid = static_cast<unsigned>(groups < 1 ? 1 : groups);
    return g;
}

// red[q][row lanes] -> red[q][r * L]: a binary tree over the L lanes of each
// row (P = L rounded up to a power of two); every thread of the block calls it
template <int NQ>
__device__ __forceinline__ void row_tree_sum(float (&red)[NQ][kPtBlock], int tid, int l, int L, int P, bool row) {
    __syncthreads();
    for (int stride = P >> 1; stride >= 1; stride >>= 1) {
        if (row && l < stride && l + stride < L) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) red[q][tid] += red[q][tid + stride];
        }
        __syncthreads();
    }
}

// sum of v over the R rows of the block for lane l, in row order, returned to
// the threads of row 0 (others get 0); every thread of the block calls it
__device__ __forceinline__ float rows_sum(float* buf, float v, int tid, int r, int l, int L, int R) {
    buf[tid] = v;
    __syncthreads();
    float s = 0.f;
    if (r == 0)
        for (int rr = 0; rr < R; ++rr) s += buf[rr * L + l];
    __syncthreads();
    return s;
}

// gr = g * [out > 0] * sw, dq = -sum_j gr, dh = W2^T gr and the per-workgroup
// partials of d sw = sum gz * r, d tw = sum gz, d W2 = sum gr h^T, d b2 = sum gr
// part: [grid][6][c] = (d sw, d tw, d W2[:,0], d W2[:,1], d W2[:,2], d b2)
template <int VEC>
__global__ void __launch_bounds__(kPtBlock)
pt_relation_bwd_kernel(PtPos pos, const float* __restrict__ xyz_q, const float* __restrict__ xyz_s,
                       const int32_t* __restrict__ idx, const float* __restrict__ fk, const float* __restrict__ fq,
                       const float* __restrict__ sw, const float* __restrict__ tw, const float* __restrict__ out,
                       const float* __restrict__ g, int64_t n, int ns, int c, PtGradGeom gm,
                       float* __restrict__ gr, float* __restrict__ dq, float* dh, float* __restrict__ part) {
    __shared__ float red[3 * kPtJB][kPtBlock];
    const int tid = threadIdx.x, L = gm.L, R = gm.R;
    const int r = tid / L, l = tid % L;
    const int lpr = c / VEC;
    const int64_t groups = ceil_div(n, R);
    const PtPosRegs pr = pos_load(pos);
    for (int chunk = 0; chunk < gm.chunks; ++chunk) {
        const int chl = chunk * L + l;
        const bool chan_ok = r < R && chl < lpr;
        const int ch = chan_ok ? chl * VEC : 0;
        float w2[VEC][3], b2[VEC], s_[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
#pragma unroll
            for (int a = 0; a < 3; ++a) w2[e][a] = pos.w2[3 * (ch + e) + a];
            b2[e] = pos.b2[ch + e];
        }
        load_vec<VEC>(sw + ch, s_);
        float a_sw[VEC], a_tw[VEC], a_w2[VEC][3], a_b2[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            a_sw[e] = a_tw[e] = a_b2[e] = 0.f;
            a_w2[e][0] = a_w2[e][1] = a_w2[e][2] = 0.f;
        }
        for (int64_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
            const int64_t i = grp * R + r;
            const bool ok = chan_ok && i < n;
            const int64_t is = ok ? i : 0;
            const float qx = xyz_q[3 * is], qy = xyz_q[3 * is + 1], qz = xyz_q[3 * is + 2];
            float q[VEC], dqa[VEC];
            load_vec<VEC>(fq + is * c + ch, q);
#pragma unroll
            for (int e = 0; e < VEC; ++e) dqa[e] = 0.f;
            for (int j0 = 0; j0 < ns; j0 += kPtJB) {
#pragma unroll
                for (int jj = 0; jj < kPtJB; ++jj) {
                    const int j = j0 + jj;
                    float pa[3] = {0.f, 0.f, 0.f};
                    if (ok && j < ns) {
                        const int64_t s = idx[is * ns + j];
                        const int64_t o = (is * ns + j) * c + ch;
                        float kv[VEC], ov[VEC], gv[VEC], grv[VEC], h[3];
                        load_vec<VEC>(fk + s * c + ch, kv);
                        load_vec<VEC>(out + o, ov);
                        load_vec<VEC>(g + o, gv);
                        pos_hidden(pr, xyz_s[3 * s] - qx, xyz_s[3 * s + 1] - qy, xyz_s[3 * s + 2] - qz, h);
#pragma unroll
                        for (int e = 0; e < VEC; ++e) {
                            const float rr = (kv[e] - q[e]) + pos_channel(w2[e], b2[e], h);
                            const float gz = ov[e] > 0.f ? gv[e] : 0.f;
                            grv[e] = gz * s_[e];
                            a_sw[e] += gz * rr;
                            a_tw[e] += gz;
                            a_b2[e] += grv[e];
                            dqa[e] += grv[e];
#pragma unroll
                            for (int a = 0; a < 3; ++a) {
                                a_w2[e][a] += grv[e] * h[a];
                                pa[a] += w2[e][a] * grv[e];
                            }
                        }
                        store_vec<VEC>(gr + o, grv);
                    }
#pragma unroll
                    for (int a = 0; a < 3; ++a) red[3 * jj + a][tid] = pa[a];
                }
                row_tree_sum<3 * kPtJB>(red, tid, l, L, gm.P, r < R);
                if (r < R && i < n) {
                    for (int qd = l; qd < 3 * kPtJB; qd += L) {
                        const int j = j0 + qd / 3;
                        if (j < ns) {
                            const int64_t at = (i * ns + j) * 3 + qd % 3;
                            float v = red[qd][r * L];
                            if (chunk > 0) v = dh[at] + v;
                            dh[at] = v;
                        }
                    }
                }
                __syncthreads();
            }
            if (ok) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) dqa[e] = -dqa[e];
                store_vec<VEC>(dq + i * c + ch, dqa);
            }
        }
        float* pb = part + static_cast<int64_t>(blockIdx.x) * 6 * c;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const float v[6] = {a_sw[e], a_tw[e], a_w2[e][0], a_w2[e][1], a_w2[e][2], a_b2[e]};
#pragma unroll
            for (int qd = 0; qd < 6; ++qd) {
                const float sum = rows_sum(red[0], chan_ok ? v[qd] : 0.f, tid, r, l, L, R);
                if (r == 0 && chan_ok) pb[qd * c + ch + e] = sum;
            }
        }
    }
}

// dval = sm * g, dsm[i,j,gch] = sum_{ch = gch mod cs} g[i,ch] * val[i,j,ch]
// (into dw, then dw = sm * (dsm - sum_j sm * dsm) in place), dh = W2^T dval
// and the partials of d W2 and d b2; part: [grid][4][c]
template <int VEC>
__global__ void __launch_bounds__(kPtBlock)
pt_aggregate_bwd_kernel(PtPos pos, const float* __restrict__ xyz_q, const float* __restrict__ xyz_s,
                        const int32_t* __restrict__ idx, const float* __restrict__ fv, const float* __restrict__ w,
                        const float* __restrict__ g, int64_t n, int ns, int c, int cs, PtGradGeom gm,
                        float* __restrict__ dval, float* dw, float* dh, float* __restrict__ part) {
    __shared__ float red[3 * kPtJB][kPtBlock];
    __shared__ float prod[kPtJB][kPtBlock * VEC];
    const int tid = threadIdx.x, L = gm.L, R = gm.R;
    const int r = tid / L, l = tid % L;
    const int lpr = c / VEC;
    const int64_t groups = ceil_div(n, R);
    const PtPosRegs pr = pos_load(pos);
    for (int chunk = 0; chunk < gm.chunks; ++chunk) {
        const int chl = chunk * L + l;
        const bool chan_ok = r < R && chl < lpr;
        const int ch = chan_ok ? chl * VEC : 0;
        const int cbase = chunk * L * VEC;
        const int span = c - cbase < L * VEC ? c - cbase : L * VEC;
        float w2[VEC][3], b2[VEC];
        int wc[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
#pragma unroll
            for (int a = 0; a < 3; ++a) w2[e][a] = pos.w2[3 * (ch + e) + a];
            b2[e] = pos.b2[ch + e];
            wc[e] = (ch + e) % cs;
        }
        float a_w2[VEC][3], a_b2[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            a_b2[e] = 0.f;
            a_w2[e][0] = a_w2[e][1] = a_w2[e][2] = 0.f;
        }
        for (int64_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
            const int64_t i = grp * R + r;
            const bool ok = chan_ok && i < n;
            const int64_t is = ok ? i : 0;
            const float qx = xyz_q[3 * is], qy = xyz_q[3 * is + 1], qz = xyz_q[3 * is + 2];
            const float* wi = w + is * ns * cs;
            float gv[VEC], mx[VEC], den[VEC];
            load_vec<VEC>(g + is * c + ch, gv);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                mx[e] = wi[wc[e]];
                den[e] = 0.f;
            }
            for (int j = 1; j < ns; ++j) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) mx[e] = fmaxf(mx[e], wi[static_cast<int64_t>(j) * cs + wc[e]]);
            }
            for (int j = 0; j < ns; ++j) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) den[e] += expf(wi[static_cast<int64_t>(j) * cs + wc[e]] - mx[e]);
            }
            for (int j0 = 0; j0 < ns; j0 += kPtJB) {
#pragma unroll
                for (int jj = 0; jj < kPtJB; ++jj) {
                    const int j = j0 + jj;
                    float pa[3] = {0.f, 0.f, 0.f};
                    float pv[VEC];
#pragma unroll
                    for (int e = 0; e < VEC; ++e) pv[e] = 0.f;
                    if (ok && j < ns) {
                        const int64_t s = idx[is * ns + j];
                        const int64_t o = (is * ns + j) * c + ch;
                        float v[VEC], dv[VEC], h[3];
                        load_vec<VEC>(fv + s * c + ch, v);
                        pos_hidden(pr, xyz_s[3 * s] - qx, xyz_s[3 * s + 1] - qy, xyz_s[3 * s + 2] - qz, h);
#pragma unroll
                        for (int e = 0; e < VEC; ++e) {
                            const float val = v[e] + pos_channel(w2[e], b2[e], h);
                            const float sm = expf(wi[static_cast<int64_t>(j) * cs + wc[e]] - mx[e]) / den[e];
                            dv[e] = sm * gv[e];
                            pv[e] = gv[e] * val;
                            a_b2[e] += dv[e];
#pragma unroll
                            for (int a = 0; a < 3; ++a) {
                                a_w2[e][a] += dv[e] * h[a];
                                pa[a] += w2[e][a] * dv[e];
                            }
                        }
                        store_vec<VEC>(dval + o, dv);
                    }
#pragma unroll
                    for (int a = 0; a < 3; ++a) red[3 * jj + a][tid] = pa[a];
#pragma unroll
                    for (int e = 0; e < VEC; ++e) prod[jj][tid * VEC + e] = pv[e];
                }
                row_tree_sum<3 * kPtJB>(red, tid, l, L, gm.P, r < R);
                if (r < R && i < n) {
                    for (int qd = l; qd < 3 * kPtJB; qd += L) {
                        const int j = j0 + qd / 3;
                        if (j < ns) {
                            const int64_t at = (i * ns + j) * 3 + qd % 3;
                            float v = red[qd][r * L];
                            if (chunk > 0) v = dh[at] + v;
                            dh[at] = v;
                        }
                    }
                    // softmax column gch: its channels of this chunk, ascending
                    for (int gch = l; gch < cs; gch += L) {
                        const int x0 = ((gch - cbase) % cs + cs) % cs;
                        for (int jj = 0; jj < kPtJB; ++jj) {
                            const int j = j0 + jj;
                            if (j >= ns) break;
                            float sum = 0.f;
                            for (int x = x0; x < span; x += cs) sum += prod[jj][r * L * VEC + x];
                            const int64_t at = (i * ns + j) * cs + gch;
                            if (chunk > 0) sum = dw[at] + sum;
                            dw[at] = sum;
                        }
                    }
                }
                __syncthreads();
            }
        }
        float* pb = part + static_cast<int64_t>(blockIdx.x) * 4 * c;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const float v[4] = {a_w2[e][0], a_w2[e][1], a_w2[e][2], a_b2[e]};
#pragma unroll
            for (int qd = 0; qd < 4; ++qd) {
                const float sum = rows_sum(red[0], chan_ok ? v[qd] : 0.f, tid, r, l, L, R);
                if (r == 0 && chan_ok) pb[qd * c + ch + e] = sum;
            }
        }
    }
    // dw holds dsm, every entry written and read by the same lane:
    // dw[i,j,gch] = sm * (dsm - sum_j sm * dsm)
    for (int64_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const int64_t i = grp * R + r;
        if (r >= R || i >= n) continue;
        const float* wi = w + i * ns * cs;
        float* di = dw + i * ns * cs;
        for (int gch = l; gch < cs; gch += L) {
            float mx = wi[gch];
            for (int j = 1; j < ns; ++j) mx = fmaxf(mx, wi[static_cast<int64_t>(j) * cs + gch]);
            float den = 0.f;
            for (int j = 0; j < ns; ++j) den += expf(wi[static_cast<int64_t>(j) * cs + gch] - mx);
            float dot = 0.f;
            for (int j = 0; j < ns; ++j)
                dot += expf(wi[static_cast<int64_t>(j) * cs + gch] - mx) / den * di[static_cast<int64_t>(j) * cs + gch];
            for (int j = 0; j < ns; ++j) {
                const int64_t at = static_cast<int64_t>(j) * cs + gch;
                di[at] = expf(wi[at] - mx) / den * (di[at] - dot);
            }
        }
    }
}

// out[dst[e / c] + e % c] = sum over the workgroups' partials, in workgroup
// order; part [nblk][nq][c]; quantity q goes to outs[q] with stride strides[q]
struct PtPartOut {
    float* p[6];
    int stride[6];
};

__global__ void __launch_bounds__(kPtBlock)
pt_partials_sum_kernel(const float* __restrict__ part, int nblk, int nq, int c, PtPartOut o) {
    const int64_t total = static_cast<int64_t>(nq) * c;
    const int64_t e = blockIdx.x * static_cast<int64_t>(kPtBlock) + threadIdx.x;
    if (e >= total) return;
    const int qd = static_cast<int>(e / c), ch = static_cast<int>(e % c);
    o.p[qd][static_cast<int64_t>(ch) * o.stride[qd]] = sum_slabs(part, nblk, total, e);
}

// out[s, ch] = sum_{p in row s} wgt(t) * rows[(t / div) * ld + col0 + ch], t =
// pairs[p] ascending; wgt = weight[t], or r_t / sum_u r_u of query t / k from
// the distances (the interpolation's weights, recomputed), or 1
template <int VEC>
__global__ void __launch_bounds__(kPtBlock)
pt_gather_sum_kernel(const float* __restrict__ rows, int64_t ld, int col0, int div, const float* __restrict__ weight,
                     const float* __restrict__ dist, int k, const int64_t* __restrict__ splits,
                     const int32_t* __restrict__ pairs, int64_t n_src, int c, float* __restrict__ out) {
    const int lpr = c / VEC;
    const int64_t th = blockIdx.x * static_cast<int64_t>(kPtBlock) + threadIdx.x;
    if (th >= n_src * lpr) return;
    const int64_t s = th / lpr;
    const int ch = static_cast<int>(th % lpr) * VEC;
    float acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
    const int64_t end = splits[s + 1];
    for (int64_t p = splits[s]; p < end; ++p) {
        const int64_t t = pairs[p];
        float f[VEC];
        load_vec<VEC>(rows + (t / div) * ld + col0 + ch, f);
        if (weight) {
            const float wgt = weight[t];
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[e] += f[e] * wgt;
        } else if (dist) {
            const float* d = dist + (t / k) * k;
            float norm = 0.f;
            for (int u = 0; u < k; ++u) norm += 1.0f / (d[u] + 1e-8f);
            const float wgt = (1.0f / (d[t % k] + 1e-8f)) / norm;
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[e] += f[e] * wgt;
        } else {
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[e] += f[e];
        }
    }
    store_vec<VEC>(out + s * c + ch, acc);
}

static void pt_partials_sum(const float* part, int nblk, int nq, int c, const PtPartOut& o, hipStream_t st) {
    pt_partials_sum_kernel<<<pt_grid(static_cast<int64_t>(nq) * c), kPtBlock, 0, st>>>(part, nblk, nq, c, o);
    O3DML_LAUNCH_CHECK();
}

}  // namespace o3dml

using namespace o3dml;

O3DML_API size_t o3dml_pt_invert_plan_workspace_size(int64_t m, int64_t k, int64_t n_src) {
    (void)n_src;
    const int64_t total = m > 0 && k > 0 ? m * k : 0;
    return ws_bytes<uint32_t>(total) + prim::radix_sort_workspace_bytes<uint32_t>(total);
}

O3DML_API int o3dml_pt_invert_plan(const int32_t* idx, int64_t m, int64_t k, int64_t n_src, int64_t* inv_splits,
                                   int32_t* inv_pairs, void* workspace, size_t workspace_bytes, void* stream) {
    O3DML_GUARD_BEGIN
    const int64_t lim = int64_t(1) << 31;
    O3DML_REQUIRE(m >= 0 && m < lim && k >= 1 && k < lim && n_src >= 0 && n_src < lim,
                  "pt_invert_plan: m = %lld, k = %lld, n_src = %lld out of range", (long long)m, (long long)k,
                  (long long)n_src);
    O3DML_REQUIRE(m * k < lim, "pt_invert_plan: m * k = %lld * %lld must be below 2^31", (long long)m, (long long)k);
    hipStream_t st = as_stream(stream);
    TimedRegion tr("pt_invert_plan", st);
    const int64_t total = m * k;
    Workspace ws(workspace, workspace_bytes);
    uint32_t* skeys = ws.take<uint32_t>(total);
    prim::radix_sort_pairs<uint32_t>(reinterpret_cast<const uint32_t*>(idx), nullptr, skeys,
                                     reinterpret_cast<uint32_t*>(inv_pairs), total,
                                     prim::bits_needed(static_cast<uint64_t>(n_src)), ws, st);
    prim::segment_offsets_kernel<uint32_t><<<stream_grid(n_src + 1, 256), 256, 0, st>>>(skeys, total, n_src,
                                                                                         inv_splits);
    O3DML_LAUNCH_CHECK();
    O3DML_GUARD_END
}

O3DML_API int o3dml_pt_gather_sum(const float* rows, int64_t ld, int64_t col0, int64_t div, const float* weight,
                                  const float* dist, int64_t k, const int64_t* inv_splits, const int32_t* inv_pairs,
                                  int64_t n_src, int64_t c, float* out, void* stream) {
    O3DML_GUARD_BEGIN
    O3DML_REQUIRE(n_src >= 0 && n_src < (int64_t(1) << 31), "pt_gather_sum: n_src = %lld out of range",
                  (long long)n_src);
    O3DML_REQUIRE(c >= 1 && c <= 65536, "pt_gather_sum: c must be in 1..65536, got %lld", (long long)c);
    O3DML_REQUIRE(col0 >= 0 && ld >= col0 + c && ld < (int64_t(1) << 31),
                  "pt_gather_sum: columns %lld..%lld do not fit rows of %lld", (long long)col0,
                  (long long)(col0 + c), (long long)ld);
    O3DML_REQUIRE(div >= 1 && div <= 64, "pt_gather_sum: div must be in 1..64, got %lld", (long long)div);
    O3DML_REQUIRE(!(weight && dist), "pt_gather_sum: weight and dist are exclusive");
    O3DML_REQUIRE(!dist || (k >= 1 && k <= 8), "pt_gather_sum: k must be in 1..8 with dist, got %lld", (long long)k);
    if (n_src == 0) return 0;
    hipStream_t st = as_stream(stream);
    TimedRegion tr("pt_gather_sum", st);
    const int ci = static_cast<int>(c), c0 = static_cast<int>(col0), dv = static_cast<int>(div);
    const int ki = dist ? static_cast<int>(k) : 1;
    if (c % 4 == 0 && ld % 4 == 0 && col0 % 4 == 0 && aligned16({rows, out}))
        pt_gather_sum_kernel<4><<<pt_grid(n_src * (c / 4)), kPtBlock, 0, st>>>(rows, ld, c0, dv, weight, dist, ki,
                                                                               inv_splits, inv_pairs, n_src, ci, out);
    else
        pt_gather_sum_kernel<1><<<pt_grid(n_src * c), kPtBlock, 0, st>>>(rows, ld, c0, dv, weight, dist, ki,
                                                                         inv_splits, inv_pairs, n_src, ci, out);
    O3DML_LAUNCH_CHECK();
    O3DML_GUARD_END
}

O3DML_API size_t o3dml_pt_backward_workspace_size(int64_t c) {
    return ws_bytes<float>(static_cast<int64_t>(kPtGradBlocks) * 6 * (c > 0 ? c : 0));
}

O3DML_API int o3dml_pt_relation_backward(const float* xyz_q, const float* xyz_src, const int32_t* idx,
                                         const float* feat_k, const float* feat_q, const float* w1, const float* b1,
                                         const float* scale_p, const float* shift_p, const float* w2, const float* b2,
                                         const float* scale_w, const float* shift_w, const float* out,
                                         const float* grad_out, int64_t n, int64_t nsample, int64_t c, float* gr,
                                         float* d_feat_q, float* dh, float* d_scale_w, float* d_shift_w, float* d_w2,
                                         float* d_b2, void* workspace, size_t workspace_bytes, void* stream) {
    O3DML_GUARD_BEGIN
    pt_check_layer("pt_relation_backward", n, nsample, c);
    (void)shift_w;
    hipStream_t st = as_stream(stream);
    TimedRegion tr("pt_relation_backward", st);
    const int ns = static_cast<int>(nsample), ci = static_cast<int>(c);
    if (n == 0) {  // the sums over no pairs
        for (float* p : {d_scale_w, d_shift_w, d_b2}) fill_async(p, 0, sizeof(float) * c, st);
        fill_async(d_w2, 0, sizeof(float) * 3 * c, st);
        return 0;
    }
    const PtPos pos{w1, b1, scale_p, shift_p, w2, b2};
    const bool vec = c % 4 == 0 && aligned16({feat_k, feat_q, scale_w, out, grad_out, gr, d_feat_q});
    const PtGradGeom gm = pt_grad_geom(n, ci, vec ? 4 : 1);
    Workspace ws(workspace, workspace_bytes);
    float* part = ws.take<float>(static_cast<int64_t>(gm.grid) * 6 * c);
    if (vec)
        pt_relation_bwd_kernel<4><<<gm.grid, kPtBlock, 0, st>>>(pos, xyz_q, xyz_src, idx, feat_k, feat_q, scale_w,
                                                                shift_w, out, grad_out, n, ns, ci, gm, gr, d_feat_q,
                                                                dh, part);
    else
        pt_relation_bwd_kernel<1><<<gm.grid, kPtBlock, 0, st>>>(pos, xyz_q, xyz_src, idx, feat_k, feat_q, scale_w,
                                                                shift_w, out, grad_out, n, ns, ci, gm, gr, d_feat_q,
                                                                dh, part);
    O3DML_LAUNCH_CHECK();
    const PtPartOut po{{d_scale_w, d_shift_w, d_w2, d_w2 + 1, d_w2 + 2, d_b2}, {1, 1, 3, 3, 3, 1}};
    pt_partials_sum(part, static_cast<int>(gm.grid), 6, ci, po, st);
    O3DML_GUARD_END
}

O3DML_API int o3dml_pt_aggregate_backward(const float* xyz_q, const float* xyz_src, const int32_t* idx,
                                          const float* feat_v, const float* weight, const float* w1, const float* b1,
                                          const float* scale_p, const float* shift_p, const float* w2,
                                          const float* b2, const float* grad_out, int64_t n, int64_t nsample,
                                          int64_t c, int64_t share_planes, float* d_val, float* d_weight, float* dh,
                                          float* d_w2, float* d_b2, void* workspace, size_t workspace_bytes,
                                          void* stream) {
    O3DML_GUARD_BEGIN
    pt_check_layer("pt_aggregate_backward", n, nsample, c);
    O3DML_REQUIRE(share_planes >= 1 && c % share_planes == 0,
                  "pt_aggregate_backward: c = %lld is not a multiple of share_planes = %lld", (long long)c,
                  (long long)share_planes);
    hipStream_t st = as_stream(stream);
    TimedRegion tr("pt_aggregate_backward", st);
    const int ns = static_cast<int>(nsample), ci = static_cast<int>(c), cs = static_cast<int>(c / share_planes);
    if (n == 0) {
        fill_async(d_b2, 0, sizeof(float) * c, st);
        fill_async(d_w2, 0, sizeof(float) * 3 * c, st);
        return 0;
    }
    const PtPos pos{w1, b1, scale_p, shift_p, w2, b2};
    const bool vec = c % 4 == 0 && aligned16({feat_v, grad_out, d_val});
    const PtGradGeom gm = pt_grad_geom(n, ci, vec ? 4 : 1);
    Workspace ws(workspace, workspace_bytes);
    float* part = ws.take<float>(static_cast<int64_t>(gm.grid) * 4 * c);
    if (vec)
        pt_aggregate_bwd_kernel<4><<<gm.grid, kPtBlock, 0, st>>>(pos, xyz_q, xyz_src, idx, feat_v, weight, grad_out, n,
                                                                 ns, ci, cs, gm, d_val, d_weight, dh, part);
    else
        pt_aggregate_bwd_kernel<1><<<gm.grid, kPtBlock, 0, st>>>(pos, xyz_q, xyz_src, idx, feat_v, weight, grad_out, n,
                                                                 ns, ci, cs, gm, d_val, d_weight, dh, part);
    O3DML_LAUNCH_CHECK();
    const PtPartOut po{{d_w2, d_w2 + 1, d_w2 + 2, d_b2, nullptr, nullptr}, {3, 3, 3, 1, 0, 0}};
    pt_partials_sum(part, static_cast<int>(gm.grid), 4, ci, po, st);
    O3DML_GUARD_END
}
