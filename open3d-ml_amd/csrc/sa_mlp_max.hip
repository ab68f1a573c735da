// sa_mlp_max.hip — a PointNet++ set-abstraction level in one kernel: the rows
// of every group gathered, pushed through the shared MLP and max-reduced
// (ml3d/torch/utils/pointnet/pointnet2_utils.py QueryAndGroup / GroupAll, then
// the mlps and the max_pool2d of ml3d/torch/models/utils/pointnet
// PointnetSAModuleMSG.forward).
//
// The contract.  Contiguous arrays:
//   xyz      f32 [B,N,3]
//   new_xyz  f32 [B,M,3]   or null (no centre is subtracted: GroupAll)
//   features f32 [B,N,C]   or null (C = 0)
//   idx      i32 [B,M,S]   rows of the same cloud, 0 <= idx < N; or null = identity
//                          (then M = 1, S = N: GroupAll)
//   use_xyz  row r of group (b,m) = [xyz[b,idx] - new_xyz[b,m] | features[b,idx]]
//            (3 + C values), or the features alone (C values) when off
//   layers   L in 1..4, widths c_0 = row width, c_1..c_L; layer l: h = relu(W_l h + b_l),
//            W_l [c_l, c_{l-1}], BatchNorm already folded in, every layer followed by ReLU
//   out      f32 [B,M,c_L] = max over the S rows of the last layer's output
// The centre subtraction is one rounded f32 subtraction; the products are exact
// f32 accumulated in f32 (v_mfma_f32_32x32x2_f32) in ascending k, the bias added
// last.  Every output element is written, nothing is accumulated across
// workgroups and there are no atomics: run-to-run bitwise equal, correct on an
// output that was not cleared.  Inputs are finite.  An index outside [0, N) is
// clamped into the cloud (never read out of bounds); its result is unspecified.
// Limits, returned as status before any launch: L in 1..4, S >= 1, c_0 <= 1027,
// c_l <= 512, B * N and B * M below 2^31.
//
// Packed weights (o3dml_sa_mlp_max_packed_size, built by the caller once per
// call): layer after layer, W_l transposed [kpad_l][cpad_l] row-major followed
// by b_l [cpad_l]; kpad_l = c_{l-1} rounded up to 8 (the k loop's step),
// cpad_l = c_l rounded up to 32 (the MFMA tile); the padding is zeros, so odd
// widths need no special case in the inner loop: a padded input column
// multiplies a zero weight row, a padded output column is relu(0 + 0) = 0.
//
// Mapping.  A workgroup of 4 waves owns a tile of R = 64 rows (R = 32 when the
// hidden buffers of 64 rows do not fit the LDS, or when S <= 32 and 64-row
// tiles would be fewer than the 256 CUs).  S <= R: the tile holds
// floor(R / S) whole groups; S > R: a workgroup walks one group in row tiles
// and keeps the running maximum per output column in LDS (each column has one
// owner lane, so that needs no barrier).  Rows of a tile that belong to no group
// repeat the tile's last real row (a zero row would answer relu(b) pushed
// through the layers) and are left out of the maximum.
//   layer 1   streams its input in chunks of 64 channels: gathered from the
//             cloud (L2-resident) into LDS [R][65], multiplied, next chunk;
//   hidden    activations ping-pong between two LDS buffers [R][cpad + 1] (odd
//             stride: the 32 rows an MFMA A read touches lie on 32 banks; the
//             accumulator write-back runs along a row);
//   weights   read from L2 as B operands: a wave's load is two runs of 32
//             consecutive floats of the transposed matrix;
//   tiles     per pass wave w takes the column tiles w and w + 4 of a block of
//             8 (256 columns) for all R rows: 2 x 2 accumulators of 32 x 32, so
//             one A read feeds two MFMAs and one B load feeds two;
//   last      layer: bias + ReLU in the accumulators, then the maximum over the
//             registers and the two lane halves that hold a group's rows, one
//             store per output element.  It is never written to LDS.
#include "common.hpp"

namespace o3dml {

constexpr int kSaThreads = 256;
constexpr int kSaKC = 64;  // channels of a first-layer chunk
constexpr int kSaMaxLayers = 4;
constexpr int kSaMaxWidth = 512;
constexpr int kSaMaxIn = 1027;
constexpr size_t kSaLdsMax = 160 * 1024;  // LDS of a gfx950 CU
constexpr int kSaFillUnits = 256;         // one workgroup per CU

typedef float sa_f32x16 __attribute__((ext_vector_type(16)));

struct SaPlan {
    int L, c0, cout;
    int kpad[kSaMaxLayers], cpad[kSaMaxLayers];
    int woff[kSaMaxLayers], boff[kSaMaxLayers];  // float offsets into the packed buffer
    int ld[2];                                   // row strides of the two hidden buffers
};

// acc[i][j] += A[32 i .. 32 i + 31][0 .. klen) * W[0 .. klen)[tile j]; a points at
// row li, column lh of the A rows, w at row lh, column li of the first tile.
template <int NR, int NC>
__device__ __forceinline__ void sa_mma(const float* a, int lda, const float* __restrict__ w, int ldw, int klen,
                                       sa_f32x16 (&acc)[NR][2]) {
    for (int k0 = 0; k0 < klen; k0 += 8) {  // klen is a multiple of 8: four k steps with their loads in flight together
        float av[4][NR], bv[4][NC];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
#pragma unroll
            for (int j = 0; j < NC; ++j) bv[s][j] = w[static_cast<int64_t>(k0 + 2 * s) * ldw + 128 * j];
#pragma unroll
            for (int i = 0; i < NR; ++i) av[s][i] = a[32 * i * lda + k0 + 2 * s];
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int i = 0; i < NR; ++i)
#pragma unroll
                for (int j = 0; j < NC; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s][i], bv[s][j], acc[i][j], 0, 0, 0);
    }
}

template <int NR>
__global__ void __launch_bounds__(kSaThreads)
sa_mlp_max_kernel(const float* __restrict__ xyz, const float* __restrict__ new_xyz, const float* __restrict__ feat,
                  const int32_t* __restrict__ idx, int64_t N, int64_t M, int S, int C, int use_xyz, int64_t groups,
                  int64_t units, SaPlan P, const float* __restrict__ packed, float* __restrict__ out) {
    constexpr int R = 32 * NR;
    constexpr int LDC = kSaKC + 1;
    extern __shared__ float sa_lds[];
    int* srow = reinterpret_cast<int*>(sa_lds);  // [R] row of the cloud, b * N + i
    float* ctr = sa_lds + R;                     // [R][3] the centre subtracted from it
    float* omax = ctr + 3 * R;                   // [cpad of the last layer] running maximum (S > R)
    float* chunk = omax + kSaMaxWidth;           // [R][LDC]
    float* hidden = chunk + R * LDC;             // buffer 0 [R][ld[0]], then buffer 1 [R][ld[1]]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const bool packs = S <= R;
    const int G = packs ? R / S : 1;               // groups of a tile
    const int tiles = packs ? 1 : (S + R - 1) / R;  // row tiles of a group

    for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
        const int64_t group0 = u * G;
        const int ngroups = groups - group0 < G ? static_cast<int>(groups - group0) : G;
        for (int t = 0; t < tiles; ++t) {
            const int valid = packs ? ngroups * S : (S - t * R < R ? S - t * R : R);
            __syncthreads();  // the rows of the tile before are no longer read
            if (tid < R) {
                const int v = tid < valid ? tid : valid - 1;  // rows past the end repeat the last real one
                const int64_t g = packs ? group0 + v / S : group0;
                const int j = packs ? v % S : t * R + v;
                int64_t i = idx ? idx[g * S + j] : j;
                i = i < 0 ? 0 : (i >= N ? N - 1 : i);
                srow[tid] = static_cast<int>((g / M) * N + i);
#pragma unroll
                for (int d = 0; d < 3; ++d) ctr[3 * tid + d] = new_xyz ? new_xyz[3 * g + d] : 0.f;
            }

            for (int l = 0; l < P.L; ++l) {
                const bool last = l == P.L - 1;
                const int ntile = P.cpad[l] / 32, ldw = P.cpad[l];
                const float* wl = packed + P.woff[l];
                const float* bl = packed + P.boff[l];
                for (int t0 = wave; t0 - wave < ntile; t0 += 8) {  // the same trip count in every wave
                    const int nc = t0 >= ntile ? 0 : (t0 + 4 < ntile ? 2 : 1);
                    const float* wp = wl + static_cast<int64_t>(lh) * ldw + 32 * t0 + li;
                    sa_f32x16 acc[NR][2];
#pragma unroll
                    for (int i = 0; i < NR; ++i)
#pragma unroll
                        for (int j = 0; j < 2; ++j)
#pragma unroll
                            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
                    if (l == 0) {
                        for (int k0 = 0; k0 < P.kpad[0]; k0 += kSaKC) {
                            __syncthreads();  // srow / ctr written; the chunk before is no longer read
#pragma unroll 8
                            for (int e = tid; e < R * kSaKC; e += kSaThreads) {
                                const int row = e / kSaKC, k = k0 + e % kSaKC;
                                float v = 0.f;
                                if (k < P.c0) {
                                    const int64_t s = srow[row];
                                    if (use_xyz)
                                        v = k < 3 ? xyz[3 * s + k] - ctr[3 * row + k] : feat[s * C + (k - 3)];
                                    else
                                        v = feat[s * C + k];
                                }
                                chunk[row * LDC + e % kSaKC] = v;
                            }
                            __syncthreads();
                            const int klen = P.kpad[0] - k0 < kSaKC ? P.kpad[0] - k0 : kSaKC;
                            const float* a = chunk + li * LDC + lh;
                            const float* w = wp + static_cast<int64_t>(k0) * ldw;
                            if (nc == 2) sa_mma<NR, 2>(a, LDC, w, ldw, klen, acc);
                            else if (nc == 1) sa_mma<NR, 1>(a, LDC, w, ldw, klen, acc);
                        }
                    } else {
                        const int lda = P.ld[(l - 1) & 1];
                        const float* a = hidden + (((l - 1) & 1) ? R * P.ld[0] : 0) + li * lda + lh;
                        if (nc == 2) sa_mma<NR, 2>(a, lda, wp, ldw, P.kpad[l], acc);
                        else if (nc == 1) sa_mma<NR, 1>(a, lda, wp, ldw, P.kpad[l], acc);
                    }
                    // lane, register r of acc[i][j]: column li of tile t0 + 4 j, row 32 i + (r & 3) + 8 (r >> 2) + 4 lh
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        if (j >= nc) break;
                        const int col = 32 * (t0 + 4 * j) + li;
                        const float bb = bl[col];
                        if (!last) {
                            float* dst = hidden + ((l & 1) ? R * P.ld[0] : 0) + col;
                            const int ldd = P.ld[l & 1];
#pragma unroll
                            for (int i = 0; i < NR; ++i)
#pragma unroll
                                for (int r = 0; r < 16; ++r) {
                                    const int row = 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lh;
                                    const float v = acc[i][j][r] + bb;
                                    dst[row * ldd] = v > 0.f ? v : 0.f;
                                }
                            continue;
                        }
                        // every value is >= 0 after the ReLU, so 0 is neutral for the maximum
                        for (int gi = 0; gi < (packs ? ngroups : 1); ++gi) {
                            const int lo = packs ? gi * S : 0, hi = packs ? lo + S : valid;
                            float m = 0.f;
#pragma unroll
                            for (int i = 0; i < NR; ++i)
#pragma unroll
                                for (int r = 0; r < 16; ++r) {
                                    const int row = 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lh;
                                    const float v = acc[i][j][r] + bb;
                                    m = row >= lo && row < hi && v > m ? v : m;
                                }
                            const float o = __shfl_xor(m, 32, 64);
                            m = o > m ? o : m;
                            if (lh == 0) {
                                if (!packs) {
                                    if (t > 0) m = omax[col] > m ? omax[col] : m;
                                    omax[col] = m;  // read and written by this lane alone
                                }
                                if (t == tiles - 1 && col < P.cout) out[(group0 + gi) * P.cout + col] = m;
                            }
                        }
                    }
                }
                __syncthreads();  // the layer's output is complete, its input free to be overwritten
            }
        }
    }
}

// widths [L + 1] -> plan; false when a limit is exceeded (message set)
static bool sa_plan(int L, const int32_t* widths, SaPlan& P, int64_t& total) {
    if (L < 1 || L > kSaMaxLayers) {
        set_error("sa_mlp_max: layers must be in 1..%d, got %d", kSaMaxLayers, L);
        return false;
    }
    if (widths[0] < 1 || widths[0] > kSaMaxIn) {
        set_error("sa_mlp_max: row width c_0 must be in 1..%d, got %d", kSaMaxIn, widths[0]);
        return false;
    }
    P = SaPlan{};
    P.L = L;
    P.c0 = widths[0];
    P.cout = widths[L];
    total = 0;
    for (int l = 0; l < L; ++l) {
        if (widths[l + 1] < 1 || widths[l + 1] > kSaMaxWidth) {
            set_error("sa_mlp_max: width c_%d must be in 1..%d, got %d", l + 1, kSaMaxWidth, widths[l + 1]);
            return false;
        }
        P.kpad[l] = (widths[l] + 7) / 8 * 8;
        P.cpad[l] = (widths[l + 1] + 31) / 32 * 32;
        P.woff[l] = static_cast<int>(total);
        total += static_cast<int64_t>(P.kpad[l]) * P.cpad[l];
        P.boff[l] = static_cast<int>(total);
        total += P.cpad[l];
        if (l < L - 1 && P.cpad[l] + 1 > P.ld[l & 1]) P.ld[l & 1] = P.cpad[l] + 1;
    }
    return true;
}

static size_t sa_lds_bytes(const SaPlan& P, int R) {
    return sizeof(float) * (static_cast<size_t>(R) * (4 + kSaKC + 1 + P.ld[0] + P.ld[1]) + kSaMaxWidth);
}

}  // namespace o3dml

using namespace o3dml;

O3DML_API int64_t o3dml_sa_mlp_max_packed_size(int n_layers, const int32_t* widths) {
    SaPlan P;
    int64_t total = 0;
    if (!widths || !sa_plan(n_layers, widths, P, total)) return -1;
    return total;
}

O3DML_API int o3dml_sa_mlp_max(const float* xyz, const float* new_xyz, const float* features, const int32_t* idx,
                               int64_t B, int64_t N, int64_t M, int64_t S, int64_t C, int use_xyz, int n_layers,
                               const int32_t* widths, const float* packed, int64_t packed_len, float* out,
                               void* stream) {
    O3DML_GUARD_BEGIN
    O3DML_REQUIRE(B >= 0 && M >= 0 && N >= 0 && C >= 0, "sa_mlp_max: B, N, M, C must not be negative");
    O3DML_REQUIRE(S >= 1 && S < (int64_t(1) << 31), "sa_mlp_max: S must be >= 1, got %lld", (long long)S);
    O3DML_REQUIRE(B * N < (int64_t(1) << 31) && B * M < (int64_t(1) << 31),
                  "sa_mlp_max: B * N = %lld and B * M = %lld must be below 2^31", (long long)(B * N), (long long)(B * M));
    O3DML_REQUIRE(widths != nullptr, "sa_mlp_max: widths is null");
    SaPlan P;
    int64_t total = 0;
    if (!sa_plan(n_layers, widths, P, total)) throw Error{2};
    O3DML_REQUIRE(use_xyz || C > 0, "sa_mlp_max: no features and use_xyz is off");
    O3DML_REQUIRE(P.c0 == (use_xyz ? 3 : 0) + C, "sa_mlp_max: c_0 = %d, but a row has %lld values", P.c0,
                  (long long)((use_xyz ? 3 : 0) + C));
    O3DML_REQUIRE((C > 0) == (features != nullptr), "sa_mlp_max: features must be given exactly when C > 0");
    O3DML_REQUIRE(packed_len == total, "sa_mlp_max: packed weights hold %lld floats, the widths need %lld",
                  (long long)packed_len, (long long)total);
    O3DML_REQUIRE(idx != nullptr || (M == 1 && S == N), "sa_mlp_max: without idx M must be 1 and S = N");
    const int64_t groups = B * M;
    if (groups == 0) return 0;
    O3DML_REQUIRE(N >= 1, "sa_mlp_max: the cloud is empty");
    // 32-row tiles when 64 rows do not fit, and when groups of at most 32 rows would otherwise leave
    // CUs without a workgroup (the RCNN's GroupAll level: 100 groups of 32 rows)
    const int R = sa_lds_bytes(P, 64) <= kSaLdsMax && !(S <= 32 && ceil_div(groups, 64 / S) < kSaFillUnits) ? 64 : 32;
    const size_t lds = sa_lds_bytes(P, R);
    O3DML_REQUIRE(lds <= kSaLdsMax, "sa_mlp_max: hidden widths need %zu bytes of LDS (limit %zu)", lds, kSaLdsMax);
    const int64_t units = S <= R ? ceil_div(groups, R / S) : groups;
    const unsigned grid = static_cast<unsigned>(units < (1 << 20) ? units : (1 << 20));
    hipStream_t st = as_stream(stream);
    static const bool attr = [] {  // more than the default 64 KiB of dynamic LDS
        return hipFuncSetAttribute(reinterpret_cast<const void*>(&sa_mlp_max_kernel<1>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, kSaLdsMax) == hipSuccess &&
               hipFuncSetAttribute(reinterpret_cast<const void*>(&sa_mlp_max_kernel<2>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, kSaLdsMax) == hipSuccess;
    }();
    O3DML_REQUIRE(attr || lds <= 64 * 1024, "sa_mlp_max: the device refused %zu bytes of LDS", lds);
    TimedRegion tr("sa_mlp_max", st);
    if (R == 64)
        sa_mlp_max_kernel<2><<<grid, kSaThreads, lds, st>>>(xyz, new_xyz, features, idx, N, M, static_cast<int>(S),
                                                           static_cast<int>(C), use_xyz, groups, units, P, packed, out);
    else
        sa_mlp_max_kernel<1><<<grid, kSaThreads, lds, st>>>(xyz, new_xyz, features, idx, N, M, static_cast<int>(S),
                                                           static_cast<int>(C), use_xyz, groups, units, P, packed, out);
    O3DML_LAUNCH_CHECK();
    O3DML_GUARD_END
}
