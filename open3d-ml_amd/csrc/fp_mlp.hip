// fp_mlp.hip — a PointNet++ feature-propagation module in one kernel: the
// three-point inverse-distance interpolation of the known features, the
// concatenation with the unknown points' own features and the shared MLP
// (ml3d/torch/modules/pointnet.py:252-298 PointnetFPModule.forward, with
// three_nn left to o3dml_three_nn).
//
// The contract.  Contiguous arrays, channels-last:
//   known_feats   f32 [B,m,C2]   C2 >= 1, m >= 1
//   unknown_feats f32 [B,n,C1]   or null (C1 = 0)
//   dist2         f32 [B,n,3]    as o3dml_three_nn writes it: squared distances,
//                                +inf in a slot that no known point filled (m < 3)
//   idx           i32 [B,n,3]    rows of the same batch item's known points
//   layers        L in 1..4, widths c_0 = C2 + C1, c_1..c_L; layer l:
//                 h = relu(W_l h + b_l), W_l [c_l, c_{l-1}], BatchNorm already
//                 folded in, every layer followed by ReLU
//   out           f32 [B,n,c_L]
// Row i of batch item b is [ sum_j w_j known_feats[b, idx[b,i,j]] | unknown_feats[b,i] ]
// with r_j = 1 / (sqrt(dist2_j) + 1e-8), w_j = r_j / (r_0 + r_1 + r_2), all IEEE
// f32 (correctly rounded sqrt and divisions), so a +inf slot has r_j = w_j = 0
// exactly and adds 0 * (a finite feature) = 0.  The sum is
// fma(w_2, f_2, fma(w_1, f_1, w_0 f_0)) as in three_interpolate; the layers'
// products are exact f32 accumulated in f32 (v_mfma_f32_32x32x2_f32) in
// ascending k, the bias added last.  Every output element is written, nothing
// is accumulated across workgroups and there are no atomics: run-to-run bitwise
// equal, correct on an output that was not cleared.  Features are finite.  An
// index outside [0, m) is clamped (never read out of bounds); its result is
// unspecified.  Limits, returned as status before any launch: L in 1..4,
// c_0 <= 2048, c_l <= 512, B * n and B * m below 2^31.
//
// Packed weights: the layout of sa_mlp_max.hip (layer after layer W_l
// transposed [kpad_l][cpad_l], then b_l [cpad_l]; kpad_l = c_{l-1} rounded up
// to 8, cpad_l = c_l rounded up to 32, zero padding), sized by
// o3dml_fp_mlp_packed_size under this file's own c_0 limit.
//
// Design.  There are no groups and no reduction here: a row is a point, a tile
// is 32 consecutive rows of the flattened [B * n] and the last tile is simply
// short (its missing rows repeat the last real one and are never stored).
// What costs is the first layer's input: c_0 up to 2048 values per row, three
// scattered source rows behind every value below C2.
//   tile      R = 32 rows, the rows of one v_mfma_f32_32x32x2_f32, whatever the
//             shape.  The RPN's modules have 16384, 4096, 1024 and 256 rows:
//             only the first would give every one of the 256 CUs a 64-row
//             tile, and the deep ones (1536 -> 512 -> 512 on 256 rows) are
//             bound by how many CUs take part at all: 8 tiles of 32 rows, each
//             about 110 us of MFMA issue on one CU.  A 64-row variant of this
//             kernel (2 x 2 accumulators per wave) needs more than the 256
//             registers a lane of a 512-thread workgroup has and spilled, so
//             it is not built.  Spreading one tile's columns over workgroups
//             would put the hidden activations in global memory behind a
//             second launch.
//   workgroup 8 waves (512 threads), two per SIMD.  Wave w owns the 32-column
//             tiles w and w + 8 of a layer, so one pass covers the widest
//             layer (16 tiles = 512 columns) and the first layer's input is
//             gathered exactly once (sa_mlp_max walks it once per 256
//             columns): this is what serves the few-row shapes, where one
//             workgroup's stream of up to 4 MB of weights is the latency.
//             Each wave streams an eighth of a layer's weights (a B load is
//             two runs of 32 consecutive floats of the transposed matrix,
//             from L2), one A read from LDS feeds two MFMAs, four k steps'
//             loads are in flight together and the SIMD's other wave covers
//             what latency is left.
//   grid      min(tiles, 1024) workgroups that walk the tiles with that
//             stride.
//   meta      once per tile, thread r < 32 turns row r's dist2 and idx into
//             three weights and three source rows (b * m + clamped index) in
//             LDS: the sqrt and the three divisions are done once per row,
//             not once per chunk.
//   stream    layer 1 takes its input in chunks of 64 channels, LDS
//             [32][65].  A chunk is loaded by all 8 waves: wave w, pass i
//             handles row w + 8 i, lane = channel, so a wave reads 256
//             consecutive bytes of each of the three source rows (below C2)
//             or of the point's own row (from C2 up).  A chunk that straddles
//             C2 is a per-lane select, not a branch; channels past c_0 are
//             zeros.
//   overlap   the chunk is double-buffered: the 12 to 16 loads of chunk c + 1
//             are issued into registers before the MFMAs of chunk c, the
//             weighted sums are formed and written to the other buffer after
//             them, then one barrier.  LDS: 4 * 32 * (6 + 2 * 65 + ld0 + ld1)
//             bytes, 149 KiB of the 160 at 512, 512, x (ld = 513 twice), so
//             the second buffer always fits.
//   hidden    activations ping-pong between two LDS buffers [32][cpad + 1] as in
//             sa_mlp_max (odd stride: the 32 rows of an A read lie on 32
//             banks, the write-back runs along a row).
//   last      layer: bias + ReLU in the accumulators and straight to `out`:
//             a register of a wave is two runs of 32 consecutive floats of
//             two rows, 128-byte stores.  Never written to LDS.
#include "common.hpp"

namespace o3dml {

constexpr int kFpThreads = 512;
constexpr int kFpWaves = kFpThreads / 64;
constexpr int kFpR = 32;                          // rows of a tile
constexpr int kFpKC = 64;                         // channels of a first-layer chunk = lanes of a wave
constexpr int kFpLDC = kFpKC + 1;                 // its row stride in LDS
constexpr int kFpPasses = kFpR / kFpWaves;        // values of a chunk per lane
constexpr int kFpMaxLayers = 4;
constexpr int kFpMaxWidth = 512;
constexpr int kFpMaxIn = 2048;
constexpr size_t kFpLdsMax = 160 * 1024;  // LDS of a gfx950 CU
constexpr int kFpGridMax = 1024;

typedef float fp_f32x16 __attribute__((ext_vector_type(16)));

struct FpPlan {
    int L, c0, cout;
    int kpad[kFpMaxLayers], cpad[kFpMaxLayers];
    int woff[kFpMaxLayers], boff[kFpMaxLayers];  // float offsets into the packed buffer
    int ld[2];                                   // row strides of the two hidden buffers
};

// acc[j] += A[0 .. 31][0 .. klen) * W[0 .. klen)[tile j]; a points at
// row li, column lh of the A rows, w at row lh, column li of the wave's first
// tile; its second tile lies 8 tiles (256 columns) further.
template <int NC>
__device__ __forceinline__ void fp_mma(const float* a, int lda, const float* __restrict__ w, int ldw, int klen,
                                       fp_f32x16 (&acc)[2]) {
    for (int k0 = 0; k0 < klen; k0 += 8) {  // klen is a multiple of 8: four k steps with their loads in flight together
        float av[4], bv[4][NC];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
#pragma unroll
            for (int j = 0; j < NC; ++j) bv[s][j] = w[static_cast<int64_t>(k0 + 2 * s) * ldw + 32 * kFpWaves * j];
            av[s] = a[k0 + 2 * s];
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int j = 0; j < NC; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], bv[s][j], acc[j], 0, 0, 0);
    }
}

// The raw values of the chunk at channel k0 for this lane: pass i is row
// wave + 8 i, channel k = k0 + lane.  Below C2 the three source rows' values,
// from C2 up the row's own value in f[i][0]; zeros past c_0.  Nothing branches
// per lane, so all of a chunk's loads are in flight together: a lane at or
// past C2 reads column 0 of the source rows (one address per row for the
// lanes that share it) and drops it; the unknown side is visited only by the
// chunks that reach it, again at a clamped column.
__device__ __forceinline__ void fp_chunk_load(const float* __restrict__ known, const float* __restrict__ unknown,
                                              const int* srow, int64_t row0, int valid, int C2, int C1, int k0,
                                              int lane, int wave, float (&f)[kFpPasses][3]) {
    const int k = k0 + lane;
    const bool below = k < C2, own = !below && k < C2 + C1;
    const int kk = below ? k : 0, ku = own ? k - C2 : 0;
#pragma unroll
    for (int i = 0; i < kFpPasses; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float v = known[static_cast<int64_t>(srow[3 * (wave + kFpWaves * i) + j]) * C2 + kk];
            f[i][j] = below ? v : 0.f;
        }
    if (C1 > 0 && k0 + kFpKC > C2) {
#pragma unroll
        for (int i = 0; i < kFpPasses; ++i) {
            const int row = wave + kFpWaves * i;
            const float u = unknown[(row0 + (row < valid ? row : valid - 1)) * C1 + ku];
            f[i][0] = own ? u : f[i][0];
        }
    }
}

__device__ __forceinline__ void fp_chunk_store(float* buf, const float* swt, int C2, int k0, int lane, int wave,
                                               const float (&f)[kFpPasses][3]) {
#pragma unroll
    for (int i = 0; i < kFpPasses; ++i) {
        const int row = wave + kFpWaves * i;
        const float* w = swt + 3 * row;
        const float v = __builtin_fmaf(w[2], f[i][2], __builtin_fmaf(w[1], f[i][1], w[0] * f[i][0]));
        buf[row * kFpLDC + lane] = k0 + lane < C2 ? v : f[i][0];
    }
}

__global__ void __launch_bounds__(kFpThreads)
fp_mlp_kernel(const float* __restrict__ known, const float* __restrict__ unknown, const float* __restrict__ dist2,
              const int32_t* __restrict__ idx, int64_t rows, int64_t n, int64_t m, int C2, int C1, int64_t tiles,
              FpPlan P, const float* __restrict__ packed, float* __restrict__ out) {
    constexpr int R = kFpR, KC = kFpKC, LDC = kFpLDC;
    extern __shared__ float fp_lds[];
    int* srow = reinterpret_cast<int*>(fp_lds);  // [R][3] source rows of the known features, b * m + index
    float* swt = fp_lds + 3 * R;                 // [R][3] their weights
    float* chunk = swt + 3 * R;                  // two buffers [R][LDC]
    float* hidden = chunk + 2 * R * LDC;         // buffer 0 [R][ld[0]], then buffer 1 [R][ld[1]]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int nchunk = (P.kpad[0] + KC - 1) / KC;

    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row0 = tile * R;
        const int valid = rows - row0 < R ? static_cast<int>(rows - row0) : R;
        // the barrier that ends the last layer of the tile before lies behind every read of its LDS
        if (tid < R) {
            const int64_t g = row0 + (tid < valid ? tid : valid - 1);  // rows past the end repeat the last real one
            const int64_t b = g / n;
            float r[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                r[j] = 1.0f / (sqrtf(dist2[3 * g + j]) + 1e-8f);
                int64_t s = idx[3 * g + j];
                s = s < 0 ? 0 : (s >= m ? m - 1 : s);
                srow[3 * tid + j] = static_cast<int>(b * m + s);
            }
            const float sum = r[0] + r[1] + r[2];
#pragma unroll
            for (int j = 0; j < 3; ++j) swt[3 * tid + j] = r[j] / sum;
        }
        __syncthreads();
        float f[kFpPasses][3];
        fp_chunk_load(known, unknown, srow, row0, valid, C2, C1, 0, lane, wave, f);
        fp_chunk_store(chunk, swt, C2, 0, lane, wave, f);
        __syncthreads();

        for (int l = 0; l < P.L; ++l) {
            const bool last = l == P.L - 1;
            const int ntile = P.cpad[l] / 32, ldw = P.cpad[l];
            const int nc = wave >= ntile ? 0 : (wave + kFpWaves < ntile ? 2 : 1);
            const float* wp = packed + P.woff[l] + static_cast<int64_t>(lh) * ldw + 32 * wave + li;
            const float* bl = packed + P.boff[l];
            fp_f32x16 acc[2];
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
            if (l == 0) {
                for (int c = 0; c < nchunk; ++c) {  // the same trip count in every wave
                    const int k0 = c * KC;
                    const bool more = c + 1 < nchunk;
                    if (more) fp_chunk_load(known, unknown, srow, row0, valid, C2, C1, k0 + KC, lane, wave, f);
                    const int klen = P.kpad[0] - k0 < KC ? P.kpad[0] - k0 : KC;
                    const float* a = chunk + (c & 1) * R * LDC + li * LDC + lh;
                    const float* w = wp + static_cast<int64_t>(k0) * ldw;
                    if (nc == 2) fp_mma<2>(a, LDC, w, ldw, klen, acc);
                    else if (nc == 1) fp_mma<1>(a, LDC, w, ldw, klen, acc);
                    if (more) fp_chunk_store(chunk + ((c + 1) & 1) * R * LDC, swt, C2, k0 + KC, lane, wave, f);
                    __syncthreads();  // chunk c + 1 is written, chunk c no longer read
                }
            } else {
                const int lda = P.ld[(l - 1) & 1];
                const float* a = hidden + (((l - 1) & 1) ? R * P.ld[0] : 0) + li * lda + lh;
                if (nc == 2) fp_mma<2>(a, lda, wp, ldw, P.kpad[l], acc);
                else if (nc == 1) fp_mma<1>(a, lda, wp, ldw, P.kpad[l], acc);
            }
            // lane, register r of acc[j]: column li of tile wave + 8 j, row (r & 3) + 8 (r >> 2) + 4 lh
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if (j >= nc) break;
                const int col = 32 * (wave + kFpWaves * j) + li;
                const float bb = bl[col];
                if (!last) {
                    float* dst = hidden + ((l & 1) ? R * P.ld[0] : 0) + col;
                    const int ldd = P.ld[l & 1];
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = (r & 3) + 8 * (r >> 2) + 4 * lh;
                        const float v = acc[j][r] + bb;
                        dst[row * ldd] = v > 0.f ? v : 0.f;
                    }
                } else if (col < P.cout) {
                    float* dst = out + row0 * P.cout + col;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = (r & 3) + 8 * (r >> 2) + 4 * lh;
                        const float v = acc[j][r] + bb;
                        if (row < valid) dst[static_cast<int64_t>(row) * P.cout] = v > 0.f ? v : 0.f;
                    }
                }
            }
            __syncthreads();  // the layer's output is complete, its input free to be overwritten
        }
    }
}

// widths [L + 1] -> plan; false when a limit is exceeded (message set)
static bool fp_plan(int L, const int32_t* widths, FpPlan& P, int64_t& total) {
    if (L < 1 || L > kFpMaxLayers) {
        set_error("fp_mlp: layers must be in 1..%d, got %d", kFpMaxLayers, L);
        return false;
    }
    if (widths[0] < 1 || widths[0] > kFpMaxIn) {
        set_error("fp_mlp: row width c_0 must be in 1..%d, got %d", kFpMaxIn, widths[0]);
        return false;
    }
    P = FpPlan{};
    P.L = L;
    P.c0 = widths[0];
    P.cout = widths[L];
    total = 0;
    for (int l = 0; l < L; ++l) {
        if (widths[l + 1] < 1 || widths[l + 1] > kFpMaxWidth) {
            set_error("fp_mlp: width c_%d must be in 1..%d, got %d", l + 1, kFpMaxWidth, widths[l + 1]);
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

static size_t fp_lds_bytes(const FpPlan& P) {
    return sizeof(float) * kFpR * (6 + 2 * kFpLDC + P.ld[0] + P.ld[1]);
}

}  // namespace o3dml

using namespace o3dml;

O3DML_API int64_t o3dml_fp_mlp_packed_size(int n_layers, const int32_t* widths) {
    FpPlan P;
    int64_t total = 0;
    if (!widths || !fp_plan(n_layers, widths, P, total)) return -1;
    return total;
}

O3DML_API int o3dml_fp_mlp(const float* known_feats, const float* unknown_feats, const float* dist2,
                           const int32_t* idx, int64_t B, int64_t n, int64_t m, int64_t C2, int64_t C1, int n_layers,
                           const int32_t* widths, const float* packed, int64_t packed_len, float* out, void* stream) {
    O3DML_GUARD_BEGIN
    O3DML_REQUIRE(B >= 0 && n >= 0 && m >= 0 && C1 >= 0, "fp_mlp: B, n, m, C1 must not be negative");
    O3DML_REQUIRE(C2 >= 1, "fp_mlp: C2 must be >= 1, got %lld", (long long)C2);
    O3DML_REQUIRE(B * n < (int64_t(1) << 31) && B * m < (int64_t(1) << 31),
                  "fp_mlp: B * n = %lld and B * m = %lld must be below 2^31", (long long)(B * n), (long long)(B * m));
    O3DML_REQUIRE(widths != nullptr, "fp_mlp: widths is null");
    FpPlan P;
    int64_t total = 0;
    if (!fp_plan(n_layers, widths, P, total)) throw Error{2};
    O3DML_REQUIRE(P.c0 == C2 + C1, "fp_mlp: c_0 = %d, but a row has %lld + %lld values", P.c0, (long long)C2,
                  (long long)C1);
    O3DML_REQUIRE((C1 > 0) == (unknown_feats != nullptr), "fp_mlp: unknown_feats must be given exactly when C1 > 0");
    O3DML_REQUIRE(packed_len == total, "fp_mlp: packed weights hold %lld floats, the widths need %lld",
                  (long long)packed_len, (long long)total);
    const int64_t rows = B * n;
    if (rows == 0) return 0;
    O3DML_REQUIRE(m >= 1, "fp_mlp: there are no known points");
    const size_t lds = fp_lds_bytes(P);
    O3DML_REQUIRE(lds <= kFpLdsMax, "fp_mlp: hidden widths need %zu bytes of LDS (limit %zu)", lds, kFpLdsMax);
    const int64_t tiles = ceil_div(rows, kFpR);
    const unsigned grid = static_cast<unsigned>(tiles < kFpGridMax ? tiles : kFpGridMax);
    hipStream_t st = as_stream(stream);
    static const bool attr =  // more than the default 64 KiB of dynamic LDS
        hipFuncSetAttribute(reinterpret_cast<const void*>(&fp_mlp_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            kFpLdsMax) == hipSuccess;
    O3DML_REQUIRE(attr || lds <= 64 * 1024, "fp_mlp: the device refused %zu bytes of LDS", lds);
    TimedRegion tr("fp_mlp", st);
    fp_mlp_kernel<<<grid, kFpThreads, lds, st>>>(known_feats, unknown_feats, dist2, idx, rows, n, m, static_cast<int>(C2),
                                                 static_cast<int>(C1), tiles, P, packed, out);
    O3DML_LAUNCH_CHECK();
    O3DML_GUARD_END
}
