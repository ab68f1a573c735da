// voxel_conv3d.hip — the dense 3x3x3 convolution of PVCNN's voxel branch with
// its folded BatchNorm and LeakyReLU in one kernel (ml3d/torch/models/pvcnn.py
// PVConv voxel_layers: Conv3d(k = 3, stride 1, padding 1) -> BatchNorm3d ->
// LeakyReLU(0.1), twice per block).
//
// The contract.  Contiguous float32:
//   grid    [B,Cin,r,r,r]   as o3dml_avg_voxelize_forward writes it, voxel
//                           (x,y,z) at (x*r + y)*r + z
//   packed  the weights of a Conv3d(Cin, Cout, 3, stride 1, padding 1) with the
//           BatchNorm already folded in, then the bias (layout below)
//   out     [B,Cout,r,r,r]  = act(bias[co] + sum over (ci, dx, dy, dz) of
//           W[co,ci,dx,dy,dz] * grid[b,ci,x+dx-1,y+dy-1,z+dz-1]), a
//           cross-correlation, positions outside the grid counting as zeros;
//           act(v) = v > 0 ? v : v * negative_slope, or v when no slope is given
// Products are exact f32 accumulated in f32 (v_mfma_f32_32x32x2_f32) in one
// fixed order of k: channel chunks of 8 ascending, inside a chunk the 27 taps
// ascending, inside a tap the channels ascending; the bias is added last.
// Every output element is written, nothing is accumulated across workgroups,
// there are no atomics and no memset: run-to-run bitwise equal, correct on an
// output that was not cleared.  Inputs are finite.  Limits, returned as status
// before any launch: r >= 1 with r^3 below 2^31, Cin >= 1, Cout in 1..512, the
// packed buffer below 2^31 floats, the number of workgroups below 2^31.
//
// Packed weights (o3dml_voxel_conv3d_packed_size floats): tap-major
// [27][kpad][cpad] with tap = (dx*3 + dy)*3 + dz, kpad = Cin rounded up to 8
// (the k loop's step), cpad = Cout rounded up to 32, then the bias [cpad]; the
// padding is zeros, so the inner loop has no special case for odd widths.
//
// Design.  An implicit GEMM out[co, v] = sum over (tap, ci) of
// W[co, ci, tap] * in[ci, v + off(tap)], K = 27 * Cin.
//   sides     Cout is the MFMA row side (the weights are the A operand), the
//             voxels are the column side (B operand).  A lane of the result
//             then holds one voxel (lane & 31) and 16 output channels, so one
//             store instruction writes, per output channel, 32 consecutive
//             voxels along z: two 128-byte runs per instruction and no trip
//             through LDS.  With voxels on the row side a store would put 32
//             channels of one voxel r^3 floats apart.  The weights' operand
//             load is the run of 32 consecutive floats [tap][ci][co .. co+32)
//             of the packed buffer.
//   tile      32 voxels: ZT = 32 along z of one y row, or ZT = 16 along z of
//             two adjacent y rows (the r = 16 grids: 32 contiguous floats of
//             the output all the same).  ZT is the one that pads r less.
//   workgroup 4 waves (256 threads) own a box of TX x TY x ZT output voxels of
//             one batch item and NC row tiles of 32 output channels:
//             wave w owns NV voxel tiles and all NC channel tiles, an NC x NV
//             block of accumulators, so one weight load feeds NV MFMAs and one
//             LDS read NC.  Boxes: ZT 32: 2 x 4 x 32 (NV 2), 2 x 2 x 32 (NV 1);
//             ZT 16: 4 x 4 x 16 (NV 2), 2 x 4 x 16 (NV 1).  grid.x walks the
//             boxes, grid.y the groups of NC channel tiles.
//   rule      NC = 4, 2 or 1 for at least 4, 2, 1 channel tiles; NV = 2.  While
//             boxes * groups is below the 256 CUs, first NV drops to 1 (half
//             the box, the halo's share goes up), then NC halves (Cout split
//             across workgroups, each reading the input again).  At B = 8 the
//             r = 32 layers run 1024 boxes of 2 x 4 x 32, the r = 16 layers 256
//             workgroups of 2 x 4 x 16 with all of Cout.  K is never split.
//   stream    the input comes in chunks of 8 channels.  A chunk's halo box,
//             (TX + 2)(TY + 2)(ZT + 2) voxels per channel, is loaded by all
//             256 threads: thread t owns the positions t, t + 256, .. of the
//             box in flat order (z fastest: runs of ZT + 2 consecutive floats)
//             in each of the 8 channels, so its offsets are computed once per
//             workgroup; a position outside the grid or a channel past Cin is
//             a zero, so the padding lives in the load and the 27 taps are 27
//             shifted views of the same block.  An input value is read once
//             per workgroup (plus halo) and used 27 * 32 * NC times.
//   overlap   double-buffered as in fp_mlp.hip: the loads of chunk c + 1 go
//             into registers before the MFMAs of chunk c and into the other
//             buffer after them; one barrier per chunk.
//   LDS       [8][CS] per buffer, a channel laid out [TX + 2][TY + 2][YS].  A
//             B read is one ds_read_b32: lanes 0..31 take k, lanes 32..63
//             k + 1, lane & 31 the voxel.  Banks are 4 bytes wide.
//             ZT 32: YS = 34; 32 addresses at stride 1 are 32 distinct banks.
//             ZT 16: YS = 48: the two rows start 48 = 16 (mod 32) apart, so
//             they cover banks [s, s + 16) and [s + 16, s + 32): distinct.
//             (YS = 18 would put two banks under both rows.)
//             CS = the channel's size rounded up to 32 (mod 64): the k + 1
//             half lies 32 banks from the k half, so the 64 addresses are
//             distinct counted over 64 banks as well as over 32 per half.
//             Bytes: 2 * 8 * CS * 4 = 54 KB (2 x 4 x 32), 74 KB (2 x 4 x 16),
//             110 KB (4 x 4 x 16).
//   weights   from L2 straight into registers; the largest layer's are
//             1.8 MB and every workgroup reads the same ones.
//   pipeline  per tap 4 k steps; the 4 (NC + NV) operand loads of tap t + 1
//             are issued before the 4 NC NV MFMAs of tap t.
//   epilogue  bias and LeakyReLU in the accumulators, then the stores above.
//             Each is one rounded f32 operation whether the compiler packs two
//             lanes' worth into one instruction or not, so this file needs no
//             -packed-fp32-ops line in the Makefile.
#include "common.hpp"

namespace o3dml {

constexpr int kVcThreads = 256;
constexpr int kVcWaves = kVcThreads / 64;
constexpr int kVcKC = 8;           // channels of a chunk = 4 k steps
constexpr int kVcMaxCout = 512;
constexpr int kVcCUs = 256;        // workgroups the rule wants at least
constexpr size_t kVcLdsMax = 160 * 1024;

typedef float vc_f32x16 __attribute__((ext_vector_type(16)));

template <int ZT, int NV>
struct VcGeom {
    static constexpr int YT = 32 / ZT;                                // y rows of a tile
    static constexpr int NT = kVcWaves * NV;                          // tiles of a box
    static constexpr int TYT = ZT == 32 ? (NV == 2 ? 4 : 2) : 2;      // tiles along y
    static constexpr int TX = NT / TYT, TY = TYT * YT;
    static constexpr int HX = TX + 2, HY = TY + 2, HZ = ZT + 2;
    static constexpr int HALO = HX * HY * HZ;                         // values of a channel
    static constexpr int YS = ZT == 32 ? HZ : 48;
    static constexpr int XS = HY * YS;
    static constexpr int CS = (HX * XS + 31) / 64 * 64 + 32;          // >= HX * XS, 32 (mod 64)
    static constexpr int NP = (HALO + kVcThreads - 1) / kVcThreads;   // positions of a channel per thread
    static constexpr size_t LDS = sizeof(float) * 2 * kVcKC * CS;
};

struct VcArgs {
    const float* in;
    const float* packed;
    float* out;
    int Cin, Cout, r, kpad, cpad;
    int nbx, nby, nbz;
    float slope;
    int has_slope;
};

template <int ZT, int NV, int NC>
__global__ void __launch_bounds__(kVcThreads) voxel_conv3d_kernel(VcArgs a) {
    using G = VcGeom<ZT, NV>;
    constexpr int KC = kVcKC;
    extern __shared__ float vc_lds[];  // two buffers [KC][CS]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int ly = ZT == 32 ? 0 : li >> 4, lz = ZT == 32 ? li : li & 15;
    int box = blockIdx.x;
    const int z0 = (box % a.nbz) * ZT;
    box /= a.nbz;
    const int y0 = (box % a.nby) * G::TY;
    box /= a.nby;
    const int x0 = (box % a.nbx) * G::TX;
    const int b = box / a.nbx;
    const int r = a.r;
    const int64_t r3 = static_cast<int64_t>(r) * r * r;
    const float* __restrict__ inb = a.in + static_cast<int64_t>(b) * a.Cin * r3;

    // A thread owns the positions p = tid + 256 i of a channel's halo box in every channel of a chunk: where
    // they lie in a channel of the grid (-1: outside it, a zero) and in a channel of the LDS block (-1: no such p)
    int goff[G::NP], loff[G::NP];
#pragma unroll
    for (int i = 0; i < G::NP; ++i) {
        const int p = tid + kVcThreads * i;
        const int hx = p / (G::HY * G::HZ), hy = p / G::HZ % G::HY, hz = p % G::HZ;
        const int x = x0 - 1 + hx, y = y0 - 1 + hy, z = z0 - 1 + hz;
        const bool ok = p < G::HALO && x >= 0 && x < r && y >= 0 && y < r && z >= 0 && z < r;
        goff[i] = ok ? (x * r + y) * r + z : -1;
        loff[i] = p < G::HALO ? hx * G::XS + hy * G::YS + hz : -1;
    }
    auto chunk_load = [&](int k0, float (&f)[KC][G::NP]) {
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            const float* __restrict__ ch = inb + (k0 + k) * r3;
            const bool live = k0 + k < a.Cin;
#pragma unroll
            for (int i = 0; i < G::NP; ++i) f[k][i] = live && goff[i] >= 0 ? ch[goff[i]] : 0.f;
        }
    };
    auto chunk_store = [&](float* buf, const float (&f)[KC][G::NP]) {
#pragma unroll
        for (int k = 0; k < KC; ++k)
#pragma unroll
            for (int i = 0; i < G::NP; ++i)
                if (loff[i] >= 0) buf[k * G::CS + loff[i]] = f[k][i];
    };

    // this lane's voxel of tile j in the halo block (tap 0, channel lh), and its column of channel tile i
    const int ctiles = a.cpad / 32, tile0 = blockIdx.y * NC;
    int xoff[NV];
    unsigned woff[NC];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int t = wave * NV + j;
        xoff[j] = lh * G::CS + t / G::TYT * G::XS + (t % G::TYT * G::YT + ly) * G::YS + lz;
    }
#pragma unroll
    for (int i = 0; i < NC; ++i) {  // a tile past the last repeats it and is not stored
        const int tile = tile0 + i < ctiles ? tile0 + i : ctiles - 1;
        woff[i] = lh * a.cpad + 32 * tile + li;
    }

    vc_f32x16 acc[NC][NV];
#pragma unroll
    for (int i = 0; i < NC; ++i)
#pragma unroll
        for (int j = 0; j < NV; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;

    float f[KC][G::NP];
    chunk_load(0, f);
    chunk_store(vc_lds, f);
    __syncthreads();

    const int nchunk = a.kpad / KC;
    const int64_t tapstride = static_cast<int64_t>(a.kpad) * a.cpad;
    for (int c = 0; c < nchunk; ++c) {
        const bool more = c + 1 < nchunk;
        if (more) chunk_load((c + 1) * KC, f);
        const float* xb = vc_lds + (c & 1) * KC * G::CS;
        const float* __restrict__ wb = a.packed + static_cast<int64_t>(c) * KC * a.cpad;
        // the operands of a tap's 4 k steps
        auto load = [&](int tap, float (&wv)[4][NC], float (&xv)[4][NV]) {
            const int toff = tap / 9 * G::XS + tap / 3 % 3 * G::YS + tap % 3;
            const float* __restrict__ wt = wb + tap * tapstride;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
#pragma unroll
                for (int i = 0; i < NC; ++i) wv[s][i] = (wt + 2 * s * a.cpad)[woff[i]];
#pragma unroll
                for (int j = 0; j < NV; ++j) xv[s][j] = xb[xoff[j] + toff + 2 * s * G::CS];
            }
        };
        auto mma = [&](const float (&wv)[4][NC], const float (&xv)[4][NV]) {
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int i = 0; i < NC; ++i)
#pragma unroll
                    for (int j = 0; j < NV; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[s][i], xv[s][j], acc[i][j], 0, 0, 0);
        };
        float w0[4][NC], x0v[4][NV], w1[4][NC], x1v[4][NV];
        load(0, w0, x0v);
#pragma unroll 1
        for (int tap = 0; tap < 26; tap += 2) {
            load(tap + 1, w1, x1v);
            mma(w0, x0v);
            load(tap + 2, w0, x0v);
            mma(w1, x1v);
        }
        mma(w0, x0v);  // tap 26
        if (more) chunk_store(vc_lds + ((c + 1) & 1) * KC * G::CS, f);
        __syncthreads();  // chunk c + 1 is written, chunk c no longer read
    }

    // lane, register q of acc[i][j]: voxel li of tile wave * NV + j, channel 32 tile + (q & 3) + 8 (q >> 2) + 4 lh
    const float* __restrict__ bias = a.packed + 27 * tapstride;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        if (tile0 + i >= ctiles) break;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int t = wave * NV + j;
            const int x = x0 + t / G::TYT, y = y0 + t % G::TYT * G::YT + ly, z = z0 + lz;
            const bool inside = x < r && y < r && z < r;
            float* dst = a.out + static_cast<int64_t>(b) * a.Cout * r3 + (static_cast<int64_t>(x) * r + y) * r + z;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int co = 32 * (tile0 + i) + (q & 3) + 8 * (q >> 2) + 4 * lh;
                float v = acc[i][j][q] + bias[co];
                if (a.has_slope) v = v > 0.f ? v : v * a.slope;
                if (inside && co < a.Cout) dst[co * r3] = v;
            }
        }
    }
}

// (Cin, Cout) -> padded widths and the packed length; false when a limit is exceeded (message set)
static bool vc_plan(int64_t Cin, int64_t Cout, int& kpad, int& cpad, int64_t& total) {
    if (Cout < 1 || Cout > kVcMaxCout) {
        set_error("voxel_conv3d: Cout must be in 1..%d, got %lld", kVcMaxCout, (long long)Cout);
        return false;
    }
    if (Cin < 1 || Cin > (int64_t(1) << 24)) {
        set_error("voxel_conv3d: Cin must be in 1..%d, got %lld", 1 << 24, (long long)Cin);
        return false;
    }
    kpad = static_cast<int>((Cin + kVcKC - 1) / kVcKC * kVcKC);
    cpad = static_cast<int>((Cout + 31) / 32 * 32);
    total = 27 * static_cast<int64_t>(kpad) * cpad + cpad;
    if (total >= (int64_t(1) << 31)) {
        set_error("voxel_conv3d: the packed weights of %lld -> %lld hold %lld floats, the limit is 2^31 - 1",
                  (long long)Cin, (long long)Cout, (long long)total);
        return false;
    }
    return true;
}

template <int ZT, int NV, int NC>
static void vc_launch(const VcArgs& a, int64_t B, int groups, hipStream_t st) {
    using G = VcGeom<ZT, NV>;
    static_assert(G::LDS <= kVcLdsMax, "the two chunk buffers must fit the LDS of a CU");
    static const bool attr =  // more than the default 64 KiB of dynamic LDS
        G::LDS <= 64 * 1024 ||
        hipFuncSetAttribute(reinterpret_cast<const void*>(&voxel_conv3d_kernel<ZT, NV, NC>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(G::LDS)) == hipSuccess;
    O3DML_REQUIRE(attr, "voxel_conv3d: the device refused %zu bytes of LDS", G::LDS);
    const dim3 grid(static_cast<unsigned>(B * a.nbx * a.nby * a.nbz), static_cast<unsigned>(groups));
    voxel_conv3d_kernel<ZT, NV, NC><<<grid, kVcThreads, G::LDS, st>>>(a);
}

}  // namespace o3dml

using namespace o3dml;

O3DML_API int64_t o3dml_voxel_conv3d_packed_size(int64_t Cin, int64_t Cout) {
    int kpad, cpad;
    int64_t total = 0;
    return vc_plan(Cin, Cout, kpad, cpad, total) ? total : -1;
}

O3DML_API int o3dml_voxel_conv3d(const float* grid, const float* packed, int64_t packed_len, int64_t B, int64_t Cin,
                                 int64_t Cout, int64_t r, int has_slope, float negative_slope, float* out,
                                 void* stream) {
    O3DML_GUARD_BEGIN
    O3DML_REQUIRE(B >= 0, "voxel_conv3d: B must not be negative");
    O3DML_REQUIRE(r >= 1 && r <= 1290, "voxel_conv3d: r must be in 1..1290 (r^3 below 2^31), got %lld", (long long)r);
    VcArgs a{};
    int64_t total = 0;
    if (!vc_plan(Cin, Cout, a.kpad, a.cpad, total)) throw Error{2};
    O3DML_REQUIRE(packed_len == total, "voxel_conv3d: packed weights hold %lld floats, %lld -> %lld needs %lld",
                  (long long)packed_len, (long long)Cin, (long long)Cout, (long long)total);
    if (B == 0) return 0;
    // the tile: the ZT that pads r less; the block: as large as still gives every CU a workgroup
    const int zt = (r + 15) / 16 * 16 < (r + 31) / 32 * 32 ? 16 : 32;
    const int ctiles = a.cpad / 32;
    int nv = 2, nc = ctiles >= 4 ? 4 : (ctiles >= 2 ? 2 : 1);
    int64_t boxes = 0;
    int groups = 0;
    for (;;) {
        const int tyt = zt == 32 ? (nv == 2 ? 4 : 2) : 2;
        const int tx = kVcWaves * nv / tyt, ty = tyt * (32 / zt);
        a.nbx = static_cast<int>(ceil_div(r, tx));
        a.nby = static_cast<int>(ceil_div(r, ty));
        a.nbz = static_cast<int>(ceil_div(r, zt));
        boxes = B * a.nbx * a.nby * a.nbz;
        groups = (ctiles + nc - 1) / nc;
        if (boxes * groups >= kVcCUs) break;
        if (nv == 2) nv = 1;
        else if (nc > 1) nc /= 2;
        else break;
    }
    O3DML_REQUIRE(boxes < (int64_t(1) << 31), "voxel_conv3d: %lld boxes of output voxels, the limit is 2^31 - 1",
                  (long long)boxes);
    a.in = grid;
    a.packed = packed;
    a.out = out;
    a.Cin = static_cast<int>(Cin);
    a.Cout = static_cast<int>(Cout);
    a.r = static_cast<int>(r);
    a.slope = negative_slope;
    a.has_slope = has_slope != 0;
    hipStream_t st = as_stream(stream);
    TimedRegion tr("voxel_conv3d", st);
#define VC_CASE(ZT, NV, NC) \
    if (zt == ZT && nv == NV && nc == NC) vc_launch<ZT, NV, NC>(a, B, groups, st)
    VC_CASE(32, 2, 4); VC_CASE(32, 2, 2); VC_CASE(32, 2, 1); VC_CASE(32, 1, 4); VC_CASE(32, 1, 2); VC_CASE(32, 1, 1);
    VC_CASE(16, 2, 4); VC_CASE(16, 2, 2); VC_CASE(16, 2, 1); VC_CASE(16, 1, 4); VC_CASE(16, 1, 2); VC_CASE(16, 1, 1);
#undef VC_CASE
    O3DML_LAUNCH_CHECK();
    O3DML_GUARD_END
}
