// voxel_conv3d_grad.hip — the weight and bias gradients of the dense 3x3x3
// convolution of voxel_conv3d.hip (PVConv voxel_layers in training).  The data
// gradient needs no kernel of its own: it is voxel_conv3d on the transposed,
// flipped weights (ops.voxel_conv3d_grad_input).
//
// The contract.  Contiguous float32 in the layouts of voxel_conv3d.hip:
//   grid      [B,Cin,r,r,r]     the convolution's input
//   grad_out  [B,Cout,r,r,r]    gradient w.r.t. the convolution's output
//   dweight   [Cout,Cin,3,3,3]  = sum over b and (x,y,z) of grad_out[b,co,x,y,z]
//             * grid[b,ci,x+dx-1,y+dy-1,z+dz-1], positions outside the grid
//             counting as zeros (torch's Conv3d.weight layout)
//   dbias     [Cout] or null    = sum over b and voxels of grad_out[b,co,.]
// Products are exact f32 accumulated in f32 (v_mfma_f32_32x32x2_f32, k =
// voxels) in one fixed order: inside a slab the boxes ascending, inside a box
// the (y, z) positions ascending with the two x planes of the box as the two k
// of a step; then the slabs ascending.  No atomics, no memset: every element
// of dweight and dbias is written, the workspace needs no clearing, run to run
// the result is bitwise equal.  Inputs are finite.  Limits, returned as status
// before any launch: r in 1..1290, Cin in 1..2^24, Cout in 1..512, the number
// of boxes and the padded output below 2^31, the workspace as large as
// o3dml_voxel_conv3d_wgrad_workspace_size says.
//
// The slab rule.  With box = 2 x 4 x ZT voxels (ZT = 16 or 32, the one that
// pads r less, as the forward chooses), boxes = B * ceil(r/2) * ceil(r/4) *
// ceil(r/ZT) and blocks = ceil(Cout/32) * ceil(Cin/32):
//     S = min(ceil(256 / blocks), max(1, boxes / 2)), at least 1.
// Enough slabs that blocks * S reaches the 256 CUs, but never fewer than two
// boxes to a slab: a slab's partial block (108 KB written, read once more by
// the reduction) costs more traffic than a box's loads (up to 137 KB read).
// Slab s owns the boxes [s * boxes / S, (s + 1) * boxes / S) of the flat
// (batch, x, y, z) box list.  Workspace: S * blocks * 27 * 1024 floats of
// partial blocks plus S * ceil(Cout/32) * 32 of partial bias sums; blocks * S
// stays below 256 + blocks, so 128 -> 128 (16 blocks, S = 16) takes 28 MB and
// no shape with Cin, Cout <= 512 more than 57 MB.
//
// Design.  A GEMM dW[co, (tap, ci)] = sum over voxels v of
// grad_out[co, v] * grid[ci, v + off(tap)]: M = Cout, N = 27 Cin, K = B r^3.
//   block     a workgroup (4 waves) owns 32 output channels x 32 input channels
//             x all 27 taps and one slab of K: 27 accumulator tiles of 32 x 32.
//             Wave w owns the taps 7w .. 7w + 6 (wave 3: six taps), 7 tiles =
//             112 accumulator registers.  A = grad_out: row = lane & 31 = co;
//             B = grid at the tap's shift: column = lane & 31 = ci; lane >> 5
//             picks the k of the step.  A wave reads A once per k step and
//             uses it for its 7 tiles; its 7 B reads are 7 shifted views of
//             the one halo block in LDS, as the forward's taps are.
//   dbias     wave 3's seventh tile takes B = 1.0: every column of it is the
//             row sum of grad_out, on the MFMA that wave would otherwise idle
//             on, with no extra LDS read.  Only the workgroups of input-channel
//             block 0 store it (lane column 0), and only when dbias is asked.
//   k pairs   the two k of a step are the voxels (x0, y, z) and (x0 + 1, y, z)
//             of the box, not neighbours along z: see LDS.  One step per (y, z)
//             of the box plane, 4 * ZT steps a box.
//   per box   all 256 threads load the halo box (4 x 6 x (ZT + 2) positions) of
//             the 32 input channels, thread t owning the positions t, t + 256,
//             .. in each channel, and the plain box of the 32 grad_out
//             channels; a position outside the grid or a channel past Cin /
//             Cout is a zero, so all padding lives in the load.  Then the k
//             steps, the operands of step s + 1 read before the MFMAs of step
//             s.  The accumulators stay in registers from box to box; the
//             partial block is stored once per workgroup, tile by tile as
//             [tap][co][ci]: 32 lanes write 32 consecutive floats.
//   LDS       single-buffered: the two blocks of the 2 x 4 x 32 box take 152 KB
//             of the 160 KB, so there is no second buffer and one workgroup
//             per CU; loads and MFMAs of one workgroup do not overlap (two
//             barriers per box).  Double-buffering through registers would
//             hold 134 values per thread beside 112 accumulators; halving the
//             chunk to 16 input channels would double the reads of grad_out.
//             Neither was taken.
//             halo  [32][CS], a channel laid out [4][XS] with rows of YS =
//                   ZT + 2.   grad_out [32][GS], a channel laid out [2][PS].
//             A read is one ds_read_b32 in which lane & 31 walks channels and
//             lane >> 5 the two x planes.  CS and GS are odd, so the 32
//             channels of a half fall on 32 distinct banks; XS and PS are 32
//             (mod 64), so the other half lies 32 banks further: the 64
//             addresses are distinct counted over 64 banks as well as over 32
//             per half.  (Neighbours along z, one bank apart, would share 31
//             banks between the halves.)
//             ZT 32: YS 34, XS 224 (6 * 34 = 204 up), CS 897, PS 160, GS 321:
//             114,816 + 41,088 = 155,904 bytes.
//             ZT 16: YS 18, XS 160 (108 up), CS 641, PS 96, GS 193: 106,752.
//   grid      x = input-channel blocks, y = output-channel blocks, z = slabs.
//   reduce    voxel_conv3d_wgrad_reduce: one thread per element of the padded
//             block list, reading the slabs ascending (coalesced: consecutive
//             threads, consecutive floats) and writing dweight[co][ci][tap],
//             the transpose from tile order; the last ceil(Cout/32) * 32
//             threads do the same for dbias.
//   9 -> 64   the first layer fills 9 of the 32 columns of its tiles, so 72 %
//             of its MFMA work multiplies zeros.  No 16-wide column variant:
//             the layer is 2 % of the model's convolution arithmetic.
#include "common.hpp"

namespace o3dml {

constexpr int kVgThreads = 256;
constexpr int kVgCUs = 256;
constexpr int kVgMaxCout = 512;
constexpr int kVgTile = 27 * 1024;  // floats of a partial block
constexpr size_t kVgLdsMax = 160 * 1024;

typedef float vg_f32x16 __attribute__((ext_vector_type(16)));

template <int ZT>
struct VgGeom {
    static constexpr int TX = 2, TY = 4;
    static constexpr int HX = TX + 2, HY = TY + 2, HZ = ZT + 2;
    static constexpr int HALO = HX * HY * HZ;
    static constexpr int YS = HZ;
    static constexpr int XS = (HY * YS + 31) / 64 * 64 + 32;  // >= HY * YS, 32 (mod 64)
    static constexpr int CS = HX * XS + 1;                    // odd
    static constexpr int NP = (HALO + kVgThreads - 1) / kVgThreads;
    static constexpr int PLANE = TY * ZT;                     // k steps of a box
    static constexpr int PS = PLANE + 32;                     // 32 (mod 64) for 64 and 128
    static constexpr int GS = TX * PS + 1;                    // odd
    static constexpr int BOXV = TX * PLANE;
    static constexpr int GSTEP = kVgThreads / BOXV;           // grad_out channels per pass of the 256 threads
    static constexpr size_t LDS = sizeof(float) * 32 * (CS + GS);
    static_assert(XS % 64 == 32 && PS % 64 == 32 && CS % 2 == 1 && GS % 2 == 1, "bank layout");
    static_assert(BOXV <= kVgThreads && kVgThreads % BOXV == 0, "a thread owns one voxel of the grad_out box");
};

struct VgArgs {
    const float* in;
    const float* gout;
    float* ws;       // [S][cot][cit][27][32][32]
    float* wsb;      // [S][cot][32], null without dbias
    int Cin, Cout, r;
    int nbx, nby, nbz;
    int64_t boxes;
    int S;
};

template <int ZT>
__global__ void __launch_bounds__(kVgThreads) voxel_conv3d_wgrad_kernel(VgArgs a) {
    using G = VgGeom<ZT>;
    extern __shared__ float vg_lds[];
    float* xs = vg_lds;                // halo block [32][CS]
    float* gs = vg_lds + 32 * G::CS;   // grad_out block [32][GS]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int cit = blockIdx.x, cot = blockIdx.y, slab = blockIdx.z;
    const int r = a.r;
    const int64_t r3 = static_cast<int64_t>(r) * r * r;
    const int ci0 = cit * 32, co0 = cot * 32;
    const bool ones = wave == 3;  // slot 6 of wave 3 is the bias tile

    // this wave's 7 views of the halo block: tap = 7 wave + j at (dx, dy, dz); lane li's channel, plane lh
    int toff[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const int tap = ones && j == 6 ? 0 : 7 * wave + j;
        toff[j] = li * G::CS + (lh + tap / 9) * G::XS + tap / 3 % 3 * G::YS + tap % 3;
    }
    const int aoff = li * G::GS + lh * G::PS;

    vg_f32x16 acc[7];
#pragma unroll
    for (int j = 0; j < 7; ++j)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[j][q] = 0.f;

    const int64_t box_begin = a.boxes * slab / a.S, box_end = a.boxes * (slab + 1) / a.S;
    for (int64_t bx = box_begin; bx < box_end; ++bx) {
        int64_t box = bx;
        const int z0 = static_cast<int>(box % a.nbz) * ZT;
        box /= a.nbz;
        const int y0 = static_cast<int>(box % a.nby) * G::TY;
        box /= a.nby;
        const int x0 = static_cast<int>(box % a.nbx) * G::TX;
        const int64_t b = box / a.nbx;
        const float* __restrict__ inb = a.in + (b * a.Cin + ci0) * r3;
        const float* __restrict__ gob = a.gout + (b * a.Cout + co0) * r3;

        if (bx != box_begin) __syncthreads();  // the previous box is no longer read
        // halo block: positions tid + 256 i of a channel, in each of the 32 channels
#pragma unroll
        for (int i = 0; i < G::NP; ++i) {
            const int p = tid + kVgThreads * i;
            if (p >= G::HALO) break;
            const int hx = p / (G::HY * G::HZ), hy = p / G::HZ % G::HY, hz = p % G::HZ;
            const int x = x0 - 1 + hx, y = y0 - 1 + hy, z = z0 - 1 + hz;
            const bool ok = x >= 0 && x < r && y >= 0 && y < r && z >= 0 && z < r;
            const int goff = ok ? (x * r + y) * r + z : -1;
            float* dst = xs + hx * G::XS + hy * G::YS + hz;
#pragma unroll 8
            for (int c = 0; c < 32; ++c)
                dst[c * G::CS] = goff >= 0 && ci0 + c < a.Cin ? inb[c * r3 + goff] : 0.f;
        }
        // grad_out block: voxel tid % BOXV of the box, channels tid / BOXV + GSTEP i
        {
            const int v = tid % G::BOXV, vx = v / G::PLANE, vy = v / ZT % G::TY, vz = v % ZT;
            const int x = x0 + vx, y = y0 + vy, z = z0 + vz;
            const int goff = x < r && y < r && z < r ? (x * r + y) * r + z : -1;
            float* dst = gs + vx * G::PS + vy * ZT + vz;
#pragma unroll 8
            for (int c = tid / G::BOXV; c < 32; c += G::GSTEP)
                dst[c * G::GS] = goff >= 0 && co0 + c < a.Cout ? gob[c * r3 + goff] : 0.f;
        }
        __syncthreads();

        // k steps: s = y * ZT + z of the box plane; the halo view of (y, z) starts at y * YS + z
        auto load = [&](int s, float& av, float (&bv)[7]) {
            const int hoff = s / ZT * G::YS + s % ZT;
            av = gs[aoff + s];
#pragma unroll
            for (int j = 0; j < 7; ++j) bv[j] = xs[toff[j] + hoff];
            if (ones) bv[6] = 1.f;
        };
        auto mma = [&](float av, const float (&bv)[7]) {
#pragma unroll
            for (int j = 0; j < 7; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[j], acc[j], 0, 0, 0);
        };
        float a0, a1, b0[7], b1[7];
        load(0, a0, b0);
#pragma unroll 2
        for (int s = 0; s < G::PLANE - 2; s += 2) {
            load(s + 1, a1, b1);
            mma(a0, b0);
            load(s + 2, a0, b0);
            mma(a1, b1);
        }
        load(G::PLANE - 1, a1, b1);
        mma(a0, b0);
        mma(a1, b1);
    }

    // lane, register q of acc[j]: column li (ci), row (q & 3) + 8 (q >> 2) + 4 lh (co)
    const int64_t block = (static_cast<int64_t>(slab) * gridDim.y + cot) * gridDim.x + cit;
    float* __restrict__ out = a.ws + block * kVgTile;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        if (ones && j == 6) break;
        float* tile = out + (7 * wave + j) * 1024 + li;
#pragma unroll
        for (int q = 0; q < 16; ++q) tile[32 * ((q & 3) + 8 * (q >> 2) + 4 * lh)] = acc[j][q];
    }
    if (ones && cit == 0 && a.wsb != nullptr && li == 0) {
        float* bsum = a.wsb + (static_cast<int64_t>(slab) * gridDim.y + cot) * 32;
#pragma unroll
        for (int q = 0; q < 16; ++q) bsum[(q & 3) + 8 * (q >> 2) + 4 * lh] = acc[6][q];
    }
}

struct VgReduceArgs {
    const float* ws;
    const float* wsb;
    float* dweight;
    float* dbias;  // null: not asked for
    int Cin, Cout, cit_n, cot_n, S;
};

// thread i < total: element i of the padded block list [cot][cit][27][32][32]; the next cot_n * 32: dbias
__global__ void __launch_bounds__(256) voxel_conv3d_wgrad_reduce_kernel(VgReduceArgs a) {
    const int64_t total = static_cast<int64_t>(a.cot_n) * a.cit_n * kVgTile;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < total) {
        const int col = static_cast<int>(i & 31), row = static_cast<int>(i >> 5) & 31;
        const int64_t t = i >> 10;
        const int tap = static_cast<int>(t % 27), blk = static_cast<int>(t / 27);
        const int co = blk / a.cit_n * 32 + row, ci = blk % a.cit_n * 32 + col;
        if (co >= a.Cout || ci >= a.Cin) return;
        float sum = a.ws[i];
        for (int s = 1; s < a.S; ++s) sum += a.ws[s * total + i];
        a.dweight[(static_cast<int64_t>(co) * a.Cin + ci) * 27 + tap] = sum;
    } else if (a.dbias != nullptr) {
        const int64_t co = i - total;
        if (co >= a.Cout) return;
        const int64_t stride = static_cast<int64_t>(a.cot_n) * 32;
        float sum = a.wsb[co];
        for (int s = 1; s < a.S; ++s) sum += a.wsb[s * stride + co];
        a.dbias[co] = sum;
    }
}

struct VgPlan {
    int zt, nbx, nby, nbz, cit_n, cot_n, S;
    int64_t boxes, ws_floats;
};

// the box, the slab count and the workspace of (B, Cin, Cout, r); false when a limit is exceeded (message set)
static bool vg_plan(int64_t B, int64_t Cin, int64_t Cout, int64_t r, VgPlan& p) {
    if (B < 0) {
        set_error("voxel_conv3d_wgrad: B must not be negative");
        return false;
    }
    if (r < 1 || r > 1290) {
        set_error("voxel_conv3d_wgrad: r must be in 1..1290 (r^3 below 2^31), got %lld", (long long)r);
        return false;
    }
    if (Cout < 1 || Cout > kVgMaxCout) {
        set_error("voxel_conv3d_wgrad: Cout must be in 1..%d, got %lld", kVgMaxCout, (long long)Cout);
        return false;
    }
    if (Cin < 1 || Cin > (int64_t(1) << 24)) {
        set_error("voxel_conv3d_wgrad: Cin must be in 1..%d, got %lld", 1 << 24, (long long)Cin);
        return false;
    }
    p.zt = (r + 15) / 16 * 16 < (r + 31) / 32 * 32 ? 16 : 32;
    p.nbx = static_cast<int>(ceil_div(r, 2));
    p.nby = static_cast<int>(ceil_div(r, 4));
    p.nbz = static_cast<int>(ceil_div(r, p.zt));
    p.boxes = B * p.nbx * p.nby * p.nbz;
    p.cit_n = static_cast<int>(ceil_div(Cin, 32));
    p.cot_n = static_cast<int>(ceil_div(Cout, 32));
    const int64_t blocks = static_cast<int64_t>(p.cit_n) * p.cot_n;
    if (p.boxes >= (int64_t(1) << 31) || blocks * kVgTile >= (int64_t(1) << 31)) {
        set_error("voxel_conv3d_wgrad: %lld boxes of voxels and %lld padded gradient floats, the limit of each is "
                  "2^31 - 1", (long long)p.boxes, (long long)(blocks * kVgTile));
        return false;
    }
    int64_t S = ceil_div(kVgCUs, blocks);
    if (S > p.boxes / 2) S = p.boxes / 2;
    if (S < 1) S = 1;
    p.S = static_cast<int>(S);
    p.ws_floats = S * (blocks * kVgTile + p.cot_n * 32);
    return true;
}

template <int ZT>
static void vg_launch(const VgArgs& a, const VgPlan& p, hipStream_t st) {
    using G = VgGeom<ZT>;
    static_assert(G::LDS <= kVgLdsMax, "the halo and grad_out blocks must fit the LDS of a CU");
    static const bool attr =  // more than the default 64 KiB of dynamic LDS
        hipFuncSetAttribute(reinterpret_cast<const void*>(&voxel_conv3d_wgrad_kernel<ZT>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(G::LDS)) == hipSuccess;
    O3DML_REQUIRE(attr, "voxel_conv3d_wgrad: the device refused %zu bytes of LDS", G::LDS);
    const dim3 grid(static_cast<unsigned>(p.cit_n), static_cast<unsigned>(p.cot_n), static_cast<unsigned>(p.S));
    voxel_conv3d_wgrad_kernel<ZT><<<grid, kVgThreads, G::LDS, st>>>(a);
}

}  // namespace o3dml

using namespace o3dml;

O3DML_API int64_t o3dml_voxel_conv3d_wgrad_workspace_size(int64_t B, int64_t Cin, int64_t Cout, int64_t r) {
    VgPlan p{};
    return vg_plan(B, Cin, Cout, r, p) ? p.ws_floats : -1;
}

O3DML_API int o3dml_voxel_conv3d_wgrad(const float* grid, const float* grad_out, int64_t B, int64_t Cin, int64_t Cout,
                                       int64_t r, float* dweight, float* dbias, float* ws, int64_t ws_len,
                                       void* stream) {
    O3DML_GUARD_BEGIN
    VgPlan p{};
    if (!vg_plan(B, Cin, Cout, r, p)) throw Error{2};
    O3DML_REQUIRE(ws != nullptr && ws_len >= p.ws_floats,
                  "voxel_conv3d_wgrad: the workspace holds %lld floats, B %lld, %lld -> %lld at r %lld needs %lld",
                  (long long)ws_len, (long long)B, (long long)Cin, (long long)Cout, (long long)r,
                  (long long)p.ws_floats);
    const int64_t blocks = static_cast<int64_t>(p.cit_n) * p.cot_n;
    VgArgs a{};
    a.in = grid;
    a.gout = grad_out;
    a.ws = ws;
    a.wsb = dbias != nullptr ? ws + p.S * blocks * kVgTile : nullptr;
    a.Cin = static_cast<int>(Cin);
    a.Cout = static_cast<int>(Cout);
    a.r = static_cast<int>(r);
    a.nbx = p.nbx;
    a.nby = p.nby;
    a.nbz = p.nbz;
    a.boxes = p.boxes;
    a.S = p.S;
    hipStream_t st = as_stream(stream);
    {
        TimedRegion tr("voxel_conv3d_wgrad", st);
        if (p.zt == 32) vg_launch<32>(a, p, st);
        else vg_launch<16>(a, p, st);
        O3DML_LAUNCH_CHECK();
    }
    VgReduceArgs ra{a.ws, a.wsb, dweight, dbias, a.Cin, a.Cout, p.cit_n, p.cot_n, p.S};
    const int64_t threads = blocks * kVgTile + p.cot_n * 32;
    TimedRegion tr("voxel_conv3d_wgrad_reduce", st);
    voxel_conv3d_wgrad_reduce_kernel<<<static_cast<unsigned>(ceil_div(threads, 256)), 256, 0, st>>>(ra);
    O3DML_LAUNCH_CHECK();
    O3DML_GUARD_END
}
