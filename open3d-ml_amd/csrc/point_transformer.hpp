// point_transformer.hpp — what the forward kernels (point_transformer.hip) and
// the backward kernels (point_transformer_grad.hip) of PointTransformer share:
// the positional encoding's device functions (so both recompute the same
// bits), the 16-byte / one-channel row access and the argument checks.
#pragma once

#include <cmath>
#include <initializer_list>

#include "common.hpp"

namespace o3dml {

constexpr int kPtBlock = 256;

// linear_p[0..2]: Linear(3,3), BatchNorm1d(3) folded to sc / sh, ReLU
struct PtPos {
    const float* w1;  // [3,3]
    const float* b1;  // [3]
    const float* sc;  // [3]
    const float* sh;  // [3]
    const float* w2;  // [c,3]  linear_p[3]
    const float* b2;  // [c]
};

struct PtPosRegs {
    float w1[9], b1[3], sc[3], sh[3];
};

__device__ __forceinline__ PtPosRegs pos_load(const PtPos& p) {
    PtPosRegs r;
#pragma unroll
    for (int a = 0; a < 9; ++a) r.w1[a] = p.w1[a];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        r.b1[a] = p.b1[a];
        r.sc[a] = p.sc[a];
        r.sh[a] = p.sh[a];
    }
    return r;
}

__device__ __forceinline__ void pos_hidden(const PtPosRegs& r, float dx, float dy, float dz, float (&h)[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float l = __builtin_fmaf(r.w1[3 * a + 2], dz, __builtin_fmaf(r.w1[3 * a + 1], dy, r.w1[3 * a] * dx)) +
                        r.b1[a];
        h[a] = fmaxf(r.sc[a] * l + r.sh[a], 0.f);
    }
}

__device__ __forceinline__ float pos_channel(const float (&w2)[3], float b2, const float (&h)[3]) {
    return __builtin_fmaf(w2[2], h[2], __builtin_fmaf(w2[1], h[1], w2[0] * h[0])) + b2;
}

template <int VEC>
__device__ __forceinline__ void load_vec(const float* __restrict__ p, float (&v)[VEC]) {
    if constexpr (VEC == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) v[e] = p[e];
    }
}

template <int VEC>
__device__ __forceinline__ void store_vec(float* __restrict__ p, const float (&v)[VEC]) {
    if constexpr (VEC == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) p[e] = v[e];
    }
}

// what a lane keeps of the positional encoding for its VEC channels
template <int VEC>
struct PtLane {
    PtPosRegs pr;
    float w2[VEC][3], b2[VEC];
    float qx, qy, qz;
    __device__ __forceinline__ void init(const PtPos& p, const float* __restrict__ xyz_q, int64_t i, int ch) {
        pr = pos_load(p);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
#pragma unroll
            for (int a = 0; a < 3; ++a) w2[e][a] = p.w2[3 * (ch + e) + a];
            b2[e] = p.b2[ch + e];
        }
        qx = xyz_q[3 * i];
        qy = xyz_q[3 * i + 1];
        qz = xyz_q[3 * i + 2];
    }
    __device__ __forceinline__ void encode(const float* __restrict__ xyz_s, int64_t s, float (&p)[VEC]) const {
        float h[3];
        pos_hidden(pr, xyz_s[3 * s] - qx, xyz_s[3 * s + 1] - qy, xyz_s[3 * s + 2] - qz, h);
#pragma unroll
        for (int e = 0; e < VEC; ++e) p[e] = pos_channel(w2[e], b2[e], h);
    }
};

inline bool aligned16(std::initializer_list<const void*> ps) {
    for (const void* p : ps)
        if (reinterpret_cast<uintptr_t>(p) & 15) return false;
    return true;
}

inline unsigned pt_grid(int64_t lanes) { return static_cast<unsigned>(ceil_div(lanes, kPtBlock)); }

inline void pt_check_layer(const char* what, int64_t n, int64_t nsample, int64_t c) {
    O3DML_REQUIRE(n >= 0 && n < (int64_t(1) << 31), "%s: n = %lld out of range", what, (long long)n);
    O3DML_REQUIRE(nsample >= 1 && nsample <= 64, "%s: nsample must be in 1..64, got %lld", what, (long long)nsample);
    O3DML_REQUIRE(c >= 1 && c <= 65536, "%s: c must be in 1..65536, got %lld", what, (long long)c);
}

}  // namespace o3dml
