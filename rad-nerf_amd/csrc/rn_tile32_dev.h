// rn_tile32_dev.h -- the fp32 matrix-core machine on 32-sample tiles, shared by the inference kernel (rn_fused.hip), the
// fused training network (rn_train_head.hip; rn_train_head_f16.hip and the backward walk both arithmetics share,
// rn_train_head_walk_dev.h, keep the tiles and their VALU rows), the torso layer (rn_torso.hip, rn_train_torso.hip) and
// the per-MLP training kernels (rn_mlp.hip).
//
// One wavefront owns 32 samples.  v_mfma_f32_32x32x2_f32 puts the output row on the register index and the sample on the
// lane, so the accumulators of a 64-row layer (two row tiles of 16 registers) ARE the B operand of the next layer; the k
// order that results (kmap) is baked into the packed weight images.  A "native tile" in memory is that register layout
// spelled out: [2 row tiles][16 registers][64 lanes] floats, every row a coalesced 256-B store.
#pragma once

#include "rn_common.h"

namespace rn {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// Output row (within a 32-row tile) that register r of lane half h holds.
__host__ __device__ constexpr int rowmap(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
// k index (within a 64-wide hidden vector) that lane-half h feeds at MFMA step s when the B operand is
// register (s & 15) of row tile (s >> 4) of the previous layer's accumulators.
__host__ __device__ constexpr int kmap(int s, int h) { return 32 * (s >> 4) + rowmap(s & 15, h); }

// floats per MFMA step of a 64-row layer in a packed weight image: [2 h][32 j][2 row tiles] -> lane (j, h) reads one float2
constexpr int kStep = 128;
// the same for a 32-row layer (one row tile): [2 h][32 j] -> lane (j, h) reads one float
constexpr int kS32 = 64;

// max(x, 0) as ONE v_max_i32 on the bit pattern (a non-negative float is a non-negative integer, a negative one a negative
// integer); fmaxf(x, 0) costs two VALU instructions because IEEE mode first quiets a possible signalling NaN.
__device__ __forceinline__ float relu_bits(float x) {
    const int b = __float_as_int(x);
    return __int_as_float(b > 0 ? b : 0);
}

__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
#ifdef RN_EXP_NO_MFMA  // experiment only: keep the data dependence, drop the matrix instruction
    c[0] += a * b;
    return c;
#else
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
#endif
}

// Accumulators of one 64-row layer for the 32 samples of a tile: [row tile], row on the register index, sample on the lane.
struct Acc32 {
    f32x16 v[2];
};

__device__ __forceinline__ void acc_zero(Acc32 &a) {
#pragma unroll
    for (int rt = 0; rt < 2; rt++)
#pragma unroll
        for (int r = 0; r < 16; r++) a.v[rt][r] = 0.0f;
}
// accumulator rows of lane half h: 32 rt + rowmap(r, h) -> four consecutive floats per r >> 2
__device__ __forceinline__ void acc_bias(Acc32 &a, const float *bias64, int h) {
#pragma unroll
    for (int rt = 0; rt < 2; rt++)
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const float4 b = *reinterpret_cast<const float4 *>(bias64 + 32 * rt + 8 * g + 4 * h);
            a.v[rt][4 * g + 0] = b.x; a.v[rt][4 * g + 1] = b.y; a.v[rt][4 * g + 2] = b.z; a.v[rt][4 * g + 3] = b.w;
        }
}
__device__ __forceinline__ void acc_relu(Acc32 &a) {
#pragma unroll
    for (int rt = 0; rt < 2; rt++)
#pragma unroll
        for (int r = 0; r < 16; r++) a.v[rt][r] = relu_bits(a.v[rt][r]);
}

// one MFMA step of a 64-row layer: weights of step s from LDS (one float2 = both row tiles), B operand b
__device__ __forceinline__ void step32(Acc32 &a, const float *wl, int s, int lane_off, float b) {
    const float2 w = *reinterpret_cast<const float2 *>(wl + s * kStep + lane_off);
    a.v[0] = mfma32(w.x, b, a.v[0]);
    a.v[1] = mfma32(w.y, b, a.v[1]);
}

// 64 -> 64 layer whose input is the previous layer's accumulators (32 steps)
__device__ __forceinline__ void layer_from_acc(Acc32 &out, const Acc32 &in, const float *wl, int lane_off) {
#pragma unroll
    for (int s = 0; s < 32; s++) step32(out, wl, s, lane_off, in.v[s >> 4][s & 15]);
}

// out[o] = sum_k in[k] * W[o][k]: each lane half sums the k's it holds, one cross-half shuffle adds the other half's
template <int NOUT>
__device__ __forceinline__ void valu_out(const Acc32 &in, const float *wl, int h, float (&out)[NOUT]) {
#pragma unroll
    for (int o = 0; o < NOUT; o++) {
        float p = 0.0f;
        const float *wo = wl + (o * 2 + h) * 32;
#pragma unroll
        for (int g = 0; g < 8; g++) {
            const float4 w = *reinterpret_cast<const float4 *>(wo + 4 * g);
            const int rt = g >> 2, r = (g & 3) * 4;
            p = __builtin_fmaf(in.v[rt][r + 0], w.x, p);
            p = __builtin_fmaf(in.v[rt][r + 1], w.y, p);
            p = __builtin_fmaf(in.v[rt][r + 2], w.z, p);
            p = __builtin_fmaf(in.v[rt][r + 3], w.w, p);
        }
        out[o] = p + __shfl_xor(p, 32, 64);
    }
}

// the backward pass of valu_out: g[k] += sum_o W[o][k] d[o] for the k's this lane holds (the transposed narrow layer)
template <int NOUT>
__device__ __forceinline__ void valu_out_T(Acc32 &g, const float *wl, int h, const float (&d)[NOUT]) {
#pragma unroll
    for (int o = 0; o < NOUT; o++) {
        const float *wo = wl + (o * 2 + h) * 32;
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const float4 w = *reinterpret_cast<const float4 *>(wo + 4 * q);
            const int rt = q >> 2, r = (q & 3) * 4;
            g.v[rt][r + 0] = __builtin_fmaf(w.x, d[o], g.v[rt][r + 0]);
            g.v[rt][r + 1] = __builtin_fmaf(w.y, d[o], g.v[rt][r + 1]);
            g.v[rt][r + 2] = __builtin_fmaf(w.z, d[o], g.v[rt][r + 2]);
            g.v[rt][r + 3] = __builtin_fmaf(w.w, d[o], g.v[rt][r + 3]);
        }
    }
}
// the backward pass of a ReLU: g = (saved activation > 0) ? g : 0, the saved native tile read row by row
__device__ __forceinline__ void relu_mask(Acc32 &g, const float *__restrict__ saved, int lane) {
    float hv[32];
#pragma unroll
    for (int q = 0; q < 32; q++) hv[q] = saved[q * 64 + lane];
#pragma unroll
    for (int rt = 0; rt < 2; rt++)
#pragma unroll
        for (int r = 0; r < 16; r++) g.v[rt][r] = hv[rt * 16 + r] > 0.0f ? g.v[rt][r] : 0.0f;
}

// accumulators <-> native tile
__device__ __forceinline__ void tile_store(float *__restrict__ dst, const Acc32 &a, int lane) {
#pragma unroll
    for (int rt = 0; rt < 2; rt++)
#pragma unroll
        for (int r = 0; r < 16; r++) dst[(rt * 16 + r) * 64 + lane] = a.v[rt][r];
}
__device__ __forceinline__ void tile_load(const float *__restrict__ src, Acc32 &a, int lane) {
#pragma unroll
    for (int rt = 0; rt < 2; rt++)
#pragma unroll
        for (int r = 0; r < 16; r++) a.v[rt][r] = src[(rt * 16 + r) * 64 + lane];
}

// ---- 32-row layers: one row tile of 16 registers
__device__ __forceinline__ f32x16 zero16() {
    f32x16 a;
#pragma unroll
    for (int r = 0; r < 16; r++) a[r] = 0.0f;
    return a;
}
__device__ __forceinline__ void store16(float *__restrict__ dst, const f32x16 &a, int lane) {
#pragma unroll
    for (int r = 0; r < 16; r++) dst[r * 64 + lane] = a[r];
}
__device__ __forceinline__ void relu_mask16(f32x16 &g, const float *__restrict__ saved, int lane) {
    float hv[16];
#pragma unroll
    for (int r = 0; r < 16; r++) hv[r] = saved[r * 64 + lane];
#pragma unroll
    for (int r = 0; r < 16; r++) g[r] = hv[r] > 0.0f ? g[r] : 0.0f;
}

}  // namespace rn
