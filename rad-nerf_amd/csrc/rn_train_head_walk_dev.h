// rn_train_head_walk_dev.h -- the backward tile walk of the fused training network, written once for both arithmetics
// (rn_train_head.hip: fp32 matrix cores; rn_train_head_f16.hip: 16-bit operands, fp32 sums).
//
// One wavefront owns 32 samples and walks the saved tile back.  Everything here is fp32 and the same for both arithmetics:
// the live count, sigmoid' / trunc_exp' / tanh' from the saved outputs, the ReLU masks from the saved activations, the
// narrow layers (VALU rows), dy_dx of the ambient grid, and every store -- the pre-activation gradients of the workspace
// (rn_train_head_dev.h) and the level-major feature gradients have ONE writer text.  An arithmetic A supplies only the places
// where a weight fragment meets a B operand:
//   kLdsBwd, fill_bwd(lds, image)     floats of LDS, and the copy of the transposed weights and the narrow rows into it
//   RT_C1, RT_S2R, RT_A2              where the narrow rows sit in that LDS
//   layer_T(out, dy, WT_*)            out = W^T dy (WT_C0, WT_S2, WT_S1, WT_A1; WT_S0: row tile 0 = d enc_x, 1 = d enc_w)
//   a0_T(x0, dz)                      x0 += W_amb0[:, 0:32]^T dz, the 32-row contribution of ambient L0 to d enc_x
// The order of floating-point operations per value is the arithmetic's own and the build has -ffp-contract=off: whatever the
// schedule, the bits are those of the two kernels each arithmetic used to spell out.  The parameter block is taken by value
// (a reference handed to a helper made the compiler keep the block in memory: DESIGN.md on the inference tile loops).
// The FORWARD walk stays two kernel bodies (k_train_fwd, k_train_fwd_h16): written once on an arithmetic like this one,
// k_train_fwd_h16 measured 1 to 2 % slower than its own body ("One backward walk"); they share select_h below.
#pragma once

#include "rn_train_head_dev.h"

namespace rn {
namespace th {

__device__ __forceinline__ float select_h(float lo, float hi, int h) {   // h ? hi : lo without a dynamic register index
    const uint32_t m = 0u - (uint32_t)h;
    return __uint_as_float((__float_as_uint(lo) & ~m) | (__float_as_uint(hi) & m));
}

template <class A>
__device__ __forceinline__ void train_bwd_tiles(BwdParams p, float *lds) {
    const uint32_t M = live_count(p.M, p.m_dev);
    const uint32_t n_tiles = (M + 31u) >> 5;
    if (blockIdx.x * kWaves >= n_tiles) return;
    A::fill_bwd(lds, p.image);
    __syncthreads();
    const Ws ws = make_ws(p.ws, p.M);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, h = lane >> 5;
    const A ar(lds, j, h);

    for (uint32_t tile = blockIdx.x * kWaves + wave; tile < n_tiles; tile += gridDim.x * kWaves) {
        const uint32_t sample = tile * 32 + j;
        const bool live = sample < M;
        Acc32 g, w;
        // ---- colour net: sigmoid', last layer transposed (VALU rows), ReLU mask
        {
            float d[3] = {0.0f, 0.0f, 0.0f};
            if (live) {
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const float y = p.rgbs[3 * (size_t)sample + c];
                    d[c] = p.g_rgbs[3 * (size_t)sample + c] * ((1.0f - y) * y);
                }
            }
            if (h == 0) {
#pragma unroll
                for (int c = 0; c < 3; c++) ws.dprec[3 * (size_t)sample + c] = d[c];
            }
            acc_zero(g);
            valu_out_T<3>(g, lds + A::RT_C1, h, d);
        }
        relu_mask(g, ws.hc0 + (size_t)tile * kTile32, lane);
        tile_store(ws.dzc0 + (size_t)tile * kTile32, g, lane);
        ar.layer_T(w, g, A::WT_C0);   // d geo_feat
        tile_store(ws.dgeo + (size_t)tile * kTile32, w, lane);
        // ---- sigma net
        {
            float d[1] = {0.0f};
            if (live) d[0] = p.g_sigmas[sample] * expf(fminf(fmaxf(ws.sraw[sample], -15.0f), 15.0f));   // activation.py:13-17
            if (h == 0) ws.dsraw[sample] = d[0];
            ar.layer_T(g, w, A::WT_S2);
            valu_out_T<1>(g, lds + A::RT_S2R, h, d);
        }
        relu_mask(g, ws.hs1 + (size_t)tile * kTile32, lane);
        tile_store(ws.dzs1 + (size_t)tile * kTile32, g, lane);
        ar.layer_T(w, g, A::WT_S1);
        relu_mask(w, ws.hs0 + (size_t)tile * kTile32, lane);
        tile_store(ws.dzs0 + (size_t)tile * kTile32, w, lane);
        // d [enc_x | enc_w]: row tile 0 = enc_x, row tile 1 = enc_w, register 2 q + c of half h = (level 2 q + h, channel c)
        ar.layer_T(g, w, A::WT_S0);
        f32x16 x0 = g.v[0];
        const f32x16 x1 = g.v[1];
        // ---- ambient grid: feature gradients out (level-major), input gradient = sum_l g . dy_dx (gridencoder.cu:342-368);
        // the encoder sees (ambient + 1) / 2 (gridencoder/grid.py:151, bound = 1): a factor 1/2 on the way back
        float da[2] = {0.0f, 0.0f};
        {
            const float *dw = ws.dw + (size_t)tile * kTile32;
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const float g0 = x1[2 * q], g1 = x1[2 * q + 1];
                const float d00 = dw[(4 * q + 0) * 64 + lane], d01 = dw[(4 * q + 1) * 64 + lane];
                const float d10 = dw[(4 * q + 2) * 64 + lane], d11 = dw[(4 * q + 3) * 64 + lane];
                da[0] = __builtin_fmaf(g0, d00, da[0]); da[0] = __builtin_fmaf(g1, d01, da[0]);
                da[1] = __builtin_fmaf(g0, d10, da[1]); da[1] = __builtin_fmaf(g1, d11, da[1]);
                if (live) *reinterpret_cast<float2 *>(p.g_enc_w + ((size_t)(2 * q + h) * p.M + sample) * 2) = make_float2(g0, g1);
            }
            da[0] += __shfl_xor(da[0], 32, 64);
            da[1] += __shfl_xor(da[1], 32, 64);
        }
        // ---- ambient net: + the direct gradients of the ambient output, tanh'
        {
            float d[2] = {0.0f, 0.0f};
            if (live) {
                const float a0v = p.ambient[2 * (size_t)sample], a1v = p.ambient[2 * (size_t)sample + 1];
                float t0 = 0.5f * da[0], t1 = 0.5f * da[1];
                if (p.g_ambient) { t0 += p.g_ambient[2 * (size_t)sample]; t1 += p.g_ambient[2 * (size_t)sample + 1]; }
                if (p.g_ambient_abs) {   // d |a| = sign(a), 0 at 0
                    const float ga = p.g_ambient_abs[sample];
                    t0 += a0v > 0.0f ? ga : (a0v < 0.0f ? -ga : 0.0f);
                    t1 += a1v > 0.0f ? ga : (a1v < 0.0f ? -ga : 0.0f);
                }
                d[0] = t0 * (1.0f - a0v * a0v);
                d[1] = t1 * (1.0f - a1v * a1v);
            }
            if (h == 0) { ws.daraw[2 * (size_t)sample] = d[0]; ws.daraw[2 * (size_t)sample + 1] = d[1]; }
            acc_zero(g);
            valu_out_T<2>(g, lds + A::RT_A2, h, d);
        }
        relu_mask(g, ws.ha1 + (size_t)tile * kTile32, lane);
        tile_store(ws.dza1 + (size_t)tile * kTile32, g, lane);
        ar.layer_T(w, g, A::WT_A1);
        relu_mask(w, ws.ha0 + (size_t)tile * kTile32, lane);
        tile_store(ws.dza0 + (size_t)tile * kTile32, w, lane);
        ar.a0_T(x0, w);
        if (live) {
#pragma unroll
            for (int q = 0; q < 8; q++)
                *reinterpret_cast<float2 *>(p.g_enc_x + ((size_t)(2 * q + h) * p.M + sample) * 2) = make_float2(x0[2 * q], x0[2 * q + 1]);
        }
    }
}

}  // namespace th
}  // namespace rn
