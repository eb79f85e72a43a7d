// rn_nerf_image_dev.h -- the packed fp32 FORWARD weight image of the per-sample network and the first-layer biases of the
// per-call constants.  The training network (k_train_fwd / k_train_bwd, image built by k_train_pack, which appends its
// transposed image) reads the layout below layer by layer; the inference kernel (k_nerf_fused, image built by k_pack_nerf)
// reads the same layout with the geo_feat layer folded into the colour net's first layer (further down).
#pragma once

#include "rn_fused_dev.h"

namespace rn {

// ---- packed weight image (floats) --------------------------------------------------------------------
// MFMA layers: [step][h][col j][row tile] -> lane (j, h) reads one float2 per step (kStep floats per step).
constexpr int OFF_A0 = 0;                            // ambient L0, enc_x part : 16 steps
constexpr int OFF_A1 = OFF_A0 + 16 * kStep;          // ambient L1            : 32 steps
constexpr int OFF_A2 = OFF_A1 + 32 * kStep;          // ambient L2 (VALU)     : [2 out][2 h][32]
constexpr int OFF_S0 = OFF_A2 + 128;                 // sigma L0 (enc_x|enc_w): 32 steps
constexpr int OFF_S1 = OFF_S0 + 32 * kStep;          // sigma L1              : 32 steps
constexpr int OFF_S2 = OFF_S1 + 32 * kStep;          // sigma L2 rows 1..64   : 32 steps
constexpr int OFF_S2R = OFF_S2 + 32 * kStep;         // sigma L2 row 0 (VALU) : [2 h][32]
constexpr int OFF_C0 = OFF_S2R + 64;                 // color L0 (sh | geo)   : 8 + 32 steps
constexpr int OFF_C1 = OFF_C0 + 40 * kStep;          // color L1 (VALU)       : [3 out][2 h][32]
constexpr int kPacked = OFF_C1 + 192;                // 23936 floats
constexpr int kBias = 192;                           // amb | sig | col, 64 each

// Element q0 of a block of narrow (VALU) rows: [out][h][q], q = rt * 16 + r, from row-major src[out][64].
__device__ __forceinline__ float valu_image_elem(int q0, const float *src) {
    const int o = q0 / 64, h = (q0 % 64) / 32, q = q0 % 32;
    return src[o * 64 + 32 * (q >> 4) + rowmap(q & 15, h)];
}

// Element e (< kPacked) of the forward image.
__device__ __forceinline__ float nerf_image_elem(const RawW &w, int e) {
    const int ldA0 = 32 + (int)w.audio_dim, ldS0 = 64 + (int)w.has_eye, ldC0 = 80 + (int)w.ind_dim;
    enum { GATHER, ACC, COLOR };
    auto mfma_elem = [&](int q, const float *src, int ld, int kind) -> float {
        const int s = q / kStep, rem = q % kStep;
        const int h = rem / 64, j = (rem % 64) / 2, rt = rem % 2;
        const int row = 32 * rt + j;
        int k;
        if (kind == GATHER) k = 4 * (s >> 1) + 2 * h + (s & 1);   // gather rounds: half h holds level 2 (s / 2) + h, steps = its 2 features
        else if (kind == ACC) k = kmap(s, h);                      // previous accumulators
        else k = (s < 8) ? 2 * s + h : 16 + kmap(s - 8, h);        // color L0: sh pairs then geo accumulators
        return src[row * ld + k];
    };
    if (e < OFF_A1) return mfma_elem(e - OFF_A0, w.amb_w0, ldA0, GATHER);
    if (e < OFF_A2) return mfma_elem(e - OFF_A1, w.amb_w1, 64, ACC);
    if (e < OFF_S0) return valu_image_elem(e - OFF_A2, w.amb_w2);
    if (e < OFF_S1) return mfma_elem(e - OFF_S0, w.sig_w0, ldS0, GATHER);
    if (e < OFF_S2) return mfma_elem(e - OFF_S1, w.sig_w1, 64, ACC);
    if (e < OFF_S2R) return mfma_elem(e - OFF_S2, w.sig_w2 + 64, 64, ACC);   // rows 1..64 = geo_feat
    if (e < OFF_C0) return valu_image_elem(e - OFF_S2R, w.sig_w2);                 // row 0 = sigma
    if (e < OFF_C1) return mfma_elem(e - OFF_C0, w.col_w0, ldC0, COLOR);
    return valu_image_elem(e - OFF_C1, w.col_w1);
}

// ---- inference image (floats) ---------------------------------------------------------------------------
// sigma_net's last layer and color_net's first are both linear without a bias, and at inference nothing but the colour
// net reads geo_feat (nerf/network.py:266-276), so W_col0[:, 16:80] (W_sig2[1:65, :] a) is ONE 64 x 64 matrix applied to
// the sigma net's last hidden activations a.  The inference image holds that product in place of the geo_feat layer:
// the training image up to and including sigma L1 (same offsets), then
constexpr int IOFF_S2R = OFF_S2;                     // sigma L2 row 0 (VALU)          : [2 h][32]
constexpr int IOFF_C0 = IOFF_S2R + 64;               // color L0 (sh | folded geo_feat): 8 + 32 steps
constexpr int IOFF_C1 = IOFF_C0 + 40 * kStep;        // color L1 (VALU)                : [3 out][2 h][32]
constexpr int kInferPacked = IOFF_C1 + 192;          // 19840 floats
static_assert(kInferPacked == kPacked - 32 * kStep && kInferPacked % 4 == 0, "inference image = training image less the geo_feat layer");

// (W_col0[:, 16:80] W_sig2[1:65, :])[row][k]: a 64-term sum accumulated in double and rounded once, so the image costs the
// product one rounding, not 64.
__device__ __forceinline__ float nerf_folded_elem(const RawW &w, int row, int k) {
    const float *c0 = w.col_w0 + row * (80 + (int)w.ind_dim) + 16;   // this row's geo_feat columns
    const float *s2 = w.sig_w2 + 64 + k;                             // column k of rows 1..64
    double acc = 0.0;
    for (int m = 0; m < 64; m++) acc += (double)c0[m] * (double)s2[m * 64];
    return (float)acc;
}

// Element e (< kInferPacked) of the inference image.
__device__ __forceinline__ float nerf_infer_image_elem(const RawW &w, int e) {
    if (e < IOFF_S2R) return nerf_image_elem(w, e);
    if (e < IOFF_C0) return nerf_image_elem(w, e - IOFF_S2R + OFF_S2R);
    if (e >= IOFF_C1) return nerf_image_elem(w, e - IOFF_C1 + OFF_C1);
    const int q = e - IOFF_C0, s = q / kStep;
    if (s < 8) return nerf_image_elem(w, q + OFF_C0);   // sh steps
    const int rem = q % kStep, h = rem / 64, j = (rem % 64) / 2, rt = rem % 2;
    return nerf_folded_elem(w, 32 * rt + j, kmap(s - 8, h));   // previous accumulators = the sigma net's hidden activations
}

// Value t (< kBias) of the first-layer biases of the per-call constants: the columns of the three first layers that
// multiply the audio code, the eye value and the individual code (nerf/network.py:236, 262, 274) times those inputs.
__device__ __forceinline__ float nerf_const_bias(const RawW &w, const float *enc_a, const float *eye, const float *ind_code, int t) {
    const int row = t & 63;
    float acc = 0.0f;
    if (t < 64) {
        const float *r = w.amb_w0 + row * (32 + w.audio_dim) + 32;
        for (uint32_t a = 0; a < w.audio_dim; a++) acc += r[a] * enc_a[a];
    } else if (t < 128) {
        if (w.has_eye) acc = w.sig_w0[row * 65 + 64] * eye[0];
    } else {
        const float *r = w.col_w0 + row * (80 + w.ind_dim) + 80;
        for (uint32_t c = 0; c < w.ind_dim; c++) acc += r[c] * ind_code[c];
    }
    return acc;
}

}  // namespace rn
