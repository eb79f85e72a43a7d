// rn_torso_dev.h -- the torso layer (NeRFNetwork.forward_torso, nerf/network.py:188-219) described once for its inference
// pass (rn_torso.hip) and its training kernels (rn_train_torso.hip): the raw weight descriptor, the packed fp32 FORWARD
// weight image, the pose encoding, the first-layer biases of the constant columns and the output activation.  The
// training image appends its transposed part and the constants (rn_train_torso.hip).
#pragma once

#include "rn_freq_dev.h"
#include "rn_nerf_image_dev.h"

namespace rn {

struct RawT {
    const float *def_w0, *def_w1, *def_w2, *tor_w0, *tor_w1, *tor_w2;
    uint32_t ind_dim;
};
inline RawT raw_t(const rn_torso_weights_t *w) {
    return RawT{w->def_w0, w->def_w1, w->def_w2, w->tor_w0, w->tor_w1, w->tor_w2, w->ind_dim};
}
static inline int check_torso_weights(const rn_torso_weights_t *w, const char *what) {
    RN_REQUIRE(w && w->def_w0 && w->def_w1 && w->def_w2 && w->tor_w0 && w->tor_w1 && w->tor_w2, "%s: null weight pointer", what);
    return RN_OK;
}

// ---- packed forward image (floats) --------------------------------------------------------------------
// 64-row MFMA layers as in rn_nerf_image_dev.h (kStep floats per step); 32-row layers: [step][h][row j], lane (j, h) reads
// one float per step (kS32 floats per step).
constexpr int TOFF_D0 = 0;                           // deform L0, enc_x part         : 21 steps, k = 2 s + h
constexpr int TOFF_D1 = TOFF_D0 + 21 * kStep;        // deform L1                     : 32 steps
constexpr int TOFF_D2 = TOFF_D1 + 32 * kStep;        // deform L2 (VALU)              : [2 out][2 h][32]
constexpr int TOFF_T0 = TOFF_D2 + 128;               // torso L0 (grid | enc_x), 32 rows: 16 + 21 steps
constexpr int TOFF_T1 = TOFF_T0 + 37 * kS32;         // torso L1, 32 rows             : 16 steps
constexpr int TOFF_T2 = TOFF_T1 + 16 * kS32;         // torso L2 (VALU)               : [4 out][2 h][16]
constexpr int kTorsoPacked = TOFF_T2 + 128;          // 10432 floats
static_assert(kTorsoPacked == 10432 && kTorsoPacked % 4 == 0, "the torso forward image");
constexpr int kTorsoBias = 96;                       // first-layer biases of the constant columns: deform 64 | torso 32

// Element e (< kTorsoPacked) of the forward image.  The 32 grid features are columns 0..31 of torso L0; their 16 steps are
// in level order (k = 2 s + h: both lane halves hold both channels of every level, the inference kernel) or, GATHER, in
// the order the training forward gathers in (lane half h holds level 2 (s / 2) + h, steps = its 2 channels).
template <bool GATHER>
__device__ __forceinline__ float torso_image_elem(const RawT &w, int e) {
    const int ldD0 = 96 + (int)w.ind_dim, ldT0 = 128 + (int)w.ind_dim;
    if (e < TOFF_D2) {   // 64 rows: [step][h][col j][row tile]
        const int q = e < TOFF_D1 ? e - TOFF_D0 : e - TOFF_D1, s = q / kStep, rem = q % kStep;
        const int h = rem / 64, row = 32 * (rem % 2) + (rem % 64) / 2;
        return e < TOFF_D1 ? w.def_w0[row * ldD0 + 2 * s + h] : w.def_w1[row * 64 + kmap(s, h)];
    }
    if (e < TOFF_T0) return valu_image_elem(e - TOFF_D2, w.def_w2);
    if (e < TOFF_T2) {   // 32 rows: [step][h][row j]
        const int q = e < TOFF_T1 ? e - TOFF_T0 : e - TOFF_T1, s = q / kS32, rem = q % kS32, h = rem / 32, j = rem % 32;
        if (e >= TOFF_T1) return w.tor_w1[j * 32 + rowmap(s, h)];   // previous accumulators (one row tile)
        return w.tor_w0[j * ldT0 + (GATHER && s < 16 ? 4 * (s >> 1) + 2 * h + (s & 1) : 2 * s + h)];
    }
    const int q0 = e - TOFF_T2, o = q0 / 32, h = (q0 % 32) / 16, r = q0 % 16;
    return w.tor_w2[o * 32 + rowmap(r, h)];
}

// ---- constant columns ------------------------------------------------------------------------------------
// Element c (< 54) of enc_pose = freq(poses6, 4) (network.py:197), the layout of k_freq_forward.
__device__ __forceinline__ float enc_pose_elem(const float *poses6, int c) {
    float v;
    if (c < 6) v = poses6[c];
    else {
        const int col = c / 6 - 1, d = c % 6, f = col / 2;
        const float a = freq_angle(poses6[d], f);
        v = (col & 1) ? freq_cos(a) : freq_sin(a);
    }
    return v;
}

// Value t (< kTorsoBias) of the first-layer biases: the constant columns [enc_pose | c] of the deformation net's (t < 64) and
// the torso net's first layer times those inputs (network.py:201, 212).  w by value: k_torso_fused hands in a member of its
// parameter block, and a reference to that changes its instruction stream past the prologue (see rn_fused_dev.h).
__device__ __forceinline__ float torso_const_bias(const RawT w, const float *enc_pose, const float *ind_code, int t) {
    const float *r = t < 64 ? w.def_w0 + t * (96 + (int)w.ind_dim) + 42 : w.tor_w0 + (t - 64) * (128 + (int)w.ind_dim) + 74;
    float acc = 0.0f;
    for (int k = 0; k < 54; k++) acc += r[k] * enc_pose[k];
    for (uint32_t c = 0; c < w.ind_dim; c++) acc += r[54 + c] * ind_code[c];
    return acc;
}

// alpha and colour of the torso net's four outputs
__device__ __forceinline__ float sigmoid_out(float x) { return 1.0f / (1.0f + expf(-x)); }

}  // namespace rn
