// rn_train_head_dev.h -- what the two arithmetics of the fused training network share (rn_train_head.hip: fp32 matrix cores;
// rn_train_head_f16.hip: 16-bit operands, fp32 sums): the layout of the fp32 weight image of a step and its elements, the
// workspace of native tiles, the parameter blocks of the forward and the backward kernel, and the host side of the pack,
// forward and backward entries.  Both arithmetics write the same fp32 image and the same fp32 workspace, so everything
// downstream of the two network kernels (weight gradients, input gradients, table scatters) reads either one's results; the
// tile walk that writes the workspace is rn_train_head_walk_dev.h.
#pragma once

#include "rn_nerf_image_dev.h"

#include "../../include/radnerf_train.h"

namespace rn {
namespace th {

// The weight image of a step: forward image (rn_nerf_image_dev.h, the inference kernel's) | transposed image | biases.
// ---- transposed image: T[s][h][j][rt] = W[kmap(s, h)][column(32 rt + j)] ---------------------------------------------
constexpr int T_C0 = 0;                    // d geo_feat   = W_col0[:, 16:80]^T dZ_c0
constexpr int T_S2 = T_C0 + 32 * kStep;    // d h_s1       = W_sig2[1:65]^T d geo_feat
constexpr int T_S1 = T_S2 + 32 * kStep;
constexpr int T_S0 = T_S1 + 32 * kStep;    // d [enc_x | enc_w] = W_sig0[:, 0:64]^T dZ_s0, output rows in gather order (below)
constexpr int T_A1 = T_S0 + 32 * kStep;
constexpr int T_A0 = T_A1 + 32 * kStep;    // d enc_x += W_amb0[:, 0:32]^T dZ_a0 : 32 steps x [2 h][32 j]
constexpr int N_C1 = T_A0 + 32 * 64;       // narrow rows again: [3][2 h][32]
constexpr int N_S2R = N_C1 + 192;          // [2 h][32]
constexpr int N_A2 = N_S2R + 64;           // [2][2 h][32]
constexpr int kBwd = N_A2 + 128;           // 22912 floats
constexpr int kImage = kPacked + kBwd + kBias;

// Output row j of a 32-row tile sits in register r of lane half hh with rowmap(r, hh) == j.  The grid-feature gradients want
// register 2 q + c of lane half hh to be (level 2 q + hh, channel c), the layout the forward gathers in: feature 4 q + 2 hh + c.
__host__ __device__ constexpr int gather_feature(int j) {
    const int hh = (j >> 2) & 1, r = (j & 3) + 4 * (j >> 3);
    return 4 * (r >> 1) + 2 * hh + (r & 1);
}

// Element e (< kImage) of the fp32 image.  ind_code: the code itself, already moved to the picked row of the table.
__device__ __forceinline__ float train_image_elem(const RawW &w, const float *__restrict__ enc_a, const float *__restrict__ eye,
                                                  const float *__restrict__ ind_code, int e) {
    const int ldA0 = 32 + (int)w.audio_dim, ldS0 = 64 + (int)w.has_eye, ldC0 = 80 + (int)w.ind_dim;   // row strides of the first layers
    auto t_elem = [&](int q, const float *src, int ld, int col0, bool gather) -> float {   // transposed 64-row layer
        const int s = q / kStep, rem = q % kStep;
        const int h = rem / 64, j = (rem % 64) / 2, rt = rem % 2;
        const int col = gather ? 32 * rt + gather_feature(j) : 32 * rt + j;
        return src[kmap(s, h) * ld + col0 + col];
    };
    if (e < kPacked) return nerf_image_elem(w, e);
    if (e < kPacked + kBwd) {
        const int t = e - kPacked;
        if (t < T_S2) return t_elem(t - T_C0, w.col_w0, ldC0, 16, false);
        if (t < T_S1) return t_elem(t - T_S2, w.sig_w2 + 64, 64, 0, false);
        if (t < T_S0) return t_elem(t - T_S1, w.sig_w1, 64, 0, false);
        if (t < T_A1) return t_elem(t - T_S0, w.sig_w0, ldS0, 0, true);
        if (t < T_A0) return t_elem(t - T_A1, w.amb_w1, 64, 0, false);
        if (t < N_C1) {
            const int q = t - T_A0, s = q / 64, rem = q % 64, h = rem / 32, j = rem % 32;
            return w.amb_w0[kmap(s, h) * ldA0 + gather_feature(j)];
        }
        if (t < N_S2R) return valu_image_elem(t - N_C1, w.col_w1);
        if (t < N_A2) return valu_image_elem(t - N_S2R, w.sig_w2);
        return valu_image_elem(t - N_A2, w.amb_w2);
    }
    return nerf_const_bias(w, enc_a, eye, ind_code, e - kPacked - kBwd);   // first-layer biases of the per-call constants
}

// ---- workspace ----------------------------------------------------------------------------------------------------------
// native tiles ([registers][64 lanes] floats per 32-sample tile) and per-sample rows, one contiguous region each
struct Ws {
    float *ex, *ew;          // grid features, 16 registers: register 2 q + c of half h = level 2 q + h, channel c
    float *dw;               // d enc_w / d (normalised ambient coordinate), 32 registers: 4 q + 2 d + c of half h
    float *sh;               // SH basis, 8 registers: register q of half h = sh[2 q + h]
    float *ha0, *ha1, *hs0, *hs1, *geo, *hc0;        // 32 registers each
    float *dza0, *dza1, *dzs0, *dzs1, *dgeo, *dzc0;  // pre-activation gradients (backward), 32 registers each
    float *sraw;             // [M_pad] sigma_net output row 0
    float *daraw, *dsraw, *dprec;   // [M_pad, 2], [M_pad], [M_pad, 3]: gradients of the narrow layers' outputs
};
constexpr uint32_t kTile16 = 16 * 64, kTile32 = 32 * 64, kTile8 = 8 * 64;
constexpr uint32_t kWsPerTile = 2 * kTile16 + kTile32 + kTile8 + 12 * kTile32 + 32 * 7;

__host__ __device__ inline Ws make_ws(float *base, uint32_t M) {
    const size_t nt = (M + 31u) >> 5;
    Ws w;
    float *p = base;
    w.ex = p; p += nt * kTile16;
    w.ew = p; p += nt * kTile16;
    w.dw = p; p += nt * kTile32;
    w.sh = p; p += nt * kTile8;
    w.ha0 = p; p += nt * kTile32;
    w.ha1 = p; p += nt * kTile32;
    w.hs0 = p; p += nt * kTile32;
    w.hs1 = p; p += nt * kTile32;
    w.geo = p; p += nt * kTile32;
    w.hc0 = p; p += nt * kTile32;
    w.dza0 = p; p += nt * kTile32;
    w.dza1 = p; p += nt * kTile32;
    w.dzs0 = p; p += nt * kTile32;
    w.dzs1 = p; p += nt * kTile32;
    w.dgeo = p; p += nt * kTile32;
    w.dzc0 = p; p += nt * kTile32;
    w.sraw = p; p += nt * 32;
    w.daraw = p; p += nt * 64;
    w.dsraw = p; p += nt * 32;
    w.dprec = p; p += nt * 96;
    return w;
}

constexpr int kThreads = 512, kWaves = kThreads / kWave;   // two waves per SIMD: a 4096-ray step is ~1 tile per wave slot

struct FwdParams {
    const float *xyzs, *dirs;
    uint32_t M;
    const int32_t *m_dev;
    GridArgs gx, gw;
    const float *image;
    float bound;
    float *sigmas, *rgbs, *ambient, *ambient_abs, *xn, *wn;
    float *ws;
};

struct BwdParams {
    const float *g_sigmas, *g_rgbs, *g_ambient, *g_ambient_abs;
    const float *rgbs, *ambient;
    uint32_t M;
    const int32_t *m_dev;
    const float *image;
    float *ws;
    float *g_enc_x, *g_enc_w;   // [16, M, 2]
};

static inline int check_w(const rn_nerf_weights_t *w) {
    RN_REQUIRE(w && w->amb_w0 && w->amb_w1 && w->amb_w2 && w->sig_w0 && w->sig_w1 && w->sig_w2 && w->col_w0 && w->col_w1,
               "train_head: null weight pointer");
    RN_REQUIRE(w->has_eye <= 1, "train_head: has_eye must be 0 or 1");
    return RN_OK;
}

// ---- host side of the pack / forward / backward entries -------------------------------------------------------------------
// Written once; an entry hands over its arithmetic's kernel (a kernel is launched from its own translation unit) and its
// name `what` for the messages.
typedef void (*PackKernel)(RawW, const float *, const float *, const float *, const int64_t *, float *);

// elems: threads of the pack launch.  row: `ind` is the table individual_codes, ind_index picks its row on the device.
static inline int pack(PackKernel kernel, int elems, const char *what, const rn_nerf_weights_t *w, const float *enc_a, const float *eye,
                       const float *ind, const int64_t *ind_index, bool row, float *image, rn_stream_t stream) {
    if (int rc = check_w(w)) return rc;
    RN_REQUIRE(image && ((uintptr_t)image & 15u) == 0, "%s: image must be 16-byte aligned", what);
    RN_REQUIRE((enc_a || w->audio_dim == 0) && (eye || !w->has_eye) && (ind || w->ind_dim == 0), "%s: null constant", what);
    RN_REQUIRE(!row || (ind && ind_index && w->ind_dim), "%s: the code table and its row index are required", what);
    hipLaunchKernelGGL(kernel, dim3(div_up(elems, 256)), dim3(256), 0, as_stream(stream), raw_w(w), enc_a, eye, ind, ind_index, image);
    return check_launch(what);
}

static inline int forward(void (*kernel)(FwdParams), const char *what, const float *xyzs, const float *dirs, uint32_t M, const int32_t *m_dev,
                          const rn_grid_t *grid_xyz, const rn_grid_t *grid_amb, const float *image, float bound, float *sigmas, float *rgbs,
                          float *ambient, float *ambient_abs, float *xn, float *wn, float *workspace, rn_stream_t stream) {
    if (M == 0) return RN_OK;
    if (int rc = check_train_grid(grid_xyz, 3, "train_head: xyz")) return rc;
    if (int rc = check_train_grid(grid_amb, 2, "train_head: ambient")) return rc;
    RN_REQUIRE(xyzs && dirs && image && sigmas && rgbs && ambient && xn && wn && workspace, "%s: null pointer", what);
    RN_REQUIRE(((uintptr_t)image & 15u) == 0 && ((uintptr_t)workspace & 15u) == 0, "%s: image / workspace must be 16-byte aligned", what);
    FwdParams p{xyzs, dirs, M, m_dev, grid_args(grid_xyz), grid_args(grid_amb), image, bound, sigmas, rgbs, ambient, ambient_abs, xn, wn, workspace};
    hipLaunchKernelGGL(kernel, dim3(tile_blocks((M + 31u) >> 5, kWaves, 1)), dim3(kThreads), 0, as_stream(stream), p);
    return check_launch(what);
}

// image16: the backward kernel copies 16-bit images out of `image` 16 bytes at a time
static inline int backward(void (*kernel)(BwdParams), bool image16, const char *what, const float *grad_sigmas, const float *grad_rgbs,
                           const float *grad_ambient, const float *grad_ambient_abs, const float *rgbs, const float *ambient, uint32_t M,
                           const int32_t *m_dev, const float *image, float *workspace, float *grad_enc_x, float *grad_enc_w, rn_stream_t stream) {
    if (M == 0) return RN_OK;
    RN_REQUIRE(grad_sigmas && grad_rgbs && rgbs && ambient && image && workspace && grad_enc_x && grad_enc_w, "%s: null pointer", what);
    RN_REQUIRE(!image16 || ((uintptr_t)image & 15u) == 0, "%s: image must be 16-byte aligned", what);
    RN_REQUIRE(((uintptr_t)grad_enc_x & 7u) == 0 && ((uintptr_t)grad_enc_w & 7u) == 0, "%s: feature gradients must be 8-byte aligned", what);
    BwdParams p{grad_sigmas, grad_rgbs, grad_ambient, grad_ambient_abs, rgbs, ambient, M, m_dev, image, workspace, grad_enc_x, grad_enc_w};
    hipLaunchKernelGGL(kernel, dim3(tile_blocks((M + 31u) >> 5, kWaves, 1)), dim3(kThreads), 0, as_stream(stream), p);
    return check_launch(what);
}

}  // namespace th
}  // namespace rn
