// rn_train_torso.hip -- the torso layer of the TRAINING step as one forward and one backward kernel (gfx950).
//
// C ABI: include/radnerf_train.h (rn_train_torso_*).  What is computed: NeRFNetwork.forward_torso (nerf/network.py:188-219) and
// its autograd per covered pixel.  The machine is rn_train_head.hip's (one wavefront owns 32 pixels, v_mfma_f32_32x32x2_f32,
// native tiles), the arithmetic k_torso_fused's (rn_torso.hip):
//
//  * k_train_torso_fwd: x = xy * shrink; enc_x = freq(x, 10) in registers (lane half h holds the features of coordinate h: they
//    are the k = 2 s + h of MFMA step s); deformation net 42 (+ bias) -> 64 -> 64 -> 2; u = clamp(x + dx, -1, 1); the 16 levels of
//    the 2-D grid with dy_dx (lane half h gathers level 2 r + h in round r); torso net 32 + 42 (+ bias) -> 32 -> 32 -> 4 on ONE row
//    tile (its true width); sigmoid.  Saved as native tiles: the four post-ReLU hidden activations, the grid features,
//    d enc / d wn and the clamp mask.  enc_x is recomputed where it is needed.
//  * k_train_torso_bwd: the same tile walked back: sigmoid', the torso net transposed with ReLU masks, the feature gradients of the
//    grid out level-major ([16, P, 2]), d wn = sum g dy_dx inside the tile, the clamp's mask, the deformation net transposed.
//  * k_train_torso_wgrad / _wreduce / _const: the six weight gradients on the machine of rn_wgrad_dev.h; [enc_x | 1] is an operand
//    computed from xy while a tile is staged; the column of ones gives the bias gradients, from which the gradients of the
//    constant columns (pose encoding, individual code) and of the code follow.
// The table gradient is rn_grid_scatter_jobs (rn_grid_scatter.hip) with one D = 2 job.
#include "rn_torso_dev.h"
#include "rn_wgrad_dev.h"

#include "../../include/radnerf_train.h"

namespace rn {
namespace tt {

// ---- the weight image of a step: forward (rn_torso_dev.h, grid steps in gather order) | transposed | constants --------------
constexpr int kFwd = kTorsoPacked;
constexpr int B_T2 = 0;                    // (relative to the transposed image) the narrow rows again
constexpr int B_T1 = B_T2 + 128;           // d h_t0 = W_tor1^T dZ_t1
constexpr int B_T0 = B_T1 + 16 * kS32;     // d grid features = W_tor0[:, 0:32]^T dZ_t0, output rows in gather order
constexpr int B_D2 = B_T0 + 16 * kS32;
constexpr int B_D1 = B_D2 + 128;           // d h_d0 = W_def1^T dZ_d1
constexpr int kBwd = B_D1 + 32 * kStep;    // 6400 floats
constexpr int C_DEF = 0, C_TOR = 64, C_POSE = kTorsoBias;   // first-layer biases of the constant columns, enc_pose [54]
constexpr int kConst = 152;
constexpr int kImage = kFwd + kBwd + kConst;
constexpr int kPackBlocks = (kFwd + kBwd + 255) / 256;   // workgroups of k_train_torso_pack that write weights; one more: the constants

// Output row j of a 32-row tile sits in register r of lane half hh with rowmap(r, hh) == j; the grid features want register
// 2 q + c of lane half hh to be (level 2 q + hh, channel c), the order the forward gathers in: feature 4 q + 2 hh + c.
__host__ __device__ constexpr int gather_feature(int j) {
    const int hh = (j >> 2) & 1, r = (j & 3) + 4 * (j >> 3);
    return 4 * (r >> 1) + 2 * hh + (r & 1);
}

// Element t (< kBwd) of the transposed image: the narrow layers as the forward image has them, the MFMA layers transposed
__device__ __forceinline__ float torso_bwd_image_elem(const RawT &w, int t) {
    if (t < B_T1) return torso_image_elem<true>(w, TOFF_T2 + t - B_T2);
    if (t >= B_D2 && t < B_D1) return torso_image_elem<true>(w, TOFF_D2 + t - B_D2);
    if (t < B_D2) {   // 32 rows: [step][h][row j]
        const int q = t < B_T0 ? t - B_T1 : t - B_T0, s = q / kS32, rem = q % kS32, h = rem / 32, j = rem % 32;
        return t < B_T0 ? w.tor_w1[rowmap(s, h) * 32 + j] : w.tor_w0[rowmap(s, h) * (128 + (int)w.ind_dim) + gather_feature(j)];
    }
    const int q = t - B_D1, s = q / kStep, rem = q % kStep, h = rem / 64, j = (rem % 64) / 2, rt = rem % 2;
    return w.def_w1[kmap(s, h) * 64 + 32 * rt + j];
}

__global__ void __launch_bounds__(256) k_train_torso_pack(RawT w, const float *__restrict__ poses6, const float *__restrict__ ind_code,
                                                          float *__restrict__ image) {
    if (blockIdx.x == kPackBlocks) {
        // the last workgroup: enc_pose once, then the constant columns folded into the first layers as biases.  enc_pose stays in
        // the image: the constants' gradients need it
        __shared__ float enc_pose[54];
        float *c = image + kFwd + kBwd;
        const int t = threadIdx.x;
        if (t < 54) enc_pose[t] = enc_pose_elem(poses6, t);
        __syncthreads();
        if (t < C_POSE) c[t] = torso_const_bias(w, enc_pose, ind_code, t);
        else if (t < kConst) c[t] = t < C_POSE + 54 ? enc_pose[t - C_POSE] : 0.0f;
        return;
    }
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < kFwd + kBwd) image[e] = e < kFwd ? torso_image_elem<true>(w, e) : torso_bwd_image_elem(w, e - kFwd);
}

// ---- workspace: native tiles ([registers][64 lanes] floats per 32-pixel tile) and per-pixel rows -------------------------------
struct Ws {
    float *hd0, *hd1;          // deformation net, post-ReLU, 32 registers
    float *ht0, *ht1;          // torso net, post-ReLU, 16 registers
    float *eg;                 // grid features, 16 registers: register 2 q + c of half h = level 2 q + h, channel c
    float *dw;                 // d enc / d wn, 32 registers: 4 q + 2 d + c of half h
    float *mask;               // the clamp passes the gradient of coordinate d: 2 registers (both halves alike)
    float *dzd0, *dzd1, *dzt0, *dzt1;   // pre-activation gradients (backward)
    float *ddx, *dto;          // [P_pad, 2], [P_pad, 4]: gradients of the narrow layers' outputs
};
constexpr uint32_t kTile32 = 32 * 64, kTile16 = 16 * 64, kTile2 = 2 * 64;
constexpr uint32_t kWsPerTile = 4 * kTile32 + 4 * kTile16 + kTile16 + kTile32 + kTile2 + 32 * 6;

__host__ __device__ inline Ws make_ws(float *base, uint32_t P) {
    const size_t nt = (P + 31u) >> 5;
    Ws w;
    float *p = base;
    w.hd0 = p; p += nt * kTile32;
    w.hd1 = p; p += nt * kTile32;
    w.dzd0 = p; p += nt * kTile32;
    w.dzd1 = p; p += nt * kTile32;
    w.dw = p; p += nt * kTile32;
    w.ht0 = p; p += nt * kTile16;
    w.ht1 = p; p += nt * kTile16;
    w.dzt0 = p; p += nt * kTile16;
    w.dzt1 = p; p += nt * kTile16;
    w.eg = p; p += nt * kTile16;
    w.mask = p; p += nt * kTile2;
    w.ddx = p; p += nt * 64;
    w.dto = p; p += nt * 128;
    return w;
}

constexpr int kThreads = 256, kWaves = kThreads / kWave;   // a 4096-ray torso step is ~41 tiles: spread them over many CUs

struct FwdParams {
    const float *xy;
    uint32_t P;
    const int32_t *p_dev;
    float shrink;
    GridArgs gt;
    const float *image;
    float *alpha, *color, *dx, *wn;
    float *ws;
};

__global__ void __launch_bounds__(kThreads) k_train_torso_fwd(FwdParams p) {
    __shared__ __attribute__((aligned(16))) float lds[kFwd + C_POSE];
    __shared__ LevelPlan plan_t[16];
    const uint32_t P = live_count(p.P, p.p_dev);
    const uint32_t n_tiles = (P + 31u) >> 5;
    if (blockIdx.x * kWaves >= n_tiles) return;
    for (int i = threadIdx.x; i < kFwd / 4; i += kThreads) reinterpret_cast<float4 *>(lds)[i] = reinterpret_cast<const float4 *>(p.image)[i];
    if (threadIdx.x < C_POSE) lds[kFwd + threadIdx.x] = p.image[kFwd + kBwd + threadIdx.x];
    if (threadIdx.x < 16) {
        const int t = threadIdx.x;
        const uint32_t o = (uint32_t)p.gt.offsets[t];
        plan_t[t] = plan_level<2>(p.gt.lc.scale[t], p.gt.lc.resolution[t], o, (uint32_t)p.gt.offsets[t + 1] - o, p.gt.gridtype, 8u);
    }
    __syncthreads();
    const Ws ws = make_ws(p.ws, p.P);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int lane_off = h * 64 + j * 2, lane_off32 = h * 32 + j;
    const float *bias_def = lds + kFwd + C_DEF, *bias_tor = lds + kFwd + C_TOR;
    const float *table = static_cast<const float *>(p.gt.table);

    for (uint32_t tile = blockIdx.x * kWaves + wave; tile < n_tiles; tile += gridDim.x * kWaves) {
        const uint32_t px = tile * 32 + j;   // both lane halves work on the same 32 pixels
        const bool live = px < P;
        // x = x * torso_shrink; enc_x = freq(x, 10) (network.py:194, 198): [x, sin(2^f x), cos(2^f x)]_f.  Feature 2 s + h
        // belongs to coordinate h for every s: a lane computes the 21 features of its half's coordinate
        float x0 = 0.0f, x1 = 0.0f;
        if (live) { x0 = p.xy[2 * (size_t)px] * p.shrink; x1 = p.xy[2 * (size_t)px + 1] * p.shrink; }
        float fq[21];
        {
            const float xs = h ? x1 : x0;
            fq[0] = xs;
#pragma unroll
            for (int f = 0; f < 10; f++) {
                const float a = freq_angle(xs, f);
                fq[1 + 2 * f] = freq_sin(a);
                fq[2 + 2 * f] = freq_cos(a);
            }
        }
        // ---- deformation net: [enc_x | enc_pose | c] -> 64 -> 64 -> 2
        Acc32 a0, a1;
        acc_bias(a0, bias_def, h);
#pragma unroll
        for (int s = 0; s < 21; s++) step32(a0, lds + TOFF_D0, s, lane_off, fq[s]);
        acc_relu(a0);
        tile_store(ws.hd0 + (size_t)tile * kTile32, a0, lane);
        acc_zero(a1);
        layer_from_acc(a1, a0, lds + TOFF_D1, lane_off);
        acc_relu(a1);
        tile_store(ws.hd1 + (size_t)tile * kTile32, a1, lane);
        float dxy[2];
        valu_out<2>(a1, lds + TOFF_D2, h, dxy);
        // ---- x = clamp(x + dx, -1, 1); the torso grid (bound = 1) with d enc / d input
        f32x16 t0;
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const float4 b = *reinterpret_cast<const float4 *>(bias_tor + 8 * g + 4 * h);
            t0[4 * g] = b.x; t0[4 * g + 1] = b.y; t0[4 * g + 2] = b.z; t0[4 * g + 3] = b.w;
        }
        {
            const float u0 = x0 + dxy[0], u1 = x1 + dxy[1];
            float in[2] = {(fminf(fmaxf(u0, -1.0f), 1.0f) + 1.0f) / 2.0f, (fminf(fmaxf(u1, -1.0f), 1.0f) + 1.0f) / 2.0f};
            const bool on = live && !(in[0] < 0 || in[0] > 1 || in[1] < 0 || in[1] > 1);
            if (live && h == 0) {
                p.dx[2 * (size_t)px] = dxy[0];
                p.dx[2 * (size_t)px + 1] = dxy[1];
                p.wn[2 * (size_t)px] = in[0];
                p.wn[2 * (size_t)px + 1] = in[1];
            }
            float *mk = ws.mask + (size_t)tile * kTile2;   // torch's clamp passes the gradient on [-1, 1], the ends included
            mk[lane] = (u0 >= -1.0f && u0 <= 1.0f) ? 1.0f : 0.0f;
            mk[64 + lane] = (u1 >= -1.0f && u1 <= 1.0f) ? 1.0f : 0.0f;
            float *eg = ws.eg + (size_t)tile * kTile16, *dw = ws.dw + (size_t)tile * kTile32;
            LevelFetch<float, 2, 2> f;
#pragma unroll 1
            for (int r = 0; r < 8; r++) {
                float f0 = 0.0f, f1 = 0.0f, g[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                if (on) {
                    issue_planned<float, 2, 2, false, false>(table, plan_t[2 * r + h], in, f);
                    float res[2], grads[4];
                    blend_level<float, 2, 2, true>(f, plan_t[2 * r + h].scale, res, grads);
                    f0 = res[0];
                    f1 = res[1];
#pragma unroll
                    for (int q = 0; q < 4; q++) g[q] = grads[q];
                }
                t0 = mfma32(lds[TOFF_T0 + (2 * r) * kS32 + lane_off32], f0, t0);
                t0 = mfma32(lds[TOFF_T0 + (2 * r + 1) * kS32 + lane_off32], f1, t0);
                eg[(2 * r) * 64 + lane] = f0;
                eg[(2 * r + 1) * 64 + lane] = f1;
#pragma unroll
                for (int q = 0; q < 4; q++) dw[(4 * r + q) * 64 + lane] = g[q];
            }
        }
        // ---- torso net: [grid | enc_x | enc_pose | c] -> 32 -> 32 -> 4, sigmoid
#pragma unroll
        for (int s = 0; s < 21; s++) t0 = mfma32(lds[TOFF_T0 + (16 + s) * kS32 + lane_off32], fq[s], t0);
#pragma unroll
        for (int r = 0; r < 16; r++) t0[r] = relu_bits(t0[r]);
        store16(ws.ht0 + (size_t)tile * kTile16, t0, lane);
        f32x16 t1 = zero16();
#pragma unroll
        for (int s = 0; s < 16; s++) t1 = mfma32(lds[TOFF_T1 + s * kS32 + lane_off32], t0[s], t1);
#pragma unroll
        for (int r = 0; r < 16; r++) t1[r] = relu_bits(t1[r]);
        store16(ws.ht1 + (size_t)tile * kTile16, t1, lane);
        float o4[4];
#pragma unroll
        for (int o = 0; o < 4; o++) {
            float s = 0.0f;
            const float *wo = lds + TOFF_T2 + (o * 2 + h) * 16;
#pragma unroll
            for (int r = 0; r < 16; r++) s = __builtin_fmaf(t1[r], wo[r], s);
            o4[o] = s + __shfl_xor(s, 32, 64);
        }
        if (live && h == 0) {
            p.alpha[px] = sigmoid_out(o4[0]);
#pragma unroll
            for (int c = 0; c < 3; c++) p.color[3 * (size_t)px + c] = sigmoid_out(o4[1 + c]);
        }
    }
}

struct BwdParams {
    const float *g_alpha, *g_color, *g_dx;   // each may be null
    const float *alpha, *color;
    uint32_t P;
    const int32_t *p_dev;
    const float *image;
    float *ws;
    float *g_feat;   // [16, P, 2]
};

__global__ void __launch_bounds__(kThreads) k_train_torso_bwd(BwdParams p) {
    __shared__ __attribute__((aligned(16))) float lds[kBwd];
    const uint32_t P = live_count(p.P, p.p_dev);
    const uint32_t n_tiles = (P + 31u) >> 5;
    if (blockIdx.x * kWaves >= n_tiles) return;
    for (int i = threadIdx.x; i < kBwd / 4; i += kThreads)
        reinterpret_cast<float4 *>(lds)[i] = reinterpret_cast<const float4 *>(p.image + kFwd)[i];
    __syncthreads();
    const Ws ws = make_ws(p.ws, p.P);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int lane_off = h * 64 + j * 2, lane_off32 = h * 32 + j;

    for (uint32_t tile = blockIdx.x * kWaves + wave; tile < n_tiles; tile += gridDim.x * kWaves) {
        const uint32_t px = tile * 32 + j;
        const bool live = px < P;
        // ---- torso net: sigmoid', last layer transposed, ReLU masks
        f32x16 g = zero16();
        {
            float d[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (live) {
                if (p.g_alpha) {
                    const float y = p.alpha[px];
                    d[0] = p.g_alpha[px] * ((1.0f - y) * y);
                }
                if (p.g_color) {
#pragma unroll
                    for (int c = 0; c < 3; c++) {
                        const float y = p.color[3 * (size_t)px + c];
                        d[1 + c] = p.g_color[3 * (size_t)px + c] * ((1.0f - y) * y);
                    }
                }
            }
            if (h == 0) {
#pragma unroll
                for (int o = 0; o < 4; o++) ws.dto[4 * (size_t)px + o] = d[o];
            }
#pragma unroll
            for (int o = 0; o < 4; o++) {
                const float *wo = lds + B_T2 + (o * 2 + h) * 16;
#pragma unroll
                for (int r = 0; r < 16; r++) g[r] = __builtin_fmaf(wo[r], d[o], g[r]);
            }
        }
        relu_mask16(g, ws.ht1 + (size_t)tile * kTile16, lane);
        store16(ws.dzt1 + (size_t)tile * kTile16, g, lane);
        f32x16 w = zero16();
#pragma unroll
        for (int s = 0; s < 16; s++) w = mfma32(lds[B_T1 + s * kS32 + lane_off32], g[s], w);
        relu_mask16(w, ws.ht0 + (size_t)tile * kTile16, lane);
        store16(ws.dzt0 + (size_t)tile * kTile16, w, lane);
        // d grid features: register 2 q + c of half h = (level 2 q + h, channel c); nothing flows back into enc_x
        f32x16 xg = zero16();
#pragma unroll
        for (int s = 0; s < 16; s++) xg = mfma32(lds[B_T0 + s * kS32 + lane_off32], w[s], xg);
        // ---- the grid: feature gradients out (level-major), input gradient = sum_l g . dy_dx (gridencoder.cu:342-368); the
        // encoder sees (u + 1) / 2 (gridencoder/grid.py:151, bound = 1): a factor 1/2 on the way back
        float da[2] = {0.0f, 0.0f};
        {
            const float *dw = ws.dw + (size_t)tile * kTile32;
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const float g0 = xg[2 * q], g1 = xg[2 * q + 1];
                const float d00 = dw[(4 * q + 0) * 64 + lane], d01 = dw[(4 * q + 1) * 64 + lane];
                const float d10 = dw[(4 * q + 2) * 64 + lane], d11 = dw[(4 * q + 3) * 64 + lane];
                da[0] = __builtin_fmaf(g0, d00, da[0]); da[0] = __builtin_fmaf(g1, d01, da[0]);
                da[1] = __builtin_fmaf(g0, d10, da[1]); da[1] = __builtin_fmaf(g1, d11, da[1]);
                if (live) *reinterpret_cast<float2 *>(p.g_feat + ((size_t)(2 * q + h) * p.P + px) * 2) = make_float2(g0, g1);
            }
            da[0] += __shfl_xor(da[0], 32, 64);
            da[1] += __shfl_xor(da[1], 32, 64);
        }
        // ---- the clamp (passes where -1 <= x + dx <= 1), + the direct gradient of dx; deformation net transposed
        Acc32 gd, wd;
        {
            float d[2] = {0.0f, 0.0f};
            if (live) {
                const float *mk = ws.mask + (size_t)tile * kTile2;
                d[0] = mk[lane] != 0.0f ? 0.5f * da[0] : 0.0f;
                d[1] = mk[64 + lane] != 0.0f ? 0.5f * da[1] : 0.0f;
                if (p.g_dx) { d[0] += p.g_dx[2 * (size_t)px]; d[1] += p.g_dx[2 * (size_t)px + 1]; }
            }
            if (h == 0) { ws.ddx[2 * (size_t)px] = d[0]; ws.ddx[2 * (size_t)px + 1] = d[1]; }
            acc_zero(gd);
            valu_out_T<2>(gd, lds + B_D2, h, d);
        }
        relu_mask(gd, ws.hd1 + (size_t)tile * kTile32, lane);
        tile_store(ws.dzd1 + (size_t)tile * kTile32, gd, lane);
        acc_zero(wd);
        layer_from_acc(wd, gd, lds + B_D1, lane_off);
        relu_mask(wd, ws.hd0 + (size_t)tile * kTile32, lane);
        tile_store(ws.dzd0 + (size_t)tile * kTile32, wd, lane);
    }
}

// ---- weight gradients ---------------------------------------------------------------------------------------------------
// The pipeline and the operand family OpT are rn_wgrad_dev.h; here are the operands of the torso's six jobs.
using wgrad::OpT;
using wgrad::PHI_ENC;
using wgrad::PHI_STD;
using wgrad::RJob;

constexpr int kJobs = 6;
enum { J_D0 = 0, J_D1, J_D2, J_T0, J_T1, J_T2 };
typedef OpT<0, 32, PHI_STD, 0, 0, false> OpN64;            // a 64-feature native tile
typedef OpT<0, 16, PHI_STD, 0, 0, false> OpN32;            // a 32-feature native tile
typedef OpT<2, 0, 0, 0, 0, false> OpRm2;
typedef OpT<4, 0, 0, 0, 0, false> OpRm4;
typedef OpT<0, 0, 0, 0, 0, true, true> OpFreq1;            // [enc_x | 1], enc_x computed from xy
typedef OpT<0, 16, PHI_ENC, 0, 0, true, true> OpEncFreq1;  // [grid | enc_x | 1]

struct WArgs {
    float *ws;
    const float *xy;
    float shrink;
    uint32_t P;
    const int32_t *p_dev;
    uint32_t parts;
    float *partial;     // [kJobs][parts][wgrad::kPartial]
};

__global__ void __launch_bounds__(wgrad::kThreads, 2) k_train_torso_wgrad(WArgs p) {
    __shared__ __attribute__((aligned(16))) float lds[wgrad::kLdsFloats];
    const uint32_t job = blockIdx.x / p.parts, part = blockIdx.x % p.parts;
    const uint32_t M = live_count(p.P, p.p_dev), n_tiles = (M + 31u) >> 5;
    const Ws w = make_ws(p.ws, p.P);
    float *partial = p.partial + (size_t)job * p.parts * wgrad::kPartial;
    auto nat64 = [&](const float *s) { return OpN64{nullptr, s}; };
    auto nat32 = [&](const float *s) { return OpN32{nullptr, s}; };
    switch (job) {
    case J_D0: wgrad::run(nat64(w.dzd0), OpFreq1{nullptr, nullptr, nullptr, p.xy, p.shrink, M}, n_tiles, M, part, p.parts, partial, lds); break;
    case J_D1: wgrad::run(nat64(w.dzd1), nat64(w.hd0), n_tiles, M, part, p.parts, partial, lds); break;
    case J_D2: wgrad::run(OpRm2{w.ddx}, nat64(w.hd1), n_tiles, M, part, p.parts, partial, lds); break;
    case J_T0: wgrad::run(nat32(w.dzt0), OpEncFreq1{nullptr, w.eg, nullptr, p.xy, p.shrink, M}, n_tiles, M, part, p.parts, partial, lds); break;
    case J_T1: wgrad::run(nat32(w.dzt1), nat32(w.ht0), n_tiles, M, part, p.parts, partial, lds); break;
    default: wgrad::run(OpRm4{w.dto}, nat32(w.ht1), n_tiles, M, part, p.parts, partial, lds); break;
    }
}

typedef wgrad::RArgs<kJobs> RArgs;
__global__ void __launch_bounds__(256) k_train_torso_wreduce(RArgs p) { wgrad::wreduce_jobs(p); }

// The constant columns [enc_pose | c] entered the first layers as biases (k_train_torso_pack).  With b_def [64] / b_tor [32] the
// bias gradients:  gW_def0[:, 42:] = b_def (x) [enc_pose | c],  gW_tor0[:, 74:] = b_tor (x) [enc_pose | c],
//                  g_c = W_def0[:, 96:]^T b_def + W_tor0[:, 128:]^T b_tor
struct CArgs {
    RawT w;
    const float *enc_pose, *ind_code;
    const float *gb;    // b_def [64] | b_tor [32]
    float *g_d0, *g_t0, *g_c;
};
__global__ void __launch_bounds__(256) k_train_torso_const(CArgs p) {
    const uint32_t n = 54 + p.w.ind_dim, ldD0 = 96 + p.w.ind_dim, ldT0 = 128 + p.w.ind_dim;
    if (blockIdx.x < 2) {
        const bool is_def = blockIdx.x == 0;
        const uint32_t rows = is_def ? 64 : 32, ld = is_def ? ldD0 : ldT0, c0 = is_def ? 42 : 74;
        const float *gb = p.gb + (is_def ? 0 : 64);
        float *gW = is_def ? p.g_d0 : p.g_t0;
        for (uint32_t e = threadIdx.x; e < rows * n; e += 256) {
            const uint32_t u = e / n, a = e - u * n;
            gW[u * ld + c0 + a] = gb[u] * (a < 54 ? p.enc_pose[a] : p.ind_code[a - 54]);
        }
    } else if (p.g_c) {
        for (uint32_t a = threadIdx.x; a < p.w.ind_dim; a += 256) {
            float s = 0.0f;
            for (uint32_t u = 0; u < 64; u++) s += p.w.def_w0[u * ldD0 + 96 + a] * p.gb[u];
            for (uint32_t u = 0; u < 32; u++) s += p.w.tor_w0[u * ldT0 + 128 + a] * p.gb[64 + u];
            p.g_c[a] = s;
        }
    }
}

// ---- loss of a torso step -------------------------------------------------------------------------------------------------
// Scatter-back of the compact rows, blend over the background, MSE + entropy and their gradients (nerf/renderer.py:286-302,
// nerf/utils.py:749, 783-791), one pass over the N pixels in k_train_head_loss's shape: one workgroup, a double accumulator, a
// fixed summation order.  `covered` is ascending (rn_torso_select), so pixel n finds its compact row by bisection instead of
// through a scattered index map that would have to be written and read back inside the launch; every output element has one
// writer.  Uncovered pixels: alpha 0, pred = bg bit for bit, and their share of both means.
constexpr int kLossThreads = 1024;
__global__ void __launch_bounds__(kLossThreads)
k_train_torso_loss(const float *__restrict__ alpha_c, const float *__restrict__ color_c, const int32_t *__restrict__ covered, uint32_t P,
                   const int32_t *__restrict__ p_dev, const float *__restrict__ bg, uint32_t bg_stride, const float *__restrict__ target,
                   uint32_t target_stride, uint32_t N, float *__restrict__ loss, float *__restrict__ pred, float *__restrict__ alpha_full,
                   float *__restrict__ g_alpha_c, float *__restrict__ g_color_c) {
    __shared__ double red[kLossThreads / kWave];
    const uint32_t count = live_count(P, p_dev);
    const float inv_n = 1.0f / (float)N;
    double acc = 0.0;
    for (uint32_t n = threadIdx.x; n < N; n += kLossThreads) {
        uint32_t lo = 0, hi = count;                 // first row whose pixel index is >= n
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if ((uint32_t)covered[mid] < n) lo = mid + 1; else hi = mid;
        }
        const bool on = lo < count && (uint32_t)covered[lo] == n;
        const float w = on ? alpha_c[lo] : 0.0f;
        float mse = 0.0f, ga = 0.0f;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float b = bg[(size_t)n * bg_stride + c];
            const float col = on ? color_c[3 * (size_t)lo + c] : 0.0f;
            const float pr = on ? col * w + b * (1.0f - w) : b;      // renderer.py:299
            pred[3 * (size_t)n + c] = pr;
            const float d = pr - target[(size_t)n * target_stride + c];
            mse += d * d;
            const float gp = 2.0f * d * (inv_n / 3.0f);
            if (on) g_color_c[3 * (size_t)lo + c] = w * gp;
            ga += (col - b) * gp;
        }
        alpha_full[n] = w;
        const float a = fminf(fmaxf(w, 1e-5f), 1.0f - 1e-5f);
        const float la = log2f(a), lb = log2f(1.0f - a);
        const float ent = -a * la - (1.0f - a) * lb;
        const bool inside = w >= 1e-5f && w <= 1.0f - 1e-5f;         // clamp passes the gradient on [1e-5, 1 - 1e-5]
        if (on) g_alpha_c[lo] = ga + (inside ? 1e-4f * inv_n * (lb - la) : 0.0f);
        acc += (double)(mse / 3.0f) * inv_n + 1e-4 * (double)ent * inv_n;
    }
    const double t = block_sum_first<double, kLossThreads>(acc, red);
    if (threadIdx.x == 0) loss[0] = (float)t;
}

constexpr uint32_t kWPartsMax = 128;
constexpr uint32_t kBlocksMax = 1u << 16;
// workgroups of the forward / backward launch: one per kWaves tiles, at most one round of two per CU; RN_TORSO_TRAIN_BLOCKS caps
// it further (read at every launch: a test runs the grid-stride loop at a small P with it)
static uint32_t launch_blocks(uint32_t P) {
    const uint32_t blocks = tile_blocks((P + 31u) >> 5, kWaves, 2);
    const uint32_t knob = env_uint_clamped("RN_TORSO_TRAIN_BLOCKS", kBlocksMax, kBlocksMax);
    return blocks < knob ? blocks : knob;
}
static uint32_t wparts(uint32_t P) {   // workgroups (= partial sums) per weight-gradient job: never more than tiles
    static const uint32_t n = env_uint_clamped("RN_TORSO_TRAIN_WPARTS", 64, kWPartsMax);
    const uint32_t n_tiles = (P + 31u) >> 5;
    return n < n_tiles ? n : n_tiles;
}

}  // namespace tt
}  // namespace rn

using namespace rn;
using namespace rn::tt;

extern "C" {

size_t rn_train_torso_image_floats(void) { return (size_t)kImage; }
size_t rn_train_torso_workspace_floats(uint32_t P) { return (size_t)((P + 31u) >> 5) * kWsPerTile; }
size_t rn_train_torso_wgrad_workspace(void) { return ((size_t)kJobs * kWPartsMax * wgrad::kPartial + 128) * sizeof(float); }

int rn_train_torso_pack(const rn_torso_weights_t *w, const float *poses6, const float *ind_code, float *image, rn_stream_t stream) {
    if (int rc = check_torso_weights(w, "train_torso_pack")) return rc;
    RN_REQUIRE(poses6 && image, "train_torso_pack: null pointer");
    RN_REQUIRE(ind_code || w->ind_dim == 0, "train_torso_pack: null pointer (ind_code with ind_dim > 0)");
    RN_REQUIRE(((uintptr_t)image & 15u) == 0, "train_torso_pack: image must be 16-byte aligned");
    hipLaunchKernelGGL(k_train_torso_pack, dim3(kPackBlocks + 1), dim3(256), 0, as_stream(stream), raw_t(w), poses6, ind_code, image);
    return check_launch("train_torso_pack");
}

int rn_train_torso_forward(const float *xy, uint32_t P, const int32_t *p_dev, float torso_shrink, const rn_grid_t *grid_torso,
                           const float *image, float *alpha, float *color, float *dx, float *wn, float *workspace,
                           rn_stream_t stream) {
    if (P == 0) return RN_OK;
    if (int rc = check_train_grid(grid_torso, 2, "train_torso_forward: torso")) return rc;
    RN_REQUIRE(xy && image && alpha && color && dx && wn && workspace, "train_torso_forward: null pointer");
    RN_REQUIRE(((uintptr_t)image & 15u) == 0 && ((uintptr_t)workspace & 15u) == 0, "train_torso_forward: image / workspace must be 16-byte aligned");
    RN_REQUIRE(((uintptr_t)grid_torso->embeddings & 7u) == 0, "train_torso_forward: the table must be 8-byte aligned");
    RN_REQUIRE(torso_shrink > 0.0f, "train_torso_forward: torso_shrink must be positive");
    FwdParams p{xy, P, p_dev, torso_shrink, grid_args(grid_torso), image, alpha, color, dx, wn, workspace};
    hipLaunchKernelGGL(k_train_torso_fwd, dim3(launch_blocks(P)), dim3(kThreads), 0, as_stream(stream), p);
    return check_launch("train_torso_forward");
}

int rn_train_torso_backward(const float *grad_alpha, const float *grad_color, const float *grad_dx, const float *alpha,
                            const float *color, uint32_t P, const int32_t *p_dev, const float *image, float *workspace,
                            float *grad_feat, rn_stream_t stream) {
    if (P == 0) return RN_OK;
    RN_REQUIRE(alpha && color && image && workspace && grad_feat, "train_torso_backward: null pointer");
    RN_REQUIRE(((uintptr_t)image & 15u) == 0 && ((uintptr_t)workspace & 15u) == 0, "train_torso_backward: image / workspace must be 16-byte aligned");
    RN_REQUIRE(((uintptr_t)grad_feat & 7u) == 0, "train_torso_backward: feature gradients must be 8-byte aligned");
    BwdParams p{grad_alpha, grad_color, grad_dx, alpha, color, P, p_dev, image, workspace, grad_feat};
    hipLaunchKernelGGL(k_train_torso_bwd, dim3(launch_blocks(P)), dim3(kThreads), 0, as_stream(stream), p);
    return check_launch("train_torso_backward");
}

int rn_train_torso_weight_grads(const rn_torso_weights_t *w, const float *xy, float torso_shrink, const float *ind_code, uint32_t P,
                                const int32_t *p_dev, const float *image, const float *workspace,
                                const rn_train_torso_grads_t *g, void *wgrad_workspace, rn_stream_t stream) {
    if (P == 0) return RN_OK;
    if (int rc = check_torso_weights(w, "train_torso_weight_grads")) return rc;
    RN_REQUIRE(xy && image && workspace && g && wgrad_workspace, "train_torso_weight_grads: null pointer");
    RN_REQUIRE(g->def_w0 && g->def_w1 && g->def_w2 && g->tor_w0 && g->tor_w1 && g->tor_w2, "train_torso_weight_grads: null gradient pointer");
    RN_REQUIRE(w->ind_dim == 0 || (ind_code && g->ind_code), "train_torso_weight_grads: null pointer (ind_code with ind_dim > 0)");
    RN_REQUIRE(((uintptr_t)workspace & 15u) == 0 && ((uintptr_t)wgrad_workspace & 15u) == 0,
               "train_torso_weight_grads: workspaces must be 16-byte aligned");
    RN_REQUIRE(torso_shrink > 0.0f, "train_torso_weight_grads: torso_shrink must be positive");
    hipStream_t s = as_stream(stream);
    float *partial = static_cast<float *>(wgrad_workspace);
    float *gb = partial + (size_t)kJobs * kWPartsMax * wgrad::kPartial;
    WArgs a{const_cast<float *>(workspace), xy, torso_shrink, P, p_dev, wparts(P), partial};
    hipLaunchKernelGGL(k_train_torso_wgrad, dim3(kJobs * a.parts), dim3(wgrad::kThreads), 0, s, a);
    const uint32_t ldD0 = 96 + w->ind_dim, ldT0 = 128 + w->ind_dim;
    RArgs r{};
    r.partial = partial;
    r.parts = a.parts;
    r.job[J_D0] = RJob{g->def_w0, 64, 42, ldD0, 42, gb};
    r.job[J_D1] = RJob{g->def_w1, 64, 64, 64, -1, nullptr};
    r.job[J_D2] = RJob{g->def_w2, 2, 64, 64, -1, nullptr};
    r.job[J_T0] = RJob{g->tor_w0, 32, 74, ldT0, 74, gb + 64};
    r.job[J_T1] = RJob{g->tor_w1, 32, 32, 32, -1, nullptr};
    r.job[J_T2] = RJob{g->tor_w2, 4, 32, 32, -1, nullptr};
    hipLaunchKernelGGL(k_train_torso_wreduce, dim3(div_up(wgrad::kPartial, 256), kJobs), dim3(256), 0, s, r);
    CArgs c{raw_t(w), image + kFwd + kBwd + C_POSE, ind_code, gb, g->def_w0, g->tor_w0, w->ind_dim ? g->ind_code : nullptr};
    hipLaunchKernelGGL(k_train_torso_const, dim3(3), dim3(256), 0, s, c);
    return check_launch("train_torso_weight_grads");
}

int rn_train_torso_loss(const float *alpha_c, const float *color_c, const int32_t *covered, uint32_t P, const int32_t *p_dev,
                        const float *bg, uint32_t bg_stride, const float *target, uint32_t target_stride, uint32_t N, float *loss,
                        float *pred, float *alpha_full, float *grad_alpha_c, float *grad_color_c, rn_stream_t stream) {
    if (N == 0) return RN_OK;
    RN_REQUIRE(bg && target && loss && pred && alpha_full, "train_torso_loss: null pointer");
    RN_REQUIRE(P == 0 || (alpha_c && color_c && covered && grad_alpha_c && grad_color_c), "train_torso_loss: null pointer (compact rows with P > 0)");
    RN_REQUIRE(bg_stride >= 3 && target_stride >= 3, "train_torso_loss: row strides of bg / target must be at least 3 floats");
    hipLaunchKernelGGL(k_train_torso_loss, dim3(1), dim3(kLossThreads), 0, as_stream(stream), alpha_c, color_c, covered, P, p_dev, bg,
                       bg_stride, target, target_stride, N, loss, pred, alpha_full, grad_alpha_c, grad_color_c);
    return check_launch("train_torso_loss");
}

}  // extern "C"
