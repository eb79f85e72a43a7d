// rn_train_head.hip -- the per-sample network of the TRAINING step as one forward and one backward kernel (gfx950).
//
// C ABI: include/radnerf_train.h.  What is computed: NeRFNetwork.forward (nerf/network.py:222-283) and its autograd as
// Trainer.train_step runs it on the ~60 k samples of a 4096-ray batch (nerf/utils.py:718-806, nerf/renderer.py:206-223).
// How (MI355X-first; the inference kernel's machine, rn_fused.hip, made differentiable):
//
//  * k_train_fwd: one wavefront owns 32 samples; lane half h gathers level 2 r + h in round r, the two features are the B
//    operands of two v_mfma_f32_32x32x2_f32 steps of both first layers that read enc_x; a layer's accumulators (sample on
//    the lane, output row on the register index) ARE the next layer's B operand.  Everything the backward pass needs is
//    stored in that register layout -- a "native tile" is [register][64 lanes] floats, i.e. every store is a coalesced 256-B
//    row: the post-ReLU hidden activations of the five hidden layers, geo_feat, the grid features (they are operands of the
//    weight gradients) and d enc_w / d ambient of the 2-D grid.
//  * k_train_bwd: the same tile walked back.  dX = W^T dY is a forward layer with the transposed weight image, ReLU masks
//    come from the saved activations, tanh' / sigmoid' / trunc_exp' from the saved outputs.  The gradient with respect to
//    the ambient coordinates (sum over levels of g * dy_dx, gridencoder.cu:342-368) is taken inside the tile.  Feature
//    gradients of both grids leave level-major ([L, M, 2]: one coalesced 256-B row per level and lane half).
//  * k_train_wgrad: dW = dZ X^T for all eight layers in one launch, on the weight-gradient machine of rn_wgrad_dev.h (shared
//    with rn_mlp.hip); k_train_wreduce folds its per-workgroup partial sums into the nn.Linear layout.  The columns of the
//    per-call constants (audio code, eye, individual code) ride along as one more feature that is 1 for every sample: its
//    gradient column is the bias gradient, from which k_train_const derives the constants' and their columns' gradients.
// The table gradient of the two grids is rn_grid_scatter.hip.  The text of the backward walk is rn_train_head_walk_dev.h, shared
// with the 16-bit arithmetic (rn_train_head_f16.hip); here are the fp32 contractions it calls.
#include "rn_train_head_walk_dev.h"
#include "rn_wgrad_dev.h"

namespace rn {
namespace th {

// The weight image, the workspace, the parameter blocks and the host side of pack / forward / backward: rn_train_head_dev.h
// (shared with the 16-bit arithmetic).
__global__ void __launch_bounds__(256) k_train_pack(RawW w, const float *__restrict__ enc_a, const float *__restrict__ eye,
                                                    const float *__restrict__ ind_code, const int64_t *__restrict__ ind_index,
                                                    float *__restrict__ image) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= kImage) return;
    if (ind_index) ind_code += (size_t)ind_index[0] * w.ind_dim;   // ind_code = the table individual_codes, row picked on the device
    image[e] = train_image_elem(w, enc_a, eye, ind_code, e);
}

__global__ void __launch_bounds__(kThreads) k_train_fwd(FwdParams p) {
    // gather rounds in flight per wave (xyz grid / ambient grid).  Measured at 62 k samples (tools/bench_train_head.py): <1,1>
    // 82.5 us, <1,2> 82.4, <2,2> 84.5, <2,4> 85.9 -- with one tile per wave the two waves of a SIMD already hide each other's
    // gathers; more rounds in flight only cost registers
    constexpr int GX = 1, GA = 1;
    __shared__ __attribute__((aligned(16))) float lds[kPacked + kBias];
    __shared__ LevelPlan plan_x[16], plan_w[16];
    const uint32_t M = live_count(p.M, p.m_dev);
    const uint32_t n_tiles = (M + 31u) >> 5;
    if (blockIdx.x * kWaves >= n_tiles) return;
    for (int i = threadIdx.x; i < kPacked / 4; i += kThreads) reinterpret_cast<float4 *>(lds)[i] = reinterpret_cast<const float4 *>(p.image)[i];
    if (threadIdx.x < kBias) lds[kPacked + threadIdx.x] = p.image[kPacked + kBwd + threadIdx.x];
    if (threadIdx.x < 16) {
        const int t = threadIdx.x;
        const uint32_t ox = (uint32_t)p.gx.offsets[t], ow = (uint32_t)p.gw.offsets[t];
        plan_x[t] = plan_level<3>(p.gx.lc.scale[t], p.gx.lc.resolution[t], ox, (uint32_t)p.gx.offsets[t + 1] - ox, p.gx.gridtype, 8u);
        plan_w[t] = plan_level<2>(p.gw.lc.scale[t], p.gw.lc.resolution[t], ow, (uint32_t)p.gw.offsets[t + 1] - ow, p.gw.gridtype, 8u);
    }
    __syncthreads();
    const Ws ws = make_ws(p.ws, p.M);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int lane_off = h * 64 + j * 2;
    const float *bias_amb = lds + kPacked, *bias_sig = lds + kPacked + 64, *bias_col = lds + kPacked + 128;
    const float *tx = static_cast<const float *>(p.gx.table), *tw = static_cast<const float *>(p.gw.table);

    for (uint32_t tile = blockIdx.x * kWaves + wave; tile < n_tiles; tile += gridDim.x * kWaves) {
        const uint32_t sample = tile * 32 + j;   // both lane halves work on the same 32 samples
        const bool live = sample < M;
        Acc32 a0, a1, a2;
        acc_bias(a0, bias_amb, h);   // ambient L0, start = W0[:, 32:] enc_a
        acc_bias(a2, bias_sig, h);   // sigma   L0, start = W0[:, 64] eye
        // ---- xyz grid (gridencoder/grid.py:145-161)
        {
            float in[3] = {0.0f, 0.0f, 0.0f};
            bool on = live;
            if (live) {
#pragma unroll
                for (int d = 0; d < 3; d++) {
                    in[d] = (p.xyzs[3 * (size_t)sample + d] + p.bound) / (2 * p.bound);
                    on = on && !(in[d] < 0 || in[d] > 1);
                }
                if (h == 0) { p.xn[3 * (size_t)sample] = in[0]; p.xn[3 * (size_t)sample + 1] = in[1]; p.xn[3 * (size_t)sample + 2] = in[2]; }
            }
            float *ex = ws.ex + (size_t)tile * kTile16;
            LevelFetch<float, 3, 2> f[GX];
#pragma unroll 1
            for (int r0 = 0; r0 < 8; r0 += GX) {
                if (on) {
#pragma unroll
                    for (int i = 0; i < GX; i++) issue_planned<float, 3, 2, false, false>(tx, plan_x[2 * (r0 + i) + h], in, f[i]);
                }
#pragma unroll
                for (int i = 0; i < GX; i++) {
                    const int r = r0 + i;
                    float f0 = 0.0f, f1 = 0.0f;
                    if (on) {
                        float res[2], dummy[1];
                        blend_level<float, 3, 2, false>(f[i], 0.0f, res, dummy);
                        f0 = res[0];
                        f1 = res[1];
                    }
                    step32(a0, lds + OFF_A0, 2 * r, lane_off, f0);
                    step32(a2, lds + OFF_S0, 2 * r, lane_off, f0);
                    step32(a0, lds + OFF_A0, 2 * r + 1, lane_off, f1);
                    step32(a2, lds + OFF_S0, 2 * r + 1, lane_off, f1);
                    ex[(2 * r) * 64 + lane] = f0;
                    ex[(2 * r + 1) * 64 + lane] = f1;
                }
            }
        }
        // ---- ambient net: [enc_x | enc_a] 96 -> 64 -> 64 -> 2, tanh
        acc_relu(a0);
        tile_store(ws.ha0 + (size_t)tile * kTile32, a0, lane);
        acc_zero(a1);
        layer_from_acc(a1, a0, lds + OFF_A1, lane_off);
        acc_relu(a1);
        tile_store(ws.ha1 + (size_t)tile * kTile32, a1, lane);
        float amb[2];
        valu_out<2>(a1, lds + OFF_A2, h, amb);
        amb[0] = tanhf(amb[0]);
        amb[1] = tanhf(amb[1]);
        // ---- ambient grid (+ d enc_w / d input): enc_w -> sigma L0 steps 16..31
        {
            float in[2] = {(amb[0] + 1.0f) / 2.0f, (amb[1] + 1.0f) / 2.0f};
            const bool on = live && !(in[0] < 0 || in[0] > 1 || in[1] < 0 || in[1] > 1);
            if (live && h == 0) {
                p.ambient[2 * (size_t)sample] = amb[0];
                p.ambient[2 * (size_t)sample + 1] = amb[1];
                if (p.ambient_abs) p.ambient_abs[sample] = fabsf(amb[0]) + fabsf(amb[1]);
                p.wn[2 * (size_t)sample] = in[0];
                p.wn[2 * (size_t)sample + 1] = in[1];
            }
            float *ew = ws.ew + (size_t)tile * kTile16, *dw = ws.dw + (size_t)tile * kTile32;
            LevelFetch<float, 2, 2> f[GA];
#pragma unroll 1
            for (int r0 = 0; r0 < 8; r0 += GA) {
                if (on) {
#pragma unroll
                    for (int i = 0; i < GA; i++) issue_planned<float, 2, 2, false, false>(tw, plan_w[2 * (r0 + i) + h], in, f[i]);
                }
#pragma unroll
                for (int i = 0; i < GA; i++) {
                    const int r = r0 + i;
                    float f0 = 0.0f, f1 = 0.0f, g[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                    if (on) {
                        float res[2], grads[4];
                        blend_level<float, 2, 2, true>(f[i], plan_w[2 * r + h].scale, res, grads);
                        f0 = res[0];
                        f1 = res[1];
#pragma unroll
                        for (int q = 0; q < 4; q++) g[q] = grads[q];
                    }
                    step32(a2, lds + OFF_S0, 16 + 2 * r, lane_off, f0);
                    step32(a2, lds + OFF_S0, 16 + 2 * r + 1, lane_off, f1);
                    ew[(2 * r) * 64 + lane] = f0;
                    ew[(2 * r + 1) * 64 + lane] = f1;
#pragma unroll
                    for (int q = 0; q < 4; q++) dw[(4 * r + q) * 64 + lane] = g[q];
                }
            }
        }
        // ---- sigma net: [enc_x | enc_w | eye] 65 -> 64 -> 64 -> 1 + 64
        acc_relu(a2);
        tile_store(ws.hs0 + (size_t)tile * kTile32, a2, lane);
        acc_zero(a1);
        layer_from_acc(a1, a2, lds + OFF_S1, lane_off);
        acc_relu(a1);
        tile_store(ws.hs1 + (size_t)tile * kTile32, a1, lane);
        {
            float raw[1];
            valu_out<1>(a1, lds + OFF_S2R, h, raw);
            if (h == 0) {
                ws.sraw[sample] = raw[0];
                if (live) p.sigmas[sample] = expf(raw[0]);   // trunc_exp forward (activation.py:9-11)
            }
        }
        acc_zero(a0);
        layer_from_acc(a0, a1, lds + OFF_S2, lane_off);   // geo_feat (no activation)
        tile_store(ws.geo + (size_t)tile * kTile32, a0, lane);
        // ---- color net: [SH(d) | geo_feat | ind_code] 84 -> 64 -> 3, sigmoid
        acc_bias(a1, bias_col, h);
        {
            float sh[16];
            float dx = 0.0f, dy = 0.0f, dz = 0.0f;
            if (live) {
                dx = p.dirs[3 * (size_t)sample]; dy = p.dirs[3 * (size_t)sample + 1]; dz = p.dirs[3 * (size_t)sample + 2];
            }
            sh_basis<4>(dx, dy, dz, sh);
            float *st = ws.sh + (size_t)tile * kTile8;
#pragma unroll
            for (int s = 0; s < 8; s++) {
                const float b = select_h(sh[2 * s], sh[2 * s + 1], h);   // lane half h supplies k = 2 s + h
                step32(a1, lds + OFF_C0, s, lane_off, b);
                st[s * 64 + lane] = b;
            }
        }
#pragma unroll
        for (int s = 0; s < 32; s++) step32(a1, lds + OFF_C0, 8 + s, lane_off, a0.v[s >> 4][s & 15]);
        acc_relu(a1);
        tile_store(ws.hc0 + (size_t)tile * kTile32, a1, lane);
        {
            float rgb[3];
            valu_out<3>(a1, lds + OFF_C1, h, rgb);
            if (live && h == 0) {
#pragma unroll
                for (int c = 0; c < 3; c++) p.rgbs[3 * (size_t)sample + c] = 1.0f / (1.0f + expf(-rgb[c]));
            }
        }
    }
}

// The fp32 arithmetic of the backward tile walk (rn_train_head_walk_dev.h): v_mfma_f32_32x32x2_f32, one float of B per lane and
// step, k in kmap order.  LDS = transposed image | narrow rows.
struct ArithF32 {
    static constexpr int kLdsBwd = kBwd;
    static constexpr int RT_C1 = N_C1, RT_S2R = N_S2R, RT_A2 = N_A2;
    static constexpr int WT_C0 = T_C0, WT_S2 = T_S2, WT_S1 = T_S1, WT_S0 = T_S0, WT_A1 = T_A1;   // floats into the LDS
    const float *lds;
    int lane_off, j, h;
    __device__ ArithF32(const float *l, int j_, int h_) : lds(l), lane_off(h_ * 64 + j_ * 2), j(j_), h(h_) {}

    static __device__ __forceinline__ void fill_bwd(float *lds, const float *image) {
        for (int i = threadIdx.x; i < kBwd / 4; i += kThreads) reinterpret_cast<float4 *>(lds)[i] = reinterpret_cast<const float4 *>(image + kPacked)[i];
    }
    __device__ __forceinline__ void layer_T(Acc32 &out, const Acc32 &dy, int at) const {
        acc_zero(out);
        layer_from_acc(out, dy, lds + at, lane_off);
    }
    __device__ __forceinline__ void a0_T(f32x16 &x0, const Acc32 &dz) const {
#pragma unroll
        for (int s = 0; s < 32; s++) x0 = mfma32(lds[T_A0 + s * 64 + h * 32 + j], dz.v[s >> 4][s & 15], x0);
    }
};

__global__ void __launch_bounds__(kThreads) k_train_bwd(BwdParams p) {
    __shared__ __attribute__((aligned(16))) float lds[ArithF32::kLdsBwd];
    train_bwd_tiles<ArithF32>(p, lds);
}

// ---- input gradients (--train_camera) -----------------------------------------------------------------------------------
// d loss / d xyzs and d loss / d dirs from what k_train_bwd left behind.  The tile and lane roles are the forward's: one wavefront
// owns 32 samples, lane half h walks levels 2 r + h.
//  * xyzs: the corners of every level are gathered AGAIN (same plan, same loads as k_train_fwd, so the same cell) and blended
//    with the DYDX form of blend_level; grad = sum_l sum_c g_enc_x[l, b, c] * dy_dx[b, l, :, c] / (2 bound)
//    (gridencoder.cu:342-368 + the normalisation of gridencoder/grid.py:151).  A sample outside [0, 1] gets exactly 0
//    (gridencoder.cu:146-156 leaves its dy_dx zero).
//  * dirs: g_sh[k] = sum_o W_col0[o][k] dzc0[b, o] (k < 16) from the native dzc0 tile -- a lane holds 32 of the 64 rows o of
//    its sample, W_col0[:, 0:16] sits in LDS row-major, both lane halves read one row each (broadcast) -- then
//    J_SH(dirs[b])^T g_sh (shencoder.cu:359-382); the two halves' partial sums meet in one shuffle per component.
// Rows from the live count up to the capacity M are written as zeros (they belong to no ray; a consumer that sums every row
// must not meet uninitialised memory).
struct IgParams {
    const float *xn, *dirs, *g_enc_x;
    uint32_t M;
    const int32_t *m_dev;
    GridArgs gx;
    const float *image;
    float *ws;
    float bound;
    float *g_xyzs, *g_dirs;
};
constexpr int kIgThreads = 256, kIgWaves = kIgThreads / kWave;

template <int G>   // gather rounds in flight per wave: nothing but the blend sits between two rounds here, so two hide more latency
__global__ void __launch_bounds__(kIgThreads) k_train_input_grads(IgParams p) {
    __shared__ __attribute__((aligned(16))) float wc0[64 * 16];   // W_col0[o][k], k < 16
    __shared__ LevelPlan plan_x[16];
    const uint32_t M = live_count(p.M, p.m_dev);
    const uint32_t n_live = (M + 31u) >> 5, n_tiles = (p.M + 31u) >> 5;
    for (int e = threadIdx.x; e < 64 * 16; e += kIgThreads) {   // forward image, colour L0, SH steps: [k / 2][k % 2][o % 32][o / 32]
        const int o = e >> 4, k = e & 15;
        wc0[e] = p.image[OFF_C0 + (k >> 1) * kStep + (k & 1) * 64 + (o & 31) * 2 + (o >> 5)];
    }
    if (threadIdx.x < 16) {
        const int t = threadIdx.x;
        const uint32_t ox = (uint32_t)p.gx.offsets[t];
        plan_x[t] = plan_level<3>(p.gx.lc.scale[t], p.gx.lc.resolution[t], ox, (uint32_t)p.gx.offsets[t + 1] - ox, p.gx.gridtype, 8u);
    }
    __syncthreads();
    const Ws ws = make_ws(p.ws, p.M);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, h = lane >> 5;
    const float *tx = static_cast<const float *>(p.gx.table);

    for (uint32_t tile = blockIdx.x * kIgWaves + wave; tile < n_tiles; tile += gridDim.x * kIgWaves) {
        const uint32_t sample = tile * 32 + j;
        const bool live = sample < M;
        float gx[3] = {0.0f, 0.0f, 0.0f}, gd[3] = {0.0f, 0.0f, 0.0f};
        if (tile < n_live) {   // wave-uniform: the tiles past the live count have no saved state, only zeros to write
            // ---- xyz grid
            float in[3] = {0.0f, 0.0f, 0.0f};
            bool on = live;
            if (live) {
#pragma unroll
                for (int d = 0; d < 3; d++) {
                    in[d] = p.xn[3 * (size_t)sample + d];
                    on = on && !(in[d] < 0 || in[d] > 1);
                }
            }
            LevelFetch<float, 3, 2> f[G];
#pragma unroll 1
            for (int r0 = 0; r0 < 8; r0 += G) {
                float2 g[G];
                if (on) {
#pragma unroll
                    for (int i = 0; i < G; i++) {
                        issue_planned<float, 3, 2, false, false>(tx, plan_x[2 * (r0 + i) + h], in, f[i]);
                        g[i] = *reinterpret_cast<const float2 *>(p.g_enc_x + ((size_t)(2 * (r0 + i) + h) * p.M + sample) * 2);
                    }
#pragma unroll
                    for (int i = 0; i < G; i++) {
                        float res[2], dydx[6];
                        blend_level<float, 3, 2, true>(f[i], plan_x[2 * (r0 + i) + h].scale, res, dydx);
#pragma unroll
                        for (int d = 0; d < 3; d++) {
                            gx[d] = __builtin_fmaf(g[i].x, dydx[2 * d], gx[d]);
                            gx[d] = __builtin_fmaf(g[i].y, dydx[2 * d + 1], gx[d]);
                        }
                    }
                }
            }
            // ---- SH: this lane's 32 rows of dzc0 against W_col0[:, 0:16]
            float gs[16];
#pragma unroll
            for (int k = 0; k < 16; k++) gs[k] = 0.0f;
            const float *dz = ws.dzc0 + (size_t)tile * kTile32;
            // (a rolled loop on purpose: fully unrolled, the 512 weights a lane reads are invariant over the tile loop and the
            // compiler keeps them all in registers)
#pragma unroll 4
            for (int q = 0; q < 32; q++) {
                const float d = dz[q * 64 + lane];
                const float4 *wr = reinterpret_cast<const float4 *>(wc0 + (32 * (q >> 4) + rowmap(q & 15, 0) + 4 * h) * 16);
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const float4 w = wr[u];
                    gs[4 * u + 0] = __builtin_fmaf(w.x, d, gs[4 * u + 0]);
                    gs[4 * u + 1] = __builtin_fmaf(w.y, d, gs[4 * u + 1]);
                    gs[4 * u + 2] = __builtin_fmaf(w.z, d, gs[4 * u + 2]);
                    gs[4 * u + 3] = __builtin_fmaf(w.w, d, gs[4 * u + 3]);
                }
            }
            float dx = 0.0f, dy = 0.0f, dzz = 0.0f;
            if (live) {
                dx = p.dirs[3 * (size_t)sample]; dy = p.dirs[3 * (size_t)sample + 1]; dzz = p.dirs[3 * (size_t)sample + 2];
            }
            float jac[16];
            sh_jac<4, 0>(dx, dy, dzz, jac);
#pragma unroll
            for (int k = 1; k < 16; k++) gd[0] = __builtin_fmaf(jac[k], gs[k], gd[0]);   // k = 0: the constant term
            sh_jac<4, 1>(dx, dy, dzz, jac);
#pragma unroll
            for (int k = 1; k < 16; k++) gd[1] = __builtin_fmaf(jac[k], gs[k], gd[1]);
            sh_jac<4, 2>(dx, dy, dzz, jac);
#pragma unroll
            for (int k = 1; k < 16; k++) gd[2] = __builtin_fmaf(jac[k], gs[k], gd[2]);
        }
#pragma unroll
        for (int d = 0; d < 3; d++) {
            gx[d] += __shfl_xor(gx[d], 32, 64);
            gd[d] += __shfl_xor(gd[d], 32, 64);
        }
        if (sample < p.M) {   // lane half 0 writes the position row, lane half 1 the direction row
            float *dst = (h == 0 ? p.g_xyzs : p.g_dirs) + 3 * (size_t)sample;
#pragma unroll
            for (int d = 0; d < 3; d++) dst[d] = live ? (h == 0 ? gx[d] / (2 * p.bound) : gd[d]) : 0.0f;
        }
    }
}

// ---- weight gradients ---------------------------------------------------------------------------------------------------
// The pipeline (staged tiles, prefetch schedule, multiply, partial store, reduce) and the operand family OpT are
// rn_wgrad_dev.h; here are the operands of the head's eight jobs.
using wgrad::OpT;
using wgrad::PHI_ENC;
using wgrad::PHI_SH;
using wgrad::PHI_STD;
using wgrad::RJob;

constexpr int kJobs = 8;
enum { J_A0 = 0, J_A1, J_A2, J_S0, J_S1, J_S2, J_C0, J_C1 };
typedef OpT<0, 32, PHI_STD, 0, 0, false> OpStd;                 // a 64-feature native tile
typedef OpT<0, 16, PHI_ENC, 0, 0, true> OpEncX1;                // [enc_x | 1]
typedef OpT<0, 16, PHI_ENC, 16, PHI_ENC, true> OpEncXW1;        // [enc_x | enc_w | 1]
typedef OpT<0, 8, PHI_SH, 32, PHI_STD, true> OpShGeo1;          // [sh | geo_feat | 1]
typedef OpT<2, 0, 0, 0, 0, false> OpRm2;
typedef OpT<3, 0, 0, 0, 0, false> OpRm3;
typedef OpT<1, 32, PHI_STD, 0, 0, false> OpRm1Std;              // [d sigma_raw | d geo_feat]

struct WArgs {
    float *ws;
    uint32_t M;
    const int32_t *m_dev;
    uint32_t parts;
    float *partial;     // [kJobs][parts][wgrad::kPartial]
};

__global__ void __launch_bounds__(wgrad::kThreads, 2) k_train_wgrad(WArgs p) {
    __shared__ __attribute__((aligned(16))) float lds[wgrad::kLdsFloats];
    const uint32_t job = blockIdx.x / p.parts, part = blockIdx.x % p.parts;
    const uint32_t M = live_count(p.M, p.m_dev), n_tiles = (M + 31u) >> 5;
    const Ws w = make_ws(p.ws, p.M);
    float *partial = p.partial + (size_t)job * p.parts * wgrad::kPartial;
    switch (job) {
    case J_A0: wgrad::run(OpStd{nullptr, w.dza0, nullptr}, OpEncX1{nullptr, w.ex, nullptr}, n_tiles, M, part, p.parts, partial, lds); break;
    case J_A1: wgrad::run(OpStd{nullptr, w.dza1, nullptr}, OpStd{nullptr, w.ha0, nullptr}, n_tiles, M, part, p.parts, partial, lds); break;
    case J_A2: wgrad::run(OpRm2{w.daraw, nullptr, nullptr}, OpStd{nullptr, w.ha1, nullptr}, n_tiles, M, part, p.parts, partial, lds); break;
    case J_S0: wgrad::run(OpStd{nullptr, w.dzs0, nullptr}, OpEncXW1{nullptr, w.ex, w.ew}, n_tiles, M, part, p.parts, partial, lds); break;
    case J_S1: wgrad::run(OpStd{nullptr, w.dzs1, nullptr}, OpStd{nullptr, w.hs0, nullptr}, n_tiles, M, part, p.parts, partial, lds); break;
    case J_S2: wgrad::run(OpRm1Std{w.dsraw, w.dgeo, nullptr}, OpStd{nullptr, w.hs1, nullptr}, n_tiles, M, part, p.parts, partial, lds); break;
    case J_C0: wgrad::run(OpStd{nullptr, w.dzc0, nullptr}, OpShGeo1{nullptr, w.sh, w.geo}, n_tiles, M, part, p.parts, partial, lds); break;
    default: wgrad::run(OpRm3{w.dprec, nullptr, nullptr}, OpStd{nullptr, w.hc0, nullptr}, n_tiles, M, part, p.parts, partial, lds); break;
    }
}

typedef wgrad::RArgs<kJobs> RArgs;
__global__ void __launch_bounds__(256) k_train_wreduce(RArgs p) { wgrad::wreduce_jobs(p); }

// The per-call constants enter the first layers as biases (k_train_pack).  With gb = the bias gradient [64]:
//   d constant[a] = sum_u W0[u][c0 + a] gb[u]        d W0[u][c0 + a] = gb[u] constant[a]
struct CArgs {
    RawW w;
    const float *enc_a, *eye, *ind_code;
    const float *gb;    // [3][64]
    float *g_a0, *g_s0, *g_c0, *g_enc_a, *g_eye, *g_ind;
    const int64_t *ind_index;   // non-NULL: ind_code / g_ind are the tables [ind_rows, ind_dim]; the row is picked here and the
    uint32_t ind_rows;          // rest of the gradient table is written as zeros (what index_select's backward builds in two launches)
};
__global__ void __launch_bounds__(256) k_train_const(CArgs p) {
    const int which = blockIdx.x;
    const float *W, *c, *gb = p.gb + 64 * which;
    float *gW, *gc;
    uint32_t n, ld, c0;
    if (which >= 3) {           // extra workgroups (row form only): zeros for the other rows of the code gradient table
        const size_t row = (size_t)p.ind_index[0], nd = p.w.ind_dim, total = (size_t)p.ind_rows * nd;
        for (size_t e = (size_t)(which - 3) * 256 + threadIdx.x; e < total; e += (size_t)(gridDim.x - 3) * 256)
            if (e / nd != row) p.g_ind[e] = 0.0f;
        return;
    }
    if (which == 0) { W = p.w.amb_w0; c = p.enc_a; gW = p.g_a0; gc = p.g_enc_a; n = p.w.audio_dim; c0 = 32; }
    else if (which == 1) { W = p.w.sig_w0; c = p.eye; gW = p.g_s0; gc = p.g_eye; n = p.w.has_eye; c0 = 64; }
    else {
        W = p.w.col_w0; c = p.ind_code; gW = p.g_c0; gc = p.g_ind; n = p.w.ind_dim; c0 = 80;
        if (p.ind_index) { c += (size_t)p.ind_index[0] * n; if (gc) gc += (size_t)p.ind_index[0] * n; }
    }
    ld = c0 + n;
    for (uint32_t e = threadIdx.x; e < 64 * n; e += 256) {
        const uint32_t u = e / n, a = e - u * n;
        gW[u * ld + c0 + a] = gb[u] * c[a];
    }
    for (uint32_t a = threadIdx.x; a < n; a += 256) {
        float s = 0.0f;
        for (uint32_t u = 0; u < 64; u++) s += W[u * ld + c0 + a] * gb[u];
        if (gc) gc[a] = s;
    }
}

// ---- loss on the composited rays -----------------------------------------------------------------------------------------
constexpr int kLossThreads = 1024;
__global__ void __launch_bounds__(kLossThreads) k_train_head_loss(const float *__restrict__ image, const float *__restrict__ ws,
                                                                  const float *__restrict__ ambient, const float *__restrict__ bg,
                                                                  uint32_t bg_stride, const float *__restrict__ target, uint32_t target_stride,
                                                                  const float *__restrict__ face, uint32_t face_stride,
                                                                  const float *__restrict__ w_amb, uint32_t N, float *__restrict__ loss,
                                                                  float *__restrict__ pred, float *__restrict__ g_image,
                                                                  float *__restrict__ g_ws, float *__restrict__ g_amb) {
    __shared__ double red[kLossThreads / kWave];
    const float wa = w_amb[0];
    const float inv_n = 1.0f / (float)N;
    double acc = 0.0;
    for (uint32_t n = threadIdx.x; n < N; n += kLossThreads) {
        const float w = ws[n];
        const float tr = 1.0f - w;                     // nerf/renderer.py:306: image + (1 - weights_sum) * bg, clamp [0, 1]
        float mse = 0.0f, gws_blend = 0.0f;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float b = bg[(size_t)n * bg_stride + c];
            const float raw = image[n * 3 + c] + tr * b;
            const float pr = fminf(fmaxf(raw, 0.0f), 1.0f);
            if (pred) pred[n * 3 + c] = pr;
            const float d = pr - target[(size_t)n * target_stride + c];
            mse += d * d;
            const float gp = (raw >= 0.0f && raw <= 1.0f) ? 2.0f * d * (inv_n / 3.0f) : 0.0f;   // clamp passes the gradient on [0, 1]
            g_image[n * 3 + c] = gp;
            gws_blend -= gp * b;
        }
        const float a = fminf(fmaxf(w, 1e-5f), 1.0f - 1e-5f);
        const float la = log2f(a), lb = log2f(1.0f - a);
        const float ent = -a * la - (1.0f - a) * lb;
        const bool inside = w >= 1e-5f && w <= 1.0f - 1e-5f;
        g_ws[n] = gws_blend + (inside ? 1e-4f * inv_n * (lb - la) : 0.0f);
        const float keep = 1.0f - face[(size_t)n * face_stride];
        g_amb[n] = wa * inv_n * keep;
        acc += (double)(mse / 3.0f) * inv_n + 1e-4 * (double)ent * inv_n + (double)wa * (double)(ambient[n] * keep) * inv_n;
    }
    const double t = block_sum_first<double, kLossThreads>(acc, red);
    if (threadIdx.x == 0) loss[0] = (float)t;
}

// A term on `pred` that the caller computed (the patch / lips term of nerf/utils.py:757-781) joins the loss above: its gradient
// g_pred = d term / d pred goes back through the clamp and the blend into the gradients k_train_head_loss wrote.  One thread per
// ray; `raw` is recomputed by the expression above, so `pass` is the clamp decision the loss kernel took.
__global__ void __launch_bounds__(256) k_train_head_loss_chain(const float *__restrict__ image, const float *__restrict__ ws,
                                                               const float *__restrict__ bg, uint32_t bg_stride,
                                                               const float *__restrict__ g_pred, uint32_t N, const float *__restrict__ term,
                                                               float *__restrict__ loss, float *__restrict__ g_image,
                                                               float *__restrict__ g_ws) {
    const uint32_t n = blockIdx.x * 256 + threadIdx.x;
    if (n == 0) loss[0] += term[0];
    if (n >= N) return;
    const float tr = 1.0f - ws[n];
    float gws = g_ws[n];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float b = bg[(size_t)n * bg_stride + c];
        const float raw = image[n * 3 + c] + tr * b;
        const float gp = (raw >= 0.0f && raw <= 1.0f) ? g_pred[n * 3 + c] : 0.0f;
        g_image[n * 3 + c] += gp;
        gws -= gp * b;
    }
    g_ws[n] = gws;
}

// ---- batch gather ---------------------------------------------------------------------------------------------------------
// A training batch = n rows picked from a per-pixel table [n_px, row_floats] whose columns are up to 8 sections (rays_o | rays_d |
// bg_coords | bg_color | target | face ...): ONE kernel writes every section as its own contiguous [n, width] array (the
// operators want contiguous rays), where stock indexing takes one gather + one strided copy per section.
struct GatherArgs {
    uint32_t width[8], col0[8], out0[8];   // section widths, first column in the table row, first float in `out`
    uint32_t sections, row_floats;
};
__global__ void __launch_bounds__(256) k_batch_gather(const float *__restrict__ table, const int64_t *__restrict__ idx, uint32_t n,
                                                      GatherArgs a, float *__restrict__ out) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n * a.row_floats) return;
    const uint32_t r = t / a.row_floats, c = t - r * a.row_floats;
    uint32_t sec = 0;
    while (sec + 1 < a.sections && c >= a.col0[sec + 1]) sec++;
    out[a.out0[sec] + r * a.width[sec] + (c - a.col0[sec])] = table[(size_t)idx[r] * a.row_floats + c];
}

constexpr uint32_t kWPartsMax = 256;
static uint32_t wparts() {   // workgroups (= partial sums) per weight-gradient job
    static const uint32_t n = env_uint_clamped("RN_TRAIN_WPARTS", 128, kWPartsMax);   // measured at 62 k samples: 64 parts 76 us, 96: 80, 128: 71, 192: 85
    return n;
}

}  // namespace th
}  // namespace rn

using namespace rn;
using namespace rn::th;

extern "C" {

size_t rn_train_head_image_floats(void) { return (size_t)kImage; }
size_t rn_train_head_workspace_floats(uint32_t M) { return (size_t)((M + 31u) >> 5) * kWsPerTile; }
size_t rn_train_head_wgrad_workspace(void) { return ((size_t)kJobs * kWPartsMax * wgrad::kPartial + 192) * sizeof(float); }

int rn_train_head_pack(const rn_nerf_weights_t *w, const float *enc_a, const float *eye, const float *ind_code, float *image,
                       rn_stream_t stream) {
    return pack(k_train_pack, kImage, "train_head_pack", w, enc_a, eye, ind_code, nullptr, false, image, stream);
}

int rn_train_head_pack_row(const rn_nerf_weights_t *w, const float *enc_a, const float *eye, const float *ind_table,
                           const int64_t *ind_index, float *image, rn_stream_t stream) {
    return pack(k_train_pack, kImage, "train_head_pack_row", w, enc_a, eye, ind_table, ind_index, true, image, stream);
}

int rn_train_head_forward(const float *xyzs, const float *dirs, uint32_t M, const int32_t *m_dev, const rn_grid_t *grid_xyz,
                          const rn_grid_t *grid_amb, const float *image, float bound, float *sigmas, float *rgbs,
                          float *ambient, float *ambient_abs, float *xn, float *wn, float *workspace, rn_stream_t stream) {
    return forward(k_train_fwd, "train_head_forward", xyzs, dirs, M, m_dev, grid_xyz, grid_amb, image, bound, sigmas, rgbs, ambient,
                   ambient_abs, xn, wn, workspace, stream);
}

int rn_train_head_backward(const float *grad_sigmas, const float *grad_rgbs, const float *grad_ambient,
                           const float *grad_ambient_abs, const float *rgbs, const float *ambient, uint32_t M,
                           const int32_t *m_dev, const float *image, float *workspace, float *grad_enc_x, float *grad_enc_w,
                           rn_stream_t stream) {
    return backward(k_train_bwd, false, "train_head_backward", grad_sigmas, grad_rgbs, grad_ambient, grad_ambient_abs, rgbs, ambient, M,
                    m_dev, image, workspace, grad_enc_x, grad_enc_w, stream);
}

int rn_train_head_input_grads(const float *xn, const float *dirs, const float *grad_enc_x, uint32_t M, const int32_t *m_dev,
                              const rn_grid_t *grid_xyz, const float *image, const float *workspace, float bound,
                              float *grad_xyzs, float *grad_dirs, rn_stream_t stream) {
    if (M == 0) return RN_OK;
    if (int rc = check_train_grid(grid_xyz, 3, "train_head: xyz")) return rc;
    RN_REQUIRE(xn && dirs && grad_enc_x && image && workspace && grad_xyzs && grad_dirs, "train_head_input_grads: null pointer");
    RN_REQUIRE(((uintptr_t)grad_enc_x & 7u) == 0, "train_head_input_grads: feature gradients must be 8-byte aligned");
    RN_REQUIRE(bound > 0.0f, "train_head_input_grads: bound must be positive");
    IgParams p{xn, dirs, grad_enc_x, M, m_dev, grid_args(grid_xyz), image, const_cast<float *>(workspace), bound, grad_xyzs, grad_dirs};
    // tiles of the capacity: the rows past the live count are zero-filled by the same launch.  110 VGPRs: 4 waves per SIMD = 4
    // workgroups of 4 waves per CU
    const uint32_t blocks = tile_blocks((M + 31u) >> 5, kIgWaves, 4);
    hipLaunchKernelGGL((k_train_input_grads<2>), dim3(blocks), dim3(kIgThreads), 0, as_stream(stream), p);
    return check_launch("train_head_input_grads");
}

static int weight_grads(const rn_nerf_weights_t *w, const float *enc_a, const float *eye, const float *ind_code, const int64_t *ind_index,
                        uint32_t ind_rows, uint32_t M, const int32_t *m_dev, const float *workspace, const rn_train_head_grads_t *g,
                        void *wgrad_workspace, rn_stream_t stream) {
    if (int rc = check_w(w)) return rc;
    RN_REQUIRE(M > 0 && workspace && g && wgrad_workspace, "train_head_weight_grads: null pointer / M == 0");
    RN_REQUIRE(g->amb_w0 && g->amb_w1 && g->amb_w2 && g->sig_w0 && g->sig_w1 && g->sig_w2 && g->col_w0 && g->col_w1,
               "train_head_weight_grads: null gradient pointer");
    RN_REQUIRE((enc_a || w->audio_dim == 0) && (eye || !w->has_eye) && (ind_code || w->ind_dim == 0), "train_head_weight_grads: null constant");
    hipStream_t s = as_stream(stream);
    float *partial = static_cast<float *>(wgrad_workspace);
    float *gb = partial + (size_t)kJobs * kWPartsMax * wgrad::kPartial;
    WArgs a{const_cast<float *>(workspace), M, m_dev, wparts(), partial};
    hipLaunchKernelGGL(k_train_wgrad, dim3(kJobs * a.parts), dim3(wgrad::kThreads), 0, s, a);
    const uint32_t ldA0 = 32 + w->audio_dim, ldS0 = 64 + w->has_eye, ldC0 = 80 + w->ind_dim;
    RArgs r{};
    r.partial = partial;
    r.parts = a.parts;
    r.job[J_A0] = RJob{g->amb_w0, 64, 32, ldA0, 32, gb};
    r.job[J_A1] = RJob{g->amb_w1, 64, 64, 64, -1, nullptr};
    r.job[J_A2] = RJob{g->amb_w2, 2, 64, 64, -1, nullptr};
    r.job[J_S0] = RJob{g->sig_w0, 64, 64, ldS0, 64, gb + 64};
    r.job[J_S1] = RJob{g->sig_w1, 64, 64, 64, -1, nullptr};
    r.job[J_S2] = RJob{g->sig_w2, 65, 64, 64, -1, nullptr};
    r.job[J_C0] = RJob{g->col_w0, 64, 80, ldC0, 80, gb + 128};
    r.job[J_C1] = RJob{g->col_w1, 3, 64, 64, -1, nullptr};
    hipLaunchKernelGGL(k_train_wreduce, dim3(div_up(wgrad::kPartial, 256), kJobs), dim3(256), 0, s, r);
    CArgs c{raw_w(w), enc_a, eye, ind_code, gb, g->amb_w0, g->sig_w0, g->col_w0, g->enc_a, g->eye, g->ind_code, ind_index, ind_rows};
    const uint32_t zero_blocks = ind_index ? (div_up(ind_rows * w->ind_dim, 1024) < 64u ? div_up(ind_rows * w->ind_dim, 1024) : 64u) : 0u;
    hipLaunchKernelGGL(k_train_const, dim3(3 + zero_blocks), dim3(256), 0, s, c);
    return check_launch("train_head_weight_grads");
}

int rn_train_head_weight_grads(const rn_nerf_weights_t *w, const float *enc_a, const float *eye, const float *ind_code,
                               uint32_t M, const int32_t *m_dev, const float *workspace, const rn_train_head_grads_t *g,
                               void *wgrad_workspace, rn_stream_t stream) {
    return weight_grads(w, enc_a, eye, ind_code, nullptr, 0, M, m_dev, workspace, g, wgrad_workspace, stream);
}

int rn_train_head_weight_grads_row(const rn_nerf_weights_t *w, const float *enc_a, const float *eye, const float *ind_table,
                                   const int64_t *ind_index, uint32_t ind_rows, uint32_t M, const int32_t *m_dev, const float *workspace,
                                   const rn_train_head_grads_t *g, void *wgrad_workspace, rn_stream_t stream) {
    RN_REQUIRE(ind_table && ind_index && ind_rows && g && g->ind_code && w && w->ind_dim,
               "train_head_weight_grads_row: the code table, its row index and the gradient table are required");
    return weight_grads(w, enc_a, eye, ind_table, ind_index, ind_rows, M, m_dev, workspace, g, wgrad_workspace, stream);
}

}  // extern "C"

extern "C" {

int rn_train_batch_gather(const float *table, uint32_t row_floats, const int64_t *idx, uint32_t n, const uint32_t *widths,
                          uint32_t sections, float *out, rn_stream_t stream) {
    if (n == 0) return RN_OK;
    RN_REQUIRE(table && idx && widths && out && sections >= 1 && sections <= 8, "train_batch_gather: null pointer / 1 .. 8 sections");
    GatherArgs a{};
    uint32_t col = 0;
    for (uint32_t i = 0; i < sections; i++) {
        RN_REQUIRE(widths[i] > 0, "train_batch_gather: section %u has width 0", i);
        a.width[i] = widths[i];
        a.col0[i] = col;
        a.out0[i] = col * n;      // sections follow each other in `out`: [n, w0] | [n, w1] | ...
        col += widths[i];
    }
    RN_REQUIRE(col == row_floats, "train_batch_gather: the section widths must add up to the row length");
    a.sections = sections;
    a.row_floats = row_floats;
    hipLaunchKernelGGL(k_batch_gather, dim3(div_up(n * row_floats, 256)), dim3(256), 0, as_stream(stream), table, idx, n, a, out);
    return check_launch("train_batch_gather");
}

int rn_train_head_loss(const float *image, const float *weights_sum, const float *ambient, const float *bg, uint32_t bg_stride,
                       const float *target, uint32_t target_stride, const float *face, uint32_t face_stride, const float *w_amb,
                       uint32_t N, float *loss, float *pred, float *grad_image, float *grad_weights_sum, float *grad_ambient,
                       rn_stream_t stream) {
    RN_REQUIRE(N > 0, "train_head_loss: N must be positive");
    RN_REQUIRE(image && weights_sum && ambient && bg && target && face && w_amb && loss && grad_image && grad_weights_sum && grad_ambient,
               "train_head_loss: null pointer");
    hipLaunchKernelGGL(k_train_head_loss, dim3(1), dim3(kLossThreads), 0, as_stream(stream), image, weights_sum, ambient, bg, bg_stride, target,
                       target_stride, face, face_stride, w_amb, N, loss, pred, grad_image, grad_weights_sum, grad_ambient);
    return check_launch("train_head_loss");
}

int rn_train_head_loss_chain(const float *image, const float *weights_sum, const float *bg, uint32_t bg_stride, const float *g_pred,
                             uint32_t N, const float *term, float *loss, float *grad_image, float *grad_weights_sum,
                             rn_stream_t stream) {
    RN_REQUIRE(N > 0 && N <= (1u << 30), "train_head_loss_chain: N must be in [1, 2^30]");
    RN_REQUIRE(image && weights_sum && bg && g_pred && term && loss && grad_image && grad_weights_sum, "train_head_loss_chain: null pointer");
    hipLaunchKernelGGL(k_train_head_loss_chain, dim3(div_up(N, 256)), dim3(256), 0, as_stream(stream), image, weights_sum, bg, bg_stride,
                       g_pred, N, term, loss, grad_image, grad_weights_sum);
    return check_launch("train_head_loss_chain");
}

}  // extern "C"
