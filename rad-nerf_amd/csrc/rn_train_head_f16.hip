// rn_train_head_f16.hip -- the fused training network with 16-bit matrix products (opt-in: RN_TRAIN_MLP=f16).
//
// C ABI: include/radnerf_train.h (the *_h16 entries).  Same computation, same tile ownership and same saved state as
// rn_train_head.hip (the backward walk is the same text, rn_train_head_walk_dev.h) -- one wavefront owns 32 samples, a layer's
// accumulators (sample on the lane, output row on the register index) are the next layer's B operand, everything the backward
// pass and the weight gradients read is stored as fp32 native tiles in the workspace of rn_train_head_dev.h -- but the contractions of the 64-row layers run on v_mfma_f32_32x32x8f16
// (K = 8 only: DESIGN.md section 3 on the K = 16 form) with fp32 accumulators.  This is the arithmetic of the reference's `-O`
// runs for its eight nn.Linear layers (nerf/utils.py:1168-1172: fp16 operands, fp32 sums).
//
//  * Weights are rounded to half once, by the pack kernel (round to nearest even); the fp32 image of rn_train_head.hip is
//    written too, unchanged, and the 16-bit forward and transposed images follow it.
//  * A 32x32 accumulator tile holds, in registers 4 g .. 4 g + 3 of lane half h, the rows 8 g + 4 h .. 8 g + 4 h + 3: exactly
//    the four k a lane half supplies to one K = 8 instruction.  So the B operand of k-block b = 4 rt + g of the next layer is
//    four accumulator registers rounded to half -- no shuffle, no staging, and k runs in natural order (the fp32 kernels need
//    kmap).  The grid features arrive the same way: lane half h gathers level 2 r + h in round r, two rounds are one k-block.
//  * Backward: dX = W^T dY on the transposed 16-bit image.  dY is scaled per tile and per layer before it is rounded: the
//    largest magnitude of the tile's dY (a wave reduction) is brought just below 2^15 by a power of two, the accumulators are
//    multiplied by the inverse power.  Nothing is kept on the host and a gradient 2^-20 times smaller gives bit for bit
//    2^-20 times the result.  A tile whose dY is all zero skips the products.
//  * fp32 as in rn_train_head.hip: gathers and interpolation, dy_dx of the ambient grid, SH, tanh / trunc_exp / sigmoid, the
//    narrow layers (VALU rows), the first-layer biases of the per-call constants, every saved tile, the pre-activation
//    gradients and the level-major feature gradients.  No float atomics: two runs give the same bits.
#include "rn_train_head_walk_dev.h"

namespace rn {
namespace th {

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

// ---- 16-bit images (appended to the fp32 image) --------------------------------------------------------------------------
// One k-block = 8 k of a 64-row layer: [2 row tiles][2 h][32 rows i][4 k] halves -> lane (i, h) reads 8 bytes per row tile.
// Element e of lane half h is k = 8 b + 4 h + e where the B operand is a previous layer's accumulators (or the SH basis), and
// feature 8 b + 4 (e >> 1) + 2 h + (e & 1) where it is two gather rounds (level 2 r + h, channel c = feature 4 r + 2 h + c).
constexpr int kHB = 2 * 2 * 32 * 4;           // halves per k-block of a 64-row layer
constexpr int kHB32 = kHB / 2;                // ... of a 32-row layer
constexpr int HF_A0 = 0;                      // ambient L0, enc_x        : 4 k-blocks (gather)
constexpr int HF_A1 = HF_A0 + 4;              // ambient L1               : 8
constexpr int HF_S0 = HF_A1 + 8;              // sigma L0, enc_x | enc_w  : 4 + 4 (gather)
constexpr int HF_S1 = HF_S0 + 8;              // sigma L1                 : 8
constexpr int HF_S2 = HF_S1 + 8;              // sigma L2 rows 1..64      : 8
constexpr int HF_C0 = HF_S2 + 8;              // colour L0, sh | geo_feat : 2 + 8
constexpr int kHFwdBlocks = HF_C0 + 10;       // 46
constexpr int kHFwdHalves = kHFwdBlocks * kHB;
// transposed: element e of lane half h is the forward OUTPUT unit 8 b + 4 h + e, row i of row tile rt the forward input
constexpr int HT_C0 = 0, HT_S2 = 8, HT_S1 = 16, HT_S0 = 24, HT_A1 = 32;   // 8 k-blocks each
constexpr int kHT_A0 = 40 * kHB;              // halves: d enc_x += W_amb0[:, 0:32]^T dZ_a0, 8 k-blocks of a 32-row layer
constexpr int kHBwdHalves = kHT_A0 + 8 * kHB32;
constexpr int kHFwdFloats = kHFwdHalves / 2, kHBwdFloats = kHBwdHalves / 2;   // in 4-byte units
constexpr int kHFwdOff = kImage, kHBwdOff = kImage + kHFwdFloats;
constexpr int kImageH16 = kHBwdOff + kHBwdFloats;
static_assert(kImage % 4 == 0 && kHFwdFloats % 4 == 0 && kHBwdFloats % 4 == 0, "the 16-bit images are copied to LDS 16 bytes at a time");

__global__ void __launch_bounds__(256) k_train_pack_h16(RawW w, const float *__restrict__ enc_a, const float *__restrict__ eye,
                                                        const float *__restrict__ ind_code, const int64_t *__restrict__ ind_index,
                                                        float *__restrict__ image) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < kImage) {   // today's fp32 image, unchanged
        if (ind_index) ind_code += (size_t)ind_index[0] * w.ind_dim;
        image[e] = train_image_elem(w, enc_a, eye, ind_code, e);
        return;
    }
    const int ldA0 = 32 + (int)w.audio_dim, ldS0 = 64 + (int)w.has_eye, ldC0 = 80 + (int)w.ind_dim;
    int q = e - kImage;   // one half per thread
    float v;
    if (q < kHFwdHalves) {
        const int b = q / kHB, rem = q % kHB;
        const int rt = rem / 256, h = (rem % 256) / 128, i = (rem % 128) / 4, el = rem % 4;
        const int row = 32 * rt + i;
        auto acc_k = [&](int b0) { return 8 * (b - b0) + 4 * h + el; };
        auto gather_k = [&](int b0) { return 8 * (b - b0) + 4 * (el >> 1) + 2 * h + (el & 1); };
        if (b < HF_A1) v = w.amb_w0[row * ldA0 + gather_k(HF_A0)];
        else if (b < HF_S0) v = w.amb_w1[row * 64 + acc_k(HF_A1)];
        else if (b < HF_S1) v = w.sig_w0[row * ldS0 + gather_k(HF_S0)];
        else if (b < HF_S2) v = w.sig_w1[row * 64 + acc_k(HF_S1)];
        else if (b < HF_C0) v = w.sig_w2[(1 + row) * 64 + acc_k(HF_S2)];
        else v = w.col_w0[row * ldC0 + acc_k(HF_C0)];   // sh: k-blocks 0, 1 = columns 0..15; geo_feat: columns 16..79
    } else {
        q -= kHFwdHalves;
        if (q >= kHBwdHalves) return;
        if (q < kHT_A0) {
            const int b = q / kHB, rem = q % kHB;
            const int rt = rem / 256, h = (rem % 256) / 128, i = (rem % 128) / 4, el = rem % 4;
            const int o = 8 * (b & 7) + 4 * h + el, col = 32 * rt + i;
            if (b < HT_S2) v = w.col_w0[o * ldC0 + 16 + col];
            else if (b < HT_S1) v = w.sig_w2[(1 + o) * 64 + col];
            else if (b < HT_S0) v = w.sig_w1[o * 64 + col];
            else if (b < HT_A1) v = w.sig_w0[o * ldS0 + 32 * rt + gather_feature(i)];
            else v = w.amb_w1[o * 64 + col];
        } else {
            const int t = q - kHT_A0, b = t / kHB32, rem = t % kHB32;
            const int h = rem / 128, i = (rem % 128) / 4, el = rem % 4;
            v = w.amb_w0[(8 * b + 4 * h + el) * ldA0 + gather_feature(i)];
        }
    }
    reinterpret_cast<_Float16 *>(image + kImage)[e - kImage] = (_Float16)v;
}

__device__ __forceinline__ f32x16 mfma8h(f16x4 a, f16x4 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x8f16(a, b, c, 0, 0, 0); }

// one k-block of a 64-row layer: both row tiles' weight fragments from LDS, B fragment b
__device__ __forceinline__ void hblock(Acc32 &a, const _Float16 *wl, int kb, int lane_off4, f16x4 b) {
    const f16x4 w0 = *reinterpret_cast<const f16x4 *>(wl + kb * kHB + lane_off4);
    const f16x4 w1 = *reinterpret_cast<const f16x4 *>(wl + kb * kHB + 256 + lane_off4);
    a.v[0] = mfma8h(w0, b, a.v[0]);
    a.v[1] = mfma8h(w1, b, a.v[1]);
}

__device__ __forceinline__ f16x4 frag4(float v0, float v1, float v2, float v3) {
    f16x4 r;
    r[0] = (_Float16)v0; r[1] = (_Float16)v1; r[2] = (_Float16)v2; r[3] = (_Float16)v3;
    return r;
}
// registers 4 g .. 4 g + 3 of row tile rt, times `scale`, rounded to half: the B fragment of k-block 4 rt + g of the next layer
__device__ __forceinline__ f16x4 acc_frag4(const Acc32 &in, int rt, int g, float scale) {
    return frag4(in.v[rt][4 * g] * scale, in.v[rt][4 * g + 1] * scale, in.v[rt][4 * g + 2] * scale, in.v[rt][4 * g + 3] * scale);
}
__device__ __forceinline__ f16x4 acc_frag4(const Acc32 &in, int rt, int g) {
    return frag4(in.v[rt][4 * g], in.v[rt][4 * g + 1], in.v[rt][4 * g + 2], in.v[rt][4 * g + 3]);
}

// 64 -> 64 layer whose input is the previous layer's accumulators (8 k-blocks from kb0)
__device__ __forceinline__ void hlayer_from_acc(Acc32 &out, const Acc32 &in, const _Float16 *wl, int kb0, int lane_off4) {
#pragma unroll
    for (int b = 0; b < 8; b++) hblock(out, wl, kb0 + b, lane_off4, acc_frag4(in, b >> 2, b & 3));
}

// LDS of the forward kernel (floats): 16-bit forward image | narrow fp32 rows | first-layer biases
constexpr int LF_A2 = kHFwdFloats, LF_S2R = LF_A2 + 128, LF_C1 = LF_S2R + 64, LF_BIAS = LF_C1 + 192, kLdsFwd = LF_BIAS + kBias;

__global__ void __launch_bounds__(kThreads) k_train_fwd_h16(FwdParams p) {
    __shared__ __attribute__((aligned(16))) float lds[kLdsFwd];
    __shared__ LevelPlan plan_x[16], plan_w[16];
    const uint32_t M = live_count(p.M, p.m_dev);
    const uint32_t n_tiles = (M + 31u) >> 5;
    if (blockIdx.x * kWaves >= n_tiles) return;
    for (int i = threadIdx.x; i < kHFwdFloats / 4; i += kThreads)
        reinterpret_cast<float4 *>(lds)[i] = reinterpret_cast<const float4 *>(p.image + kHFwdOff)[i];
    if (threadIdx.x < 128) lds[LF_A2 + threadIdx.x] = p.image[OFF_A2 + threadIdx.x];
    if (threadIdx.x < 64) lds[LF_S2R + threadIdx.x] = p.image[OFF_S2R + threadIdx.x];
    if (threadIdx.x < 192) lds[LF_C1 + threadIdx.x] = p.image[OFF_C1 + threadIdx.x];
    if (threadIdx.x < kBias) lds[LF_BIAS + threadIdx.x] = p.image[kPacked + kBwd + threadIdx.x];
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
    const int lane_off4 = (h * 32 + j) * 4;
    const _Float16 *wl = reinterpret_cast<const _Float16 *>(lds);
    const float *bias_amb = lds + LF_BIAS, *bias_sig = lds + LF_BIAS + 64, *bias_col = lds + LF_BIAS + 128;
    const float *tx = static_cast<const float *>(p.gx.table), *tw = static_cast<const float *>(p.gw.table);

    for (uint32_t tile = blockIdx.x * kWaves + wave; tile < n_tiles; tile += gridDim.x * kWaves) {
        const uint32_t sample = tile * 32 + j;   // both lane halves work on the same 32 samples
        const bool live = sample < M;
        Acc32 a0, a1, a2;
        acc_bias(a0, bias_amb, h);   // ambient L0, start = W0[:, 32:] enc_a (fp32)
        acc_bias(a2, bias_sig, h);   // sigma   L0, start = W0[:, 64] eye
        // ---- xyz grid: two gather rounds = one k-block of both first layers
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
            LevelFetch<float, 3, 2> f[2];
#pragma unroll 1
            for (int q = 0; q < 4; q++) {
                if (on) {
#pragma unroll
                    for (int i = 0; i < 2; i++) issue_planned<float, 3, 2, false, false>(tx, plan_x[2 * (2 * q + i) + h], in, f[i]);
                }
                float fv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    if (on) {
                        float res[2], dummy[1];
                        blend_level<float, 3, 2, false>(f[i], 0.0f, res, dummy);
                        fv[2 * i] = res[0];
                        fv[2 * i + 1] = res[1];
                    }
                    ex[(2 * (2 * q + i)) * 64 + lane] = fv[2 * i];
                    ex[(2 * (2 * q + i) + 1) * 64 + lane] = fv[2 * i + 1];
                }
                const f16x4 b = frag4(fv[0], fv[1], fv[2], fv[3]);
                hblock(a0, wl, HF_A0 + q, lane_off4, b);
                hblock(a2, wl, HF_S0 + q, lane_off4, b);
            }
        }
        // ---- ambient net: [enc_x | enc_a] 96 -> 64 -> 64 -> 2, tanh
        acc_relu(a0);
        tile_store(ws.ha0 + (size_t)tile * kTile32, a0, lane);
        acc_zero(a1);
        hlayer_from_acc(a1, a0, wl, HF_A1, lane_off4);
        acc_relu(a1);
        tile_store(ws.ha1 + (size_t)tile * kTile32, a1, lane);
        float amb[2];
        valu_out<2>(a1, lds + LF_A2, h, amb);
        amb[0] = tanhf(amb[0]);
        amb[1] = tanhf(amb[1]);
        // ---- ambient grid (+ d enc_w / d input): enc_w -> sigma L0 k-blocks 4..7
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
            LevelFetch<float, 2, 2> f[2];
#pragma unroll 1
            for (int q = 0; q < 4; q++) {
                if (on) {
#pragma unroll
                    for (int i = 0; i < 2; i++) issue_planned<float, 2, 2, false, false>(tw, plan_w[2 * (2 * q + i) + h], in, f[i]);
                }
                float fv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    const int r = 2 * q + i;
                    float g[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                    if (on) {
                        float res[2], grads[4];
                        blend_level<float, 2, 2, true>(f[i], plan_w[2 * r + h].scale, res, grads);
                        fv[2 * i] = res[0];
                        fv[2 * i + 1] = res[1];
#pragma unroll
                        for (int c = 0; c < 4; c++) g[c] = grads[c];
                    }
                    ew[(2 * r) * 64 + lane] = fv[2 * i];
                    ew[(2 * r + 1) * 64 + lane] = fv[2 * i + 1];
#pragma unroll
                    for (int c = 0; c < 4; c++) dw[(4 * r + c) * 64 + lane] = g[c];
                }
                hblock(a2, wl, HF_S0 + 4 + q, lane_off4, frag4(fv[0], fv[1], fv[2], fv[3]));
            }
        }
        // ---- sigma net: [enc_x | enc_w | eye] 65 -> 64 -> 64 -> 1 + 64
        acc_relu(a2);
        tile_store(ws.hs0 + (size_t)tile * kTile32, a2, lane);
        acc_zero(a1);
        hlayer_from_acc(a1, a2, wl, HF_S1, lane_off4);
        acc_relu(a1);
        tile_store(ws.hs1 + (size_t)tile * kTile32, a1, lane);
        {
            float raw[1];
            valu_out<1>(a1, lds + LF_S2R, h, raw);
            if (h == 0) {
                ws.sraw[sample] = raw[0];
                if (live) p.sigmas[sample] = expf(raw[0]);   // trunc_exp forward (activation.py:9-11)
            }
        }
        acc_zero(a0);
        hlayer_from_acc(a0, a1, wl, HF_S2, lane_off4);   // geo_feat (no activation)
        tile_store(ws.geo + (size_t)tile * kTile32, a0, lane);
        // ---- colour net: [SH(d) | geo_feat | ind_code] 84 -> 64 -> 3, sigmoid
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
            for (int s = 0; s < 8; s++) st[s * 64 + lane] = select_h(sh[2 * s], sh[2 * s + 1], h);   // the fp32 kernels' tile: register s of half h = sh[2 s + h]
#pragma unroll
            for (int b = 0; b < 2; b++)   // lane half h supplies k = 8 b + 4 h + e
                hblock(a1, wl, HF_C0 + b, lane_off4,
                       frag4(select_h(sh[8 * b], sh[8 * b + 4], h), select_h(sh[8 * b + 1], sh[8 * b + 5], h),
                             select_h(sh[8 * b + 2], sh[8 * b + 6], h), select_h(sh[8 * b + 3], sh[8 * b + 7], h)));
        }
        hlayer_from_acc(a1, a0, wl, HF_C0 + 2, lane_off4);
        acc_relu(a1);
        tile_store(ws.hc0 + (size_t)tile * kTile32, a1, lane);
        {
            float rgb[3];
            valu_out<3>(a1, lds + LF_C1, h, rgb);
            if (live && h == 0) {
#pragma unroll
                for (int c = 0; c < 3; c++) p.rgbs[3 * (size_t)sample + c] = 1.0f / (1.0f + expf(-rgb[c]));
            }
        }
    }
}

// ---- backward --------------------------------------------------------------------------------------------------------------
// The power of two that brings the largest magnitude of the tile's dY into [2^14, 2^15), and its inverse; false where the
// tile's dY is all zero.  The exponent is clamped so that both factors are normal numbers.
__device__ __forceinline__ bool tile_scale(const Acc32 &g, float &scale, float &inv) {
    int m = 0;
#pragma unroll
    for (int rt = 0; rt < 2; rt++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int b = __float_as_int(g.v[rt][r]) & 0x7fffffff;
            m = b > m ? b : m;
        }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int o = __shfl_xor(m, off, 64);
        m = o > m ? o : m;
    }
    int eb = m >> 23;
    eb = eb < 15 ? 15 : (eb > 254 ? 254 : eb);
    scale = __int_as_float((268 - eb) << 23);   // 2^(14 - (eb - 127))
    inv = __int_as_float((eb - 14) << 23);
    return m != 0;
}
__device__ __forceinline__ void acc_mul(Acc32 &a, float f) {
#pragma unroll
    for (int rt = 0; rt < 2; rt++)
#pragma unroll
        for (int r = 0; r < 16; r++) a.v[rt][r] *= f;
}
// out = W^T dY for a 64 -> 64 layer on the transposed 16-bit image (k-blocks from kb0); `out` comes back zero for a zero dY
__device__ __forceinline__ void hlayer_T(Acc32 &out, const Acc32 &dy, const _Float16 *wl, int kb0, int lane_off4) {
    acc_zero(out);
    float scale, inv;
    if (tile_scale(dy, scale, inv)) {   // uniform over the wave
#pragma unroll
        for (int b = 0; b < 8; b++) hblock(out, wl, kb0 + b, lane_off4, acc_frag4(dy, b >> 2, b & 3, scale));
        acc_mul(out, inv);
    }
}

// The 16-bit arithmetic of the backward tile walk (rn_train_head_walk_dev.h).
// LDS (floats): transposed 16-bit image | narrow fp32 rows (N_C1 | N_S2R | N_A2 of the fp32 image, in that order).
struct ArithF16 {
    static constexpr int RT_C1 = kHBwdFloats, RT_S2R = RT_C1 + 192, RT_A2 = RT_S2R + 64, kLdsBwd = RT_A2 + 128;
    static constexpr int WT_C0 = HT_C0, WT_S2 = HT_S2, WT_S1 = HT_S1, WT_S0 = HT_S0, WT_A1 = HT_A1;   // first k-block of the layer
    const _Float16 *wl;
    int lane_off4;
    __device__ ArithF16(const float *lds, int j, int h) : wl(reinterpret_cast<const _Float16 *>(lds)), lane_off4((h * 32 + j) * 4) {}

    static __device__ __forceinline__ void fill_bwd(float *lds, const float *image) {
        for (int i = threadIdx.x; i < kHBwdFloats / 4; i += kThreads)
            reinterpret_cast<float4 *>(lds)[i] = reinterpret_cast<const float4 *>(image + kHBwdOff)[i];
        if (threadIdx.x < 384) lds[RT_C1 + threadIdx.x] = image[kPacked + N_C1 + threadIdx.x];
    }
    __device__ __forceinline__ void layer_T(Acc32 &out, const Acc32 &dy, int kb0) const { hlayer_T(out, dy, wl, kb0, lane_off4); }
    // a 32-row layer, scaled like the others, added after the unscaling
    __device__ __forceinline__ void a0_T(f32x16 &x0, const Acc32 &dz) const {
        float scale, inv;
        if (tile_scale(dz, scale, inv)) {
            f32x16 xa = zero16();
#pragma unroll
            for (int b = 0; b < 8; b++)
                xa = mfma8h(*reinterpret_cast<const f16x4 *>(wl + kHT_A0 + b * kHB32 + lane_off4), acc_frag4(dz, b >> 2, b & 3, scale), xa);
#pragma unroll
            for (int r = 0; r < 16; r++) x0[r] += xa[r] * inv;
        }
    }
};

__global__ void __launch_bounds__(kThreads) k_train_bwd_h16(BwdParams p) {
    __shared__ __attribute__((aligned(16))) float lds[ArithF16::kLdsBwd];
    train_bwd_tiles<ArithF16>(p, lds);
}

constexpr int kPackElems = kImage + kHFwdHalves + kHBwdHalves;   // one thread per fp32 element, then one per half

}  // namespace th
}  // namespace rn

using namespace rn;
using namespace rn::th;

extern "C" {

size_t rn_train_head_image_floats_h16(void) { return (size_t)kImageH16; }

int rn_train_head_pack_h16(const rn_nerf_weights_t *w, const float *enc_a, const float *eye, const float *ind_code, float *image,
                           rn_stream_t stream) {
    return pack(k_train_pack_h16, kPackElems, "train_head_pack_h16", w, enc_a, eye, ind_code, nullptr, false, image, stream);
}

int rn_train_head_pack_row_h16(const rn_nerf_weights_t *w, const float *enc_a, const float *eye, const float *ind_table,
                               const int64_t *ind_index, float *image, rn_stream_t stream) {
    return pack(k_train_pack_h16, kPackElems, "train_head_pack_row_h16", w, enc_a, eye, ind_table, ind_index, true, image, stream);
}

int rn_train_head_forward_h16(const float *xyzs, const float *dirs, uint32_t M, const int32_t *m_dev, const rn_grid_t *grid_xyz,
                              const rn_grid_t *grid_amb, const float *image, float bound, float *sigmas, float *rgbs,
                              float *ambient, float *ambient_abs, float *xn, float *wn, float *workspace, rn_stream_t stream) {
    return forward(k_train_fwd_h16, "train_head_forward_h16", xyzs, dirs, M, m_dev, grid_xyz, grid_amb, image, bound, sigmas, rgbs, ambient,
                   ambient_abs, xn, wn, workspace, stream);
}

int rn_train_head_backward_h16(const float *grad_sigmas, const float *grad_rgbs, const float *grad_ambient,
                               const float *grad_ambient_abs, const float *rgbs, const float *ambient, uint32_t M,
                               const int32_t *m_dev, const float *image, float *workspace, float *grad_enc_x, float *grad_enc_w,
                               rn_stream_t stream) {
    return backward(k_train_bwd_h16, true, "train_head_backward_h16", grad_sigmas, grad_rgbs, grad_ambient, grad_ambient_abs, rgbs, ambient,
                    M, m_dev, image, workspace, grad_enc_x, grad_enc_w, stream);
}

}  // extern "C"
