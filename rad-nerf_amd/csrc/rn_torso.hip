// rn_torso.hip -- the torso pass of a frame with the final blend as its epilogue (gfx950).
//
// C ABI: include/radnerf_fused.h (rn_torso_*, rn_blend_frame).  What is computed: nerf/renderer.py:269-299 and
// nerf/network.py:188-219 per background pixel, and the blend of renderer.py:306-311.  k_torso_fused keeps the older
// 64-sample form of the fused network kernel: two column tiles per wave on v_mfma_f32_32x32x2_f32, one v_permlane32_swap
// per feature pair to build both B operands; the weights sit in LDS, the per-frame inputs enter as accumulator biases.
// k_torso_planned is the same pass over a torso plan (rn_torso_plan_*): the covered pixels and their position encoding, built
// once per view, so that a frame runs the covered pixels as dense 32-sample tiles (rn_tile32_dev.h) and computes no sine.
#include "rn_torso_dev.h"

#include "../../include/radnerf_train.h"   // rn_torso_select: the covered pixels of a training step

namespace rn {

// ---- 64-sample tiles (two column tiles per wave)
// one MFMA step of a 64-row layer: weights of step s from LDS, B operands b0 / b1 for the two column tiles
__device__ __forceinline__ void step64(Acc &a, const float *wl, int s, int lane_off, float b0, float b1) {
    const float2 w = *reinterpret_cast<const float2 *>(wl + s * kStep + lane_off);
    a.v[0][0] = mfma32(w.x, b0, a.v[0][0]);
    a.v[1][0] = mfma32(w.x, b1, a.v[1][0]);
    a.v[0][1] = mfma32(w.y, b0, a.v[0][1]);
    a.v[1][1] = mfma32(w.y, b1, a.v[1][1]);
}

// 64 -> 64 layer whose input is the previous layer's accumulators (32 steps)
__device__ __forceinline__ void layer_from_acc(Acc &out, const Acc &in, const float *wl, int lane_off) {
#pragma unroll
    for (int s = 0; s < 32; s++) step64(out, wl, s, lane_off, in.v[0][s >> 4][s & 15], in.v[1][s >> 4][s & 15]);
}

// "one sample per lane" feature pair (f0, f1) -> B operands of column tile 0 and 1
__device__ __forceinline__ void to_b_operands(float f0, float f1, float &b0, float &b1) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(f0), __float_as_uint(f1), false, false);
    b0 = __uint_as_float(r[0]);
    b1 = __uint_as_float(r[1]);
}

// ==========================================================================================================
// Torso pass (nerf/renderer.py:269-299, nerf/network.py:188-219) and final blend (renderer.py:306-311)
//
// The packed weight image and the constant columns are rn_torso_dev.h's; k_torso_fused reads the grid steps of torso L0 in
// level order.
#ifndef RN_TORSO_GROUP
#define RN_TORSO_GROUP 2
#endif
constexpr int kTorsoGroup = RN_TORSO_GROUP;  // torso-grid levels gathered together (divides 16)

__global__ void __launch_bounds__(256) k_pack_torso(RawT w, float *__restrict__ packed) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < kTorsoPacked) packed[e] = torso_image_elem<false>(w, e);
}

struct BlendArgs {   // final blend folded into the torso pass (renderer.py:306-311; rn_torso_blend_frame)
    float *image;
    const float *weights_sum;
    float *depth;
    const float *nears, *fars;
    uint8_t *u8;
};

struct TorsoParams {
    const float *bg_coords;
    uint32_t N;
    const float *density_grid;
    uint32_t G;
    float thresh;
    const float *poses6, *ind_code;
    float shrink;
    RawT w;
    const float *packed;
    GridArgs gt;
    const float *bg_in;
    float *bg_out, *alpha_out, *deform_out;
    BlendArgs blend;
};

// image = clamp(image + (1 - weights_sum) * bg, 0, 1); depth = max(depth - near, 0) / (far - near)  [, uint8 frame]
__device__ __forceinline__ void blend_pixel(const BlendArgs &b, size_t px, const float (&bg)[3]) {
    const float w = 1 - b.weights_sum[px];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float v = b.image[3 * px + c] + w * bg[c];
        v = fminf(fmaxf(v, 0.0f), 1.0f);
        b.image[3 * px + c] = v;
        if (b.u8) b.u8[3 * px + c] = (uint8_t)(v * 255.0f);
    }
    const float dd = b.depth[px] - b.nears[px];
    b.depth[px] = fmaxf(dd, 0.0f) / (b.fars[px] - b.nears[px]);
}

// F.grid_sample(bilinear, zeros, align_corners=True) of the [G,G] torso grid at (gx, gy) (renderer.py:282)
__device__ __forceinline__ float sample_torso_grid(const float *__restrict__ img, uint32_t G, float gx, float gy) {
    const float ix = ((gx + 1.f) / 2) * (float)(G - 1);
    const float iy = ((gy + 1.f) / 2) * (float)(G - 1);
    const float ix_nw = floorf(ix), iy_nw = floorf(iy);
    const float ix_se = ix_nw + 1, iy_se = iy_nw + 1;
    const float nw = (ix_se - ix) * (iy_se - iy), ne = (ix - ix_nw) * (iy_se - iy);
    const float sw = (ix_se - ix) * (iy - iy_nw), se = (ix - ix_nw) * (iy - iy_nw);
    const int x0 = (int)ix_nw, y0 = (int)iy_nw, x1 = x0 + 1, y1 = y0 + 1;
    const int g = (int)G;
    float out = 0.0f;
    if (x0 >= 0 && x0 < g && y0 >= 0 && y0 < g) out += img[y0 * g + x0] * nw;
    if (x1 >= 0 && x1 < g && y0 >= 0 && y0 < g) out += img[y0 * g + x1] * ne;
    if (x0 >= 0 && x0 < g && y1 >= 0 && y1 < g) out += img[y1 * g + x0] * sw;
    if (x1 >= 0 && x1 < g && y1 >= 0 && y1 < g) out += img[y1 * g + x1] * se;
    return out;
}

template <typename TT, bool BLEND>
__global__ void __launch_bounds__(kFusedThreads, 2) k_torso_fused(TorsoParams p) {
    __shared__ __attribute__((aligned(16))) float lds[kTorsoPacked + kTorsoBias + 64];
    __shared__ LevelPlan plan_t[16];
    float *bias_def = lds + kTorsoPacked, *bias_tor = bias_def + 64, *enc_pose = bias_tor + 32;
    if (threadIdx.x >= 64 && threadIdx.x < 80) {
        const int t = threadIdx.x - 64;
        const uint32_t o = (uint32_t)p.gt.offsets[t];
        plan_t[t] = plan_level<2>(p.gt.lc.scale[t], p.gt.lc.resolution[t], o, (uint32_t)p.gt.offsets[t + 1] - o, p.gt.gridtype,
                                  (uint32_t)sizeof(TT) * 2u);
    }

    for (int i = threadIdx.x; i < kTorsoPacked / 4; i += kFusedThreads)
        reinterpret_cast<float4 *>(lds)[i] = reinterpret_cast<const float4 *>(p.packed)[i];
    if (threadIdx.x < 54) enc_pose[threadIdx.x] = enc_pose_elem(p.poses6, threadIdx.x);
    __syncthreads();
    // the constant columns as biases: deform 64 | torso 32
    if (threadIdx.x < kTorsoBias) bias_def[threadIdx.x] = torso_const_bias(p.w, enc_pose, p.ind_code, threadIdx.x);
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int lane_off = h * 64 + j * 2, lane_off32 = h * 32 + j;
    const uint32_t n_tiles = (p.N + 63u) >> 6;

    for (uint32_t tile = blockIdx.x * kWavesPerBlock + wave; tile < n_tiles; tile += gridDim.x * kWavesPerBlock) {
        const uint32_t px = tile * 64 + lane;
        const bool in_range = px < p.N;
        float cx = 0.0f, cy = 0.0f;
        bool on = false;
        if (in_range) {
            cx = p.bg_coords[2 * (size_t)px]; cy = p.bg_coords[2 * (size_t)px + 1];
            on = sample_torso_grid(p.density_grid, p.G, cx, cy) > p.thresh;
        }
        float bgc[3] = {1.0f, 1.0f, 1.0f};
        if (in_range && p.bg_in) { bgc[0] = p.bg_in[3 * (size_t)px]; bgc[1] = p.bg_in[3 * (size_t)px + 1]; bgc[2] = p.bg_in[3 * (size_t)px + 2]; }
        if (__ballot(on) == 0ull) {  // no torso pixel in this tile: background passes through
            if (in_range) {
                if (p.bg_out) { p.bg_out[3 * (size_t)px] = bgc[0]; p.bg_out[3 * (size_t)px + 1] = bgc[1]; p.bg_out[3 * (size_t)px + 2] = bgc[2]; }
                if constexpr (BLEND) blend_pixel(p.blend, px, bgc);
                if (p.alpha_out) p.alpha_out[px] = 0.0f;
                if (p.deform_out) { p.deform_out[2 * (size_t)px] = 0.0f; p.deform_out[2 * (size_t)px + 1] = 0.0f; }
            }
            continue;
        }
        // x = x * torso_shrink; enc_x = freq(x, deg 10) (network.py:194,198): [x, sin(2^f x), cos(2^f x)]_f
        const float x0 = cx * p.shrink, x1 = cy * p.shrink;
        float bq[2][21];
        {
            float fq[42];
            fq[0] = x0; fq[1] = x1;
#pragma unroll
            for (int f = 0; f < 10; f++) {
                const float a0 = freq_angle(x0, f), a1 = freq_angle(x1, f);
                fq[2 + 4 * f + 0] = on ? freq_sin(a0) : 0.0f;
                fq[2 + 4 * f + 1] = on ? freq_sin(a1) : 0.0f;
                fq[2 + 4 * f + 2] = on ? freq_cos(a0) : 0.0f;
                fq[2 + 4 * f + 3] = on ? freq_cos(a1) : 0.0f;
            }
            if (!on) { fq[0] = 0.0f; fq[1] = 0.0f; }
#pragma unroll
            for (int s = 0; s < 21; s++) to_b_operands(fq[2 * s], fq[2 * s + 1], bq[0][s], bq[1][s]);
        }
        // deform net 104 -> 64 -> 64 -> 2
        Acc a0, a1;
        acc_bias(a0, bias_def, h);
#pragma unroll
        for (int s = 0; s < 21; s++) step64(a0, lds + TOFF_D0, s, lane_off, bq[0][s], bq[1][s]);
        acc_relu(a0);
        acc_zero(a1);
        layer_from_acc(a1, a0, lds + TOFF_D1, lane_off);
        acc_relu(a1);
        float dxy[2];
        {
            float part[2][2];
            valu_out<2>(a1, lds + TOFF_D2, h, part);
            dxy[0] = h ? part[1][0] : part[0][0];
            dxy[1] = h ? part[1][1] : part[0][1];
        }
        // x = clamp(x + dx, -1, 1); torso grid (bound = 1)
        float bg_[2][16];
        {
            float in[2] = {(fminf(fmaxf(x0 + dxy[0], -1.0f), 1.0f) + 1.0f) / 2.0f,
                           (fminf(fmaxf(x1 + dxy[1], -1.0f), 1.0f) + 1.0f) / 2.0f};
            const bool ok = on && !(in[0] < 0 || in[0] > 1 || in[1] < 0 || in[1] > 1);
            // kTorsoGroup levels in flight (the deform net's accumulators are dead by now): the 16 gathers are a latency chain
            // of one tile, and a torso launch is one tile per wave
            LevelFetch<TT, 2, 2> f[kTorsoGroup];
#pragma unroll
            for (int g = 0; g < 16; g += kTorsoGroup) {
                if (ok) {
#pragma unroll
                    for (int i = 0; i < kTorsoGroup; i++)
                        issue_planned<TT, 2, 2, false>(static_cast<const TT *>(p.gt.table), plan_t[g + i], in, f[i]);
                }
#pragma unroll
                for (int i = 0; i < kTorsoGroup; i++) {
                    float f0 = 0.0f, f1 = 0.0f;
                    if (ok) {
                        TT res[2];
                        TT dummy[1];
                        blend_level<TT, 2, 2, false>(f[i], 0.0f, res, dummy);
                        f0 = to_f<TT>(res[0]);
                        f1 = to_f<TT>(res[1]);
                    }
                    to_b_operands(f0, f1, bg_[0][g + i], bg_[1][g + i]);
                }
            }
        }
        // torso net 136 -> 32 -> 32 -> 4 : a single 32-row tile
        f32x16 t0[2], t1[2];
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const float4 b = *reinterpret_cast<const float4 *>(bias_tor + 8 * g + 4 * h);
            t0[0][4 * g] = b.x; t0[0][4 * g + 1] = b.y; t0[0][4 * g + 2] = b.z; t0[0][4 * g + 3] = b.w;
            t0[1][4 * g] = b.x; t0[1][4 * g + 1] = b.y; t0[1][4 * g + 2] = b.z; t0[1][4 * g + 3] = b.w;
        }
#pragma unroll
        for (int s = 0; s < 16; s++) {
            const float wv = lds[TOFF_T0 + s * kS32 + lane_off32];
            t0[0] = mfma32(wv, bg_[0][s], t0[0]); t0[1] = mfma32(wv, bg_[1][s], t0[1]);
        }
#pragma unroll
        for (int s = 0; s < 21; s++) {
            const float wv = lds[TOFF_T0 + (16 + s) * kS32 + lane_off32];
            t0[0] = mfma32(wv, bq[0][s], t0[0]); t0[1] = mfma32(wv, bq[1][s], t0[1]);
        }
#pragma unroll
        for (int r = 0; r < 16; r++) { t0[0][r] = fmaxf(t0[0][r], 0.0f); t0[1][r] = fmaxf(t0[1][r], 0.0f); t1[0][r] = 0.0f; t1[1][r] = 0.0f; }
#pragma unroll
        for (int s = 0; s < 16; s++) {
            const float wv = lds[TOFF_T1 + s * kS32 + lane_off32];
            t1[0] = mfma32(wv, t0[0][s], t1[0]); t1[1] = mfma32(wv, t0[1][s], t1[1]);
        }
        float o4[4];
#pragma unroll
        for (int o = 0; o < 4; o++) {
            float p0 = 0.0f, p1 = 0.0f;
            const float *wo = lds + TOFF_T2 + (o * 2 + h) * 16;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                p0 = __builtin_fmaf(fmaxf(t1[0][r], 0.0f), wo[r], p0);
                p1 = __builtin_fmaf(fmaxf(t1[1][r], 0.0f), wo[r], p1);
            }
            p0 += __shfl_xor(p0, 32, 64);
            p1 += __shfl_xor(p1, 32, 64);
            o4[o] = h ? p1 : p0;
        }
        if (in_range) {
            float alpha = 0.0f, col[3] = {0.0f, 0.0f, 0.0f};
            if (on) {
                alpha = sigmoid_out(o4[0]);
#pragma unroll
                for (int c = 0; c < 3; c++) col[c] = sigmoid_out(o4[1 + c]);
            }
            // bg = torso_color * alpha + bg * (1 - alpha)  (renderer.py:299)
            float bgf[3];
#pragma unroll
            for (int c = 0; c < 3; c++) bgf[c] = col[c] * alpha + bgc[c] * (1 - alpha);
            if (p.bg_out) {
#pragma unroll
                for (int c = 0; c < 3; c++) p.bg_out[3 * (size_t)px + c] = bgf[c];
            }
            if constexpr (BLEND) blend_pixel(p.blend, px, bgf);
            if (p.alpha_out) p.alpha_out[px] = alpha;
            if (p.deform_out) { p.deform_out[2 * (size_t)px] = on ? dxy[0] : 0.0f; p.deform_out[2 * (size_t)px + 1] = on ? dxy[1] : 0.0f; }
        }
    }
}

// Pixels the torso layer covers: bilinear occupancy of the 2-D torso grid above the threshold (renderer.py:281-283).  Used by
// the differentiable (training) formulation, which gathers those pixels for the PyTorch layers; inference goes through
// k_torso_fused, which tests the same expression per pixel.
__global__ void __launch_bounds__(256)
k_torso_mask(const float *__restrict__ bg_coords, uint32_t N, const float *__restrict__ grid, uint32_t G, float thresh,
             uint8_t *__restrict__ mask) {
    const uint32_t n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    mask[n] = sample_torso_grid(grid, G, bg_coords[2 * (size_t)n], bg_coords[2 * (size_t)n + 1]) > thresh ? 1 : 0;
}

// The same test as a stable compaction on the device: covered[0 .. count) = the covered pixel indices ascending (torch.nonzero's
// order), xy_c their coordinates, for a training step that never tells the host how many there are.  The threshold is
// min(thresh, *mean_dev), read here, so a captured launch follows an occupancy refresh.  ONE workgroup walks the pixels
// kSelectThreads at a time: ballot + mbcnt rank inside a wave, the waves' counts through LDS (two buffers in turn: one barrier
// per round), the running total in a register.  A training batch is 4 096 .. 65 536 pixels: 4 .. 64 rounds.
constexpr int kSelectThreads = 1024;
__global__ void __launch_bounds__(kSelectThreads)
k_torso_select(const float *__restrict__ bg_coords, uint32_t N, const float *__restrict__ grid, uint32_t G, float thresh,
               const float *__restrict__ mean_dev, int32_t *__restrict__ covered, float *__restrict__ xy_c,
               int32_t *__restrict__ count) {
    constexpr int kWaves = kSelectThreads / kWave;
    __shared__ uint32_t wave_cnt[2][kWaves];
    if (mean_dev) thresh = fminf(thresh, mean_dev[0]);
    const uint32_t wave = threadIdx.x >> 6;
    uint32_t base = 0;
    for (uint32_t n0 = 0, round = 0; n0 < N; n0 += kSelectThreads, round++) {
        const uint32_t n = n0 + threadIdx.x;
        float cx = 0.0f, cy = 0.0f;
        bool on = false;
        if (n < N) {
            cx = bg_coords[2 * (size_t)n]; cy = bg_coords[2 * (size_t)n + 1];
            on = sample_torso_grid(grid, G, cx, cy) > thresh;
        }
        const unsigned long long mask = __ballot(on);
        uint32_t *cnt = wave_cnt[round & 1];
        if ((threadIdx.x & 63) == 0) cnt[wave] = (uint32_t)__popcll(mask);
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < (uint32_t)kWaves; w++) {
            const uint32_t cw = cnt[w];
            before += (w < wave) ? cw : 0u;
            total += cw;
        }
        if (on) {
            const uint32_t row = base + before + ballot_prefix(mask);
            covered[row] = (int32_t)n;
            *reinterpret_cast<float2 *>(xy_c + 2 * (size_t)row) = make_float2(cx, cy);
        }
        base += total;
    }
    if (threadIdx.x == 0) count[0] = (int32_t)base;
}

// renderer.py:306-311
__global__ void __launch_bounds__(256)
k_blend(float *__restrict__ image, const float *__restrict__ weights_sum, const float *__restrict__ bg,
        float *__restrict__ depth, const float *__restrict__ nears, const float *__restrict__ fars, uint32_t N,
        uint8_t *__restrict__ u8) {
    const uint32_t n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float b[3] = {1.0f, 1.0f, 1.0f};
    if (bg) { b[0] = bg[3 * (size_t)n]; b[1] = bg[3 * (size_t)n + 1]; b[2] = bg[3 * (size_t)n + 2]; }
    blend_pixel(BlendArgs{image, weights_sum, depth, nears, fars, u8}, n, b);
}

// ==========================================================================================================
// The torso plan: what the pass computes from (bg_coords, occupancy grid, thresh, shrink) alone, built once for a view and
// read by every frame after it: the covered pixels in ascending order (32 to a tile), a per-pixel flag, and enc_x =
// freq(x * shrink, 10) of the covered pixels as the B operands of the 21 first-layer steps (native tiles: row s = the
// operand of step s, one coalesced 256-B row).  That is the 40 sines and cosines per pixel with their large-argument
// reduction, two thirds of k_torso_fused's VALU work.  The frame feeds them to the same MFMA chains in the same order
// (bias first, then the steps), so a planned frame equals k_torso_fused's bit for bit on every pixel.
//
// Layout (bytes; every part 256-aligned): count int32 | on flag u8 [N] | on-list int32 [N] | their xy float2 [N] | enc_x.
constexpr size_t kPlanAlign = 256;
constexpr uint32_t kPlanTileFloats = 21 * 64;   // 21 operand rows of 64 lanes per 32-pixel tile
__host__ __device__ constexpr size_t plan_up(size_t b) { return (b + kPlanAlign - 1) / kPlanAlign * kPlanAlign; }
struct PlanView {
    int32_t *count;
    uint8_t *flags;
    int32_t *on_list;
    float *xy;
    float *enc;
};
__host__ __device__ inline size_t plan_head_bytes(uint32_t N) {
    return kPlanAlign + plan_up(N) + plan_up(4 * (size_t)N) + plan_up(8 * (size_t)N);
}
__host__ __device__ inline PlanView plan_view(void *plan, uint32_t N) {
    unsigned char *b = static_cast<unsigned char *>(plan);
    PlanView v;
    v.count = reinterpret_cast<int32_t *>(b); b += kPlanAlign;
    v.flags = b; b += plan_up(N);
    v.on_list = reinterpret_cast<int32_t *>(b); b += plan_up(4 * (size_t)N);
    v.xy = reinterpret_cast<float *>(b); b += plan_up(8 * (size_t)N);
    v.enc = reinterpret_cast<float *>(b);
    return v;
}

// the 21 features of coordinate xs = x[h] * shrink that lane half h feeds: feature 2 s + h of enc_x at MFMA step s
__device__ __forceinline__ void enc_x_half(float xs, float (&fq)[21]) {
    fq[0] = xs;
#pragma unroll
    for (int f = 0; f < 10; f++) {
        const float a = freq_angle(xs, f);
        fq[1 + 2 * f] = freq_sin(a);
        fq[2 + 2 * f] = freq_cos(a);
    }
}

// enc_x of every 32-pixel tile of the on-list: one wave per tile.  Lanes past the end of the list store zeros.
constexpr int kPlanThreads = 256, kPlanWaves = kPlanThreads / kWave;
__global__ void __launch_bounds__(kPlanThreads)
k_torso_plan_enc(const float *__restrict__ xy, uint32_t n_on, float shrink, float *__restrict__ enc) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, h = lane >> 5;
    const uint32_t tile = blockIdx.x * kPlanWaves + wave;
    if (tile >= (n_on + 31u) >> 5) return;
    const uint32_t i = tile * 32 + j;
    float fq[21];
#pragma unroll
    for (int s = 0; s < 21; s++) fq[s] = 0.0f;
    if (i < n_on) enc_x_half(xy[2 * (size_t)i + h] * shrink, fq);
    float *dst = enc + (size_t)tile * kPlanTileFloats;
#pragma unroll
    for (int s = 0; s < 21; s++) dst[s * 64 + lane] = fq[s];
}

struct PlannedParams {
    const uint8_t *flags;
    const int32_t *on_list;
    const float *xy;
    const float *enc;
    uint32_t N, n_on, on_blocks;
    const float *poses6, *ind_code;
    float shrink;
    RawT w;
    const float *packed;
    GridArgs gt;
    const float *bg_in;
    float *bg_out, *alpha_out, *deform_out;
    BlendArgs blend;
};

#ifndef RN_PLAN_GATHER
#define RN_PLAN_GATHER 4
#endif
// the launch bound's second argument.  Without one the compiler parks values in 64 AGPRs (119 + 64 registers, 2 waves per SIMD);
// with 2 or 3 it keeps to 122 - 124 VGPRs and 3 waves fit.  2, 3 and gather depths 2 / 4 / 8 measure the same
#ifndef RN_PLAN_WAVES_PER_SIMD
#define RN_PLAN_WAVES_PER_SIMD 2
#endif
constexpr int kPlanGather = RN_PLAN_GATHER;   // gather rounds in flight (a round = two levels, one per lane half; divides 8)
constexpr uint32_t kPlanOffPixels = 4;   // pixels per thread of a pixel-range workgroup

__device__ __forceinline__ float load_nt(const float *p) { return __builtin_nontemporal_load(p); }

// The frame's torso pass + blend over a plan, one launch, two kinds of workgroup and nothing shared between them:
//  * workgroups [0, on_blocks): one 32-pixel tile of the on-list per wave on the 32-sample machine (rn_tile32_dev.h);
//  * the rest: kPlanThreads * kPlanOffPixels consecutive pixels each; every pixel whose flag is off gets what k_torso_fused
//    gives it (background passes through, blend), the on pixels are left to the tiles.
template <typename TT, bool BLEND>
__global__ void __launch_bounds__(kPlanThreads, RN_PLAN_WAVES_PER_SIMD) k_torso_planned(PlannedParams p) {
    if (blockIdx.x >= p.on_blocks) {
        const uint32_t base = (blockIdx.x - p.on_blocks) * (kPlanThreads * kPlanOffPixels) + threadIdx.x;
#pragma unroll
        for (uint32_t q = 0; q < kPlanOffPixels; q++) {
            const uint32_t px = base + q * kPlanThreads;
            if (px >= p.N || p.flags[px]) continue;
            float bgc[3] = {1.0f, 1.0f, 1.0f};
            if (p.bg_in) { bgc[0] = p.bg_in[3 * (size_t)px]; bgc[1] = p.bg_in[3 * (size_t)px + 1]; bgc[2] = p.bg_in[3 * (size_t)px + 2]; }
            if (p.bg_out) { p.bg_out[3 * (size_t)px] = bgc[0]; p.bg_out[3 * (size_t)px + 1] = bgc[1]; p.bg_out[3 * (size_t)px + 2] = bgc[2]; }
            if constexpr (BLEND) blend_pixel(p.blend, px, bgc);
            if (p.alpha_out) p.alpha_out[px] = 0.0f;
            if (p.deform_out) { p.deform_out[2 * (size_t)px] = 0.0f; p.deform_out[2 * (size_t)px + 1] = 0.0f; }
        }
        return;
    }
    __shared__ __attribute__((aligned(16))) float lds_[kTorsoPacked + kTorsoBias + 64];
    __shared__ LevelPlan plan_t[16];
    constexpr int D0 = TOFF_D0, D1 = TOFF_D1, D2 = TOFF_D2, T0 = TOFF_T0, T1 = TOFF_T1, T2 = TOFF_T2;
    const float *lds = lds_;
    float *bias_def = lds_ + kTorsoPacked, *bias_tor = bias_def + 64, *enc_pose = bias_tor + 32;
    if (threadIdx.x >= 64 && threadIdx.x < 80) {
        const int t = threadIdx.x - 64;
        const uint32_t o = (uint32_t)p.gt.offsets[t];
        plan_t[t] = plan_level<2>(p.gt.lc.scale[t], p.gt.lc.resolution[t], o, (uint32_t)p.gt.offsets[t + 1] - o, p.gt.gridtype,
                                  (uint32_t)sizeof(TT) * 2u);
    }
    for (int i = threadIdx.x; i < kTorsoPacked / 4; i += kPlanThreads)
        reinterpret_cast<float4 *>(lds_)[i] = reinterpret_cast<const float4 *>(p.packed)[i];
    if (threadIdx.x < 54) enc_pose[threadIdx.x] = enc_pose_elem(p.poses6, threadIdx.x);
    __syncthreads();
    if (threadIdx.x < kTorsoBias) bias_def[threadIdx.x] = torso_const_bias(p.w, enc_pose, p.ind_code, threadIdx.x);
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int lane_off = h * 64 + j * 2, lane_off32 = h * 32 + j;
    const uint32_t tile = blockIdx.x * kPlanWaves + wave;
    if (tile >= (p.n_on + 31u) >> 5) return;
    const uint32_t i = tile * 32 + j;   // both lane halves work on the same 32 pixels
    const bool live = i < p.n_on;
    uint32_t px = 0;
    float x0 = 0.0f, x1 = 0.0f;
    if (live) {
        px = (uint32_t)p.on_list[i];
        const float2 c = *reinterpret_cast<const float2 *>(p.xy + 2 * (size_t)i);
        x0 = c.x * p.shrink; x1 = c.y * p.shrink;
    }
    // enc_x of the tile as the plan holds it: fq[s] = this lane's B operand of first-layer step s (k = 2 s + h)
    const float *et = p.enc + (size_t)tile * kPlanTileFloats;
    float fq[21];
#pragma unroll
    for (int s = 0; s < 21; s++) fq[s] = load_nt(et + s * 64 + lane);
    // deform net 104 -> 64 -> 64 -> 2
    Acc32 a0, a1;
    acc_bias(a0, bias_def, h);
#pragma unroll
    for (int s = 0; s < 21; s++) step32(a0, lds + D0, s, lane_off, fq[s]);
    acc_relu(a0);
    acc_zero(a1);
    layer_from_acc(a1, a0, lds + D1, lane_off);
    acc_relu(a1);
    float dxy[2];
    valu_out<2>(a1, lds + D2, h, dxy);
    f32x16 t0;
#pragma unroll
    for (int g = 0; g < 4; g++) {
        const float4 b = *reinterpret_cast<const float4 *>(bias_tor + 8 * g + 4 * h);
        t0[4 * g] = b.x; t0[4 * g + 1] = b.y; t0[4 * g + 2] = b.z; t0[4 * g + 3] = b.w;
    }
    // x = clamp(x + dx, -1, 1); torso grid (bound = 1): lane half h gathers level 2 r + h in round r, one lane swap per
    // round turns its two channels into the level-ordered B operands of steps 2 r and 2 r + 1
    {
        float in[2] = {(fminf(fmaxf(x0 + dxy[0], -1.0f), 1.0f) + 1.0f) / 2.0f,
                       (fminf(fmaxf(x1 + dxy[1], -1.0f), 1.0f) + 1.0f) / 2.0f};
        const bool ok = live && !(in[0] < 0 || in[0] > 1 || in[1] < 0 || in[1] > 1);
        LevelFetch<TT, 2, 2> f[kPlanGather];
#pragma unroll
        for (int g = 0; g < 8; g += kPlanGather) {
            if (ok) {
#pragma unroll
                for (int q = 0; q < kPlanGather; q++)
                    issue_planned<TT, 2, 2, false, false>(static_cast<const TT *>(p.gt.table), plan_t[2 * (g + q) + h], in, f[q]);
            }
#pragma unroll
            for (int q = 0; q < kPlanGather; q++) {
                float f0 = 0.0f, f1 = 0.0f;
                if (ok) {
                    TT res[2];
                    TT dummy[1];
                    blend_level<TT, 2, 2, false>(f[q], 0.0f, res, dummy);
                    f0 = to_f<TT>(res[0]);
                    f1 = to_f<TT>(res[1]);
                }
                float b0, b1;
                to_b_operands(f0, f1, b0, b1);
                const int s = 2 * (g + q);
                t0 = mfma32(lds[T0 + s * kS32 + lane_off32], b0, t0);
                t0 = mfma32(lds[T0 + (s + 1) * kS32 + lane_off32], b1, t0);
            }
        }
    }
    // torso net 136 -> 32 -> 32 -> 4 on one row tile: the grid steps above, then enc_x, in k_torso_fused's order
#pragma unroll
    for (int s = 0; s < 21; s++) t0 = mfma32(lds[T0 + (16 + s) * kS32 + lane_off32], fq[s], t0);
    f32x16 t1 = zero16();
#pragma unroll
    for (int r = 0; r < 16; r++) t0[r] = fmaxf(t0[r], 0.0f);
#pragma unroll
    for (int s = 0; s < 16; s++) t1 = mfma32(lds[T1 + s * kS32 + lane_off32], t0[s], t1);
    float o4[4];
#pragma unroll
    for (int o = 0; o < 4; o++) {
        float s = 0.0f;
        const float *wo = lds + T2 + (o * 2 + h) * 16;
#pragma unroll
        for (int r = 0; r < 16; r++) s = __builtin_fmaf(fmaxf(t1[r], 0.0f), wo[r], s);
        o4[o] = s + __shfl_xor(s, 32, 64);
    }
    if (live && h == 0) {
        float bgc[3] = {1.0f, 1.0f, 1.0f};
        if (p.bg_in) { bgc[0] = p.bg_in[3 * (size_t)px]; bgc[1] = p.bg_in[3 * (size_t)px + 1]; bgc[2] = p.bg_in[3 * (size_t)px + 2]; }
        const float alpha = sigmoid_out(o4[0]);
        // bg = torso_color * alpha + bg * (1 - alpha)  (renderer.py:299)
        float bgf[3];
#pragma unroll
        for (int c = 0; c < 3; c++) bgf[c] = sigmoid_out(o4[1 + c]) * alpha + bgc[c] * (1 - alpha);
        if (p.bg_out) {
#pragma unroll
            for (int c = 0; c < 3; c++) p.bg_out[3 * (size_t)px + c] = bgf[c];
        }
        if constexpr (BLEND) blend_pixel(p.blend, px, bgf);
        if (p.alpha_out) p.alpha_out[px] = alpha;
        if (p.deform_out) { p.deform_out[2 * (size_t)px] = dxy[0]; p.deform_out[2 * (size_t)px + 1] = dxy[1]; }
    }
}

// the launch behind rn_torso_fused and rn_torso_blend_frame: one 64-pixel tile per wave, at most two workgroups per CU
template <bool BLEND>
static int launch_torso(const TorsoParams &p, int table_dtype, rn_stream_t stream, const char *what) {
    const dim3 grid(tile_blocks((p.N + 63u) >> 6, kWavesPerBlock, 2));
    if (table_dtype == RN_F32) hipLaunchKernelGGL((k_torso_fused<float, BLEND>), grid, dim3(kFusedThreads), 0, as_stream(stream), p);
    else hipLaunchKernelGGL((k_torso_fused<__half, BLEND>), grid, dim3(kFusedThreads), 0, as_stream(stream), p);
    return check_launch(what);
}

}  // namespace rn

using namespace rn;

extern "C" {

size_t rn_torso_packed_floats(void) { return (size_t)kTorsoPacked; }

int rn_torso_pack_weights(const rn_torso_weights_t *w, float *packed, rn_stream_t stream) {
    if (int rc = check_torso_weights(w, "torso_pack_weights")) return rc;
    RN_REQUIRE(packed && ((uintptr_t)packed & 15u) == 0, "torso_pack_weights: packed must be 16-byte aligned");
    hipLaunchKernelGGL(k_pack_torso, dim3(div_up(kTorsoPacked, 256)), dim3(256), 0, as_stream(stream), raw_t(w), packed);
    return check_launch("torso_pack_weights");
}

int rn_torso_fused(const float *bg_coords, uint32_t N, const float *density_grid_torso, uint32_t grid_size, float thresh,
                   const float *poses6, const float *ind_code, float torso_shrink, const rn_torso_weights_t *w,
                   const float *packed, const rn_grid_t *grid_torso, const float *bg_in, float *bg_out,
                   float *torso_alpha, float *deform, rn_stream_t stream) {
    if (N == 0) return RN_OK;
    RN_REQUIRE(bg_coords && density_grid_torso && poses6 && w && packed && (bg_out || torso_alpha), "torso_fused: null pointer");
    RN_REQUIRE(ind_code || w->ind_dim == 0, "torso_fused: ind_code required when ind_dim > 0");
    RN_REQUIRE(((uintptr_t)packed & 15u) == 0, "torso_fused: packed must be 16-byte aligned");
    if (int rc = check_fused_grid(grid_torso, 2, "torso_fused(torso grid)")) return rc;
    TorsoParams p{bg_coords, N, density_grid_torso, grid_size, thresh, poses6, ind_code, torso_shrink, raw_t(w), packed,
                  grid_args(grid_torso), bg_in, bg_out, torso_alpha, deform, BlendArgs{}};
    return launch_torso<false>(p, grid_torso->dtype, stream, "torso_fused");
}

int rn_torso_blend_frame(const float *bg_coords, uint32_t N, const float *density_grid_torso, uint32_t grid_size, float thresh,
                         const float *poses6, const float *ind_code, float torso_shrink, const rn_torso_weights_t *w,
                         const float *packed, const rn_grid_t *grid_torso, const float *bg_in, float *bg_out, float *torso_alpha,
                         float *image, const float *weights_sum, float *depth, const float *nears, const float *fars,
                         uint8_t *image_u8, rn_stream_t stream) {
    if (N == 0) return RN_OK;
    RN_REQUIRE(bg_coords && density_grid_torso && poses6 && w && packed, "torso_blend_frame: null pointer");
    RN_REQUIRE(image && weights_sum && depth && nears && fars, "torso_blend_frame: null frame buffers");
    RN_REQUIRE(ind_code || w->ind_dim == 0, "torso_blend_frame: ind_code required when ind_dim > 0");
    RN_REQUIRE(((uintptr_t)packed & 15u) == 0, "torso_blend_frame: packed must be 16-byte aligned");
    if (int rc = check_fused_grid(grid_torso, 2, "torso_blend_frame(torso grid)")) return rc;
    TorsoParams p{bg_coords, N, density_grid_torso, grid_size, thresh, poses6, ind_code, torso_shrink, raw_t(w), packed,
                  grid_args(grid_torso), bg_in, bg_out, torso_alpha, nullptr, BlendArgs{image, weights_sum, depth, nears, fars, image_u8}};
    return launch_torso<true>(p, grid_torso->dtype, stream, "torso_blend_frame");
}

size_t rn_torso_plan_bytes(uint32_t N, uint32_t n_on) {
    return plan_head_bytes(N) + (size_t)((n_on + 31u) >> 5) * kPlanTileFloats * sizeof(float);
}

int rn_torso_plan_build(const float *bg_coords, uint32_t N, const float *density_grid_torso, uint32_t grid_size, float thresh,
                        float torso_shrink, void *plan, size_t plan_bytes, uint32_t *n_on, rn_stream_t stream) {
    RN_REQUIRE(bg_coords && density_grid_torso && plan && n_on, "torso_plan_build: null pointer");
    RN_REQUIRE(N > 0 && N <= (1u << 30) && grid_size >= 2, "torso_plan_build: N = %u, grid_size = %u", N, grid_size);
    RN_REQUIRE(((uintptr_t)plan & (kPlanAlign - 1)) == 0, "torso_plan_build: plan must be 256-byte aligned");
    RN_REQUIRE(plan_bytes >= plan_head_bytes(N), "torso_plan_build: plan_bytes = %zu is less than rn_torso_plan_bytes(N, 0) = %zu", plan_bytes,
               plan_head_bytes(N));
    hipStream_t s = as_stream(stream);
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    RN_REQUIRE(hipStreamIsCapturing(s, &cap) == hipSuccess && cap == hipStreamCaptureStatusNone,
               "torso_plan_build: the stream is capturing (the build reads the covered count back)");
    const PlanView v = plan_view(plan, N);
    hipLaunchKernelGGL(k_torso_mask, dim3(div_up(N, 256)), dim3(256), 0, s, bg_coords, N, density_grid_torso, grid_size, thresh, v.flags);
    hipLaunchKernelGGL(k_torso_select, dim3(1), dim3(kSelectThreads), 0, s, bg_coords, N, density_grid_torso, grid_size, thresh,
                       (const float *)nullptr, v.on_list, v.xy, v.count);
    if (int rc = check_launch("torso_plan_build(select)")) return rc;
    int32_t count = 0;
    if (hipMemcpyAsync(&count, v.count, sizeof(count), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
        set_error("torso_plan_build: reading the covered count failed");
        return RN_ERR_LAUNCH;
    }
    RN_REQUIRE(count >= 0 && (uint32_t)count <= N, "torso_plan_build: covered count %d of %u pixels", count, N);
    *n_on = (uint32_t)count;
    if (count == 0 || plan_bytes < rn_torso_plan_bytes(N, (uint32_t)count)) return RN_OK;
    const uint32_t n_tiles = ((uint32_t)count + 31u) >> 5;
    hipLaunchKernelGGL(k_torso_plan_enc, dim3(div_up(n_tiles, kPlanWaves)), dim3(kPlanThreads), 0, s, v.xy, (uint32_t)count, torso_shrink,
                       v.enc);
    return check_launch("torso_plan_build");
}

int rn_torso_blend_frame_planned(const void *plan, size_t plan_bytes, uint32_t N, uint32_t n_on, const float *poses6, const float *ind_code,
                                 float torso_shrink, const rn_torso_weights_t *w, const float *packed, const rn_grid_t *grid_torso,
                                 const float *bg_in, float *bg_out, float *torso_alpha, float *deform, float *image,
                                 const float *weights_sum, float *depth, const float *nears, const float *fars, uint8_t *image_u8,
                                 rn_stream_t stream) {
    if (N == 0) return RN_OK;
    RN_REQUIRE(plan && poses6 && w && packed, "torso_blend_frame_planned: null pointer");
    RN_REQUIRE(image && weights_sum && depth && nears && fars, "torso_blend_frame_planned: null frame buffers");
    RN_REQUIRE(ind_code || w->ind_dim == 0, "torso_blend_frame_planned: ind_code required when ind_dim > 0");
    RN_REQUIRE(((uintptr_t)packed & 15u) == 0 && ((uintptr_t)plan & (kPlanAlign - 1)) == 0, "torso_blend_frame_planned: packed must be 16-byte, plan 256-byte aligned");
    RN_REQUIRE(n_on <= N && N <= (1u << 30) && plan_bytes >= rn_torso_plan_bytes(N, n_on),
               "torso_blend_frame_planned: a plan of %zu bytes does not hold %u covered of %u pixels", plan_bytes, n_on, N);
    if (int rc = check_fused_grid(grid_torso, 2, "torso_blend_frame_planned(torso grid)")) return rc;
    const PlanView v = plan_view(const_cast<void *>(plan), N);
    const uint32_t on_blocks = div_up((n_on + 31u) >> 5, kPlanWaves), off_blocks = div_up(N, kPlanThreads * kPlanOffPixels);
    PlannedParams p{v.flags, v.on_list, v.xy, v.enc, N, n_on, on_blocks, poses6, ind_code, torso_shrink, raw_t(w), packed,
                    grid_args(grid_torso), bg_in, bg_out, torso_alpha, deform, BlendArgs{image, weights_sum, depth, nears, fars, image_u8}};
    const dim3 grid(on_blocks + off_blocks);
    if (grid_torso->dtype == RN_F32) hipLaunchKernelGGL((k_torso_planned<float, true>), grid, dim3(kPlanThreads), 0, as_stream(stream), p);
    else hipLaunchKernelGGL((k_torso_planned<__half, true>), grid, dim3(kPlanThreads), 0, as_stream(stream), p);
    return check_launch("torso_blend_frame_planned");
}

int rn_torso_mask(const float *bg_coords, uint32_t N, const float *density_grid_torso, uint32_t grid_size, float thresh,
                  uint8_t *mask, rn_stream_t stream) {
    if (N == 0) return RN_OK;
    RN_REQUIRE(bg_coords && density_grid_torso && mask && grid_size >= 2, "torso_mask: bad arguments");
    hipLaunchKernelGGL(k_torso_mask, dim3(div_up(N, 256)), dim3(256), 0, as_stream(stream), bg_coords, N, density_grid_torso, grid_size,
                       thresh, mask);
    return check_launch("torso_mask");
}

int rn_torso_select(const float *bg_coords, uint32_t N, const float *density_grid_torso, uint32_t grid_size, float density_thresh,
                    const float *mean_density_dev, int32_t *covered, float *xy_c, int32_t *count, rn_stream_t stream) {
    RN_REQUIRE(count, "torso_select: null pointer (count)");
    if (N == 0) return hipMemsetAsync(count, 0, sizeof(int32_t), as_stream(stream)) == hipSuccess ? RN_OK : RN_ERR_LAUNCH;
    RN_REQUIRE(bg_coords && density_grid_torso && covered && xy_c, "torso_select: null pointer");
    RN_REQUIRE(grid_size >= 2, "torso_select: grid_size must be at least 2");
    RN_REQUIRE(N <= (1u << 30), "torso_select: N = %u is more than 2^30 pixels (int32 indices)", N);
    RN_REQUIRE(((uintptr_t)xy_c & 7u) == 0, "torso_select: xy_c must be 8-byte aligned");
    hipLaunchKernelGGL(k_torso_select, dim3(1), dim3(kSelectThreads), 0, as_stream(stream), bg_coords, N, density_grid_torso, grid_size,
                       density_thresh, mean_density_dev, covered, xy_c, count);
    return check_launch("torso_select");
}

int rn_blend_frame(float *image, const float *weights_sum, const float *bg, float *depth, const float *nears,
                   const float *fars, uint32_t N, uint8_t *image_u8, rn_stream_t stream) {
    if (N == 0) return RN_OK;
    RN_REQUIRE(image && weights_sum && depth && nears && fars, "blend_frame: null pointer");
    hipLaunchKernelGGL(k_blend, dim3(div_up(N, 256)), dim3(256), 0, as_stream(stream), image, weights_sum, bg, depth, nears,
                       fars, N, image_u8);
    return check_launch("blend_frame");
}

}  // extern "C"
