// rn_fused.hip -- the fused per-sample network kernel (gfx950).
//
// C ABI: include/radnerf_fused.h (rn_nerf_*).  What is computed: nerf/network.py:222-283 per sample; the frame loop that
// feeds it is rn_head_loop.hip, the torso pass rn_torso.hip.  How (MI355X-first):
//
//  * one wavefront owns a tile of 32 samples; both lane halves work on the same samples.  A gather round has lane half
//    h fetch level 2 r + h of its sample (multires grid rows with 8-byte loads, same device code as the standalone
//    encoder, so features are bit-identical); the MLP phases run on v_mfma_f32_32x32x2_f32 (exact fp32 FMA chains):
//    outputs on the 32 rows of the tile, samples on its 32 columns, k on the lane half -- so a gathered feature IS the
//    B operand of an MFMA step (no cross-lane move) and a grid costs 8 rounds, not 16 levels, of latency.
//  * a 32x32 accumulator has the sample on the lane and the output row on the register index, i.e. it already IS the
//    B operand of the next layer (k order permuted -- the weight image is packed in that order once, on the device).
//  * all weights (79.4 KB fp32) sit in LDS for the lifetime of a persistent 768-thread workgroup (one per CU, three
//    waves per SIMD: 3 x 32 accumulator VGPRs leave room for that).  fp32 MFMA and fp32 VALU work share the FMA rate of a SIMD ("where the time goes"),
//    so the instruction stream around the MFMAs is kept short: per-level plans (rn_grid_dev.h), one-instruction ReLU.
//  * inputs that are the same for every sample of a frame (audio code, eye, individual code) never enter
//    the per-sample GEMMs: they are folded into 3 x 64 bias values per frame, used as the accumulators'
//    initial value.  Outputs narrower than a tile (ambient 2, sigma 1, rgb 3) are VALU dot products over
//    the accumulator registers + one cross-half shuffle.
//  * the geo_feat layer is not run: sigma_net's last layer and color_net's first are linear with nothing in between, so
//    the packer multiplies their 64 x 64 blocks once (rn_nerf_image_dev.h: nerf_infer_image_elem) and the colour net's
//    first layer reads the sigma net's last hidden activations directly -- 64 of a tile's 368 MFMAs and 16 KB of LDS less.
#include "rn_nerf_image_dev.h"

namespace rn {

#ifndef RN_FUSED_PAIR_HASHED
#define RN_FUSED_PAIR_HASHED 0
#endif
#ifndef RN_F32_XYZ_GROUP
#define RN_F32_XYZ_GROUP 1
#endif
#ifndef RN_F32_AMB_GROUP
#define RN_F32_AMB_GROUP 2
#endif
constexpr int kXyzGroup = RN_F32_XYZ_GROUP, kAmbGroup = RN_F32_AMB_GROUP;  // gather rounds in flight per wave (divide 8)
#ifndef RN_F32_WAVES
#define RN_F32_WAVES 12
#endif
constexpr int kF32Waves = RN_F32_WAVES, kF32Threads = kF32Waves * kWave;  // 3 waves per SIMD (accumulators: 3 x 32 VGPRs), one workgroup per CU
constexpr bool kPairHashed = RN_FUSED_PAIR_HASHED;  // aligned x-pair loads on hashed levels inside the fused kernels

constexpr int kLdsFloats = kInferPacked + kBias;     // inference image + biases: 80128 B of LDS

__global__ void __launch_bounds__(256) k_pack_nerf(RawW w, float *__restrict__ packed) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= kInferPacked) return;
    packed[e] = nerf_infer_image_elem(w, e);
}

// Per-frame bias vectors (the broadcast columns of the three first layers).
__global__ void __launch_bounds__(kBias) k_frame_bias(RawW w, const float *__restrict__ enc_a,
                                                      const float *__restrict__ eye,
                                                      const float *__restrict__ ind_code, float *__restrict__ bias) {
    const int t = threadIdx.x;
    enc_a += (size_t)blockIdx.x * w.audio_dim;      // one workgroup per frame (rn_nerf_frame_bias_batch)
    bias += (size_t)blockIdx.x * kBias;
    bias[t] = nerf_const_bias(w, enc_a, eye, ind_code, t);
}

// -DRN_PHASE_CLOCK (tools/gpu_phase_clock.sh only): lanes 0..1 of every tile overwrite their `ambient` outputs with the
// 100 MHz wall-clock ticks spent in the phases of the tile loop (xyz gather, ambient net, ambient gather, rest).
#ifdef RN_PHASE_CLOCK
#define RN_PHASE_MARK(i) const uint64_t phase_t##i = wall_clock64()
#define RN_PHASE_STORE()                                                                                        \
    if (p.ambient && lane < 2 && entry + 1 < M) {                                                               \
        p.ambient[2 * (size_t)sample] = (float)(lane ? phase_t3 - phase_t2 : phase_t1 - phase_t0);                \
        p.ambient[2 * (size_t)sample + 1] = (float)(lane ? phase_t4 - phase_t3 : phase_t2 - phase_t1);            \
    }
#else
#define RN_PHASE_MARK(i)
#define RN_PHASE_STORE()
#endif

template <typename TX, typename TW>
__global__ void __launch_bounds__(kF32Threads, kF32Waves / 4) k_nerf_fused(FusedParams p) {
    __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
    __shared__ LevelPlan plan_x[16], plan_w[16];

    uint32_t M = p.M;
    if (p.m_dev) { const uint32_t d = (uint32_t)*p.m_dev; M = d < M ? d : M; }
    const uint32_t n_tiles = (M + 31u) >> 5;
    if (workgroup_idle(n_tiles, kF32Waves)) return;

    for (int i = threadIdx.x; i < kInferPacked / 4; i += kF32Threads)
        reinterpret_cast<float4 *>(lds)[i] = reinterpret_cast<const float4 *>(p.packed)[i];
    if (threadIdx.x < kBias) lds[kInferPacked + threadIdx.x] = p.bias[threadIdx.x];
    if (threadIdx.x < 16) {
        const int t = threadIdx.x;
        const uint32_t ox = (uint32_t)p.gx.offsets[t], ow = (uint32_t)p.gw.offsets[t];
        plan_x[t] = plan_level<3>(p.gx.lc.scale[t], p.gx.lc.resolution[t], ox, (uint32_t)p.gx.offsets[t + 1] - ox,
                                  p.gx.gridtype, (uint32_t)sizeof(TX) * 2u);
        plan_w[t] = plan_level<2>(p.gw.lc.scale[t], p.gw.lc.resolution[t], ow, (uint32_t)p.gw.offsets[t + 1] - ow,
                                  p.gw.gridtype, (uint32_t)sizeof(TW) * 2u);
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int lane_off = h * 64 + j * 2;
    const float *bias_amb = lds + kInferPacked, *bias_sig = lds + kInferPacked + 64, *bias_col = lds + kInferPacked + 128;

    // direction terms (DirTerm, rn_fused_dev.h): wave-uniform, fixed for the launch
    const bool term_load = p.dt.rows && !p.dt.store, term_store = p.dt.rows && p.dt.store;
    const uint32_t step_rcp = p.dt.rows ? dir_term_step_rcp(p.dt.state) : 0u;

    const TileSchedule sched(n_tiles, kF32Waves, (uint32_t)wave);
    for (uint32_t tile = sched.first; tile < sched.end; tile += sched.stride) {
        const uint32_t entry = tile * 32 + j;  // both lane halves work on the same 32 samples
        bool live = entry < M;
        uint32_t sample = entry;  // the slot this lane's sample lives in
        if (p.slots) {
            if (live) sample = (uint32_t)p.slots[entry];
        } else if (live && p.deltas) {
            live = p.deltas[2 * (size_t)sample] != 0.0f;
        }
        if (__ballot(live) == 0ull) continue;  // whole tile dead (wave-uniform)

        // ---- xyz grid (gridencoder/grid.py:145-161: (x + bound) / (2 bound)).  Round r: lane half h gathers level
        // 2 r + h of its sample; the two features are the B operands of two MFMA steps of BOTH first layers that
        // consume enc_x (ambient L0 and sigma L0), so enc_x is never kept in registers.
        Acc32 a0, a1, a2;
        RN_PHASE_MARK(0);
        acc_bias(a0, bias_amb, h);  // ambient L0 accumulators, start = W0[:, 32:] enc_a
        acc_bias(a2, bias_sig, h);  // sigma   L0 accumulators, start = W0[:, 64] eye
        {
            float in[3] = {0.0f, 0.0f, 0.0f};
            bool on = live;
            if (live) {
#pragma unroll
                for (int d = 0; d < 3; d++) {
                    in[d] = (p.xyzs[3 * (size_t)sample + d] + p.bound) / (2 * p.bound);
                    on = on && !(in[d] < 0 || in[d] > 1);
                }
            }
            // kXyzGroup rounds in flight: independent chains (index arithmetic, loads, blends) that hide each other's latency
            LevelFetch<TX, 3, 2> f[kXyzGroup];
#pragma unroll 1
            for (int r = 0; r < 8; r += kXyzGroup) {
                if (on) {
#pragma unroll
                    for (int i = 0; i < kXyzGroup; i++)
                        issue_planned<TX, 3, 2, kPairHashed, false>(static_cast<const TX *>(p.gx.table), plan_x[2 * (r + i) + h], in, f[i]);
                }
#pragma unroll
                for (int i = 0; i < kXyzGroup; i++) {
                    float f0 = 0.0f, f1 = 0.0f;
                    if (on) {
                        TX res[2];
                        TX dummy[1];
                        blend_level<TX, 3, 2, false>(f[i], 0.0f, res, dummy);
                        f0 = to_f<TX>(res[0]);
                        f1 = to_f<TX>(res[1]);
                    }
                    step32(a0, lds + OFF_A0, 2 * (r + i), lane_off, f0);
                    step32(a2, lds + OFF_S0, 2 * (r + i), lane_off, f0);
                    step32(a0, lds + OFF_A0, 2 * (r + i) + 1, lane_off, f1);
                    step32(a2, lds + OFF_S0, 2 * (r + i) + 1, lane_off, f1);
                }
            }
        }

        // ---- ambient net: [enc_x | enc_a] 96 -> 64 -> 64 -> 2, tanh
        RN_PHASE_MARK(1);
        acc_relu(a0);
        acc_zero(a1);
        layer_from_acc(a1, a0, lds + OFF_A1, lane_off);
        acc_relu(a1);
        float amb[2];
        valu_out<2>(a1, lds + OFF_A2, h, amb);
        amb[0] = tanhf(amb[0]);
        amb[1] = tanhf(amb[1]);
        if (p.ambient && live && h == 0) {
            p.ambient[2 * (size_t)sample] = amb[0];
            p.ambient[2 * (size_t)sample + 1] = amb[1];
        }

        // ---- a0 is dead from here to the colour net: an iteration >= 1 of the frame loop fetches its ray's direction term
        // into it now (8 x 16 bytes per lane), so the loads pass under the ambient gather and the sigma net's 64 MFMAs
        if (term_load) {
            const uint32_t row = dir_term_row(p.dt.alive, step_rcp, p.dt.n_rays, live, sample);
            if (__ballot(row == ~0u) != 0ull) acc_zero(a0);  // dead lanes of a tail tile (wave-uniform: no other tile pays for it)
            if (row != ~0u) {
                // a 32-bit byte offset on the scalar base (n_rays <= 2^24, checked by rn_head_iterate_ex): a 64-bit per-lane base would be one more
                // loop-invariant register pair than this kernel has
                const float4 *src = reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(p.dt.rows) + (row * 256u + (uint32_t)h * 128u));
#pragma unroll
                for (int g = 0; g < 8; g++) {
                    const float4 t = src[g];
                    a0.v[g >> 2][4 * (g & 3) + 0] = t.x; a0.v[g >> 2][4 * (g & 3) + 1] = t.y;
                    a0.v[g >> 2][4 * (g & 3) + 2] = t.z; a0.v[g >> 2][4 * (g & 3) + 3] = t.w;
                }
            }
        }

        // ---- ambient grid: enc_w = encoder_ambient(ambient, bound=1) -> sigma L0 steps 16..31
        RN_PHASE_MARK(2);
        {
            float in[2] = {(amb[0] + 1.0f) / 2.0f, (amb[1] + 1.0f) / 2.0f};
            const bool on = live && !(in[0] < 0 || in[0] > 1 || in[1] < 0 || in[1] > 1);
            LevelFetch<TW, 2, 2> f[kAmbGroup];
#pragma unroll 1
            for (int r = 0; r < 8; r += kAmbGroup) {
                if (on) {
#pragma unroll
                    for (int i = 0; i < kAmbGroup; i++)
                        issue_planned<TW, 2, 2, kPairHashed, false>(static_cast<const TW *>(p.gw.table), plan_w[2 * (r + i) + h], in, f[i]);
                }
#pragma unroll
                for (int i = 0; i < kAmbGroup; i++) {
                    float f0 = 0.0f, f1 = 0.0f;
                    if (on) {
                        TW res[2];
                        TW dummy[1];
                        blend_level<TW, 2, 2, false>(f[i], 0.0f, res, dummy);
                        f0 = to_f<TW>(res[0]);
                        f1 = to_f<TW>(res[1]);
                    }
                    step32(a2, lds + OFF_S0, 16 + 2 * (r + i), lane_off, f0);
                    step32(a2, lds + OFF_S0, 16 + 2 * (r + i) + 1, lane_off, f1);
                }
            }
        }

        // ---- sigma net: [enc_x | enc_w | eye] 65 -> 64 -> 64 -> 1 (+ 64 geo_feat rows, folded into the colour net)
        RN_PHASE_MARK(3);
        acc_relu(a2);
        acc_zero(a1);
        layer_from_acc(a1, a2, lds + OFF_S1, lane_off);
        acc_relu(a1);
        float sigma;
        {
            float raw[1];
            valu_out<1>(a1, lds + IOFF_S2R, h, raw);
            sigma = expf(raw[0]);  // trunc_exp forward (activation.py:9-11)
        }
        if (!p.rgbs) {  // density query (NeRFNetwork.density, nerf/network.py:286-325): no SH, no colour net
            if (live && h == 0) p.sigmas[sample] = sigma;
            continue;
        }

        // ---- color net: [SH(d) | geo_feat | ind_code] 84 -> 64 -> 3, sigmoid; the geo_feat columns of its first layer are
        // packed times sigma L2's geo_feat rows, so their 32 steps take the sigma net's hidden activations (a1).
        // The bias and the 8 SH steps are the ray's direction term: the same bits for every sample of the ray (exact FMA chains
        // over the same operands in the same order), so only the loop's iteration 0 and launches outside the loop run them.
        if (!term_load) {
            acc_bias(a0, bias_col, h);
            float sh[16];
            float dx = 0.0f, dy = 0.0f, dz = 0.0f;
            if (live) {
                dx = p.dirs[3 * (size_t)sample]; dy = p.dirs[3 * (size_t)sample + 1]; dz = p.dirs[3 * (size_t)sample + 2];
            }
            sh_basis<4>(dx, dy, dz, sh);
#pragma unroll
            for (int s = 0; s < 8; s++) {
                // lane half h supplies k = 2 s + h; a bit-select, because ?: on two array elements makes the compiler
                // index sh[] dynamically and move it to LDS
                const uint32_t m = 0u - (uint32_t)h;
                const uint32_t b = (__float_as_uint(sh[2 * s]) & ~m) | (__float_as_uint(sh[2 * s + 1]) & m);
                step32(a0, lds + IOFF_C0, s, lane_off, __uint_as_float(b));
            }
            if (term_store) {  // every live sample of iteration 0 writes its ray's row (n_step > 1 there: the same bytes again)
                const uint32_t row = dir_term_row(p.dt.alive, step_rcp, p.dt.n_rays, live, sample);
                if (row != ~0u) {
                    float4 *dst = reinterpret_cast<float4 *>(reinterpret_cast<char *>(p.dt.rows) + (row * 256u + (uint32_t)h * 128u));
#pragma unroll
                    for (int g = 0; g < 8; g++)
                        dst[g] = make_float4(a0.v[g >> 2][4 * (g & 3) + 0], a0.v[g >> 2][4 * (g & 3) + 1],
                                             a0.v[g >> 2][4 * (g & 3) + 2], a0.v[g >> 2][4 * (g & 3) + 3]);
                }
            }
        }
#pragma unroll
        for (int s = 0; s < 32; s++) step32(a0, lds + IOFF_C0, 8 + s, lane_off, a1.v[s >> 4][s & 15]);
        acc_relu(a0);
        {
            float rgb[3];
            valu_out<3>(a0, lds + IOFF_C1, h, rgb);
            if (live && h == 0) {
                p.sigmas[sample] = sigma;
#pragma unroll
                for (int c = 0; c < 3; c++) p.rgbs[3 * (size_t)sample + c] = 1.0f / (1.0f + expf(-rgb[c]));
            }
        }
        RN_PHASE_MARK(4);
        RN_PHASE_STORE();
    }
}

// ---- host helpers ---------------------------------------------------------------------------------------
int check_fused_grid(const rn_grid_t *g, uint32_t D, const char *name) {
    RN_REQUIRE(g && g->embeddings && g->offsets, "%s: null grid", name);
    RN_REQUIRE(g->D == D && g->L == 16, "%s: fused path needs D=%u, L=16 (got D=%u L=%u)", name, D, g->D, g->L);
    RN_REQUIRE(g->gridtype <= 1 && (g->dtype == RN_F32 || g->dtype == RN_F16), "%s: bad gridtype/dtype", name);
    RN_REQUIRE(((uintptr_t)g->embeddings & 7u) == 0, "%s: table must be 8-byte aligned", name);
    return RN_OK;
}
static int check_w(const rn_nerf_weights_t *w) {
    RN_REQUIRE(w && w->amb_w0 && w->amb_w1 && w->amb_w2 && w->sig_w0 && w->sig_w1 && w->sig_w2 && w->col_w0 && w->col_w1,
               "nerf weights: null pointer");
    RN_REQUIRE(w->has_eye <= 1 && w->audio_dim <= 1024 && w->ind_dim <= 1024, "nerf weights: bad dims");
    return RN_OK;
}

template <typename TX, typename TW>
static void launch_fused(const FusedParams &p, hipStream_t s) {
    const uint32_t n_tiles = (p.M + 31u) >> 5;
    uint32_t blocks = div_up(n_tiles, kF32Waves);
    const uint32_t cap = (uint32_t)num_cus();  // one persistent workgroup per CU (80.1 KB of LDS each)
    if (blocks > cap) blocks = cap;
    RN_LAUNCH_TIMED((k_nerf_fused<TX, TW>), dim3(blocks), dim3(kF32Threads), s, p);
}

int run_fused(const float *xyzs, const float *dirs, const float *deltas, uint32_t M, const int32_t *m_dev, const rn_grid_t *gx,
              const rn_grid_t *gw, const float *packed, const float *bias, float bound, float *sigmas, float *rgbs, float *ambient,
              int mlp_dtype, hipStream_t s, const int32_t *slots, const DirTerm &dt) {
    FusedParams p{xyzs, dirs, deltas, M, m_dev, grid_args(gx), grid_args(gw), packed, bias, bound, sigmas, rgbs, ambient, slots, dt};
    if (mlp_dtype == RN_F32_SPLIT) {
        launch_fused_x2(p, gx->dtype, gw->dtype, (uint32_t)num_cus(), s);
    } else if (mlp_dtype == RN_F16) {
        uint32_t blocks = div_up((M + 63u) >> 6, kWavesPerBlock);
        const uint32_t cap = (uint32_t)num_cus();
        launch_fused_h16(p, gx->dtype, gw->dtype, blocks > cap ? cap : blocks, s);
    } else {
        dispatch_grid_dtypes(gx->dtype, gw->dtype, [&](auto tx, auto tw) { launch_fused<decltype(tx), decltype(tw)>(p, s); });
    }
    return RN_OK;
}

}  // namespace rn

using namespace rn;

extern "C" {

size_t rn_nerf_packed_floats(void) { return (size_t)kInferPacked; }
size_t rn_nerf_packed_floats_h16(void) { return packed_floats_h16(); }
size_t rn_nerf_packed_floats_split(void) { return packed_floats_x2(); }

int rn_nerf_pack_weights_split(const rn_nerf_weights_t *w, float *packed, rn_stream_t stream) {
    if (int rc = check_w(w)) return rc;
    RN_REQUIRE(packed && ((uintptr_t)packed & 15u) == 0, "nerf_pack_weights_split: packed must be 16-byte aligned");
    launch_pack_nerf_x2(raw_w(w), packed, as_stream(stream));
    return check_launch("nerf_pack_weights_split");
}

int rn_nerf_pack_weights_h16(const rn_nerf_weights_t *w, float *packed, rn_stream_t stream) {
    if (int rc = check_w(w)) return rc;
    RN_REQUIRE(packed && ((uintptr_t)packed & 15u) == 0, "nerf_pack_weights_h16: packed must be 16-byte aligned");
    launch_pack_nerf_h16(raw_w(w), packed, as_stream(stream));
    return check_launch("nerf_pack_weights_h16");
}
size_t rn_nerf_bias_floats(void) { return (size_t)kBias; }

int rn_nerf_pack_weights(const rn_nerf_weights_t *w, float *packed, rn_stream_t stream) {
    if (int rc = check_w(w)) return rc;
    RN_REQUIRE(packed && ((uintptr_t)packed & 15u) == 0, "nerf_pack_weights: packed must be 16-byte aligned");
    hipLaunchKernelGGL(k_pack_nerf, dim3(div_up(kInferPacked, 256)), dim3(256), 0, as_stream(stream), raw_w(w), packed);
    return check_launch("nerf_pack_weights");
}

int rn_nerf_frame_bias(const rn_nerf_weights_t *w, const float *enc_a, const float *eye, const float *ind_code,
                       float *bias, rn_stream_t stream) {
    if (int rc = check_w(w)) return rc;
    RN_REQUIRE(bias, "nerf_frame_bias: null output");
    RN_REQUIRE(enc_a || w->audio_dim == 0, "nerf_frame_bias: enc_a is required");
    RN_REQUIRE(eye || !w->has_eye, "nerf_frame_bias: eye is required when has_eye");
    RN_REQUIRE(ind_code || w->ind_dim == 0, "nerf_frame_bias: ind_code is required when ind_dim > 0");
    hipLaunchKernelGGL(k_frame_bias, dim3(1), dim3(kBias), 0, as_stream(stream), raw_w(w), enc_a, eye, ind_code, bias);
    return check_launch("nerf_frame_bias");
}

int rn_nerf_frame_bias_batch(const rn_nerf_weights_t *w, const float *enc_a, uint32_t n, const float *eye, const float *ind_code,
                             float *bias, rn_stream_t stream) {
    if (n == 0) return RN_OK;
    if (int rc = check_w(w)) return rc;
    RN_REQUIRE(bias && (enc_a || w->audio_dim == 0) && (eye || !w->has_eye) && (ind_code || w->ind_dim == 0),
               "nerf_frame_bias_batch: null pointer");
    hipLaunchKernelGGL(k_frame_bias, dim3(n), dim3(kBias), 0, as_stream(stream), raw_w(w), enc_a, eye, ind_code, bias);
    return check_launch("nerf_frame_bias_batch");
}

int rn_nerf_fused_forward(const float *xyzs, const float *dirs, const float *deltas, uint32_t M, const int32_t *m_dev,
                          const rn_grid_t *grid_xyz, const rn_grid_t *grid_amb, const float *packed, const float *bias,
                          float bound, float *sigmas, float *rgbs, float *ambient, int mlp_dtype, rn_stream_t stream) {
    if (M == 0) return RN_OK;
    RN_REQUIRE(xyzs && packed && bias && sigmas && (dirs || !rgbs), "nerf_fused_forward: null pointer");
    RN_REQUIRE(((uintptr_t)packed & 15u) == 0, "nerf_fused_forward: packed must be 16-byte aligned");
    if (int rc = check_fused_grid(grid_xyz, 3, "nerf_fused_forward(xyz grid)")) return rc;
    if (int rc = check_fused_grid(grid_amb, 2, "nerf_fused_forward(ambient grid)")) return rc;
    RN_REQUIRE(mlp_dtype == RN_F32 || mlp_dtype == RN_F16 || mlp_dtype == RN_F32_SPLIT,
               "nerf_fused_forward: mlp_dtype must be RN_F32, RN_F16 or RN_F32_SPLIT");
    run_fused(xyzs, dirs, deltas, M, m_dev, grid_xyz, grid_amb, packed, bias, bound, sigmas, rgbs, ambient, mlp_dtype,
              as_stream(stream));
    return check_launch("nerf_fused_forward");
}

}  // extern "C"
