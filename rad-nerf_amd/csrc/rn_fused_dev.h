// rn_fused_dev.h -- pieces shared by the translation units of the fused inference path: the fp32-MFMA (rn_fused.hip) and
// the 16-bit-MFMA (rn_fused_f16.hip) variants of the per-sample network kernel, the device-resident frame loop
// (rn_head_loop.hip) and the torso pass (rn_torso.hip); the training kernels (rn_train_head.hip, rn_train_torso.hip)
// reuse the parameter pieces and the grid check.  Here: 64-sample accumulator tiles and their VALU output layers (the
// 32-sample ones are in rn_tile32_dev.h), the raw weight and grid descriptors of the per-sample network (the torso layer's:
// rn_torso_dev.h), kernel parameter blocks, the tile bookkeeping (sample count, slot / liveness of an entry, direction
// load) and the launch dispatch.
#pragma once

#include "rn_dda_dev.h"
#include "rn_grid_dev.h"
#include "rn_sh_dev.h"
#include "rn_tile32_dev.h"

#include "../../include/radnerf_fused.h"

#ifndef RN_XCD_TILES
#define RN_XCD_TILES 1
#endif
#ifndef RN_TILE_CHUNK
#define RN_TILE_CHUNK 2
#endif

namespace rn {

constexpr int kFusedThreads = 512;
constexpr int kWavesPerBlock = kFusedThreads / kWave;

struct RawW {
    const float *amb_w0, *amb_w1, *amb_w2, *sig_w0, *sig_w1, *sig_w2, *col_w0, *col_w1;
    uint32_t audio_dim, has_eye, ind_dim;
};
inline RawW raw_w(const rn_nerf_weights_t *w) {
    return RawW{w->amb_w0, w->amb_w1, w->amb_w2, w->sig_w0, w->sig_w1, w->sig_w2, w->col_w0, w->col_w1,
                w->audio_dim, w->has_eye, w->ind_dim};
}

// acc[column tile][row tile]
struct Acc {
    f32x16 v[2][2];
};

__device__ __forceinline__ void acc_zero(Acc &a) {
#pragma unroll
    for (int nt = 0; nt < 2; nt++)
#pragma unroll
        for (int rt = 0; rt < 2; rt++)
#pragma unroll
            for (int r = 0; r < 16; r++) a.v[nt][rt][r] = 0.0f;
}

// accumulator rows of lane half h: 32 rt + (r & 3) + 8 (r >> 2) + 4 h -> four consecutive floats per r >> 2
__device__ __forceinline__ void acc_bias(Acc &a, const float *bias64, int h) {
#pragma unroll
    for (int rt = 0; rt < 2; rt++)
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const float4 b = *reinterpret_cast<const float4 *>(bias64 + 32 * rt + 8 * g + 4 * h);
            a.v[0][rt][4 * g + 0] = b.x; a.v[0][rt][4 * g + 1] = b.y; a.v[0][rt][4 * g + 2] = b.z; a.v[0][rt][4 * g + 3] = b.w;
            a.v[1][rt][4 * g + 0] = b.x; a.v[1][rt][4 * g + 1] = b.y; a.v[1][rt][4 * g + 2] = b.z; a.v[1][rt][4 * g + 3] = b.w;
        }
}

__device__ __forceinline__ void acc_relu(Acc &a) {
#pragma unroll
    for (int nt = 0; nt < 2; nt++)
#pragma unroll
        for (int rt = 0; rt < 2; rt++)
#pragma unroll
            for (int r = 0; r < 16; r++) a.v[nt][rt][r] = relu_bits(a.v[nt][rt][r]);
}


// out[o] (both column tiles) = sum_k in[k] * W[o][k] with the k's this lane holds; caller adds the other half
template <int NOUT>
__device__ __forceinline__ void valu_out(const Acc &in, const float *wl, int h, float (&part)[2][NOUT]) {
#pragma unroll
    for (int o = 0; o < NOUT; o++) {
        float p0 = 0.0f, p1 = 0.0f;
        const float *wo = wl + (o * 2 + h) * 32;
#pragma unroll
        for (int g = 0; g < 8; g++) {
            const float4 w = *reinterpret_cast<const float4 *>(wo + 4 * g);
            const int rt = g >> 2, r = (g & 3) * 4;
            p0 = __builtin_fmaf(in.v[0][rt][r + 0], w.x, p0); p1 = __builtin_fmaf(in.v[1][rt][r + 0], w.x, p1);
            p0 = __builtin_fmaf(in.v[0][rt][r + 1], w.y, p0); p1 = __builtin_fmaf(in.v[1][rt][r + 1], w.y, p1);
            p0 = __builtin_fmaf(in.v[0][rt][r + 2], w.z, p0); p1 = __builtin_fmaf(in.v[1][rt][r + 2], w.z, p1);
            p0 = __builtin_fmaf(in.v[0][rt][r + 3], w.w, p0); p1 = __builtin_fmaf(in.v[1][rt][r + 3], w.w, p1);
        }
        part[0][o] = p0 + __shfl_xor(p0, 32, 64);
        part[1][o] = p1 + __shfl_xor(p1, 32, 64);
    }
}


struct GridArgs {
    const void *table;
    const int32_t *offsets;
    LevelConsts lc;
    uint32_t gridtype;
};
inline GridArgs grid_args(const rn_grid_t *g) {
    return GridArgs{g->embeddings, g->offsets, make_level_consts(g->L, g->S, g->H), g->gridtype};
}

// Direction terms of the frame loop (rn_head_t.dir_term): the colour net's first-layer accumulators after the bias and the
// 8 SH(dir) steps are the same for every sample of a ray within a frame, so the launch of loop iteration 0 stores them, one
// row of 64 floats per ray ([lane half][32 accumulator registers], the register order), and the launches of the later
// iterations load them instead of recomputing them.  The ray of a sample: slot / n_step is its position in the alive list
// the iteration reads.  rows == NULL: every sample computes its own (every launch outside the loop).
struct DirTerm {
    float *rows;            // [n_rays][64], 16-byte aligned, or NULL
    const int32_t *state;   // the iteration's state bank: [2] = n_step
    const int32_t *alive;   // the alive list the iteration reads (before its compositor marks the rays that end)
    uint32_t n_rays;
    uint32_t store;         // 1: this launch writes the rows (iteration 0); 0: it reads them
};

struct FusedParams {
    const float *xyzs, *dirs, *deltas;
    uint32_t M;
    const int32_t *m_dev;
    GridArgs gx, gw;
    const float *packed, *bias;
    float bound;
    float *sigmas, *rgbs, *ambient;
    // optional list of live sample slots: entry j names the slot (row of xyzs / dirs / sigmas / rgbs / ambient) that the j-th
    // sample of the launch works on, every entry is live and M counts entries.  NULL: sample j is slot j (dead where
    // deltas[2 j] == 0).  Inside the frame loop the marchers write it, so the network skips the dead slots of rays that
    // ended in the middle of their n_step samples (16 % of the slots of the benchmark stream).
    const int32_t *slots;
    DirTerm dt;   // read by k_nerf_fused only: the 16-bit kernels wait on their gathers and spend one or two MFMAs on SH
};

// XCD-aware tile schedule.  Workgroups are dealt round-robin over the 8 XCDs (workgroup b lands on XCD b % 8; used for
// speed only -- any placement gives the same results), and every XCD has its own 4 MB L2.  Samples arrive ray-ordered,
// i.e. consecutive tiles are neighbouring pixels whose samples share most of their grid rows on the coarse and middle
// levels.  Giving each XCD one CONTIGUOUS eighth of the tiles (a band of the image) instead of every eighth workgroup's
// tiles keeps those shared rows in one L2 instead of fetching them into all eight.
struct TileSchedule {
    uint32_t first, end, stride;
    __device__ __forceinline__ TileSchedule(uint32_t n_tiles, uint32_t waves_per_block, uint32_t wave) {
        const uint32_t G = gridDim.x, b = blockIdx.x;
#if RN_XCD_TILES
        if (G >= 8 && (G & 7u) == 0) {
            const uint32_t xcd = b & 7u, local = b >> 3, per_xcd = (n_tiles + 7u) >> 3;
            const uint32_t lo = xcd * per_xcd, hi = lo + per_xcd < n_tiles ? lo + per_xcd : n_tiles;
            // Within the band, RN_TILE_CHUNK consecutive tiles go to one workgroup and the next chunk to the next
            // workgroup; a workgroup's second chunk lands on its next RN_TILE_CHUNK waves.  A launch of the frame loop
            // holds 1.0 - 2.0 tiles per wave slot of the chip, so what matters is that the tiles beyond one full round
            // are spread over all CUs (chunk < waves per workgroup) instead of doubling up a few of them.
            constexpr uint32_t C = RN_TILE_CHUNK;
            const uint32_t chunk = (C < waves_per_block && waves_per_block % C == 0) ? C : waves_per_block, B = G >> 3;
            first = lo + ((wave / chunk) * B + local) * chunk + wave % chunk;
            end = lo < hi ? hi : lo;
            stride = B * waves_per_block;
            return;
        }
#endif
        first = b * waves_per_block + wave;
        end = n_tiles;
        stride = G * waves_per_block;
    }
};

// ---- tile bookkeeping, the same in k_nerf_fused, k_nerf_fused_h16 and k_nerf_fused_x2 -------------------------------
// The helpers take the fields of FusedParams they need by value: a kernel that hands out a reference to its parameter
// block is compiled to a different instruction stream.  What is NOT here although all three kernels spell it alike: the
// fill of plan_x / plan_w and the xyz normalisation (as helpers they reorder loads / swap the operands of one packed add
// in the 16-bit kernels), and in k_nerf_fused everything but workgroup_idle() (its register allocation changes with
// launch_samples() and entry_slot(); that kernel's instruction stream is held fixed).

// sample count of the launch: the host's upper bound, clamped by the device-side count where the frame loop keeps one
__device__ __forceinline__ uint32_t launch_samples(uint32_t M, const int32_t *m_dev) {
    if (m_dev) { const uint32_t d = (uint32_t)*m_dev; M = d < M ? d : M; }
    return M;
}

// the training kernels' form: a non-positive device count means no samples
__device__ __forceinline__ uint32_t live_count(uint32_t M, const int32_t *m_dev) {
    if (!m_dev) return M;
    const int32_t d = *m_dev;
    return d <= 0 ? 0u : ((uint32_t)d < M ? (uint32_t)d : M);
}

// true where the schedule leaves this workgroup without a tile (uniform over the workgroup)
__device__ __forceinline__ bool workgroup_idle(uint32_t n_tiles, uint32_t waves_per_block) {
    const TileSchedule w0(n_tiles, waves_per_block, 0u);
    return w0.first >= w0.end;
}

// Slot and liveness of entry `entry` of the launch (the caller derives it from tile and lane: 64 entries per tile, one
// per lane, in the 16-bit kernels; 32 per tile, shared by both lane halves, in the fp32 kernel).  With a slot list every
// entry below M is live and names its slot; without one, entry j is slot j and dead where deltas[2 j] == 0.
__device__ __forceinline__ bool entry_slot(const int32_t *slots, const float *deltas, uint32_t entry, uint32_t M, uint32_t &sample) {
    bool live = entry < M;
    sample = entry;  // the slot this lane's sample lives in
    if (slots) {
        if (live) sample = (uint32_t)slots[entry];
    } else if (live && deltas) {
        live = deltas[2 * (size_t)sample] != 0.0f;
    }
    return live;
}

// view direction of a live sample into (dx, dy, dz), which the caller has zeroed (they stay 0 for a dead lane and for
// the density query, which passes no directions)
__device__ __forceinline__ void load_dir(const float *dirs, bool live, uint32_t sample, float &dx, float &dy, float &dz) {
    if (live && dirs) {
        dx = dirs[3 * (size_t)sample]; dy = dirs[3 * (size_t)sample + 1]; dz = dirs[3 * (size_t)sample + 2];
    }
}

// DirTerm: ceil(2^32 / n_step) for n_step >= 2, 0 for n_step == 1.  slot / n_step == __umulhi(slot, that) exactly while
// slot * (n_step - 1) < 2^32 (multiplier * n_step exceeds 2^32 by at most n_step - 1): n_step <= 8, so for every slot below
// 2^29 -- an integer multiply-shift, no float reciprocal.
__device__ __forceinline__ uint32_t dir_term_step_rcp(const int32_t *state) {
    const uint32_t n_step = (uint32_t)state[2];
    return n_step > 1u ? 0xFFFFFFFFu / n_step + 1u : 0u;
}
// DirTerm: the row (ray) of sample slot `sample`, or ~0u for a dead lane and for anything outside the list or the buffer
__device__ __forceinline__ uint32_t dir_term_row(const int32_t *alive, uint32_t step_rcp, uint32_t n_rays, bool live, uint32_t sample) {
    uint32_t row = ~0u;
    if (live) {
        const uint32_t pos = step_rcp ? __umulhi(sample, step_rcp) : sample;
        if (pos < n_rays) {
            const uint32_t ray = (uint32_t)alive[pos];
            if (ray < n_rays) row = ray;
        }
    }
    return row;
}

// (grid table dtypes) -> the <TX, TW> instantiation: calls f(TX{}, TW{}) with float or __half values as type tags
template <typename F>
static inline void dispatch_grid_dtypes(int gx_dtype, int gw_dtype, F &&f) {
    if (gx_dtype == RN_F32 && gw_dtype == RN_F32) f(float{}, float{});
    else if (gx_dtype == RN_F16 && gw_dtype == RN_F16) f(__half{}, __half{});
    else if (gx_dtype == RN_F32) f(float{}, __half{});
    else f(__half{}, float{});
}

// The grid check of the training entries (rn_train_head.hip, rn_train_torso.hip): `what` names the entry and the grid
static inline int check_train_grid(const rn_grid_t *g, uint32_t D, const char *what) {
    RN_REQUIRE(g && g->embeddings && g->offsets, "%s grid is null", what);
    RN_REQUIRE(g->D == D && g->L == 16 && g->dtype == RN_F32, "%s grid must be D=%u, L=16, fp32 with C=2", what, D);
    return RN_OK;
}

// Host side of the network launch (rn_fused.hip): the frame loop and the torso pass check their grids the same way, and
// the loop launches the network kernel through run_fused() -- a kernel is launched from its own translation unit.
int check_fused_grid(const rn_grid_t *g, uint32_t D, const char *name);
int run_fused(const float *xyzs, const float *dirs, const float *deltas, uint32_t M, const int32_t *m_dev, const rn_grid_t *gx,
              const rn_grid_t *gw, const float *packed, const float *bias, float bound, float *sigmas, float *rgbs, float *ambient,
              int mlp_dtype, hipStream_t s, const int32_t *slots = nullptr, const DirTerm &dt = DirTerm{});
// The 16-bit matrix-core variants (rn_fused_f16.hip); `gx_dtype` / `gw_dtype` are the grid table dtypes.
void launch_fused_h16(const FusedParams &p, int gx_dtype, int gw_dtype, uint32_t blocks, hipStream_t s);
void launch_pack_nerf_h16(const RawW &w, float *packed, hipStream_t s);
size_t packed_floats_h16();
// The split-precision variant picks its own grid (one 512-thread workgroup per CU).
void launch_fused_x2(const FusedParams &p, int gx_dtype, int gw_dtype, uint32_t n_cus, hipStream_t s);
void launch_pack_nerf_x2(const RawW &w, float *packed, hipStream_t s);
size_t packed_floats_x2();

}  // namespace rn
