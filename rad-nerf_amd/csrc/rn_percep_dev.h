// rn_percep_dev.h -- shapes, workspace layout and the split-K rule of the perceptual (LPIPS-alex) kernels (rn_percep.hip),
// shared by the host entry points and the kernels.
//
// Every map is channel-major: tap l is [C_l][2P][oh_l][ow_l] floats (images 0 .. P-1 are pred, P .. 2P-1 target), a gradient
// map [C_l][P][oh_l][ow_l] (pred half only).  A row of a map is therefore the N axis of the layer's implicit GEMM.
#pragma once

#include "rn_common.h"

namespace rn {
namespace percep {

constexpr int kLayers = 5;
constexpr uint32_t kCin[kLayers] = {3, 64, 192, 384, 256};
constexpr uint32_t kCout[kLayers] = {64, 192, 384, 256, 256};
constexpr uint32_t kKern[kLayers] = {11, 5, 3, 3, 3};
constexpr uint32_t kMinSide = 31;      // the second pool needs a 3 x 3 map
constexpr uint32_t kChannels = 64 + 192 + 384 + 256 + 256;
constexpr uint32_t kDistPos = 32;      // positions per workgroup of the distance kernel

// K of the forward GEMM of layer l, and K rounded up to the two-deep MFMA step (conv1: 363 -> 364, the extra row is zero)
__host__ __device__ constexpr uint32_t k_fwd(int l) { return kCin[l] * kKern[l] * kKern[l]; }
__host__ __device__ constexpr uint32_t k_fwd_pad(int l) { return (k_fwd(l) + 1u) & ~1u; }
__host__ __device__ constexpr uint32_t k_bwd(int l) { return kCout[l] * kKern[l] * kKern[l]; }    // always even

// ---- packed weight image (floats) -------------------------------------------------------------------------------------------
//   fwd[l]  l = 0..4: Wt[k][co], k = (ci, ky, kx) as unfold orders it       -- the A operand of the forward GEMM, co on the lanes
//   bwd[l]  l = 1..4: Wb[k][ci], k = (co, ky, kx)                           -- the A operand of the data-gradient GEMM (the
//                                                                              tap flip lives in the gather: iy = y + pad - ky)
//   bias [1152] | lin [1152] | shift [3] scale [3] pad [2]
struct ImageLayout {
    uint32_t fwd[kLayers], bwd[kLayers], bias, lin, ss, total;
};
__host__ __device__ constexpr ImageLayout image_layout() {
    ImageLayout L{};
    uint32_t at = 0;
    for (int l = 0; l < kLayers; l++) { L.fwd[l] = at; at += k_fwd_pad(l) * kCout[l]; }
    L.bwd[0] = at;
    for (int l = 1; l < kLayers; l++) { L.bwd[l] = at; at += k_bwd(l) * kCin[l]; }
    L.bias = at; at += kChannels;
    L.lin = at; at += kChannels;
    L.ss = at; at += 8;
    L.total = at;
    return L;
}
__host__ __device__ constexpr uint32_t channel_offset(int l) {
    uint32_t at = 0;
    for (int i = 0; i < l; i++) at += kCout[i];
    return at;
}

// ---- split-K rule ---------------------------------------------------------------------------------------------------------
// One wave owns one 32 x 32 output tile over one slice of K.  The slices are sized from the shape alone (not from the device, so
// the summation order is a property of the call): enough of them that tiles x slices reaches kTargetWaves, none shorter than
// kMinSteps two-deep MFMA steps.  The partial tiles are summed in slice order by the layer's epilogue kernel.
constexpr uint32_t kTargetWaves = 1024, kMinSteps = 32;
struct Split {
    uint32_t mt, nt, steps, len, S;     // tiles along M and N, MFMA steps in K, steps per slice, slices
};
static inline Split split_rule(uint32_t M, uint32_t N, uint32_t Kpad) {
    Split s;
    s.mt = M / 32u;
    s.nt = (N + 31u) / 32u;
    s.steps = Kpad / 2u;
    const uint32_t tiles = s.mt * s.nt;
    uint32_t want = (kTargetWaves + tiles - 1u) / tiles, cap = (s.steps + kMinSteps - 1u) / kMinSteps;
    if (want > cap) want = cap;
    if (want < 1u) want = 1u;
    s.len = (s.steps + want - 1u) / want;
    s.S = (s.steps + s.len - 1u) / s.len;
    return s;
}

// ---- workspace (floats) ---------------------------------------------------------------------------------------------------
struct Plan {
    uint32_t P, h, w;
    uint32_t oh[kLayers], ow[kLayers];          // tap l
    uint32_t tap[kLayers];                      // [C_l][2P][oh][ow]
    uint32_t dgrad[kLayers];                    // d value[p] / d tap l from the distance kernel, [C_l][P][oh][ow]
    uint32_t grad[kLayers];                     // full gradient of tap l (grad[4] == dgrad[4])
    uint32_t pooled;                            // gradient of a pooled conv input (conv2, conv3), before the routing
    uint32_t part;                              // split-K partial tiles
    uint32_t dist_part;                         // the distance kernel's per-workgroup sums (32 positions each)
    uint32_t vals;                              // [5][P] per-tap values
    uint64_t total;                             // floats; 0: the shape is refused
};
static inline uint32_t pool_out(uint32_t n) { return (n - 3u) / 2u + 1u; }
static inline Plan make_plan(uint32_t P, uint32_t h, uint32_t w) {
    Plan p{};
    p.P = P; p.h = h; p.w = w;
    if (P == 0 || h < kMinSide || w < kMinSide || h > 8192u || w > 8192u || P > 65536u) return p;
    p.oh[0] = (h + 4u - 11u) / 4u + 1u; p.ow[0] = (w + 4u - 11u) / 4u + 1u;
    p.oh[1] = pool_out(p.oh[0]); p.ow[1] = pool_out(p.ow[0]);
    for (int l = 2; l < kLayers; l++) { p.oh[l] = pool_out(p.oh[1]); p.ow[l] = pool_out(p.ow[1]); }
    uint64_t at = 0;
    auto take = [&](uint64_t n) { const uint64_t o = at; at += (n + 3u) & ~(uint64_t)3u; return o; };
    uint64_t off[3 * kLayers + 4];
    int q = 0;
    for (int l = 0; l < kLayers; l++) off[q++] = take((uint64_t)kCout[l] * 2u * P * p.oh[l] * p.ow[l]);
    for (int l = 0; l < kLayers; l++) off[q++] = take((uint64_t)kCout[l] * P * p.oh[l] * p.ow[l]);
    for (int l = 0; l < kLayers - 1; l++) off[q++] = take((uint64_t)kCout[l] * P * p.oh[l] * p.ow[l]);
    const uint64_t pooled1 = (uint64_t)kCin[1] * P * p.oh[1] * p.ow[1], pooled2 = (uint64_t)kCin[2] * P * p.oh[2] * p.ow[2];
    off[q++] = take(pooled1 > pooled2 ? pooled1 : pooled2);
    uint64_t part = 0;
    for (int l = 0; l < kLayers; l++) {
        const uint64_t Nf = (uint64_t)2u * P * p.oh[l] * p.ow[l], Nb = (uint64_t)P * p.oh[l] * p.ow[l];
        if (Nf >= (1ull << 28)) return p;
        const Split f = split_rule(kCout[l], (uint32_t)Nf, k_fwd_pad(l));
        const uint64_t a = (uint64_t)f.S * kCout[l] * Nf;
        part = a > part ? a : part;
        if (l > 0) {
            const Split b = split_rule(kCin[l], (uint32_t)Nb, k_bwd(l));
            const uint64_t c = (uint64_t)b.S * kCin[l] * Nb;
            part = c > part ? c : part;
        }
    }
    off[q++] = take(part);
    uint64_t dist_part = 0;
    for (int l = 0; l < kLayers; l++) dist_part += (uint64_t)P * ((p.oh[l] * p.ow[l] + kDistPos - 1u) / kDistPos);
    off[q++] = take(dist_part);
    off[q++] = take((uint64_t)kLayers * P);
    if (at >= (1ull << 31)) return p;           // every index of the kernels is a uint32_t
    q = 0;
    for (int l = 0; l < kLayers; l++) p.tap[l] = (uint32_t)off[q++];
    for (int l = 0; l < kLayers; l++) p.dgrad[l] = (uint32_t)off[q++];
    for (int l = 0; l < kLayers - 1; l++) p.grad[l] = (uint32_t)off[q++];
    p.grad[kLayers - 1] = p.dgrad[kLayers - 1];
    p.pooled = (uint32_t)off[q++];
    p.part = (uint32_t)off[q++];
    p.dist_part = (uint32_t)off[q++];
    p.vals = (uint32_t)off[q++];
    p.total = at;
    return p;
}

}  // namespace percep
}  // namespace rn
