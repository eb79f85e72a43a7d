// rn_resample_dev.h -- the tile, the staged span and the limits of the resampling kernels (rn_resample.hip), shared by the host
// entry points.  See include/radnerf_fused.h for the arithmetic.
//
// One workgroup of kTile threads writes kTile consecutive outputs, one per thread.  Its outputs t .. t + kTile - 1 read the input
// indices n(t) - W .. n(t + kTile - 1) + W with n(t) = (t M) / L; n(t + i) - n(t) <= (i M) / L + 1, so the span is at most
// span_floats() elements whatever t is.  The span is staged in LDS once (zeros where it leaves the buffer), then every thread walks
// its 2 W + 1 taps over it.
//
// The table is tap-major, [2 W + 1][L]: for a fixed tap the 64 lanes of a wave read the phases (p0 + i M) % L of ONE row of L
// floats (640 bytes at 44.1 kHz, one address at 48 kHz), and every wave of the launch walks the same rows in the same order.
// Phase-major rows [L][2 W + 1] would put every lane on a cache line of its own for each load.
#pragma once

#include "rn_common.h"

#include "../../include/radnerf_fused.h"

namespace rn {
namespace resample {

constexpr uint32_t kTile = 256;
constexpr uint32_t kMaxLdsBytes = 64u << 10;
constexpr uint32_t kMaxRatio = 1u << 20;         // L and M
constexpr uint32_t kMaxW = 1u << 16;

static inline uint64_t span_floats(uint32_t L, uint32_t M, uint32_t W) {
    return (uint64_t)(kTile - 1u) * M / L + 2ull * W + 2ull;
}

// bytes of one sample; 0: not a format
static inline uint32_t sample_bytes(int format) {
    switch (format) {
        case RN_PCM_U8: return 1u;
        case RN_PCM_S16LE: return 2u;
        case RN_PCM_S24LE: return 3u;
        case RN_PCM_S32LE: return 4u;
        case RN_PCM_F32LE: return 4u;
        default: return 0u;
    }
}

}  // namespace resample
}  // namespace rn
