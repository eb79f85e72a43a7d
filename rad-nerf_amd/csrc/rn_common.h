// rn_common.h -- shared host/device helpers for libradnerf_hip.so (gfx950 only).
//
// Built with -ffp-contract=off: float expressions that feed integer results
// (DDA cell index, lattice position) round exactly as written, which makes
// them bit-identical to the CPU oracle.  Fused multiply-adds are spelled out
// with __builtin_fmaf where a kernel wants them.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include "../../include/radnerf_hip.h"

namespace rn {

constexpr int kWave = 64;  // CDNA wavefront width

void set_error(const char *fmt, ...);
int check_launch(const char *what);
// compute units of the current device (256 where it cannot be asked); read once per process
int num_cus();
// tuning knob from the environment: the variable's value (`def` when unset) clamped to 1 .. max
uint32_t env_uint_clamped(const char *name, uint32_t def, uint32_t max);
// HIP-event timing of the dominant kernel (rn_prof_enable / rn_prof_collect)
bool prof_enabled();
void prof_pair(hipEvent_t *start, hipEvent_t *stop);
// launch with the timing events of prof_pair() attached to the dispatch (plain launch when timing is off)
#define RN_LAUNCH_TIMED(kernel, grid, block, stream, ...)                                      \
    do {                                                                                       \
        hipEvent_t rn_e0_, rn_e1_;                                                             \
        ::rn::prof_pair(&rn_e0_, &rn_e1_);                                                     \
        hipExtLaunchKernelGGL(kernel, grid, block, 0, stream, rn_e0_, rn_e1_, 0, __VA_ARGS__); \
    } while (0)

static inline uint32_t div_up(uint32_t a, uint32_t b) { return (a + b - 1) / b; }
// workgroups of a launch whose waves walk n_tiles tiles with a grid stride: one per `waves` tiles, at most `per_cu` on each CU
static inline uint32_t tile_blocks(uint32_t n_tiles, uint32_t waves, uint32_t per_cu) {
    const uint32_t blocks = div_up(n_tiles, waves), cap = per_cu * (uint32_t)num_cus();
    return blocks < cap ? blocks : cap;
}
static inline hipStream_t as_stream(rn_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

#define RN_REQUIRE(cond, ...)                 \
    do {                                      \
        if (!(cond)) {                        \
            ::rn::set_error(__VA_ARGS__);     \
            return RN_ERR_INVALID_ARG;        \
        }                                     \
    } while (0)

// ---- device helpers ------------------------------------------------------------------

__device__ __forceinline__ float clampf(float x, float lo, float hi) { return fminf(hi, fmaxf(lo, x)); }

// Morton code of a 10-bit-per-axis cell (raymarching.cu:56-71).
__device__ __forceinline__ uint32_t expand_bits(uint32_t v) {
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}
__device__ __forceinline__ uint32_t morton3D(uint32_t x, uint32_t y, uint32_t z) {
    return expand_bits(x) | (expand_bits(y) << 1) | (expand_bits(z) << 2);
}
// The same for coordinates < 256 (every occupancy grid of this repo: H = 128): expand_bits()' first step only moves bits 8 and 9.
__device__ __forceinline__ uint32_t expand_bits8(uint32_t v) {
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}
__device__ __forceinline__ uint32_t morton3D_8(uint32_t x, uint32_t y, uint32_t z) {
    return expand_bits8(x) | (expand_bits8(y) << 1) | (expand_bits8(z) << 2);
}
// raymarching.cu:73-81
__device__ __forceinline__ uint32_t morton3D_invert(uint32_t x) {
    x = x & 0x49249249u;
    x = (x | (x >> 2)) & 0xc30c30c3u;
    x = (x | (x >> 4)) & 0x0f00f00fu;
    x = (x | (x >> 8)) & 0xff0000ffu;
    x = (x | (x >> 16)) & 0x0000ffffu;
    return x;
}

// Lane index inside the wavefront and wave-level exclusive prefix of a ballot.
__device__ __forceinline__ uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
__device__ __forceinline__ uint32_t ballot_prefix(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// uniform in [0,1) with 24 random bits from a 32-bit mix (public-domain "lowbias32" finaliser applied twice): the jitter of the
// occupancy refresh and of the one-launch training marcher, identical on the CPU oracle
__host__ __device__ inline uint32_t mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
__host__ __device__ inline float hash_u01(uint32_t seed, uint32_t idx) {
    return (float)(mix32(mix32(idx) ^ seed) >> 8) * (1.0f / 16777216.0f);
}

// A size the host passes as an upper bound and the device may know better: min(n_arg, *n_dev) (n_dev may be NULL).
__device__ __forceinline__ uint32_t clamp_count(uint32_t n_arg, const int32_t *__restrict__ n_dev) {
    if (!n_dev) return n_arg;
    const uint32_t d = (uint32_t)*n_dev;
    return d < n_arg ? d : n_arg;
}

// ---- workgroup primitives (THREADS = blockDim.x, a multiple of the wave; lds: THREADS / kWave words) ------------------
// Lane 0 of every wave gets the wave's sum.
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}
// Sum over the workgroup, returned to every thread; the waves' sums are added in wave order.  Two barriers: the second one
// frees `lds` for the next call, and between them every thread has passed a barrier after whatever it wrote to LDS before.
template <typename T, int THREADS>
__device__ __forceinline__ T block_sum(T v, T *lds) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    T s = 0;
    for (int w = 0; w < THREADS / kWave; w++) s += lds[w];
    __syncthreads();
    return s;
}
// The same sum for thread 0 alone (the others get 0) behind ONE barrier: the epilogue of a kernel that publishes one number.
template <typename T, int THREADS>
__device__ __forceinline__ T block_sum_first(T v, T *lds) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    T s = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < THREADS / kWave; w++) s += lds[w];
    return s;
}
// Exclusive prefix sum over the workgroup in thread order (wave scan by __shfl_up, wave totals in LDS); *total = the sum.
// One barrier, after the write: the caller keeps `lds` free of readers of an earlier phase.
template <int THREADS>
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t *lds, uint32_t *total = nullptr) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(incl, d, 64);
        if (lane >= d) incl += t;
    }
    if (lane == 63) lds[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < THREADS / kWave; w++) {
        all += lds[w];
        before += w < wave ? lds[w] : 0u;
    }
    if (total) *total = all;
    return before + incl - v;
}

}  // namespace rn
