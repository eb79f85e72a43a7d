// rn_grid_scatter.hip -- the table gradient of the multiresolution grids in the training step (gfx950).
//
// C ABI: include/radnerf_train.h (rn_grid_scatter_*).  What is computed: the embedding gradient of gridencoder.cu:342-368
// from level-major feature gradients [L, M, 2], as rn_train_head.hip's backward kernel leaves them.
//
//  * k_grid_scatter: float atomics run at the memory side, one request per touched 64-B line per instruction
//    (MI355X_MICROARCH.md, "Global float atomics"), so a workgroup first sums its 128 samples x 2^D corners of one level in
//    an LDS table keyed by the 64-B LINE of the gradient table (8 rows x 2 channels = 16 floats per slot; the two
//    x-neighbours of a corner pair share a line 7 times out of 8, on hashed levels too: the x prime is 1) and then issues the
//    16 floats of a slot from 16 adjacent lanes -- one request per touched line instead of one per row.
//  * k_grid_bin / k_grid_scatter_buckets: the opt-in binned form for large hashed levels (below).
// What an addend is (sample load, corner weight and row), the wave-level run sum, the job description and its checks are shared
// with the operator's and the ordered route: rn_scatter_dev.h.
// The kernels keep namespace rn::th, the one they had inside rn_train_head.hip: profiles and tools match on their names.
#include "rn_fused_dev.h"
#include "rn_scatter_dev.h"

#include <stdlib.h>

namespace rn {
namespace th {

// ---- table gradient -------------------------------------------------------------------------------------------------------
#ifndef RN_SC_SLOTS
#define RN_SC_SLOTS 512
#endif
// 256 threads = (256 / 2^(D-1)) samples x 2^(D-1) x-pairs of corners; 512 slots of 16 floats + key = 35 KB of LDS: four
// workgroups per CU, so one workgroup's burst of atomics (its flush) runs under the others' loads and LDS inserts
constexpr uint32_t kScThreads = 256, kScSlots = RN_SC_SLOTS, kScProbes = 24;
constexpr uint32_t kScSlotBits = kScSlots == 1024 ? 10 : (kScSlots == 512 ? 9 : 8);
static_assert((1u << kScSlotBits) == kScSlots, "slot count must be 256, 512 or 1024");

// One level of one chunk of samples through the LDS line merge (the non-binned levels).
template <uint32_t D>
__device__ __forceinline__ void scatter_lines(const ScatterJob &j, uint32_t Mcap, uint32_t M, uint32_t *keys, float *vals, uint32_t *occupied,
                                              uint32_t block_x) {
    constexpr uint32_t P = 1u << (D - 1);            // x-pairs of corners per sample
    constexpr uint32_t kScSamples = kScThreads / P;  // lanes 0 .. S-1: pair 0 of the S samples, lanes S .. 2S-1: pair 1, ...
    if (blockIdx.y >= j.n_levels) return;
    const uint32_t level = j.level_of[blockIdx.y];
    const bool direct = (j.direct_mask >> blockIdx.y) & 1u;   // workgroup-uniform
    // small levels (few lines in all): a workgroup sums several chunks of samples in its table before it flushes -- the more
    // samples share a table, the more of their rows coincide (the ambient coordinates of a step cluster in a few cells)
    const uint32_t chunks = direct ? 1u : j.chunks_of[blockIdx.y];
    if (block_x * chunks * kScSamples >= M) return;
    if (!direct) {
        for (uint32_t i = threadIdx.x; i < kScSlots; i += kScThreads) keys[i] = kNoRow;
        for (uint32_t i = threadIdx.x; i < kScSlots * 16; i += kScThreads) vals[i] = 0.0f;
        if (threadIdx.x == 0) *occupied = 0u;
        __syncthreads();
    }
    const uint32_t off = (uint32_t)j.offsets[level];
    const uint32_t hashmap_size = (uint32_t)j.offsets[level + 1] - off;
    float *gg = j.grad_grid + (size_t)off * 2;
    const uint32_t q = threadIdx.x / kScSamples;      // this thread's x-pair: bits of q = the y (, z) corner
    const uint32_t resolution = j.lc.resolution[level];
  for (uint32_t chunk = 0; chunk < chunks; chunk++) {
    const uint32_t b = (block_x * chunks + chunk) * kScSamples + (threadIdx.x & (kScSamples - 1u));
    float in[D] = {};
    const bool live = b < M && !load_input<D>(j.inputs, b, in);     // rows at or past the live count are not read
    float pos[D], pos_deriv[D];
    uint32_t pos_grid[D];
    lattice_pos<D>(in, j.lc.scale[level], false, 0, pos, pos_deriv, pos_grid);
    float2 g = make_float2(0.0f, 0.0f);
    if (live) g = *reinterpret_cast<const float2 *>(j.grad + ((size_t)level * Mcap + b) * 2);
    {
        uint32_t pgl0[D], pgl1[D];                    // the x-pair: corners 2 q and 2 q + 1
        const float w0 = corner<D>(2u * q, pos, pos_grid, pgl0), w1 = corner<D>(2u * q + 1u, pos, pos_grid, pgl1);
        uint32_t row0 = kNoRow, row1 = kNoRow;
        if (live) {
            row0 = grid_row<D>(j.gridtype, false, hashmap_size, resolution, pgl0);
            row1 = grid_row<D>(j.gridtype, false, hashmap_size, resolution, pgl1);
        }
        float v[4] = {w0 * g.x, w0 * g.y, w1 * g.x, w1 * g.y};
        if (direct) {
            // A hashed level: the workgroup's samples never touch a line twice, so an LDS merge would spend ~3.6 clocks per lane
            // and float on LDS atomics to remove nothing.  The four floats of an x-pair (two rows that share a 64-B line 7 times out
            // of 8) leave from four ADJACENT lanes of one instruction -- one memory-side request per pair: instruction k serves the
            // pairs of lanes 16 k .. 16 k + 15, lane l carrying float (l & 3) of pair 16 k + (l >> 2).
            const uint32_t lane = threadIdx.x & 63u, f = lane & 3u;
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) {
                const int src = (int)(16u * k + (lane >> 2));
                const uint32_t r0 = (uint32_t)__shfl((int)row0, src, 64), r1 = (uint32_t)__shfl((int)row1, src, 64);
                const float a0 = __shfl(v[0], src, 64), a1 = __shfl(v[1], src, 64), a2 = __shfl(v[2], src, 64), a3 = __shfl(v[3], src, 64);
                const uint32_t row = f < 2u ? r0 : r1;
                const float val = f == 0u ? a0 : (f == 1u ? a1 : (f == 2u ? a2 : a3));
                if (row != kNoRow && val != 0.0f) atomicAdd(gg + (size_t)row * 2 + (f & 1u), val);
            }
            return;
        }
        const uint32_t rows[2] = {row0, row1};        // a run = both destination rows equal
        if (sum_runs(rows, v)) {
#pragma unroll
            for (int e = 0; e < 2; e++) {
                const uint32_t line = rows[e] >> 3, sub = rows[e] & 7u;
                uint32_t slot = (line * 2654435761u) >> (32u - kScSlotBits);
                bool placed = false;
                for (uint32_t probe = 0; probe < kScProbes; probe++) {
                    const uint32_t prev = atomicCAS(&keys[slot], kNoRow, line);
                    if (prev == kNoRow) atomicAdd(occupied, 1u);
                    if (prev == kNoRow || prev == line) { placed = true; break; }
                    slot = (slot + 1u) & (kScSlots - 1u);
                }
                if (placed) {
                    atomicAdd(&vals[slot * 16 + sub * 2], v[2 * e]);
                    atomicAdd(&vals[slot * 16 + sub * 2 + 1], v[2 * e + 1]);
                } else {   // table full around this line (never with 2-D grids): straight to memory
                    atomicAdd(gg + (size_t)rows[e] * 2, v[2 * e]);
                    atomicAdd(gg + (size_t)rows[e] * 2 + 1, v[2 * e + 1]);
                }
            }
        }
    }
    // flush when the table is filling up (spread-out samples: every chunk; clustered ones: rarely) or after the last chunk.
    // 16 adjacent lanes = the 16 floats of one 64-B line of the gradient table: one memory-side request per touched line
    __syncthreads();
    const bool last = chunk + 1 == chunks || (block_x * chunks + chunk + 1) * kScSamples >= M;
    if (last || *occupied > kScSlots / 2 - kScSlots / 8) {
        for (uint32_t i = threadIdx.x; i < kScSlots * 16; i += kScThreads) {
            const uint32_t line = keys[i >> 4];
            if (line != kNoRow) {
                const float v = vals[i];
                if (v != 0.0f) atomicAdd(gg + (size_t)line * 16 + (i & 15u), v);
                if (!last) {                                    // leave an empty table for the next chunk
                    vals[i] = 0.0f;
                    if ((i & 15u) == 15u) keys[i >> 4] = kNoRow;   // the 16 lanes of the slot have read the key above
                }
            }
        }
        if (last) return;
        __syncthreads();
        if (threadIdx.x == 0) *occupied = 0u;
        __syncthreads();
    }
  }
}


// One launch for the levels of up to two grids that are not binned (the 3-D grid's and the 2-D grid's)
template <uint32_t D0, uint32_t D1>
__global__ void __launch_bounds__(kScThreads) k_grid_scatter(ScatterJob j0, ScatterJob j1, uint32_t n_jobs, uint32_t Mcap,
                                                             const int32_t *__restrict__ m_dev) {
    __shared__ uint32_t keys[kScSlots];
    __shared__ __attribute__((aligned(16))) float vals[kScSlots * 16];
    const uint32_t M = live_count(Mcap, m_dev);
    // two jobs: their workgroups ALTERNATE along x, so that the two grids' work is resident together -- one grid's levels are bound
    // by memory-side atomic requests, the other's by LDS atomics
    __shared__ uint32_t occupied;
    if (n_jobs == 1) scatter_lines<D0>(j0, Mcap, M, keys, vals, &occupied, blockIdx.x);
    else if ((blockIdx.x & 1u) == 0) scatter_lines<D0>(j0, Mcap, M, keys, vals, &occupied, blockIdx.x >> 1);
    else scatter_lines<D1>(j1, Mcap, M, keys, vals, &occupied, blockIdx.x >> 1);
}

// Binned levels.  A level whose gradient table is much larger than what one workgroup's samples touch (the hashed levels of the
// T = 2^19 table: 65 536 lines each, touched ~5 times per launch, never twice by the same workgroup) gains nothing from a
// per-workgroup merge: every (sample, corner) is a memory-side atomic request of its own line.  Those levels are summed by TABLE
// REGION instead: pass A (k_grid_bin) appends (row, w g0, w g1) entries to the bucket that owns the row -- a bucket = 2^shift
// consecutive rows of one level -- and pass B (k_grid_scatter_buckets) has one workgroup per bucket add the bucket's entries in
// LDS and update the region with plain coalesced loads and stores: no global float atomic at all on those levels.  A workgroup
// of pass A reserves room in the buckets with one returning atomic per bucket (LDS histogram of its 256 samples x 2^D corners).
constexpr uint32_t kMaxBucketsPerLevel = 128;
struct BinPlan {
    uint32_t n_levels, level_of[kMaxLevels];   // the binned levels
    uint32_t bucket0[kMaxLevels];     // first bucket of level_of[i]
    uint32_t n_buckets[kMaxLevels];
    uint32_t shift, cap;              // rows per bucket = 1 << shift; entries a bucket has room for
    uint32_t *cursor;                 // [total buckets] entries appended (zero before pass A; pass B leaves it zero)
    uint32_t *e_row;                  // [total buckets][cap] level-local row
    float2 *e_val;                    // [total buckets][cap]
    // Entries that find their bucket full go to ONE spill list with room for every entry of a launch (it cannot overflow); each
    // pass-B workgroup picks its own out of it.  Hashed rows load the buckets evenly, so the list stays empty unless many samples
    // coincide -- correctness does not depend on the bucket size, only speed does.
    uint32_t *spill_count;            // [2]: entries spilled | pass-B workgroups that have read it (the last one resets both)
    uint32_t *spill_key;              // [spill capacity] bucket << 16 | bucket-local row (rows per bucket <= 2^13)
    float2 *spill_val;
};
constexpr uint32_t kBinThreads = 256;

template <uint32_t D>
__global__ void __launch_bounds__(kBinThreads) k_grid_bin(ScatterJob j, uint32_t Mcap, const int32_t *__restrict__ m_dev, BinPlan bp) {
    constexpr uint32_t NC = 1u << D;
    __shared__ uint32_t hist[kMaxBucketsPerLevel], base[kMaxBucketsPerLevel];
    const uint32_t M = live_count(Mcap, m_dev);
    if (blockIdx.x * kBinThreads >= M) return;
    const uint32_t li = blockIdx.y, level = bp.level_of[li];
    if (threadIdx.x < kMaxBucketsPerLevel) hist[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t off = (uint32_t)j.offsets[level];
    const uint32_t hashmap_size = (uint32_t)j.offsets[level + 1] - off;
    const uint32_t b = blockIdx.x * kBinThreads + threadIdx.x;      // one sample per thread, all 2^D corners
    float in[D] = {};
    const bool live = b < M && !load_input<D>(j.inputs, b, in);
    float pos[D], pos_deriv[D];
    uint32_t pos_grid[D];
    lattice_pos<D>(in, j.lc.scale[level], false, 0, pos, pos_deriv, pos_grid);
    float2 g = make_float2(0.0f, 0.0f);
    if (live) g = *reinterpret_cast<const float2 *>(j.grad + ((size_t)level * Mcap + b) * 2);
    const uint32_t resolution = j.lc.resolution[level];
    uint32_t rows[NC], rank[NC];
    float w[NC];
#pragma unroll
    for (uint32_t idx = 0; idx < NC; idx++) {
        uint32_t pgl[D];
        w[idx] = corner<D>(idx, pos, pos_grid, pgl);
        rows[idx] = live ? grid_row<D>(j.gridtype, false, hashmap_size, resolution, pgl) : 0u;
        rank[idx] = live ? atomicAdd(&hist[rows[idx] >> bp.shift], 1u) : 0u;
    }
    __syncthreads();
    if (threadIdx.x < bp.n_buckets[li]) {
        const uint32_t n = hist[threadIdx.x];
        base[threadIdx.x] = n ? atomicAdd(&bp.cursor[bp.bucket0[li] + threadIdx.x], n) : 0u;
    }
    __syncthreads();
    if (!live) return;
    uint32_t full = 0;                                  // corners whose bucket had no room left (normally none)
#pragma unroll
    for (uint32_t idx = 0; idx < NC; idx++) {
        const uint32_t b_ = rows[idx] >> bp.shift, at = base[b_] + rank[idx];
        if (at < bp.cap) {
            const size_t slot = (size_t)(bp.bucket0[li] + b_) * bp.cap + at;
            bp.e_row[slot] = rows[idx];
            bp.e_val[slot] = make_float2(w[idx] * g.x, w[idx] * g.y);
        } else {
            full |= 1u << idx;
        }
    }
    if (full) {                                         // the spill list (sized for every entry of the launch)
#pragma unroll
        for (uint32_t idx = 0; idx < NC; idx++) {
            if (full & (1u << idx)) {
                const uint32_t sp = atomicAdd(&bp.spill_count[0], 1u);
                bp.spill_key[sp] = ((bp.bucket0[li] + (rows[idx] >> bp.shift)) << 16) | (rows[idx] & ((1u << bp.shift) - 1u));
                bp.spill_val[sp] = make_float2(w[idx] * g.x, w[idx] * g.y);
            }
        }
    }
}

// Pass B: one workgroup per bucket.  acc[rows of the bucket][2] in LDS (32 KB for 4096 rows), the bucket's entries (and its share
// of the spill list, normally empty) added with LDS atomics from all lanes, then the region WRITTEN with plain 16-byte stores:
// every row of a binned level is written by exactly one workgroup, so those levels need neither a memset nor a global atomic.
constexpr uint32_t kBkThreads = 512;
__global__ void __launch_bounds__(kBkThreads) k_grid_scatter_buckets(const int32_t *__restrict__ offsets, float *__restrict__ grad_grid,
                                                                     BinPlan bp, uint32_t total_buckets) {
    extern __shared__ __attribute__((aligned(16))) float acc[];
    __shared__ uint32_t n_sh, spill_sh;
    const uint32_t b = blockIdx.x;
    if (b >= total_buckets) return;
    uint32_t li = 0;
    for (uint32_t i = 0; i < bp.n_levels; i++)
        if (b >= bp.bucket0[i] && b < bp.bucket0[i] + bp.n_buckets[i]) li = i;
    const uint32_t level = bp.level_of[li];
    const uint32_t rows_pb = 1u << bp.shift, local = b - bp.bucket0[li];
    const uint32_t off = (uint32_t)offsets[level], rows_level = (uint32_t)offsets[level + 1] - off;
    const uint32_t row_first = local << bp.shift;
    const uint32_t n_rows = rows_level - row_first < rows_pb ? rows_level - row_first : rows_pb;
    if (threadIdx.x == 0) {
        const uint32_t n = bp.cursor[b];
        n_sh = n < bp.cap ? n : bp.cap;
        bp.cursor[b] = 0u;                     // ready for the next launch of pass A
        spill_sh = __hip_atomic_load(&bp.spill_count[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    for (uint32_t i = threadIdx.x; i < rows_pb * 2; i += kBkThreads) acc[i] = 0.0f;
    __syncthreads();
    const uint32_t n = n_sh, n_spill = spill_sh;
    const uint32_t *er = bp.e_row + (size_t)b * bp.cap;
    const float2 *ev = bp.e_val + (size_t)b * bp.cap;
    // eight entries per thread in flight: the loads of a batch are issued together, then added (a load-add-load-add chain would
    // pay the memory latency once per entry)
    for (uint32_t i0 = 0; i0 < n; i0 += kBkThreads * 8) {
        uint32_t r[8];
        float2 v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const uint32_t i = i0 + u * kBkThreads + threadIdx.x;
            const uint32_t ic = i < n ? i : n - 1u;
            r[u] = er[ic] & (rows_pb - 1u);
            v[u] = ev[ic];
            if (i >= n) v[u] = make_float2(0.0f, 0.0f);
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            if (v[u].x != 0.0f) atomicAdd(&acc[2 * r[u]], v[u].x);
            if (v[u].y != 0.0f) atomicAdd(&acc[2 * r[u] + 1], v[u].y);
        }
    }
    for (uint32_t i = threadIdx.x; i < n_spill; i += kBkThreads) {     // normally n_spill == 0
        const uint32_t key = bp.spill_key[i];
        if ((key >> 16) == b) {
            const float2 v = bp.spill_val[i];
            atomicAdd(&acc[2 * (key & 0xffffu)], v.x);
            atomicAdd(&acc[2 * (key & 0xffffu) + 1], v.y);
        }
    }
    __syncthreads();
    float4 *dst = reinterpret_cast<float4 *>(grad_grid + ((size_t)off + row_first) * 2);   // rows are 8 B, regions start on 64-B lines
    const float4 *src = reinterpret_cast<const float4 *>(acc);
    for (uint32_t i = threadIdx.x; i < n_rows / 2; i += kBkThreads) dst[i] = src[i];
    // the last workgroup to have read the spill list empties it for the next launch
    if (threadIdx.x == 0) {
        const uint32_t done = atomicAdd(&bp.spill_count[1], 1u) + 1u;
        if (done == total_buckets) {
            __hip_atomic_store(&bp.spill_count[0], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&bp.spill_count[1], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// Which levels are binned: the HASHED ones with at least kMinBuckets buckets of 2^shift rows.  A hash spreads the rows evenly
// over the buckets whatever the samples' positions, so a bucket's load is known in advance (2x the mean + slack is never
// reached) and pass B has hundreds of equal workgroups.  Dense and tiled levels keep the per-workgroup line merge: their rows
// follow the samples' positions (the ambient coordinates of a call cluster in a few cells), which is where neighbouring samples
// share lines and where a fixed bucket size would overflow.
constexpr uint32_t kMinBuckets = 16;
static uint32_t bucket_shift() {
    static uint32_t sh = 0;
    if (!sh) {
        const char *e = getenv("RN_SCATTER_BUCKET_SHIFT");
        const long v = e ? atol(e) : 12;           // 4096 rows = 32 KB of LDS per bucket: four pass-B workgroups per CU
        sh = (uint32_t)(v < 10 ? 10 : (v > 13 ? 13 : v));
    }
    return sh;
}
static uint32_t plan_bins(const rn_grid_t *grid, const int32_t *offsets_host, uint32_t M, BinPlan &bp, bool *binned /* [L] */) {
    bp = BinPlan{};
    bp.shift = bucket_shift();
    const LevelConsts lc = make_level_consts(grid->L, grid->S, grid->H);
    uint32_t total = 0, min_b = kMaxBucketsPerLevel;
    for (uint32_t l = 0; l < grid->L; l++) {
        const uint32_t rows = (uint32_t)(offsets_host[l + 1] - offsets_host[l]);
        const bool hashed = level_is_hashed(grid->D, lc.resolution[l], rows, grid->gridtype);
        const uint32_t nb = (rows + (1u << bp.shift) - 1u) >> bp.shift;
        const bool bin = hashed && nb >= kMinBuckets && nb <= kMaxBucketsPerLevel;
        if (binned) binned[l] = bin;
        if (bin) {
            bp.level_of[bp.n_levels] = l;
            bp.bucket0[bp.n_levels] = total;
            bp.n_buckets[bp.n_levels] = nb;
            bp.n_levels++;
            total += nb;
            if (nb < min_b) min_b = nb;
        }
    }
    bp.cap = total ? (uint32_t)(2u * (((uint64_t)M << grid->D) / min_b) + 2048u) : 0u;   // 2 x the mean load of a bucket + slack
    return total;
}
// The bin workspace of a plan with `total` buckets at row capacity M, as byte offsets: cursors (zeroed once by the caller; pass B
// leaves them zero) and the two spill counters at 0 | bucket values | spill values | bucket rows | spill keys.  The spill list has
// room for every entry of a launch.
struct BinLayout { size_t e_val, spill_val, e_row, spill_key, bytes; };
static BinLayout bin_layout(uint32_t M, const rn_grid_t *grid, const BinPlan &bp, uint32_t total) {
    const size_t entries = (size_t)total * bp.cap, spill = ((size_t)M << grid->D) * bp.n_levels;
    BinLayout w;
    w.e_val = ((size_t)(total + 2) * sizeof(uint32_t) + 255u) & ~(size_t)255u;
    w.spill_val = w.e_val + entries * sizeof(float2);
    w.e_row = w.spill_val + spill * sizeof(float2);
    w.spill_key = w.e_row + entries * sizeof(uint32_t);
    w.bytes = w.spill_key + spill * sizeof(uint32_t) + 256;
    return w;
}
static bool scatter_direct_enabled() {
    static int on = -1;
    if (on < 0) { const char *e = getenv("RN_SCATTER_DIRECT"); on = e ? atoi(e) : 1; }
    return on != 0;
}
static uint32_t scatter_chunks() {
    static int n = 0;
    if (!n) { const char *e = getenv("RN_SCATTER_CHUNKS"); n = e ? atoi(e) : 8; if (n < 1) n = 1; if (n > 16) n = 16; }
    return (uint32_t)n;
}
template <uint32_t D0>
static void launch_lines(uint32_t D1, dim3 g, hipStream_t s, const ScatterJob &a, const ScatterJob &b, uint32_t n_jobs, uint32_t M,
                         const int32_t *m_dev) {
    if (D1 == 3) hipLaunchKernelGGL((k_grid_scatter<D0, 3>), g, dim3(kScThreads), 0, s, a, b, n_jobs, M, m_dev);
    else hipLaunchKernelGGL((k_grid_scatter<D0, 2>), g, dim3(kScThreads), 0, s, a, b, n_jobs, M, m_dev);
}

}  // namespace th
}  // namespace rn

using namespace rn;
using namespace rn::th;

extern "C" {

size_t rn_grid_scatter_workspace(uint32_t M, const rn_grid_t *grid, const int32_t *offsets_host) {
    if (!grid || !offsets_host || grid->L > kMaxLevels) return 0;
    BinPlan bp;
    const uint32_t total = plan_bins(grid, offsets_host, M, bp, nullptr);
    return total ? bin_layout(M, grid, bp, total).bytes : 256;
}

uint32_t rn_grid_scatter_binned_levels(const rn_grid_t *grid, const int32_t *offsets_host) {
    if (!grid || !offsets_host || grid->L > kMaxLevels) return 0;
    BinPlan bp;
    bool binned[kMaxLevels] = {};
    (void)plan_bins(grid, offsets_host, 1, bp, binned);
    uint32_t mask = 0;
    for (uint32_t l = 0; l < grid->L; l++) mask |= binned[l] ? (1u << l) : 0u;
    return mask;
}

int rn_grid_scatter_jobs(const rn_scatter_job_t *jobs, uint32_t n_jobs, uint32_t M, const int32_t *m_dev, void *workspace,
                         size_t workspace_bytes, rn_stream_t stream) {
    if (M == 0) return RN_OK;
    if (int rc = check_jobs("grid_scatter_jobs", jobs, n_jobs, 64)) return rc;
    hipStream_t s = as_stream(stream);
    ScatterJob sj[2] = {make_job(jobs[0]), n_jobs == 2 ? make_job(jobs[1]) : ScatterJob{}};
    // job 0 may have binned levels (needs the host copy of its offsets and the workspace)
    bool binned[kMaxLevels] = {};
    BinPlan bp{};
    uint32_t total = 0;
    if (jobs[0].offsets_host && workspace && workspace_bytes > 256) {
        total = plan_bins(jobs[0].grid, jobs[0].offsets_host, M, bp, binned);
        if (total) {
            const BinLayout at = bin_layout(M, jobs[0].grid, bp, total);
            RN_REQUIRE(((uintptr_t)workspace & 255u) == 0 && workspace_bytes >= at.bytes,
                       "grid_scatter_jobs: workspace too small / not 256-byte aligned");
            char *w = static_cast<char *>(workspace);
            bp.cursor = reinterpret_cast<uint32_t *>(w);
            bp.spill_count = bp.cursor + total;
            bp.e_val = reinterpret_cast<float2 *>(w + at.e_val);
            bp.spill_val = reinterpret_cast<float2 *>(w + at.spill_val);
            bp.e_row = reinterpret_cast<uint32_t *>(w + at.e_row);
            bp.spill_key = reinterpret_cast<uint32_t *>(w + at.spill_key);
        }
    }
    uint32_t max_levels = 0, max_blocks = 0;
    for (uint32_t i = 0; i < n_jobs; i++) {
        const rn_grid_t *gr = jobs[i].grid;
        const LevelConsts lc = make_level_consts(gr->L, gr->S, gr->H);
        for (uint32_t l = 0; l < gr->L; l++) {
            if (i == 0 && total && binned[l]) continue;
            // hashed (gridencoder.cu:66-84) AND large (>= 2^17 rows: a workgroup's 64 samples x 8 corners land on distinct
            // lines): straight to memory.  Needs a host view of the level sizes: jobs[i].offsets_host (else: line merge)
            bool direct = false;
            if (jobs[i].offsets_host && scatter_direct_enabled()) {
                const uint32_t rows = (uint32_t)(jobs[i].offsets_host[l + 1] - jobs[i].offsets_host[l]);
                direct = level_is_hashed(gr->D, lc.resolution[l], rows, gr->gridtype) && rows >= (1u << 17);
            }
            if (direct) sj[i].direct_mask |= 1u << sj[i].n_levels;
            uint32_t chunks = 1;
            if (!direct && jobs[i].offsets_host) {
                const uint32_t rows = (uint32_t)(jobs[i].offsets_host[l + 1] - jobs[i].offsets_host[l]);
                chunks = rows <= (1u << 16) ? scatter_chunks() : 1u;
            }
            sj[i].chunks_of[sj[i].n_levels] = chunks;
            sj[i].level_of[sj[i].n_levels++] = l;
        }
        if (sj[i].n_levels > max_levels) max_levels = sj[i].n_levels;
        const uint32_t blocks = div_up(M, kScThreads >> (jobs[i].grid->D - 1));
        if (blocks > max_blocks) max_blocks = blocks;
    }
    if (total) {
        const dim3 gb(div_up(M, kBinThreads), bp.n_levels);
        if (jobs[0].grid->D == 3) hipLaunchKernelGGL(k_grid_bin<3>, gb, dim3(kBinThreads), 0, s, sj[0], M, m_dev, bp);
        else hipLaunchKernelGGL(k_grid_bin<2>, gb, dim3(kBinThreads), 0, s, sj[0], M, m_dev, bp);
        const size_t shm = (size_t)2 * sizeof(float) << bp.shift;
        if (shm > 64 * 1024)
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k_grid_scatter_buckets), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
        hipLaunchKernelGGL(k_grid_scatter_buckets, dim3(total), dim3(kBkThreads), shm, s, jobs[0].grid->offsets, jobs[0].grad_table, bp, total);
    }
    if (max_levels) {
        const dim3 g(n_jobs == 2 ? 2 * max_blocks : max_blocks, max_levels);
        const uint32_t D1 = n_jobs == 2 ? jobs[1].grid->D : 2u;
        if (jobs[0].grid->D == 3) launch_lines<3>(D1, g, s, sj[0], sj[1], n_jobs, M, m_dev);
        else launch_lines<2>(D1, g, s, sj[0], sj[1], n_jobs, M, m_dev);
    }
    return check_launch("grid_scatter_jobs");
}

int rn_grid_scatter_binned(const float *grad, const float *inputs, uint32_t M, const int32_t *m_dev, const rn_grid_t *grid,
                           const int32_t *offsets_host, float *grad_table, void *workspace, size_t workspace_bytes, rn_stream_t stream) {
    RN_REQUIRE(offsets_host && workspace, "grid_scatter_binned: null pointer");
    const rn_scatter_job_t j{grad, inputs, grid, offsets_host, grad_table};
    return rn_grid_scatter_jobs(&j, 1, M, m_dev, workspace, workspace_bytes, stream);
}

int rn_grid_scatter_lbc(const float *grad, const float *inputs, uint32_t M, const int32_t *m_dev, const rn_grid_t *grid,
                        float *grad_table, rn_stream_t stream) {
    const rn_scatter_job_t j{grad, inputs, grid, nullptr, grad_table};
    return rn_grid_scatter_jobs(&j, 1, M, m_dev, nullptr, 0, stream);
}

}  // extern "C"
