// rn_scatter_dev.h -- what the table-gradient scatters of the grid encoder share: the operator's own (rn_grid.hip), the training
// step's atomic routes (rn_grid_scatter.hip) and its ordered route (rn_grid_scatter_ordered.hip).  Each piece is written once here
// because every route must round alike: the ordered route is held to the CPU oracle bit for bit, the atomic ones to "a row with
// one addend IS the addend" (tests/test_gpu_scatter_atomic.py, tests/test_gpu_scatter_ordered.py).
#pragma once

#include "rn_grid_dev.h"

#include "../../include/radnerf_train.h"

namespace rn {

// "no row": the key of a lane / an item that contributes nothing, and the empty slot of the LDS tables
constexpr uint32_t kNoRow = 0xffffffffu;

// GridEncoder.forward's `inputs = (inputs + bound) / (2 * bound)` (gridencoder/grid.py:149) folded into the lookup's coordinate
// load: x -> (x + add) * mul with mul = 1 / (2 * bound) in fp32 -- what the division by a host scalar computes on the device
// in PyTorch -- so the module needs no pass of its own over the coordinates.  on = 0: coordinates are used as given (the scatters
// never pass one).
struct InXform { float add, mul; uint32_t on; };

// The coordinates of sample b; true when one of them lies outside [0, 1]: such a sample contributes nothing (gridencoder.cu:113-117,
// 275-280).
template <uint32_t D>
__device__ __forceinline__ bool load_input(const float *__restrict__ inputs, uint32_t b, float (&in)[D], const InXform xf = InXform{0, 1, 0}) {
    bool oob = false;
#pragma unroll
    for (uint32_t d = 0; d < D; d++) {
        float x = inputs[(size_t)b * D + d];
        if (xf.on) x = (x + xf.add) * xf.mul;
        in[d] = x;
        oob |= (in[d] < 0 || in[d] > 1);
    }
    return oob;
}

// Corner `idx` of the cell that lattice_pos() found: its lattice coordinates (for grid_row) and its interpolation weight, the
// product in the order d = 0, 1, ... -- the reference multiplies the x term first (gridencoder.cu:298-308), and so does the oracle
// (orc_grid.c:241-251): w = ((1 * t0) * t1) * t2, every operation rounded on its own (-ffp-contract=off).
template <uint32_t D>
__device__ __forceinline__ float corner(uint32_t idx, const float (&pos)[D], const uint32_t (&pos_grid)[D], uint32_t (&pgl)[D]) {
    float w = 1;
#pragma unroll
    for (uint32_t d = 0; d < D; d++) {
        const bool hi = (idx >> d) & 1u;
        w *= hi ? pos[d] : 1 - pos[d];
        pgl[d] = pos_grid[d] + (hi ? 1u : 0u);
    }
    return w;
}

// Wave-level pre-reduction of a scatter-add.  Samples arrive ray-ordered, so neighbouring lanes often hit the same table row
// (always on the coarse levels, where a run is most of a ray; on every level of the ambient grid, whose coordinates cluster around
// 0), and plain atomics then serialise on one address -- in L2, or in an LDS table (thousands of inserts into a few dozen slots:
// 600 us per training step on the xyz grid, measured).  Consecutive lanes whose K keys are all equal form a run; a segmented
// inclusive scan (6 shuffle steps, the run heads taken from one ballot) sums the N values of each run into its last lane.  Returns
// true on the lanes that must emit their v.  Waves with few repeats (mostly distinct rows: the scan would not pay) skip it, and
// every lane with a row emits.  key[0] must be kNoRow on lanes that contribute nothing.
template <uint32_t K, uint32_t N>
__device__ __forceinline__ bool sum_runs(const uint32_t (&key)[K], float (&v)[N]) {
    const uint32_t lane = threadIdx.x & 63u;
    bool head = lane == 0;
#pragma unroll
    for (uint32_t k = 0; k < K; k++) {
        const uint32_t prev = (uint32_t)__shfl_up((int)key[k], 1, 64);   // every lane takes part: no shuffle behind a short-circuit ||
        head |= key[k] != prev;
    }
    const unsigned long long heads = __ballot(head);
    const bool valid = key[0] != kNoRow;
    if (__popcll(heads) > 40) return valid;
    // first lane of my run: highest head bit at or below my lane
    const unsigned long long below = heads & ((2ull << lane) - 1ull);
    const uint32_t start = 63u - (uint32_t)__clzll(below);
#pragma unroll
    for (uint32_t off = 1; off < 64; off <<= 1) {
        float up[N];
#pragma unroll
        for (uint32_t c = 0; c < N; c++) up[c] = __shfl_up(v[c], off, 64);
        if (lane >= start + off) {
#pragma unroll
            for (uint32_t c = 0; c < N; c++) v[c] += up[c];
        }
    }
    const bool tail = lane == 63u || ((heads >> (lane + 1)) & 1ull);
    return tail && valid;
}

namespace th {

// One grid's table gradient as the training step's scatter kernels see it: level-major feature gradients [L, M, 2] in, the
// gradient table out.  The atomic routes list the levels a launch covers; the ordered route covers all of them (n_levels = L).
struct ScatterJob {
    const float *grad, *inputs;
    const int32_t *offsets;
    float *grad_grid;
    LevelConsts lc;
    uint32_t gridtype, n_levels;
    uint32_t level_of[kMaxLevels];    // the levels this job covers (blockIdx.y indexes this list)
    uint32_t direct_mask;             // bit i: entry i of level_of goes straight to memory (a hashed level: nothing to merge)
    uint32_t chunks_of[kMaxLevels];   // line-merged levels: chunks of samples a workgroup sums in its LDS table before it flushes
};

static inline ScatterJob make_job(const rn_scatter_job_t &j) {
    ScatterJob s{};
    s.grad = j.grad;
    s.inputs = j.inputs;
    s.offsets = j.grid->offsets;
    s.grad_grid = j.grad_table;
    s.lc = make_level_consts(j.grid->L, j.grid->S, j.grid->H);
    s.gridtype = j.grid->gridtype;
    return s;
}

// What both entry points ask of their jobs.  `who`: the route's name in the error text; `table_align`: 64 bytes where a slot's 16
// floats leave as one line of the gradient table (the atomic routes), 8 where rows are stored as float2 (the ordered one).
static inline int check_jobs(const char *who, const rn_scatter_job_t *jobs, uint32_t n_jobs, uint32_t table_align) {
    RN_REQUIRE(jobs && (n_jobs == 1 || n_jobs == 2), "%s: one or two jobs", who);
    for (uint32_t i = 0; i < n_jobs; i++) {
        const rn_scatter_job_t &j = jobs[i];
        RN_REQUIRE(j.grad && j.inputs && j.grid && j.grid->offsets && j.grad_table, "%s: null pointer in job %u", who, i);
        RN_REQUIRE((j.grid->D == 2 || j.grid->D == 3) && j.grid->L >= 1 && j.grid->L <= kMaxLevels, "%s: D must be 2 or 3, L <= 32", who);
        RN_REQUIRE(((uintptr_t)j.grad_table & (table_align - 1u)) == 0 && ((uintptr_t)j.grad & 7u) == 0,
                   "%s: grad_table must be %u-byte, grad 8-byte aligned", who, table_align);
    }
    return RN_OK;
}

}  // namespace th
}  // namespace rn
