// rn_grid_scatter_ordered.hip -- the table gradient of rn_grid_scatter.hip summed in ONE fixed order (gfx950; opt-in,
// RN_TRAIN_DETERMINISTIC=1).
//
// C ABI: include/radnerf_train.h (rn_grid_scatter_ordered*).  What is computed: every row of the gradient table starts at +0.0f
// and receives its contributions w * g level by level, samples ascending, corners ascending, with sequential fp32 adds -- the
// order in which the CPU oracle's loops (oracle/orc_grid.c, orc_grid_encode_backward) reach that row.  No float atomic; two calls
// give the same bits, and the result can be held to the oracle bit for bit.  Three passes per job:
//
//  * k_ordered_keys  one item per (level, sample, corner) in that order: key = the global table row, or a sentinel past the last
//                    row for an item that contributes nothing (sample at or past the live count -- its row is not read --, or
//                    with a coordinate outside [0, 1]).
//  * a stable LSD radix sort of (key, item index) over the key's significant bits (rocPRIM radix_sort_pairs, enqueue-only): a
//                    row's items end up adjacent, still ascending in (sample, corner).
//  * k_ordered_sum   the thread that sits on the first item of a row's run walks the run, recomputes every item's w * g exactly
//                    as the oracle writes it and stores the sum with a plain store.  A run longer than a wave is walked by the
//                    whole wave: 64 lanes compute 64 contributions side by side, then every lane adds them in item order (the
//                    adds stay one chain, only the loads and multiplies run in parallel) -- never split into partial sums, which
//                    would change the bits.
// Everything is sized on the host from the row capacity M; the device count only decides which items are live.  The sample
// load, the corner's weight and row, the job description and its checks are the atomic routes' (rn_scatter_dev.h).
#include "rn_fused_dev.h"
#include "rn_scatter_dev.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

namespace rn {
namespace th {

constexpr uint32_t kOrdThreads = 256;

// The kernels take the shared ScatterJob (n_levels = L; the level list is not used) and `sentinel`, the key of an item that
// contributes nothing: it sorts behind every row.

// Lattice position of sample b at `level`: false when a coordinate lies outside [0, 1]
template <uint32_t D>
__device__ __forceinline__ bool ordered_pos(const ScatterJob &j, uint32_t level, uint32_t b, float (&pos)[D], uint32_t (&pos_grid)[D]) {
    float in[D], pos_deriv[D];
    const bool inside = !load_input<D>(j.inputs, b, in);
    lattice_pos<D>(in, j.lc.scale[level], false, 0, pos, pos_deriv, pos_grid);
    return inside;
}

// Pass 1: one thread per (level, sample); its 2^D keys are adjacent items.
template <uint32_t D>
__global__ void __launch_bounds__(kOrdThreads) k_ordered_keys(ScatterJob j, uint32_t sentinel, uint32_t Mcap,
                                                             const int32_t *__restrict__ m_dev, uint32_t *__restrict__ keys) {
    constexpr uint32_t NC = 1u << D;
    const uint32_t M = live_count(Mcap, m_dev);
    const uint32_t t = blockIdx.x * kOrdThreads + threadIdx.x;
    if (t >= j.n_levels * Mcap) return;
    const uint32_t level = t / Mcap, b = t - level * Mcap;
    uint32_t rows[NC];
#pragma unroll
    for (uint32_t c = 0; c < NC; c++) rows[c] = sentinel;
    if (b < M) {
        float pos[D];
        uint32_t pos_grid[D];
        if (ordered_pos<D>(j, level, b, pos, pos_grid)) {
            const uint32_t off = (uint32_t)j.offsets[level];
            const uint32_t hashmap_size = (uint32_t)j.offsets[level + 1] - off;
            const uint32_t resolution = j.lc.resolution[level];
#pragma unroll
            for (uint32_t c = 0; c < NC; c++) {
                uint32_t pgl[D];
                (void)corner<D>(c, pos, pos_grid, pgl);
                rows[c] = off + grid_row<D>(j.gridtype, false, hashmap_size, resolution, pgl);
            }
        }
    }
    uint32_t *dst = keys + (size_t)t * NC;
#pragma unroll
    for (uint32_t c = 0; c < NC; c += 4) *reinterpret_cast<uint4 *>(dst + c) = make_uint4(rows[c], rows[c + 1], rows[c + 2], rows[c + 3]);
}

// w * g of one item, every operation rounded on its own (corner(): orc_grid.c:241-251).  Only called for live items.
template <uint32_t D>
__device__ __forceinline__ float2 ordered_term(const ScatterJob &j, uint32_t Mcap, uint32_t item) {
    constexpr uint32_t NC = 1u << D;
    const uint32_t c = item & (NC - 1u), t = item >> D;
    const uint32_t level = t / Mcap, b = t - level * Mcap;
    float pos[D];
    uint32_t pos_grid[D], pgl[D];
    (void)ordered_pos<D>(j, level, b, pos, pos_grid);
    const float w = corner<D>(c, pos, pos_grid, pgl);
    const float2 g = *reinterpret_cast<const float2 *>(j.grad + ((size_t)level * Mcap + b) * 2);
    return make_float2(w * g.x, w * g.y);
}

// Pass 3: one thread per sorted position.
template <uint32_t D>
__global__ void __launch_bounds__(kOrdThreads) k_ordered_sum(ScatterJob j, uint32_t sentinel, uint32_t Mcap, uint32_t n_items,
                                                            const uint32_t *__restrict__ keys, const uint32_t *__restrict__ items) {
    const uint32_t i = blockIdx.x * kOrdThreads + threadIdx.x;      // n_items < 2^31: no wrap
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t key = sentinel;
    bool head = false;
    if (i < n_items) {
        key = keys[i];
        head = key != sentinel && (i == 0 || keys[i - 1] != key);
    }
    const bool wide = head && i + 64u < n_items && keys[i + 64u] == key;     // a run of more than 64 items
    if (head && !wide) {
        float2 acc = make_float2(0.0f, 0.0f);
        for (uint32_t p = i; p < n_items && p < i + 64u && keys[p] == key; p++) {
            const float2 v = ordered_term<D>(j, Mcap, items[p]);
            acc.x = acc.x + v.x;
            acc.y = acc.y + v.y;
        }
        *reinterpret_cast<float2 *>(j.grad_grid + (size_t)key * 2) = acc;
    }
    // the wave's long runs, one after the other, by all of its lanes
    unsigned long long todo = __ballot(wide);
    while (todo) {
        const int src = __builtin_ctzll(todo);
        todo &= todo - 1ull;
        const uint32_t start = (uint32_t)__shfl((int)i, src, 64), k = (uint32_t)__shfl((int)key, src, 64);
        float2 acc = make_float2(0.0f, 0.0f);
        for (uint32_t base = start;; base += 64u) {
            const uint32_t p = base + lane;
            const bool mine = p < n_items && keys[p] == k;              // sorted: the lanes of the run are a prefix of the wave
            const uint32_t cnt = (uint32_t)__popcll(__ballot(mine));
            float2 v = make_float2(0.0f, 0.0f);
            if (mine) v = ordered_term<D>(j, Mcap, items[p]);
            for (uint32_t q = 0; q < cnt; q++) {                         // one chain of adds, in item order, the same in every lane
                acc.x = acc.x + __shfl(v.x, (int)q, 64);
                acc.y = acc.y + __shfl(v.y, (int)q, 64);
            }
            if (cnt < 64u) break;
        }
        if (lane == (uint32_t)src) *reinterpret_cast<float2 *>(j.grad_grid + (size_t)k * 2) = acc;
    }
}

static inline size_t align256(size_t v) { return (v + 255u) & ~(size_t)255u; }

struct OrderedPlan {
    uint32_t n_items, sentinel, key_bits;
    size_t sort_temp, bytes;      // rocPRIM's temporary storage; the whole workspace of the job
};

// Sizes of one job at capacity M, from host data only.  false: the job is out of range.
static bool ordered_plan(const rn_scatter_job_t &j, uint32_t M, OrderedPlan &p) {
    const rn_grid_t *g = j.grid;
    const uint64_t n = ((uint64_t)g->L * M) << g->D;
    if (n >= (1ull << 31)) return false;
    p.n_items = (uint32_t)n;
    // with a host view of the level sizes the sentinel is the first row past the table and the sort stops at its top bit
    p.sentinel = j.offsets_host ? (uint32_t)j.offsets_host[g->L] : kNoRow;
    p.key_bits = 32;
    if (j.offsets_host) {
        p.key_bits = 1;
        while (p.key_bits < 32 && (p.sentinel >> p.key_bits)) p.key_bits++;
    }
    p.sort_temp = 0;
    uint32_t *none = nullptr;
    if (rocprim::radix_sort_pairs(nullptr, p.sort_temp, none, none, rocprim::counting_iterator<uint32_t>(0), none, (size_t)p.n_items, 0u,
                                  p.key_bits, (hipStream_t) nullptr) != hipSuccess)
        return false;
    // keys | sorted keys | sorted items | rocPRIM's storage
    p.bytes = 3 * align256((size_t)p.n_items * sizeof(uint32_t)) + align256(p.sort_temp) + 256;
    return true;
}

template <uint32_t D>
static int ordered_run(const ScatterJob &oj, const OrderedPlan &p, uint32_t M, const int32_t *m_dev, char *w, hipStream_t s) {
    const size_t arr = align256((size_t)p.n_items * sizeof(uint32_t));
    uint32_t *keys = reinterpret_cast<uint32_t *>(w), *keys_sorted = reinterpret_cast<uint32_t *>(w + arr);
    uint32_t *items_sorted = reinterpret_cast<uint32_t *>(w + 2 * arr);
    void *temp = w + 3 * arr;
    size_t temp_bytes = p.sort_temp;
    hipLaunchKernelGGL(k_ordered_keys<D>, dim3(div_up(oj.n_levels * M, kOrdThreads)), dim3(kOrdThreads), 0, s, oj, p.sentinel, M, m_dev,
                       keys);
    const hipError_t e = rocprim::radix_sort_pairs(temp, temp_bytes, keys, keys_sorted, rocprim::counting_iterator<uint32_t>(0), items_sorted,
                                                   (size_t)p.n_items, 0u, p.key_bits, s);
    RN_REQUIRE(e == hipSuccess, "grid_scatter_ordered: the sort could not be enqueued (%s)", hipGetErrorString(e));
    hipLaunchKernelGGL(k_ordered_sum<D>, dim3(div_up(p.n_items, kOrdThreads)), dim3(kOrdThreads), 0, s, oj, p.sentinel, M, p.n_items,
                       keys_sorted, items_sorted);
    return RN_OK;
}

}  // namespace th
}  // namespace rn

using namespace rn;
using namespace rn::th;

extern "C" {

size_t rn_grid_scatter_ordered_workspace(const rn_scatter_job_t *jobs, uint32_t n_jobs, uint32_t M) {
    if (check_jobs("grid_scatter_ordered", jobs, n_jobs, 8) != RN_OK) return 0;
    size_t need = 256;
    if (M == 0) return need;
    for (uint32_t i = 0; i < n_jobs; i++) {          // the jobs run one after the other on one stream and share the workspace
        OrderedPlan p;
        if (!ordered_plan(jobs[i], M, p)) return 0;
        if (p.bytes > need) need = p.bytes;
    }
    return need;
}

int rn_grid_scatter_ordered(const rn_scatter_job_t *jobs, uint32_t n_jobs, uint32_t M, const int32_t *m_dev, void *workspace,
                            size_t workspace_bytes, rn_stream_t stream) {
    if (M == 0) return RN_OK;
    if (int rc = check_jobs("grid_scatter_ordered", jobs, n_jobs, 8)) return rc;
    OrderedPlan plan[2];
    for (uint32_t i = 0; i < n_jobs; i++) {
        RN_REQUIRE(ordered_plan(jobs[i], M, plan[i]), "grid_scatter_ordered: L * M * 2^D must stay below 2^31 (job %u, M = %u)", i, M);
        RN_REQUIRE(workspace && ((uintptr_t)workspace & 255u) == 0 && workspace_bytes >= plan[i].bytes,
                   "grid_scatter_ordered: workspace too small (%zu bytes, job %u needs %zu) or not 256-byte aligned", workspace_bytes, i,
                   plan[i].bytes);
    }
    hipStream_t s = as_stream(stream);
    for (uint32_t i = 0; i < n_jobs; i++) {
        const rn_scatter_job_t &j = jobs[i];
        ScatterJob oj = make_job(j);
        oj.n_levels = j.grid->L;
        const int rc = j.grid->D == 3 ? ordered_run<3>(oj, plan[i], M, m_dev, static_cast<char *>(workspace), s)
                                      : ordered_run<2>(oj, plan[i], M, m_dev, static_cast<char *>(workspace), s);
        if (rc) return rc;
    }
    return check_launch("grid_scatter_ordered");
}

}  // extern "C"
