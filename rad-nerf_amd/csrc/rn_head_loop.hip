// rn_head_loop.hip -- the device-resident inference loop of a frame (gfx950): ray setup, march, composite, compaction.
//
// C ABI: include/radnerf_fused.h (rn_head_*, rn_frame_begin).  What is computed: the inference branch of
// nerf/renderer.py:225-262 per frame.  The loop keeps n_alive / step / n_step in device memory (double-buffered state
// words), so a frame is enqueued without a single host read-back; compaction is a stable ballot/mbcnt scatter.  The
// per-sample network between march and composite is rn_fused.hip's kernel, launched through run_fused().
// What happens to one ray (box test, list order, walk, compositor) is rn_ray_dev.h's / rn_dda_dev.h's, shared with the per-operator
// kernels of rn_raymarching.hip; this file owns the loop: its state words, the live list, the compaction and the launches.
#include "rn_fused_dev.h"
#include "rn_ray_dev.h"

namespace rn {

// state words (int32), two banks of 8 selected by (iteration & 1):
//   [0] n_alive  [1] step  [2] n_step  [3] M = n_alive * n_step  [4] active  [5] live-partial workgroups (0: default)
//   [6] live samples listed by the marchers of this iteration (entries of rn_head_t.live_slots); zeroed by the previous
//       iteration's compositor (by rn_head_begin for iteration 0), never by next_state()
// plus stats at [16..]: iterations that did work, live samples, sample slots.
constexpr int kLoopBlock = 256;

__device__ __forceinline__ uint32_t policy_n_step(uint32_t N, uint32_t n_alive) {
    uint32_t n_step = n_alive ? N / n_alive : 1u;   // max(min(N // n_alive, 8), 1)  (renderer.py:249)
    n_step = n_step > 8u ? 8u : n_step;
    return n_step < 1u ? 1u : n_step;
}

__device__ __forceinline__ void next_state(int32_t *st, uint32_t N, uint32_t n_alive, uint32_t step, uint32_t max_steps) {
    const uint32_t n_step = policy_n_step(N, n_alive);
    const bool active = step < max_steps && n_alive > 0;
    st[0] = (int32_t)n_alive;
    st[1] = (int32_t)step;
    st[2] = (int32_t)n_step;
    st[3] = active ? (int32_t)(n_alive * n_step) : 0;  // sample slots of the coming iteration (0: loop is over)
    st[4] = active ? 1 : 0;
    st[5] = 0;  // workgroups that hold live-sample partial sums of the coming iteration; 0 = ceil(n_alive / 256)
}

// Experiment switches (compile-time, off by default) that attribute a marcher's time, in the style of RN_EXP_NO_LOADS: each is a
// mask of marchers -- 1 = k_frame_begin, 2 = the compaction's march (k_head_compact<true>, k_head_step<true>), 4 = k_head_march --
// built without one term.  A build with any of them set renders nothing usable; it is for a profiler run only.
//   -DRN_EXP_LOOP_NO_STORES=mask   the walk without the three stores of a sample
//   -DRN_EXP_LOOP_NO_LIST=mask     without the zero fill of unused deltas rows and the live-list entry loop
//   -DRN_EXP_LOOP_NO_WALK=mask     without the walk: no lattice point is tested, every ray emits nothing
#ifndef RN_EXP_LOOP_NO_STORES
#define RN_EXP_LOOP_NO_STORES 0
#endif
#ifndef RN_EXP_LOOP_NO_LIST
#define RN_EXP_LOOP_NO_LIST 0
#endif
#ifndef RN_EXP_LOOP_NO_WALK
#define RN_EXP_LOOP_NO_WALK 0
#endif
constexpr int kMarcherFrameBegin = 1, kMarcherCompact = 2, kMarcherMarch = 4;
constexpr int exp_of(int marcher) {
    return ((RN_EXP_LOOP_NO_STORES & marcher) ? Dda::kExpNoStores : 0) | ((RN_EXP_LOOP_NO_LIST & marcher) ? Dda::kExpNoFill : 0) |
           ((RN_EXP_LOOP_NO_WALK & marcher) ? Dda::kExpNoWalk : 0);
}

// The marchers' epilogue: every lane holds `emitted` live samples in slots base .. base + emitted - 1.  One atomicAdd per
// workgroup reserves a run of the iteration's live list (its order is arrival order -- irrelevant, every sample is
// independent), a block-wide scan places each lane's entries.  Returns the workgroup's live-sample count.
template <int EXP = 0>
__device__ __forceinline__ uint32_t list_live_slots(uint32_t emitted, uint32_t base, int32_t *live_count,
                                                    int32_t *__restrict__ live_slots, uint32_t *sh /* [kLoopBlock / kWave + 1] */) {
    __syncthreads();  // sh may still be read by the caller's previous phase
    uint32_t total;
    const uint32_t before = block_exclusive_scan<kLoopBlock>(emitted, sh, &total);
    if (live_slots) {
        if (threadIdx.x == 0) sh[kLoopBlock / kWave] = total ? (uint32_t)atomicAdd(live_count, (int32_t)total) : 0u;
        __syncthreads();
        const uint32_t at = sh[kLoopBlock / kWave] + before;
        if constexpr ((EXP & Dda::kExpNoFill) == 0)
            for (uint32_t k = 0; k < emitted; k++) live_slots[at + k] = (int32_t)(base + k);
    }
    return total;
}

// near/far (raymarching.cu:91-145) + loop initialisation (renderer.py:229-237)
__global__ void __launch_bounds__(kLoopBlock)
k_head_begin(const float *__restrict__ rays_o, const float *__restrict__ rays_d, const float *__restrict__ aabb,
             uint32_t N, float min_near, uint32_t max_steps, float *__restrict__ nears, float *__restrict__ fars,
             float *__restrict__ weights_sum, float *__restrict__ depth, float *__restrict__ image,
             int32_t *__restrict__ rays_alive, float *__restrict__ rays_t, int32_t *__restrict__ state,
             uint32_t order_w) {
    const uint32_t n = blockIdx.x * kLoopBlock + threadIdx.x;
    if (n == 0) {
        next_state(state, N, N, 0, max_steps);
        state[6] = 0;
        for (int i = 8; i < 16; i++) state[i] = 0;  // statistics words [16..] accumulate across frames (caller-owned)
        state[RN_HEAD_ST_HIST] = (int32_t)N;
    }
    if (n >= N) return;
    float near, far;
    begin_ray(n, rays_o + (size_t)n * 3, rays_d + (size_t)n * 3, aabb, min_near, nears, fars, rays_t, weights_sum, depth, image, near, far);
    rays_alive[n] = (int32_t)alive_order(n, order_w);
}

// raymarching.cu:827-929 with device-resident n_alive / n_step; every slot of a live ray is written
// (unused slots get deltas = 0), so the sample buffers never need a memset.
__global__ void __launch_bounds__(kLoopBlock)
k_head_march(const int32_t *__restrict__ st, const int32_t *__restrict__ rays_alive, const float *__restrict__ rays_t,
             const float *__restrict__ rays_o, const float *__restrict__ rays_d, float bound, float dt_gamma,
             uint32_t max_steps, uint32_t C, uint32_t H, const uint8_t *__restrict__ grid,
             const float *__restrict__ fars, float *__restrict__ xyzs, float *__restrict__ dirs, float *__restrict__ deltas, int32_t *__restrict__ stats,
             uint32_t *__restrict__ block_live, int32_t *__restrict__ live_count, int32_t *__restrict__ live_slots,
             const int32_t *__restrict__ occ_box, uint32_t N) {
    const uint32_t n = blockIdx.x * kLoopBlock + threadIdx.x;
    const int index = n < N ? rays_alive[n] : 0;   // the list holds N entries: asked for before the state words are in
    if (!st[4]) return;
    const uint32_t n_alive = (uint32_t)st[0], n_step = (uint32_t)st[2];
    uint32_t emitted = 0;
    const uint32_t base = n * n_step;
    if (n < n_alive) {
        Dda s;
        s.init(rays_o + (size_t)index * 3, rays_d + (size_t)index * 3, bound, dt_gamma, max_steps, C, H, grid, fars[index]);
        if (occ_box) s.set_span(occ_box);
        emitted = s.march_slot<true, exp_of(kMarcherMarch), true>(rays_t[index], n_step, base, xyzs, dirs, deltas);  // perturb is off at inference: no noise term (renderer.py:251)
    }
    // live samples of this iteration: listed for the network kernel, and counted -- one partial sum per workgroup, added up by
    // the compaction kernel (a same-address atomic per wavefront for the statistic cost 38 us per frame)
    __shared__ uint32_t sh[kLoopBlock / kWave + 1];
    const uint32_t total = list_live_slots<exp_of(kMarcherMarch)>(emitted, base, live_count, live_slots, sh);
    if (threadIdx.x == 0) block_live[blockIdx.x] = total;
    if (n == 0) { atomicAdd(&stats[RN_HEAD_ST_ITERS], 1); atomicAdd(&stats[RN_HEAD_ST_SLOTS], (int32_t)(n_alive * n_step)); }
}

// Frame prologue in ONE launch: [ray generation (nerf/utils.py:249-333)] + near/far + loop initialisation + the march of
// iteration 0.  Slot n of the alive list is handled by lane n from start to end: it builds (or loads) the ray that the list
// order puts there, intersects it with the box, resets its accumulators and walks it for the first iteration's
// n_step = max(min(N // N, 8), 1) = 1 sample.  Nothing here depends on another lane's ray, so what used to be three
// launches (k_get_rays, k_head_begin, k_head_march) and two [N,3] round trips is one pass.
// state[6] (live-sample count of even iterations) must be zero on entry: the loop's last compaction leaves it zero.
struct RaySource {
    const float *pose;    // [3,4] / [4,4] row-major cam2world, or NULL: rays are given
    float fx, fy, cx, cy;
    uint32_t W;
};

__global__ void __launch_bounds__(kLoopBlock)
k_frame_begin(RaySource rs, float *__restrict__ rays_o, float *__restrict__ rays_d, const float *__restrict__ aabb, uint32_t N,
              float min_near, uint32_t max_steps, float bound, float dt_gamma, uint32_t C, uint32_t H,
              const uint8_t *__restrict__ grid, float *__restrict__ nears, float *__restrict__ fars, float *__restrict__ weights_sum,
              float *__restrict__ depth, float *__restrict__ image, int32_t *__restrict__ rays_alive, float *__restrict__ rays_t,
              int32_t *__restrict__ state, uint32_t order_w, float *__restrict__ xyzs, float *__restrict__ dirs,
              float *__restrict__ deltas, uint32_t *__restrict__ block_live, int32_t *__restrict__ live_slots,
              const int32_t *__restrict__ occ_box) {
    const uint32_t n = blockIdx.x * kLoopBlock + threadIdx.x;
    if (n == 0) {
        next_state(state, N, N, 0, max_steps);
        for (int i = 8; i < 16; i++) state[i] = 0;
        state[RN_HEAD_ST_HIST] = (int32_t)N;
        atomicAdd(&state[RN_HEAD_ST_ITERS], 1);
        atomicAdd(&state[RN_HEAD_ST_SLOTS], (int32_t)N);          // n_alive * n_step = N * 1
    }
    uint32_t emitted = 0;
    if (n < N) {
        const uint32_t ray = alive_order(n, order_w);
        float o[3], d[3];
        if (rs.pose) {
            pinhole_ray(ray, rs.W, rs.fx, rs.fy, rs.cx, rs.cy, rs.pose, o, d);
#pragma unroll
            for (int k = 0; k < 3; k++) { rays_d[(size_t)ray * 3 + k] = d[k]; rays_o[(size_t)ray * 3 + k] = o[k]; }
        } else {
#pragma unroll
            for (int k = 0; k < 3; k++) { o[k] = rays_o[(size_t)ray * 3 + k]; d[k] = rays_d[(size_t)ray * 3 + k]; }
        }
        float near, far;
        begin_ray(ray, o, d, aabb, min_near, nears, fars, rays_t, weights_sum, depth, image, near, far);
        rays_alive[n] = (int32_t)ray;
        // iteration 0 (k_head_march with n_alive = N, n_step = 1): slot n
        Dda s;
        s.init(o, d, bound, dt_gamma, max_steps, C, H, grid, far);
        if (occ_box) s.set_span(occ_box);
        emitted = s.march_slot<true, exp_of(kMarcherFrameBegin), true>(near, 1u, n, xyzs, dirs, deltas);
    }
    __shared__ uint32_t sh[kLoopBlock / kWave + 1];
    const uint32_t total = list_live_slots<exp_of(kMarcherFrameBegin)>(emitted, n, state + 6, live_slots, sh);
    if (threadIdx.x == 0) block_live[blockIdx.x] = total;
}

// raymarching.cu:942-1029 + per-block survivor counts for the compaction that follows.  One chunk = kLoopBlock consecutive
// entries of the alive list; COOP: the counts cross workgroups INSIDE a launch (k_head_step), so they are written with
// agent-scope atomic stores (the per-XCD L2s are not coherent with each other for plain stores).
constexpr uint32_t kTagShift = 10;               // a chunk has <= kLoopBlock = 256 survivors
constexpr uint32_t kTagMask = (1u << 22) - 1u;
constexpr uint32_t kBarrierPolls = 1u << 20;     // ~1 s of polling before a workgroup gives up waiting for a chunk's count

template <bool COOP>
__device__ __forceinline__ void composite_chunk(uint32_t c, uint32_t n_alive, uint32_t n_step, float T_thresh,
                                                int32_t *__restrict__ rays_alive, float *__restrict__ rays_t,
                                                const float *__restrict__ sigmas, const float *__restrict__ rgbs,
                                                const float *__restrict__ deltas, float *__restrict__ weights_sum,
                                                float *__restrict__ depth, float *__restrict__ image,
                                                uint32_t *__restrict__ block_counts, uint32_t *wave_cnt /* LDS [kLoopBlock / kWave] */,
                                                uint32_t tag = 0) {
    const uint32_t n = c * kLoopBlock + threadIdx.x;
    bool survive = false;
    if (n < n_alive)
        survive = composite_ray(n, n_step, T_thresh, rays_alive, rays_t, sigmas, rgbs, deltas, weights_sum, depth, image);
    const unsigned long long mask = __ballot(survive);
    if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = (uint32_t)__popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int w = 0; w < kLoopBlock / kWave; w++) s += wave_cnt[w];
        if constexpr (COOP) {
            // count + launch tag in one word: the word IS the chunk's arrival flag (k_head_step).  The first store of workgroup
            // 0 is a release: its reset of the next live-sample counter must be visible before anybody passes the barrier.
            if (c == 0) __hip_atomic_store(&block_counts[c], (tag << kTagShift) | s, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            else __hip_atomic_store(&block_counts[c], (tag << kTagShift) | s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            block_counts[c] = s;
        }
    }
}

__global__ void __launch_bounds__(kLoopBlock)
k_head_composite(const int32_t *__restrict__ st, float T_thresh, int32_t *__restrict__ rays_alive,
                 float *__restrict__ rays_t, const float *__restrict__ sigmas, const float *__restrict__ rgbs,
                 const float *__restrict__ deltas, float *__restrict__ weights_sum, float *__restrict__ depth,
                 float *__restrict__ image, uint32_t *__restrict__ block_counts, int32_t *__restrict__ st_next) {
    __shared__ uint32_t wave_cnt[kLoopBlock / kWave];
    if (!st[4]) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) st_next[6] = 0;  // the marchers of the next iteration count their live samples here
    const uint32_t n_alive = (uint32_t)st[0], n_step = (uint32_t)st[2];
    if (blockIdx.x * kLoopBlock >= n_alive) return;
    composite_chunk<false>(blockIdx.x, n_alive, n_step, T_thresh, rays_alive, rays_t, sigmas, rgbs, deltas, weights_sum, depth, image,
                           block_counts, wave_cnt);
}

// stable compaction (renderer.py:258) + loop control (renderer.py:242-249, 262) for the next iteration and, with MARCH,
// the next iteration's march as well: every workgroup adds up all survivor counts (<= 1024 words), so it knows the new
// n_alive and n_step, and a surviving ray is marched by the lane that has just computed its slot in the new list.  One
// launch (and one pass over the ray list) less per iteration; the lanes of dead rays idle, which costs nothing here:
// these launches are bound by the length of one ray's walk, not by lane throughput.
struct MarchArgs {
    const float *rays_t, *rays_o, *rays_d, *fars;
    float bound, dt_gamma;
    uint32_t cascade, grid_size;
    const uint8_t *grid;
    float *xyzs, *dirs, *deltas;
    uint32_t *block_live_next;
    int32_t *live_slots;
    const int32_t *occ_box;   // the occupied box (rn_head_t.occ_box) or NULL
};

// What a launch does when the loop is already over (st[4] == 0): carry the state over, close the frame's counters.
__device__ __forceinline__ void loop_idle(const int32_t *__restrict__ st, int32_t *__restrict__ st_next, int32_t *__restrict__ stats,
                                          uint32_t close_frame, uint32_t iter) {
    if (blockIdx.x == 0 && threadIdx.x < 8) st_next[threadIdx.x] = st[threadIdx.x];
    // close_frame (last compaction of a frame's loop): both live-sample counters back to zero for the next frame's
    // prologue; the loop is over, so rn_head_check_done has nothing to flag
    if (close_frame && blockIdx.x == 0 && threadIdx.x == 0) { stats[6] = 0; stats[8 + 6] = 0; }
    if (blockIdx.x == 0 && threadIdx.x == 0 && iter + 1 < 32) stats[RN_HEAD_ST_HIST + iter + 1] = 0;
}

// Chunk c of the n_blocks chunks of the alive list (see k_head_compact).  COOP: the survivor counts were written by other
// workgroups of THIS launch -> agent-scope atomic loads.
template <bool MARCH, bool COOP>
__device__ __forceinline__ void compact_chunk(uint32_t c, uint32_t n_blocks, const int32_t *__restrict__ st, int32_t *__restrict__ st_next,
                                              uint32_t N, uint32_t max_steps, int32_t v_in,
                                              int32_t *__restrict__ rays_out, const uint32_t *__restrict__ block_counts,
                                              const uint32_t *__restrict__ block_live, int32_t *__restrict__ stats, const MarchArgs &m,
                                              uint32_t close_frame, uint32_t iter, uint32_t tag = 0) {
    __shared__ uint32_t red[kLoopBlock / kWave];
    __shared__ uint32_t red_live[kLoopBlock / kWave];
    __shared__ uint32_t red_all[kLoopBlock / kWave];
    __shared__ uint32_t wave_off[kLoopBlock / kWave];
    // Loads that depend on nothing computed here go first: v_in = rays_in[c * kLoopBlock + threadIdx.x], asked for by the caller
    // (the list holds N entries, so it needs no state word; -1 beyond N), and, with MARCH, the ray of a survivor -- their round
    // trips pass under the count summation and its barriers instead of following them.
    float ray_o[3] = {0.0f, 0.0f, 0.0f}, ray_d[3] = {0.0f, 0.0f, 0.0f}, ray_far = 0.0f, ray_t = 0.0f;
    auto load_ray = [&](int32_t v) {
#pragma unroll
        for (int k = 0; k < 3; k++) { ray_o[k] = m.rays_o[(size_t)v * 3 + k]; ray_d[k] = m.rays_d[(size_t)v * 3 + k]; }
        ray_far = m.fars[v];
        ray_t = m.rays_t[v];
    };
    if constexpr (MARCH && !COOP) {   // (k_head_step has no registers to hold a ray across its barrier: it loads where it marches)
        if ((uint32_t)v_in < N) load_ray(v_in);   // an entry past n_alive is a leftover (not even written on a first frame): never an address
    }
    const uint32_t n_alive = (uint32_t)st[0];
    const bool last = c == n_blocks - 1;

    uint32_t part = 0, live = 0, all = 0;
    for (uint32_t b = threadIdx.x; b < n_blocks; b += kLoopBlock) {
        uint32_t cnt;
        if constexpr (COOP) {   // the grid-wide barrier: wait until chunk b's count of THIS launch has arrived
            uint32_t polls = 0;
            cnt = __hip_atomic_load(&block_counts[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            while ((cnt >> kTagShift) != tag) {
                __builtin_amdgcn_s_sleep(1);
                if (++polls > kBarrierPolls) {   // never expected with a cooperative launch; the frame is then not to be used:
                    atomicAdd(&stats[RN_HEAD_ST_STALLED], 1);      // counted, and flagged like a frame whose loop was cut short, so the
                    atomicAdd(&stats[RN_HEAD_ST_UNFINISHED], 1);   // host renders it again instead of consuming pixels built on stale counts
                    break;
                }
                cnt = __hip_atomic_load(&block_counts[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            cnt &= (1u << kTagShift) - 1u;
        } else {
            cnt = block_counts[b];
        }
        all += cnt;
        part += b < c ? cnt : 0u;
    }
    if (last) {  // the last workgroup also adds up the live-sample partial sums of this iteration's march
        const uint32_t n_live = st[5] ? (uint32_t)st[5] : n_blocks;
        for (uint32_t b = threadIdx.x; b < n_live; b += kLoopBlock) live += block_live[b];
    }
    part = wave_sum(part); live = wave_sum(live); all = wave_sum(all);   // three sums behind one barrier
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = part; red_live[threadIdx.x >> 6] = live; red_all[threadIdx.x >> 6] = all; }
    __syncthreads();
    uint32_t offset = 0, n_next = 0;
    for (int w = 0; w < kLoopBlock / kWave; w++) { offset += red[w]; n_next += red_all[w]; }

    const uint32_t n = c * kLoopBlock + threadIdx.x;
    const int32_t v = (n < n_alive) ? v_in : -1;
    const bool keep = v >= 0;
    const unsigned long long mask = __ballot(keep);
    const uint32_t within = ballot_prefix(mask);
    if ((threadIdx.x & 63) == 0) wave_off[threadIdx.x >> 6] = (uint32_t)__popcll(mask);
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) before += wave_off[w];
    const uint32_t slot = offset + before + within;
    if (keep) rays_out[slot] = v;

    const uint32_t step_next = (uint32_t)st[1] + (uint32_t)st[2];
    const uint32_t n_step_next = policy_n_step(N, n_next);
    const bool active_next = step_next < max_steps && n_next > 0;
    if (last && threadIdx.x == 0) {
        next_state(st_next, N, n_next, step_next, max_steps);
        if (iter + 1 < 32) stats[RN_HEAD_ST_HIST + iter + 1] = active_next ? (int32_t)n_next : 0;   // live rays entering iteration iter + 1
        uint32_t sum = 0;
        for (int w = 0; w < kLoopBlock / kWave; w++) sum += red_live[w];
        if (sum) atomicAdd(&stats[RN_HEAD_ST_LIVE], (int32_t)sum);
        if (close_frame) {   // what rn_head_check_done does, folded in: was the loop really over after this iteration?
            if (active_next) atomicAdd(&stats[RN_HEAD_ST_UNFINISHED], 1);
            stats[6] = 0; stats[8 + 6] = 0;   // no marcher runs after the frame's last compaction
        }
        if (MARCH && active_next) {
            st_next[5] = (int32_t)n_blocks;  // the partial sums written below are indexed by THIS launch's chunks
            atomicAdd(&stats[RN_HEAD_ST_ITERS], 1);
            atomicAdd(&stats[RN_HEAD_ST_SLOTS], (int32_t)(n_next * n_step_next));
        }
    }
    if constexpr (MARCH) {
        if (!active_next) return;  // uniform
        uint32_t emitted = 0;
        const uint32_t base = slot * n_step_next;
        if (keep) {
            if constexpr (COOP) load_ray(v);
            Dda s;
            s.init(ray_o, ray_d, m.bound, m.dt_gamma, max_steps, m.cascade, m.grid_size, m.grid, ray_far);
            if (m.occ_box) s.set_span(m.occ_box);
            emitted = s.march_slot<true, exp_of(kMarcherCompact), true>(ray_t, n_step_next, base, m.xyzs, m.dirs, m.deltas);
        }
        __shared__ uint32_t sh[kLoopBlock / kWave + 1];
        const uint32_t total = list_live_slots<exp_of(kMarcherCompact)>(emitted, base, st_next + 6, m.live_slots, sh);
        if (threadIdx.x == 0) m.block_live_next[c] = total;
    }
}

template <bool MARCH>
__global__ void __launch_bounds__(kLoopBlock)
k_head_compact(const int32_t *__restrict__ st, int32_t *__restrict__ st_next, uint32_t N, uint32_t max_steps,
               const int32_t *__restrict__ rays_in, int32_t *__restrict__ rays_out,
               const uint32_t *__restrict__ block_counts, const uint32_t *__restrict__ block_live, int32_t *__restrict__ stats,
               MarchArgs m, uint32_t close_frame, uint32_t iter) {
    const uint32_t n = blockIdx.x * kLoopBlock + threadIdx.x;
    const int32_t v_in = n < N ? rays_in[n] : -1;   // asked for before the state words are in (see compact_chunk)
    if (!st[4]) { loop_idle(st, st_next, stats, close_frame, iter); return; }
    const uint32_t n_blocks = ((uint32_t)st[0] + kLoopBlock - 1) / kLoopBlock;
    if (blockIdx.x >= n_blocks) return;
    compact_chunk<MARCH, false>(blockIdx.x, n_blocks, st, st_next, N, max_steps, v_in, rays_out, block_counts, block_live, stats, m,
                                close_frame, iter);
}

// Compositor + compaction (+ next march) of one loop iteration in ONE launch: what k_head_composite and k_head_compact do,
// with a grid-wide barrier where the kernel boundary was (the compaction needs every chunk's survivor count: the new live
// count decides the next n_step).  At most kStepGrid workgroups take part, each walking chunks b, b + G, ...; with <= 80
// VGPRs and 256 threads six of them fit on a CU, so kStepGrid workgroups are co-resident three times over on this chip --
// launches of up to three streams may overlap (the host falls back to the two-kernel form beyond that).
// The barrier has no counter (512 same-address atomics cost ~25 us here: they execute one after the other at the memory
// side): a chunk's survivor count is stored together with a per-launch tag (state[RN_HEAD_ST_BARRIER], bumped by every
// launch, never reset), and the summation every workgroup does anyway waits for each word to carry this launch's tag.
// Exit condition every wave reaches: the wait is bounded; running into the bound counts in state[RN_HEAD_ST_STALLED]
// (the host treats such a frame as not rendered) and the workgroup carries on.
constexpr uint32_t kStepGrid = 512;

template <bool MARCH>
__global__ void __launch_bounds__(kLoopBlock, 6)
k_head_step(const int32_t *__restrict__ st, int32_t *__restrict__ st_next, uint32_t N, uint32_t max_steps, float T_thresh,
            int32_t *rays_in, int32_t *__restrict__ rays_out, float *rays_t /* = m.rays_t */,
            const float *__restrict__ sigmas, const float *__restrict__ rgbs, const float *deltas /* = m.deltas */,
            float *__restrict__ weights_sum, float *__restrict__ depth, float *__restrict__ image,
            uint32_t *block_counts, const uint32_t *__restrict__ block_live, int32_t *__restrict__ stats,
            MarchArgs m, uint32_t close_frame, uint32_t iter) {
    __shared__ uint32_t wave_cnt[kLoopBlock / kWave];
    if (!st[4]) { loop_idle(st, st_next, stats, close_frame, iter); return; }
    const uint32_t n_alive = (uint32_t)st[0], n_step = (uint32_t)st[2];
    const uint32_t n_chunks = (n_alive + kLoopBlock - 1) / kLoopBlock;
    const uint32_t G = n_chunks < gridDim.x ? n_chunks : gridDim.x;
    if (blockIdx.x >= G) return;
    const uint32_t epoch = (uint32_t)stats[RN_HEAD_ST_BARRIER];   // written by the previous launch of this state's stream
    const uint32_t tag = epoch % kTagMask + 1u;                   // 1 .. 2^22 - 1; never 0: a zeroed scratch block carries no valid tag
    if (blockIdx.x == 0 && threadIdx.x == 0)
        __hip_atomic_store(&st_next[6], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // next iteration's live-sample counter
    for (uint32_t c = blockIdx.x; c < n_chunks; c += G) {
        if (c != blockIdx.x) __syncthreads();  // wave_cnt is read by thread 0 of the previous round
        composite_chunk<true>(c, n_alive, n_step, T_thresh, rays_in, rays_t, sigmas, rgbs, deltas, weights_sum, depth, image, block_counts,
                              wave_cnt, tag);
    }
    for (uint32_t c = blockIdx.x; c < n_chunks; c += G) {
        __syncthreads();  // the reduction arrays of compact_chunk are reused; all of this workgroup's counts are on their way
        const uint32_t n = c * kLoopBlock + threadIdx.x;
        compact_chunk<MARCH, true>(c, n_chunks, st, st_next, N, max_steps, n < N ? rays_in[n] : -1, rays_out, block_counts, block_live, stats, m,
                                   close_frame, iter, tag);
    }
    // every workgroup has read the epoch before it stored its first count, and nobody gets here before all counts are in
    if (blockIdx.x == 0 && threadIdx.x == 0) stats[RN_HEAD_ST_BARRIER] = (int32_t)(epoch + 1u);
}

// Was the loop over after the iterations the caller enqueued?  (`st` = the state bank the NEXT iteration would read.)
__global__ void k_head_check_done(const int32_t *__restrict__ st, int32_t *__restrict__ unfinished) {
    if (threadIdx.x == 0 && st[4]) atomicAdd(unfinished, 1);
}

// Whole-frame step schedule for a shard of the frame (see radnerf_fused.h): same policy as next_state, fed with the
// frame-wide ray and live counts.
__global__ void k_head_reschedule(int32_t *__restrict__ st, uint32_t schedule_N, const int32_t *__restrict__ alive_total) {
    if (threadIdx.x != 0 || !st[4]) return;
    const uint32_t total = (uint32_t)alive_total[0];
    uint32_t n_step = total ? schedule_N / total : 1u;
    n_step = n_step > 8u ? 8u : n_step;
    n_step = n_step < 1u ? 1u : n_step;
    st[2] = (int32_t)n_step;
    st[3] = (int32_t)((uint32_t)st[0] * n_step);
}

}  // namespace rn

using namespace rn;

extern "C" {

static int check_head(const rn_head_t *h) {
    RN_REQUIRE(h, "head: null descriptor");
    RN_REQUIRE(h->rays_o && h->rays_d && h->aabb && h->bitfield && h->nears && h->fars && h->weights_sum && h->depth &&
                   h->image && h->rays_alive_a && h->rays_alive_b && h->rays_t && h->xyzs && h->dirs && h->deltas &&
                   h->sigmas && h->rgbs && h->state && h->block_counts,
               "head: null pointer");
    RN_REQUIRE(h->N >= 1 && h->max_steps >= 1 && h->cascade >= 1 && h->cascade <= 16 && h->grid_size >= 1, "head: bad sizes");
    return RN_OK;
}

int rn_head_begin(const rn_head_t *h, rn_stream_t stream) {
    if (int rc = check_head(h)) return rc;
    const uint32_t order_w = usable_order_w(h->order_w, h->N);
    hipLaunchKernelGGL(k_head_begin, dim3(div_up(h->N, kLoopBlock)), dim3(kLoopBlock), 0, as_stream(stream), h->rays_o,
                       h->rays_d, h->aabb, h->N, h->min_near, h->max_steps, h->nears, h->fars, h->weights_sum, h->depth,
                       h->image, h->rays_alive_a, h->rays_t, h->state, order_w);
    return check_launch("head_begin");
}

int rn_head_iterate_ex(const rn_head_t *h, const rn_grid_t *grid_xyz, const rn_grid_t *grid_amb, const float *packed,
                       const float *bias, uint32_t first_iter, uint32_t n_iters, int mlp_dtype, uint32_t flags, rn_stream_t stream) {
    if (int rc = check_head(h)) return rc;
    RN_REQUIRE(mlp_dtype == RN_F32 || mlp_dtype == RN_F16 || mlp_dtype == RN_F32_SPLIT,
               "head_iterate: mlp_dtype must be RN_F32, RN_F16 or RN_F32_SPLIT");
    RN_REQUIRE(packed && bias && ((uintptr_t)packed & 15u) == 0, "head_iterate: packed/bias");
    if (int rc = check_fused_grid(grid_xyz, 3, "head_iterate(xyz grid)")) return rc;
    if (int rc = check_fused_grid(grid_amb, 2, "head_iterate(ambient grid)")) return rc;
    RN_REQUIRE(!h->dir_term || (((uintptr_t)h->dir_term & 15u) == 0 && h->N <= (1u << 24)),
               "head_iterate: dir_term must be 16-byte aligned and N <= 2^24 with it");
    hipStream_t s = as_stream(stream);
    const dim3 rgrid(div_up(h->N, kLoopBlock)), rblock(kLoopBlock);
    // caller's scratch: survivor counts | live-sample partial sums of even iterations | ... of odd iterations
    const uint32_t nb = div_up(h->N, kLoopBlock) + 1;
    uint32_t *block_live[2] = {h->block_counts + nb, h->block_counts + 2 * nb};
    for (uint32_t it = first_iter; it < first_iter + n_iters; it++) {
        int32_t *st = h->state + (it & 1u) * 8, *st_next = h->state + ((it + 1) & 1u) * 8;
        int32_t *alive = (it & 1u) ? h->rays_alive_b : h->rays_alive_a;
        int32_t *alive_next = (it & 1u) ? h->rays_alive_a : h->rays_alive_b;
        // A call marches its own first iteration; after that the compaction kernel marches the next iteration itself.
        // The last compaction of a call does not, so that a caller may adjust the schedule between calls
        // (rn_head_reschedule) -- enqueueing the loop one iteration per call reproduces the four-kernel sequence.
        if (it == first_iter && !(flags & RN_LOOP_FIRST_MARCHED))
            hipLaunchKernelGGL(k_head_march, rgrid, rblock, 0, s, st, alive, h->rays_t, h->rays_o, h->rays_d, h->bound,
                               h->dt_gamma, h->max_steps, h->cascade, h->grid_size, h->bitfield, h->fars, h->xyzs, h->dirs,
                               h->deltas, h->state, block_live[it & 1u], st + 6, h->live_slots, h->occ_box, h->N);
        // the network runs over the iteration's live list when the caller gave room for one (st[6] entries), else over all
        // st[3] slots, skipping the dead ones by their deltas
        // direction terms: iteration 0 writes each live ray's row, the later ones read theirs (DirTerm, rn_fused_dev.h)
        const DirTerm dt{h->dir_term, st, alive, h->N, it == 0 ? 1u : 0u};
        run_fused(h->xyzs, h->dirs, h->deltas, h->N, h->live_slots ? st + 6 : st + 3, grid_xyz, grid_amb, packed, bias, h->bound,
                  h->sigmas, h->rgbs, nullptr, mlp_dtype, s, h->live_slots, dt);
        const MarchArgs m{h->rays_t, h->rays_o, h->rays_d, h->fars, h->bound, h->dt_gamma, h->cascade, h->grid_size, h->bitfield,
                          h->xyzs, h->dirs, h->deltas, block_live[(it + 1) & 1u], h->live_slots, h->occ_box};
        const bool march_next = it + 1 < first_iter + n_iters;
        const uint32_t close = (!march_next && (flags & RN_LOOP_CLOSE_FRAME)) ? 1u : 0u;
        if (flags & RN_LOOP_COOP) {  // compositor + compaction (+ next march) behind one launch (k_head_step)
            // a COOPERATIVE launch: the runtime places all workgroups of the grid on the device together or refuses the launch
            // (the in-kernel barrier polls counts other workgroups of the same launch publish, so they must be resident)
            const dim3 cgrid(rgrid.x < kStepGrid ? rgrid.x : kStepGrid);
            uint32_t a_N = h->N, a_max = h->max_steps, a_close = march_next ? 0u : close, a_it = it;
            float a_T = h->T_thresh;
            const int32_t *a_st = st;
            int32_t *a_st_next = st_next, *a_alive = alive, *a_alive_next = alive_next, *a_state = h->state;
            float *a_rays_t = h->rays_t, *a_ws = h->weights_sum, *a_depth = h->depth, *a_image = h->image;
            const float *a_sig = h->sigmas, *a_rgb = h->rgbs, *a_deltas = h->deltas;
            uint32_t *a_counts = h->block_counts;
            const uint32_t *a_live = block_live[it & 1u];
            MarchArgs a_m = m;
            void *args[] = {&a_st, &a_st_next, &a_N, &a_max, &a_T, &a_alive, &a_alive_next, &a_rays_t, &a_sig, &a_rgb, &a_deltas, &a_ws,
                            &a_depth, &a_image, &a_counts, &a_live, &a_state, &a_m, &a_close, &a_it};
            const void *fn = march_next ? reinterpret_cast<const void *>(&k_head_step<true>) : reinterpret_cast<const void *>(&k_head_step<false>);
            const hipError_t e = hipLaunchCooperativeKernel(fn, cgrid, rblock, args, 0, s);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                set_error("head_iterate: cooperative launch of the one-launch loop step refused (%s); use the split loop (no RN_LOOP_COOP)",
                          hipGetErrorString(e));
                return RN_ERR_INVALID_ARG;
            }
            continue;
        }
        hipLaunchKernelGGL(k_head_composite, rgrid, rblock, 0, s, st, h->T_thresh, alive, h->rays_t, h->sigmas, h->rgbs,
                           h->deltas, h->weights_sum, h->depth, h->image, h->block_counts, st_next);
        if (march_next)
            hipLaunchKernelGGL(k_head_compact<true>, rgrid, rblock, 0, s, st, st_next, h->N, h->max_steps, alive, alive_next,
                               h->block_counts, block_live[it & 1u], h->state, m, 0u, it);
        else
            hipLaunchKernelGGL(k_head_compact<false>, rgrid, rblock, 0, s, st, st_next, h->N, h->max_steps, alive, alive_next,
                               h->block_counts, block_live[it & 1u], h->state, m, close, it);
    }
    return check_launch("head_iterate");
}

int rn_head_iterate(const rn_head_t *h, const rn_grid_t *grid_xyz, const rn_grid_t *grid_amb, const float *packed,
                    const float *bias, uint32_t first_iter, uint32_t n_iters, int mlp_dtype, rn_stream_t stream) {
    return rn_head_iterate_ex(h, grid_xyz, grid_amb, packed, bias, first_iter, n_iters, mlp_dtype, 0u, stream);
}

int rn_frame_begin(const rn_head_t *h, const float *pose, float fx, float fy, float cx, float cy, uint32_t W, rn_stream_t stream) {
    if (int rc = check_head(h)) return rc;
    RN_REQUIRE(!pose || (fx != 0.0f && fy != 0.0f && W >= 1 && h->N % W == 0), "frame_begin: bad intrinsics / image width");
    const uint32_t order_w = usable_order_w(h->order_w, h->N);
    const uint32_t nb = div_up(h->N, kLoopBlock) + 1;
    const RaySource rs{pose, fx, fy, cx, cy, W ? W : 1u};
    hipLaunchKernelGGL(k_frame_begin, dim3(div_up(h->N, kLoopBlock)), dim3(kLoopBlock), 0, as_stream(stream), rs,
                       const_cast<float *>(h->rays_o), const_cast<float *>(h->rays_d), h->aabb, h->N, h->min_near, h->max_steps, h->bound,
                       h->dt_gamma, h->cascade, h->grid_size, h->bitfield, h->nears, h->fars, h->weights_sum, h->depth, h->image,
                       h->rays_alive_a, h->rays_t, h->state, order_w, h->xyzs, h->dirs, h->deltas, h->block_counts + nb, h->live_slots,
                       h->occ_box);
    return check_launch("frame_begin");
}

int rn_head_check_done(const rn_head_t *h, uint32_t iters_done, rn_stream_t stream) {
    if (int rc = check_head(h)) return rc;
    hipLaunchKernelGGL(k_head_check_done, dim3(1), dim3(64), 0, as_stream(stream), h->state + (iters_done & 1u) * 8,
                       h->state + RN_HEAD_ST_UNFINISHED);
    return check_launch("head_check_done");
}

int rn_head_reschedule(const rn_head_t *h, uint32_t iter_done, uint32_t schedule_N, const int32_t *alive_total,
                       rn_stream_t stream) {
    if (int rc = check_head(h)) return rc;
    RN_REQUIRE(alive_total && schedule_N >= h->N, "head_reschedule: alive_total is null or schedule_N < N");
    hipLaunchKernelGGL(k_head_reschedule, dim3(1), dim3(64), 0, as_stream(stream), h->state + ((iter_done + 1) & 1u) * 8,
                       schedule_N, alive_total);
    return check_launch("head_reschedule");
}

}  // extern "C"
