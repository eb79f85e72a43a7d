// rn_wgrad_dev.h -- the weight-gradient machine of training, shared by the fused head (k_train_wgrad / k_train_wreduce,
// rn_train_head.hip), the fused torso (k_train_torso_wgrad / k_train_torso_wreduce, rn_train_torso.hip) and the per-MLP
// kernels (k_mlp_wgrad / k_mlp_wreduce, rn_mlp.hip).
//
// A job is dW[o][i] = sum over samples of A[o][s] * B[i][s] with up to 96 features per operand.  One workgroup of 256
// threads = one job x one slice of the 32-sample tiles (part, part + parts, ...).  It stages a tile of both operands
// transposed in LDS ([feature][sample parity][sample / 2], row stride kTS: a lane's 16 k-steps are contiguous), the sample
// index is the k of v_mfma_f32_32x32x2_f32, and the up to 3 x 3 output blocks of 32 x 32 are dealt round-robin to the four
// waves (<= 3 each), whose accumulators stay in registers over all tiles.  Tiles travel global -> registers two strides
// ahead of their use (two register sets, alternating): the HBM latency of a tile that is read exactly once (~3 us) is
// longer than the ~1 us of MFMA work per tile.  Per-workgroup partial sums [96 x 96] go to a workspace; wreduce() adds
// them up, one thread per element, into the nn.Linear layout (wreduce_jobs(): the body of the two fused reduce kernels,
// one launch for all jobs of a step).
//
// How a tile gets from global memory into the staged tile is the operand's business.  An operand type provides
//   Fetched                          the registers one thread holds of a tile in flight
//   kZeroStage                       true: commit() writes only the real features and wants the staged tile zeroed once
//   kMaxBlocks, blocks()             32-row blocks: compile-time bound and actual count (a constant where the type knows it)
//   fetch(f, tile)                   global -> registers
//   commit(t, f, tile, M)            registers -> staged tile t; M = live samples (rows past it stage as zeros)
// The two families: OpT<...> below (layout known at compile time: the fused head, rn_train_head.hip, and the fused torso,
// rn_train_torso.hip, whose enc_x operand is computed with rn_freq_dev.h) and Op<NATIVE> of rn_mlp.hip (run-time native
// tile / row-major matrix).
#pragma once

#include "rn_freq_dev.h"
#include "rn_tile32_dev.h"

namespace rn {
namespace wgrad {

constexpr int kThreads = 256;
constexpr int kTS = 36;                      // LDS row stride of a staged tile
constexpr int kStage = 96 * kTS;             // one operand tile: up to 96 features x 32 samples
constexpr int kLdsFloats = 2 * kStage;       // both operands
constexpr uint32_t kPartial = 96 * 96;       // floats of one workgroup's partial sum, [row][col]

template <typename OpA, typename OpB>
__device__ __forceinline__ void run(const OpA oa, const OpB ob, uint32_t n_tiles, uint32_t M, uint32_t part, uint32_t parts,
                                    float *__restrict__ partial, float *lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 31, h = lane >> 5;
    static_assert(OpA::kMaxBlocks * OpB::kMaxBlocks <= 12, "too many output blocks");
    constexpr int NQ = (OpA::kMaxBlocks * OpB::kMaxBlocks + 3) / 4;
    const int nb = (int)ob.blocks(), n_blocks = (int)oa.blocks() * nb;
    f32x16 acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[q][r] = 0.0f;
    float *ta = lds, *tb = lds + kStage;
    if constexpr (OpA::kZeroStage || OpB::kZeroStage) {   // pad features stay zero
        for (int e = threadIdx.x; e < kLdsFloats; e += kThreads) lds[e] = 0.0f;
        __syncthreads();
    }
    typename OpA::Fetched fa0, fa1;
    typename OpB::Fetched fb0, fb1;
    const uint32_t stride = parts;
    if (part < n_tiles) { oa.fetch(fa0, part); ob.fetch(fb0, part); }
    if (part + stride < n_tiles) { oa.fetch(fa1, part + stride); ob.fetch(fb1, part + stride); }
    if (part < n_tiles) { oa.commit(ta, fa0, part, M); ob.commit(tb, fb0, part, M); }
    __syncthreads();
    auto multiply = [&]() {
        // k-step t of the MFMA = samples 2 t + h of the tile: 16 consecutive floats per lane and operand
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            const int b = wave + 4 * q;   // block q of this wave -> (x, y)
            if (b < n_blocks) {
                const int bx = b / nb, by = b - bx * nb;
                const float4 *pa = reinterpret_cast<const float4 *>(ta + (32 * bx + i) * kTS + h * 16);
                const float4 *pb = reinterpret_cast<const float4 *>(tb + (32 * by + i) * kTS + h * 16);
                float4 av[4], bv[4];
#pragma unroll
                for (int u = 0; u < 4; u++) { av[u] = pa[u]; bv[u] = pb[u]; }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    acc[q] = mfma32(av[u].x, bv[u].x, acc[q]);
                    acc[q] = mfma32(av[u].y, bv[u].y, acc[q]);
                    acc[q] = mfma32(av[u].z, bv[u].z, acc[q]);
                    acc[q] = mfma32(av[u].w, bv[u].w, acc[q]);
                }
            }
        }
    };
    // iteration on tile T (in LDS): register set 0 is free (it was committed) -> fetch T + 2 strides into it; set 1 holds
    // T + 1 stride, committed after the multiply; then the same with the sets swapped
    for (uint32_t tile = part; tile < n_tiles; tile += 2 * stride) {
        if (tile + 2 * stride < n_tiles) { oa.fetch(fa0, tile + 2 * stride); ob.fetch(fb0, tile + 2 * stride); }
        multiply();
        __syncthreads();      // everybody has read this tile
        if (tile + stride < n_tiles) { oa.commit(ta, fa1, tile + stride, M); ob.commit(tb, fb1, tile + stride, M); }
        __syncthreads();
        if (tile + stride >= n_tiles) break;
        if (tile + 3 * stride < n_tiles) { oa.fetch(fa1, tile + 3 * stride); ob.fetch(fb1, tile + 3 * stride); }
        multiply();
        __syncthreads();
        if (tile + 2 * stride < n_tiles) { oa.commit(ta, fa0, tile + 2 * stride, M); ob.commit(tb, fb0, tile + 2 * stride, M); }
        __syncthreads();
    }
    // partial [row][col] of this workgroup: row = 32 x + rowmap(r, h), col = 32 y + i
    float *dst = partial + (size_t)part * kPartial;
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        const int b = wave + 4 * q;
        if (b < n_blocks) {
            const int bx = b / nb, by = b - bx * nb;
#pragma unroll
            for (int r = 0; r < 16; r++) dst[(32 * bx + rowmap(r, h)) * 96 + 32 * by + i] = acc[q][r];
        }
    }
}

// ---- operands whose layout is known at compile time (the fused training kernels) ------------------------------------------------
constexpr int PHI_STD = 0, PHI_ENC = 1, PHI_SH = 2;
template <int PHI>
__device__ __forceinline__ int phi(int q, int h) {   // feature of register q, lane half h of a native tile
    if constexpr (PHI == PHI_STD) return 32 * (q >> 4) + rowmap(q & 15, h);
    else if constexpr (PHI == PHI_ENC) return 4 * (q >> 1) + 2 * h + (q & 1);
    else return 2 * q + h;
}
// An operand = [RM row-major columns | native segment 0 (R0 registers) | native segment 1 (R1 registers) |
//               FREQ: freq(xy * shrink, 10), 42 features computed while the tile is staged | ONES: a column of ones]
template <int RM, int R0, int PHI0, int R1, int PHI1, bool ONES, bool FREQ = false>
struct OpT {
    const float *rm;   // [M_pad, RM]
    const float *s0, *s1;
    const float *xy;   // FREQ: [M, 2]; rows at or past `live` are not read
    float shrink;
    uint32_t live;
    static constexpr int kFreq = 42, kFreq0 = RM + 2 * R0 + 2 * R1;                 // features of freq(., 10) on 2 coordinates
    static constexpr int NF = kFreq0 + (FREQ ? kFreq : 0) + (ONES ? 1 : 0);         // features
    static constexpr int S0 = R0 / 4, S1 = R1 / 4;                                  // registers per thread (4 waves)
    static constexpr int kMaxBlocks = (NF + 31) / 32;
    static constexpr bool kZeroStage = true;                                        // commit() writes the NF real features only
    __device__ __forceinline__ static constexpr uint32_t blocks() { return kMaxBlocks; }
    struct Fetched {
        float v0[S0 > 0 ? S0 : 1], v1[S1 > 0 ? S1 : 1], rm, x0, x1;
    };
    __device__ __forceinline__ void fetch(Fetched &f, uint32_t tile) const {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if constexpr (S0 > 0) {
            const float *src = s0 + (size_t)tile * (R0 * 64);
#pragma unroll
            for (int i = 0; i < S0; i++) f.v0[i] = src[(wave * S0 + i) * 64 + lane];
        }
        if constexpr (S1 > 0) {
            const float *src = s1 + (size_t)tile * (R1 * 64);
#pragma unroll
            for (int i = 0; i < S1; i++) f.v1[i] = src[(wave * S1 + i) * 64 + lane];
        }
        if constexpr (RM > 0) {
            f.rm = 0.0f;
            if (threadIdx.x < 32 * RM) f.rm = rm[(size_t)tile * (32 * RM) + threadIdx.x];
        }
        if constexpr (FREQ) {   // thread t: sample t % 32 of the tile, features t / 32, t / 32 + 8, ...
            const uint32_t row = tile * 32 + (threadIdx.x & 31);
            f.x0 = 0.0f;
            f.x1 = 0.0f;
            if (row < live) { f.x0 = xy[2 * (size_t)row] * shrink; f.x1 = xy[2 * (size_t)row + 1] * shrink; }
        }
    }
    // The native and row-major segments are committed as they were saved, without a test against M: the contract (rows past
    // M stage as zeros) holds for them because their producers keep it.  The backward kernels write exact zeros into every
    // gradient row of a dead sample of the last tile, and the forward kernels compute finite activations for dead samples
    // (from zero inputs), so a dead row contributes 0 x finite.  A producer that leaves such rows unwritten, or writes
    // Inf / NaN into a dead activation row, breaks the weight gradients silently.
    __device__ __forceinline__ void commit(float *t, const Fetched &f, uint32_t tile, uint32_t M) const {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
        const int col = (j & 1) * 16 + (j >> 1);
        if constexpr (S0 > 0) {
#pragma unroll
            for (int i = 0; i < S0; i++) t[(RM + phi<PHI0>(wave * S0 + i, h)) * kTS + col] = f.v0[i];
        }
        if constexpr (S1 > 0) {
#pragma unroll
            for (int i = 0; i < S1; i++) t[(RM + 2 * R0 + phi<PHI1>(wave * S1 + i, h)) * kTS + col] = f.v1[i];
        }
        if constexpr (RM > 0) {
            if (threadIdx.x < 32 * RM) {
                const int s = threadIdx.x / RM, c = threadIdx.x % RM;
                t[c * kTS + (s & 1) * 16 + (s >> 1)] = f.rm;
            }
        }
        if constexpr (FREQ) {   // the forward's arithmetic (rn_freq_dev.h)
            const int s = threadIdx.x & 31, c0 = threadIdx.x >> 5;
            const bool on = tile * 32 + s < M;
            float *dst = t + kFreq0 * kTS + (s & 1) * 16 + (s >> 1);
            for (int c = c0; c < kFreq; c += 8) {
                float v;
                if (c < 2) v = c ? f.x1 : f.x0;
                else {
                    const int q = c - 2;
                    const float a = freq_angle((q & 1) ? f.x1 : f.x0, q >> 2);
                    v = (q & 2) ? freq_cos(a) : freq_sin(a);
                }
                dst[c * kTS] = on ? v : 0.0f;
            }
        }
        if constexpr (ONES) {   // its gradient column is the bias gradient
            if (threadIdx.x >= 64 && threadIdx.x < 96) {
                const int s = threadIdx.x - 64;
                t[(NF - 1) * kTS + (s & 1) * 16 + (s >> 1)] = (tile * 32 + s < M) ? 1.0f : 0.0f;
            }
        }
    }
};

// One job of a reduce launch (wreduce() below): where the sum of a job's partials goes
struct RJob {
    float *out;
    uint32_t rows, cols, ld;      // out[row * ld + col] for row < rows, col < cols
    int32_t bias_col;             // column of the partial that is the bias gradient (-1: none)
    float *bias_out;              // [rows]
};

// Element e = row * 96 + col of a job: the sum of its `parts` partials goes to out[row * ld + col] (row < rows, col < cols),
// or to bias_out[row] when col is bias_col (< 0: the job has none).
__device__ __forceinline__ void wreduce(const float *__restrict__ partial, uint32_t parts, uint32_t e, uint32_t rows, uint32_t cols,
                                        int32_t bias_col, float *out, uint32_t ld, float *bias_out) {
    const uint32_t row = e / 96, col = e % 96;
    const bool bias = bias_col >= 0 && (int32_t)col == bias_col;
    if (row >= rows || (col >= cols && !bias)) return;
    const float *src = partial + row * 96 + col;
    float s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t q = 0;
    for (; q + 8 <= parts; q += 8) {
#pragma unroll
        for (int u = 0; u < 8; u++) s[u] += src[(size_t)(q + u) * kPartial];
    }
    for (; q < parts; q++) s[0] += src[(size_t)q * kPartial];
    const float total = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
    if (bias) bias_out[row] = total;
    else out[row * ld + col] = total;
}

// A reduce launch of JOBS jobs whose partials follow each other in one workspace ([JOBS][parts][kPartial]): grid
// (kPartial / 256, JOBS) x 256 threads.  The fused head (8 jobs) and the fused torso (6) wrap it in a kernel each.
template <int JOBS>
struct RArgs {
    RJob job[JOBS];
    const float *partial;
    uint32_t parts;
};
template <int JOBS>
__device__ __forceinline__ void wreduce_jobs(const RArgs<JOBS> &p) {
    const RJob &job = p.job[blockIdx.y];
    wreduce(p.partial + (size_t)blockIdx.y * p.parts * kPartial, p.parts, blockIdx.x * 256 + threadIdx.x, job.rows, job.cols, job.bias_col,
            job.out, job.ld, job.bias_out);
}

}  // namespace wgrad
}  // namespace rn
