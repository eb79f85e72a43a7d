// rn_mlp.hip -- forward, backward-data and weight-gradient kernels of the path's per-sample MLPs for TRAINING (gfx950).
//
// What is computed: nerf/network.py:69-88 (`MLP`: bias-free nn.Linear stack, ReLU between layers, width 64) and its
// autograd, as the training step of nerf/utils.py:718-806 runs it on ~60 k samples per step for ambient_net (96 -> 64 ->
// 64 -> 2), sigma_net (65 -> 64 -> 64 -> 65) and color_net (84 -> 64 -> 3).  Stock PyTorch needs per layer a GEMM, a ReLU,
// a ReLU-backward, two more GEMMs (one of them a 60 k-long reduction into a 64 x 96 result) and the copies between them:
// ~150 launches per step for 10 GFLOP.  Here an MLP is three launches:
//
//   k_mlp_fwd    one wave = 32 samples; v_mfma_f32_32x32x2_f32 with the sample on the lane and the output row on the
//                register index (rn_tile32_dev.h), so a layer's accumulators ARE the next layer's B operand; the
//                post-ReLU hidden activations are saved in that native layout (coalesced 256-B rows per register).
//   k_mlp_bwd    the same machine run backwards: dX = W^T dY is a forward layer with the transposed weight image; ReLU
//                masks come from the saved activations; the pre-activation gradients dZ are saved in the native layout.
//   k_mlp_wgrad  dW = dZ X^T for every layer of the MLP in ONE launch, on the weight-gradient machine of rn_wgrad_dev.h
//                (shared with rn_train_head.hip); k_mlp_wreduce adds its per-workgroup partial sums up into the nn.Linear
//                [out, in] layout.
//
// The narrow output rows (ambient 2, sigma 1, rgb 3) are VALU dot products over the accumulator registers, as in the
// inference kernel.  fp32 throughout (exact products, fp32 accumulation): results equal torch's up to summation order.
#include "rn_wgrad_dev.h"

#include "../../include/radnerf_fused.h"

namespace rn {
namespace mlp {

constexpr int kThreads = wgrad::kThreads, kWaves = kThreads / kWave;
constexpr int kStepT = 256;  // floats per MFMA step of the input-gradient layer: [2 h][32 j][4 row tiles (3 used)]
constexpr int kTileFloats = 2048;  // native tile: [2 rt][16 r][64 lanes]

// ---- weight images ---------------------------------------------------------------------------------------------------
// forward:    L0 [in_pad / 2 steps] | L1 [32 steps] (3 layers) | last, wide rows [32 steps] (out >= 64) | last, narrow rows
//             [NN][2 h][32]  -- MFMA layers as [step][h][j][rt] = W[32 rt + j][k(step, h)]
// transposed: last wide^T [32 steps] | L1^T [32 steps] | L0^T [32 steps][2 h][32 j][4 rt] (rows = input features)
struct Dims {
    uint32_t in_dim, in_pad, out_dim, n_layers, nn, wide;   // nn = narrow rows (out_dim % 64 or out_dim), wide = out_dim >= 64
    uint32_t ld0;                                           // row stride of w0 (>= in_dim: the MLP may read a column block of a wider nn.Linear)
    __host__ __device__ uint32_t s0() const { return in_pad / 2; }
    __host__ __device__ uint32_t off_l1() const { return s0() * kStep; }
    __host__ __device__ uint32_t off_lw() const { return off_l1() + (n_layers == 3 ? 32u * kStep : 0u); }
    __host__ __device__ uint32_t off_ln() const { return off_lw() + (wide ? 32u * kStep : 0u); }
    __host__ __device__ uint32_t fwd_floats() const { return off_ln() + nn * 64u; }
    __host__ __device__ uint32_t off_tw() const { return 0; }
    __host__ __device__ uint32_t off_t1() const { return wide ? 32u * kStep : 0u; }
    __host__ __device__ uint32_t off_t0() const { return off_t1() + (n_layers == 3 ? 32u * kStep : 0u); }
    __host__ __device__ uint32_t bwd_floats() const { return off_t0() + 32u * kStepT + nn * 64u; }   // + a copy of the narrow rows
    __host__ __device__ uint32_t off_tn() const { return off_t0() + 32u * kStepT; }
    __host__ __device__ uint32_t rt_in() const { return (in_pad + 31u) / 32u; }
};

static bool make_dims(uint32_t in_dim, uint32_t out_dim, uint32_t n_layers, Dims &d, uint32_t ld0 = 0) {
    d.in_dim = in_dim;
    d.ld0 = ld0 ? ld0 : in_dim;
    d.in_pad = (in_dim + 3u) & ~3u;
    d.out_dim = out_dim;
    d.n_layers = n_layers;
    d.wide = out_dim >= 64 ? 1u : 0u;
    d.nn = d.wide ? out_dim - 64u : out_dim;
    return in_dim >= 1 && d.in_pad <= 96 && (n_layers == 2 || n_layers == 3) && d.nn <= 4 && out_dim >= 1 && out_dim <= 68;
}

__global__ void __launch_bounds__(256) k_mlp_pack(const float *__restrict__ w0, const float *__restrict__ w1,
                                                  const float *__restrict__ wl, Dims d, float *__restrict__ image) {
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    const uint32_t nf = d.fwd_floats(), nb = d.bwd_floats();
    if (e >= nf + nb) return;
    float v = 0.0f;
    if (e < nf) {
        if (e < d.off_ln()) {
            const uint32_t base = e < d.off_l1() ? 0u : (e < d.off_lw() ? d.off_l1() : d.off_lw());
            const uint32_t q = e - base, s = q / kStep, rem = q % kStep, h = rem / 64, j = (rem % 64) / 2, rt = rem % 2;
            const uint32_t row = 32 * rt + j;
            if (e < d.off_l1()) {                                  // L0: k = 4 (s / 2) + 2 h + (s & 1)
                const uint32_t k = 4 * (s >> 1) + 2 * h + (s & 1);
                v = k < d.in_dim ? w0[row * d.ld0 + k] : 0.0f;
            } else if (e < d.off_lw()) {                           // L1: k = kmap
                v = w1[row * 64 + kmap((int)s, (int)h)];
            } else {                                               // last layer, wide rows nn .. nn + 63
                v = wl[(d.nn + row) * 64 + kmap((int)s, (int)h)];
            }
        } else {                                                   // narrow rows [o][h][q]
            const uint32_t q0 = e - d.off_ln(), o = q0 / 64, h = (q0 % 64) / 32, q = q0 % 32;
            v = wl[o * 64 + 32 * (q >> 4) + rowmap((int)(q & 15), (int)h)];
        }
    } else {
        const uint32_t t = e - nf;
        if (t < d.off_t0()) {                                      // (last wide)^T or L1^T: V[row][k] = W[k][row]
            const bool is_w = d.wide && t < d.off_t1();
            const uint32_t q = t - (is_w ? 0u : d.off_t1()), s = q / kStep, rem = q % kStep, h = rem / 64, j = (rem % 64) / 2, rt = rem % 2;
            const uint32_t row = 32 * rt + j, k = (uint32_t)kmap((int)s, (int)h);
            v = is_w ? wl[(d.nn + k) * 64 + row] : w1[k * 64 + row];
        } else if (t < d.off_tn()) {                               // L0^T: rows = input features (in_pad <= 96 -> 3 row tiles of 4)
            const uint32_t q = t - d.off_t0(), s = q / kStepT, rem = q % kStepT, h = rem / 128, j = (rem % 128) / 4, rt = rem % 4;
            const uint32_t row = 32 * rt + j, k = (uint32_t)kmap((int)s, (int)h);
            v = row < d.in_dim ? w0[k * d.ld0 + row] : 0.0f;
        } else {                                                   // narrow rows again (the backward kernel stages only this image)
            const uint32_t q0 = t - d.off_tn(), o = q0 / 64, h = (q0 % 64) / 32, q = q0 % 32;
            v = wl[o * 64 + 32 * (q >> 4) + rowmap((int)(q & 15), (int)h)];
        }
    }
    image[e] = v;
}

struct FwdArgs {
    const float *x;        // [M, in_pad] row-major
    uint32_t M;
    const float *image;    // forward image
    Dims d;
    float *out;            // [M, out_dim]
    float *h0, *h1;        // native tiles [n_tiles][2048]; h1 only with 3 layers
    const float *bias0;    // [64] added to the first layer's pre-activation (nullable): the per-call constant input columns
};

template <int NN, bool WIDE, bool HID2>
__global__ void __launch_bounds__(kThreads) k_mlp_fwd(FwdArgs p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const Dims d = p.d;
    const uint32_t nf = d.fwd_floats();
    for (uint32_t i = threadIdx.x; i < nf / 4; i += kThreads) reinterpret_cast<float4 *>(lds)[i] = reinterpret_cast<const float4 *>(p.image)[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
    const int lane_off = h * 64 + j * 2;
    const uint32_t n_tiles = (p.M + 31u) >> 5;
    for (uint32_t tile = blockIdx.x * kWaves + wave; tile < n_tiles; tile += gridDim.x * kWaves) {
        const uint32_t sample = tile * 32 + j;
        const bool live = sample < p.M;
        Acc32 a, b;
        if (p.bias0) {
#pragma unroll
            for (int rt = 0; rt < 2; rt++)
#pragma unroll
                for (int r = 0; r < 16; r++) a.v[rt][r] = p.bias0[32 * rt + rowmap(r, h)];
        } else {
            acc_zero(a);
        }
        {
            const float *row = p.x + (size_t)sample * d.in_pad + 2 * h;
            const uint32_t nq = d.in_pad / 4;
            for (uint32_t q = 0; q < nq; q++) {
                float2 f = make_float2(0.0f, 0.0f);
                if (live) f = *reinterpret_cast<const float2 *>(row + 4 * q);
                step32(a, lds, 2 * q, lane_off, f.x);
                step32(a, lds, 2 * q + 1, lane_off, f.y);
            }
        }
#pragma unroll
        for (int rt = 0; rt < 2; rt++)
#pragma unroll
            for (int r = 0; r < 16; r++) a.v[rt][r] = fmaxf(a.v[rt][r], 0.0f);
        tile_store(p.h0 + (size_t)tile * kTileFloats, a, lane);
        if constexpr (HID2) {
            acc_zero(b);
            layer_from_acc(b, a, lds + d.off_l1(), lane_off);
#pragma unroll
            for (int rt = 0; rt < 2; rt++)
#pragma unroll
                for (int r = 0; r < 16; r++) a.v[rt][r] = fmaxf(b.v[rt][r], 0.0f);
            tile_store(p.h1 + (size_t)tile * kTileFloats, a, lane);
        }
        // `a` = input of the last layer
        float *orow = p.out + (size_t)sample * d.out_dim;
#pragma unroll
        for (int o = 0; o < NN; o++) {   // the narrow rows; one valu_out per row keeps store o ahead of row o + 1 (valu_out<NN>: up to 40 more VGPRs)
            float s[1];
            valu_out<1>(a, lds + d.off_ln() + o * 64, h, s);
            if (live && h == 0) orow[o] = s[0];
        }
        if constexpr (WIDE) {
            acc_zero(b);
            layer_from_acc(b, a, lds + d.off_lw(), lane_off);
            if (live) {
#pragma unroll
                for (int rt = 0; rt < 2; rt++)
#pragma unroll
                    for (int r = 0; r < 16; r++) orow[NN + 32 * rt + rowmap(r, h)] = b.v[rt][r];
            }
        }
    }
}

struct BwdArgs {
    const float *grad_out;  // [M, out_dim]
    uint32_t M;
    const float *image;     // transposed image (image + fwd_floats)
    Dims d;
    const float *h0, *h1;
    float *grad_x;          // [M, in_pad]
    float *dz0, *dz1;       // native tiles; dz1 only with 3 layers
};

template <int NN, bool WIDE, bool HID2>
__global__ void __launch_bounds__(kThreads) k_mlp_bwd(BwdArgs p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const Dims d = p.d;
    const uint32_t nb = d.bwd_floats();
    for (uint32_t i = threadIdx.x; i < nb / 4; i += kThreads) reinterpret_cast<float4 *>(lds)[i] = reinterpret_cast<const float4 *>(p.image)[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
    const int lane_off = h * 64 + j * 2;
    const uint32_t n_tiles = (p.M + 31u) >> 5;
    const uint32_t rt_in = d.rt_in();
    for (uint32_t tile = blockIdx.x * kWaves + wave; tile < n_tiles; tile += gridDim.x * kWaves) {
        const uint32_t sample = tile * 32 + j;
        const bool live = sample < p.M;
        const float *grow = p.grad_out + (size_t)sample * d.out_dim;
        Acc32 g, w;
        acc_zero(g);
        if constexpr (WIDE) {   // dH = Ww^T dWide
            acc_zero(w);
            if (live) {
#pragma unroll
                for (int rt = 0; rt < 2; rt++)
#pragma unroll
                    for (int r = 0; r < 16; r++) w.v[rt][r] = grow[NN + 32 * rt + rowmap(r, h)];
            }
            layer_from_acc(g, w, lds + d.off_tw(), lane_off);
        }
        if constexpr (NN > 0) {   // + Wn^T g_narrow
            float go[NN];
#pragma unroll
            for (int o = 0; o < NN; o++) go[o] = live ? grow[o] : 0.0f;
            valu_out_T<NN>(g, lds + d.off_tn(), h, go);
        }
        relu_mask(g, (HID2 ? p.h1 : p.h0) + (size_t)tile * kTileFloats, lane);   // ReLU of the last hidden layer
        if constexpr (HID2) {
            tile_store(p.dz1 + (size_t)tile * kTileFloats, g, lane);
            acc_zero(w);
            layer_from_acc(w, g, lds + d.off_t1(), lane_off);
            relu_mask(w, p.h0 + (size_t)tile * kTileFloats, lane);
            g = w;
        }
        tile_store(p.dz0 + (size_t)tile * kTileFloats, g, lane);
        // dX = W0^T dZ0: up to three row tiles of input features
        f32x16 x0, x1, x2;
#pragma unroll
        for (int r = 0; r < 16; r++) { x0[r] = 0.0f; x1[r] = 0.0f; x2[r] = 0.0f; }
        const float *t0 = lds + d.off_t0() + h * 128 + j * 4;
#pragma unroll
        for (int s = 0; s < 32; s++) {
            const float4 ww = *reinterpret_cast<const float4 *>(t0 + s * kStepT);
            const float bb = g.v[s >> 4][s & 15];
            x0 = mfma32(ww.x, bb, x0);
            if (rt_in > 1) x1 = mfma32(ww.y, bb, x1);
            if (rt_in > 2) x2 = mfma32(ww.z, bb, x2);
        }
        if (live) {
            float *xr = p.grad_x + (size_t)sample * d.in_pad;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint32_t c = 8 * q + 4 * h;
                if (c < d.in_pad) *reinterpret_cast<float4 *>(xr + c) = make_float4(x0[4 * q], x0[4 * q + 1], x0[4 * q + 2], x0[4 * q + 3]);
                if (32 + c < d.in_pad) *reinterpret_cast<float4 *>(xr + 32 + c) = make_float4(x1[4 * q], x1[4 * q + 1], x1[4 * q + 2], x1[4 * q + 3]);
                if (64 + c < d.in_pad) *reinterpret_cast<float4 *>(xr + 64 + c) = make_float4(x2[4 * q], x2[4 * q + 1], x2[4 * q + 2], x2[4 * q + 3]);
            }
        }
    }
}

// ---- weight gradients -------------------------------------------------------------------------------------------------
// A job: dW[o][i] = sum over samples of A[o][s] * B[i][s]; an operand is either a native tile buffer (64 features) or a
// row-major [M, ld] matrix (features col0 .. col0 + rows - 1).
struct Operand {
    const float *p;
    uint32_t native, ld, rows;  // rows: real feature count (<= 96)
    uint32_t ones;              // row-major only: one more feature that is 1 for every sample (its gradient column is the bias gradient)
};
struct WJob {
    Operand a, b;
    float *partial;             // [parts][wgrad::kPartial], this job's slice of the workspace
    float *out;                 // [a.rows, out_ld] nn.Linear layout
    uint32_t out_ld, out_cols;  // columns written (= b real features)
    float *out_bias;            // [a.rows]: the column of b's `ones` feature (nullable)
};
constexpr int kMaxJobs = 3;
struct WArgs {
    WJob job[kMaxJobs];
    uint32_t n_jobs, M, parts;  // parts: workgroups per job
};
using wgrad::kTS;

// The two operand kinds, for the pipeline of rn_wgrad_dev.h: fetch() global -> registers, commit() registers -> staged tile.
constexpr int kFetch = 12;   // 96 features x 32 samples / 256 threads
template <bool NATIVE>
struct Op {
    const Operand &op;
    uint32_t M;
    struct Fetched {
        float v[kFetch];
    };
    static constexpr int kMaxBlocks = 3;
    static constexpr bool kZeroStage = false;   // a native tile has no pad features, the row-major commit() writes its pad zeros
    __device__ __forceinline__ uint32_t blocks() const { return (op.rows + op.ones + 31u) / 32u; }
    __device__ __forceinline__ void fetch(Fetched &f, uint32_t tile) const {
        if constexpr (NATIVE) {
            const float *src = op.p + (size_t)tile * kTileFloats;
            const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
            for (int q = 0; q < 8; q++) f.v[q] = src[(wave * 8 + q) * 64 + lane];
        } else {
            const uint32_t rows_pad = (op.rows + op.ones + 31u) & ~31u;
#pragma unroll
            for (int q = 0; q < kFetch; q++) {   // consecutive threads: consecutive features of one sample
                const uint32_t e = threadIdx.x + (uint32_t)q * kThreads, s = e / rows_pad, o = e - s * rows_pad, sample = tile * 32 + s;
                // unconditional load from a clamped address (a predicated load would be a branch with its own wait); what lies
                // outside the operand is zeroed in commit(), so nothing here waits for the load
                f.v[q] = op.p[(size_t)(sample < M ? sample : M - 1u) * op.ld + (o < op.rows ? o : 0u)];
            }
        }
    }
    __device__ __forceinline__ void commit(float *t, const Fetched &f, uint32_t tile, uint32_t) const {
        if constexpr (NATIVE) {
            const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const int idx = wave * 8 + q, rt = idx >> 4, r = idx & 15;
                t[(32 * rt + rowmap(r, h)) * kTS + (j & 1) * 16 + (j >> 1)] = f.v[q];
            }
        } else {
            const uint32_t rows_pad = (op.rows + op.ones + 31u) & ~31u, n = rows_pad * 32u;
#pragma unroll
            for (int q = 0; q < kFetch; q++) {
                const uint32_t e = threadIdx.x + (uint32_t)q * kThreads, s = e / rows_pad, o = e - s * rows_pad;
                const bool in_tile = tile * 32 + s < M;
                if (e < n) t[o * kTS + (s & 1u) * 16u + (s >> 1)] = (in_tile && o < op.rows) ? f.v[q] : ((in_tile && op.ones && o == op.rows) ? 1.0f : 0.0f);
            }
        }
    }
};

// the operand kinds are compile-time inside a job (three combinations occur: dZ native x x row-major, native x native,
// grad_out row-major x native): no value of the fetch pipeline crosses a data-dependent branch
__global__ void __launch_bounds__(kThreads, 3) k_mlp_wgrad(WArgs p) {
    __shared__ __attribute__((aligned(16))) float lds[wgrad::kLdsFloats];
    const uint32_t jb = blockIdx.x / p.parts, part = blockIdx.x % p.parts;
    if (jb >= p.n_jobs) return;
    const WJob &job = p.job[jb];
    const uint32_t n_tiles = (p.M + 31u) >> 5;
    auto run = [&](const auto &a, const auto &b) { wgrad::run(a, b, n_tiles, p.M, part, p.parts, job.partial, lds); };
    if (job.a.native && job.b.native) run(Op<true>{job.a, p.M}, Op<true>{job.b, p.M});
    else if (job.a.native) run(Op<true>{job.a, p.M}, Op<false>{job.b, p.M});
    else run(Op<false>{job.a, p.M}, Op<true>{job.b, p.M});
}

__global__ void __launch_bounds__(256) k_mlp_wreduce(WArgs p) {
    const uint32_t jb = blockIdx.y;
    if (jb >= p.n_jobs) return;
    const WJob &job = p.job[jb];
    wgrad::wreduce(job.partial, p.parts, blockIdx.x * 256 + threadIdx.x, job.a.rows, job.out_cols,
                   job.out_bias && job.b.ones ? (int32_t)job.b.rows : -1, job.out, job.out_ld, job.out_bias);
}

template <typename K, typename A>
static void launch_with_lds(K kernel, dim3 grid, size_t shm, hipStream_t s, const A &args) {
    if (shm > 64 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
    hipLaunchKernelGGL(kernel, grid, dim3(kThreads), shm, s, args);
}
constexpr uint32_t kWPartsMax = 512;  // workspace is sized for this many partial sums per job
static uint32_t wparts() {            // workgroups (= partial sums) per weight-gradient job: 3 jobs x 256 = 3 workgroups per CU
    static const uint32_t n = env_uint_clamped("RN_MLP_WPARTS", 256, kWPartsMax);
    return n;
}

}  // namespace mlp
}  // namespace rn

using namespace rn;
using namespace rn::mlp;

extern "C" {

size_t rn_mlp64_image_floats(uint32_t in_dim, uint32_t out_dim, uint32_t n_layers) {
    Dims d;
    if (!make_dims(in_dim, out_dim, n_layers, d)) return 0;
    return (size_t)d.fwd_floats() + d.bwd_floats();
}

size_t rn_mlp64_tile_floats(uint32_t M) { return (size_t)((M + 31u) >> 5) * kTileFloats; }

size_t rn_mlp64_wgrad_workspace(uint32_t n_layers) { return (size_t)n_layers * kWPartsMax * wgrad::kPartial * sizeof(float); }

int rn_mlp64_pack(const float *w0, uint32_t ld0, const float *w1, const float *w_last, uint32_t in_dim, uint32_t out_dim, uint32_t n_layers,
                  float *image, rn_stream_t stream) {
    Dims d;
    RN_REQUIRE(ld0 >= in_dim, "mlp64_pack: ld0 (row stride of w0) must be >= in_dim");
    RN_REQUIRE(make_dims(in_dim, out_dim, n_layers, d, ld0), "mlp64: unsupported shape (hidden 64, 2 or 3 layers, in <= 96, out <= 4 or 64 .. 68)");
    RN_REQUIRE(w0 && w_last && image && (n_layers == 2 || w1) && ((uintptr_t)image & 15u) == 0, "mlp64_pack: null / unaligned pointer");
    const uint32_t n = d.fwd_floats() + d.bwd_floats();
    hipLaunchKernelGGL(k_mlp_pack, dim3(div_up(n, 256)), dim3(256), 0, as_stream(stream), w0, w1, w_last, d, image);
    return check_launch("mlp64_pack");
}

#define RN_MLP_DISPATCH(KERNEL, grid, shm, stream, args)                                                                          \
    do {                                                                                                                          \
        const bool hid2 = d.n_layers == 3;                                                                                        \
        if (d.wide && d.nn == 1 && hid2) launch_with_lds(KERNEL<1, true, true>, grid, shm, stream, args);                         \
        else if (d.wide && d.nn == 0 && hid2) launch_with_lds(KERNEL<0, true, true>, grid, shm, stream, args);                    \
        else if (!d.wide && d.nn == 2 && hid2) launch_with_lds(KERNEL<2, false, true>, grid, shm, stream, args);                  \
        else if (!d.wide && d.nn == 3 && !hid2) launch_with_lds(KERNEL<3, false, false>, grid, shm, stream, args);                \
        else if (!d.wide && d.nn == 4 && hid2) launch_with_lds(KERNEL<4, false, true>, grid, shm, stream, args);                  \
        else if (!d.wide && d.nn == 1 && hid2) launch_with_lds(KERNEL<1, false, true>, grid, shm, stream, args);                  \
        else {                                                                                                                    \
            ::rn::set_error("mlp64: this (out_dim, n_layers) combination is not instantiated");                                  \
            return RN_ERR_INVALID_ARG;                                                                                            \
        }                                                                                                                         \
    } while (0)

int rn_mlp64_forward(const float *x, uint32_t M, const float *image, const float *bias0, uint32_t in_dim, uint32_t out_dim,
                     uint32_t n_layers, float *out, float *h0, float *h1, rn_stream_t stream) {
    if (M == 0) return RN_OK;
    Dims d;
    RN_REQUIRE(make_dims(in_dim, out_dim, n_layers, d), "mlp64: unsupported shape (hidden 64, 2 or 3 layers, in <= 96, out <= 4 or 64 .. 68)");
    RN_REQUIRE(x && image && out && h0 && (n_layers == 2 || h1), "mlp64_forward: null pointer");
    RN_REQUIRE(((uintptr_t)x & 7u) == 0 && ((uintptr_t)image & 15u) == 0, "mlp64_forward: x must be 8-byte, image 16-byte aligned");
    FwdArgs p{x, M, image, d, out, h0, h1, bias0};
    const uint32_t blocks = tile_blocks((M + 31u) >> 5, kWaves, 2);
    const size_t shm = (size_t)d.fwd_floats() * sizeof(float);
    RN_MLP_DISPATCH(k_mlp_fwd, dim3(blocks), shm, as_stream(stream), p);
    return check_launch("mlp64_forward");
}

int rn_mlp64_backward(const float *grad_out, uint32_t M, const float *image, uint32_t in_dim, uint32_t out_dim, uint32_t n_layers,
                      const float *h0, const float *h1, float *grad_x, float *dz0, float *dz1, rn_stream_t stream) {
    if (M == 0) return RN_OK;
    Dims d;
    RN_REQUIRE(make_dims(in_dim, out_dim, n_layers, d), "mlp64: unsupported shape (hidden 64, 2 or 3 layers, in <= 96, out <= 4 or 64 .. 68)");
    RN_REQUIRE(grad_out && image && h0 && grad_x && dz0 && (n_layers == 2 || (h1 && dz1)), "mlp64_backward: null pointer");
    RN_REQUIRE(((uintptr_t)grad_x & 15u) == 0 && ((uintptr_t)image & 15u) == 0, "mlp64_backward: grad_x / image must be 16-byte aligned");
    BwdArgs p{grad_out, M, image + d.fwd_floats(), d, h0, h1, grad_x, dz0, dz1};
    RN_REQUIRE((d.fwd_floats() & 3u) == 0, "mlp64_backward: internal image alignment");
    const uint32_t blocks = tile_blocks((M + 31u) >> 5, kWaves, 2);
    const size_t shm = (size_t)d.bwd_floats() * sizeof(float);
    RN_MLP_DISPATCH(k_mlp_bwd, dim3(blocks), shm, as_stream(stream), p);
    return check_launch("mlp64_backward");
}

int rn_mlp64_weight_grads(const float *x, const float *grad_out, uint32_t M, uint32_t in_dim, uint32_t out_dim, uint32_t n_layers,
                          const float *h0, const float *h1, const float *dz0, const float *dz1, float *gw0, uint32_t ld0, float *gw1,
                          float *gw_last, float *grad_bias0, void *workspace, rn_stream_t stream) {
    Dims d;
    RN_REQUIRE(make_dims(in_dim, out_dim, n_layers, d), "mlp64: unsupported shape (hidden 64, 2 or 3 layers, in <= 96, out <= 4 or 64 .. 68)");
    RN_REQUIRE(x && grad_out && h0 && dz0 && gw0 && gw_last && workspace && (n_layers == 2 || (h1 && dz1 && gw1)), "mlp64_weight_grads: null pointer");
    RN_REQUIRE(M > 0, "mlp64_weight_grads: M must be positive");
    RN_REQUIRE(ld0 >= in_dim, "mlp64_weight_grads: ld0 (row stride of gw0) must be >= in_dim");
    RN_REQUIRE(!grad_bias0 || d.in_pad + 1u <= 96u, "mlp64_weight_grads: a bias gradient needs in_dim <= 92");
    WArgs p{};
    p.M = M;
    p.parts = wparts();
    float *ws = static_cast<float *>(workspace);
    const size_t per_job = (size_t)kWPartsMax * wgrad::kPartial;
    uint32_t n = 0;
    // L0: dW0 = dZ0 x^T
    p.job[n] = WJob{Operand{dz0, 1u, 0u, 64u, 0u}, Operand{x, 0u, d.in_pad, d.in_pad, grad_bias0 ? 1u : 0u}, ws + n * per_job, gw0, ld0, d.in_dim, grad_bias0};
    n++;
    if (n_layers == 3) {
        p.job[n] = WJob{Operand{dz1, 1u, 0u, 64u, 0u}, Operand{h0, 1u, 0u, 64u, 0u}, ws + n * per_job, gw1, 64u, 64u, nullptr};
        n++;
    }
    p.job[n] = WJob{Operand{grad_out, 0u, d.out_dim, d.out_dim, 0u}, Operand{n_layers == 3 ? h1 : h0, 1u, 0u, 64u, 0u}, ws + n * per_job, gw_last, 64u, 64u, nullptr};
    n++;
    p.n_jobs = n;
    hipLaunchKernelGGL(k_mlp_wgrad, dim3(n * p.parts), dim3(kThreads), 0, as_stream(stream), p);
    hipLaunchKernelGGL(k_mlp_wreduce, dim3(div_up(wgrad::kPartial, 256), n), dim3(256), 0, as_stream(stream), p);
    return check_launch("mlp64_weight_grads");
}

}  // extern "C"
