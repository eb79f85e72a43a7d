// rn_asr.hip -- audio features from samples: the wav2vec2 CTC model of the reference's nerf/asr.py (file mode) in fp32.
// See include/radnerf_fused.h for the arithmetic and rn_asr_dev.h for the weight image and the workspace.
//
//   k_pack_norm     positional conv: g[tap] / |v[:, :, tap]| per tap (one workgroup per tap, ordered sum)
//   k_pack          one tensor [Cout][Cin][k] -> its GEMM image [(tap, ci)][co] (a Linear is k = 1, a vector Cin = k = 1)
//   k_normalize     per window: mean, population variance, (x - mean) / sqrt(var + 1e-7)                (two-pass, ordered)
//   k_conv0         conv layer 0 (one input channel) + bias + LayerNorm + GELU, one wave per output step (VALU)
//   k_gemm          C = epilogue(A B): 128 x 128 x 16 LDS tiles, 4 waves of 2 x 2 v_mfma_f32_32x32x2_f32 tiles.  A is read
//                   through (batch stride, row stride) and a (segment length, segment stride) walk of K, so the strided
//                   convolutions and the grouped positional convolution need no im2col pass; blockIdx.z walks groups.
//                   Epilogue: + bias, GELU, + residual.  K is never split: a row's sum order does not depend on M.
//   k_gemm32        the same product on 32 x 32 tiles, one wave per tile straight from L2 (no LDS, no barrier), for a small M:
//                   the same chain over k per output, so the same bits; pick_tile chooses between the two per product
//   k_layer_norm    one row per wave, two-pass, optional GELU
//   k_pad           h [B][T][H] -> [B][T + taps][H] with taps / 2 zero rows in front
//   k_attention     one workgroup per (window, head): keys and values in LDS, a wave per query row, softmax in registers
//   k_features      the cut and the unfold -> [F][C][16]
//   k_ring_push     live mode: the kept rows of one window's logits into the feature ring, zero rows behind them
//   k_ring_window   live mode: one frame's attention window [8][C][16] out of the ring
//
// No float atomics; every sum in one fixed order.
#include "rn_asr_dev.h"
#include "rn_tile32_dev.h"

namespace rn {
namespace asr {

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

// the same bits in every lane
__device__ __forceinline__ float wave_sum_all(float v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ float wave_max_all(float v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}

// ------------------------------------------------------------------------------------------------------------------ pack
__global__ void __launch_bounds__(256) k_pack_norm(const float *__restrict__ g, const float *__restrict__ v, uint32_t rows, uint32_t taps,
                                                   float *__restrict__ scale) {
    __shared__ float lds[4];
    const uint32_t tap = blockIdx.x;
    float s = 0.0f;
    for (uint32_t r = threadIdx.x; r < rows; r += 256u) {
        const float x = v[(size_t)r * taps + tap];
        s += x * x;
    }
    s = block_sum<float, 256>(s, lds);
    if (threadIdx.x == 0) scale[tap] = g[tap] / sqrtf(s);
}

// dst[(tap * Cin + ci) * ld + col0 + co] = src[((co0 + co) * Cin + ci) * k + tap] * (scale ? scale[tap] : 1) for co < Cout,
// 0 for co in Cout .. width - 1; total = k * Cin * width
__global__ void __launch_bounds__(256) k_pack(const float *__restrict__ src, float *__restrict__ dst, uint32_t Cout, uint32_t Cin, uint32_t k,
                                              uint32_t width, uint32_t ld, uint32_t col0, uint32_t co0, const float *__restrict__ scale,
                                              size_t total) {
    const size_t idx = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (idx >= total) return;
    const uint32_t co = (uint32_t)(idx % width);
    const size_t kk = idx / width;
    const uint32_t ci = (uint32_t)(kk % Cin), tap = (uint32_t)(kk / Cin);
    float v = 0.0f;
    if (co < Cout) {
        v = src[((size_t)(co0 + co) * Cin + ci) * k + tap];
        if (scale) v *= scale[tap];
    }
    dst[kk * ld + col0 + co] = v;
}

// ------------------------------------------------------------------------------------------------------------------ input
__global__ void __launch_bounds__(256) k_normalize(const float *__restrict__ x, float *__restrict__ out, uint32_t S) {
    __shared__ float lds[4];
    const float *row = x + (size_t)blockIdx.x * S;
    float *dst = out + (size_t)blockIdx.x * S;
    float s = 0.0f;
    for (uint32_t i = threadIdx.x; i < S; i += 256u) s += row[i];
    const float mean = block_sum<float, 256>(s, lds) / (float)S;
    s = 0.0f;
    for (uint32_t i = threadIdx.x; i < S; i += 256u) {
        const float d = row[i] - mean;
        s += d * d;
    }
    const float var = block_sum<float, 256>(s, lds) / (float)S;
    const float inv = 1.0f / sqrtf(var + 1e-7f);
    for (uint32_t i = threadIdx.x; i < S; i += 256u) dst[i] = (row[i] - mean) * inv;
}

// out[b][t][c] = GELU(LN_c(bias[c] + sum_j w[j][c] x[b][t * stride + j])); the convolution is recomputed in each of the three
// passes (k multiply-adds per value) instead of being kept: no register array of a run-time length
__global__ void __launch_bounds__(256) k_conv0(const float *__restrict__ x, const float *__restrict__ w, const float *__restrict__ bias,
                                               const float *__restrict__ gamma, const float *__restrict__ beta, float *__restrict__ out,
                                               uint32_t rows, uint32_t T, uint32_t S, uint32_t C, uint32_t k, uint32_t stride, float eps) {
    __shared__ float taps[4][64];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, row = blockIdx.x * 4u + wave;
    const bool live = row < rows;
    const uint32_t b = live ? row / T : 0u, t = live ? row - b * T : 0u;
    if (lane < k) taps[wave][lane] = x[(size_t)b * S + t * stride + lane];      // t * stride + k - 1 < S by the plan
    __syncthreads();
    if (!live) return;
    const float *xs = taps[wave];
    auto conv = [&](uint32_t c) {
        float v = bias[c];
        for (uint32_t j = 0; j < k; j++) v = __builtin_fmaf(w[j * C + c], xs[j], v);
        return v;
    };
    float s = 0.0f;
    for (uint32_t c = lane; c < C; c += 64u) s += conv(c);
    const float mean = wave_sum_all(s) / (float)C;
    s = 0.0f;
    for (uint32_t c = lane; c < C; c += 64u) {
        const float d = conv(c) - mean;
        s += d * d;
    }
    const float inv = 1.0f / sqrtf(wave_sum_all(s) / (float)C + eps);
    float *dst = out + (size_t)row * C;
    for (uint32_t c = lane; c < C; c += 64u) dst[c] = gelu_erf((conv(c) - mean) * inv * gamma[c] + beta[c]);
}

// ------------------------------------------------------------------------------------------------------------------ GEMM
constexpr uint32_t kBM = 128, kBN = 128, kBK = 16, kLd = kBM + 4;     // LDS rows of 132 floats: 16-byte aligned, k-major

struct GemmArgs {
    const float *A, *W, *bias, *res;
    float *C;
    uint32_t M, N, K;
    uint32_t rows_per_batch;        // row m = (b, t): b = m / rows_per_batch
    size_t a_batch, a_row;          // A row (b, t) starts at b * a_batch + t * a_row floats
    uint32_t seg_len, seg_stride;   // k -> (k / seg_len) * seg_stride + k % seg_len floats into the row; seg_len % 4 == 0
    uint32_t ldw, ldc;              // W [K][ldw], ldw % 4 == 0; C and res [M][ldc]
    size_t a_group, w_group;        // per blockIdx.z
    uint32_t c_group;               // columns of C, res and bias per blockIdx.z
    int gelu;
};

__device__ __forceinline__ void epilogue(const GemmArgs &a, const f32x16 &acc, uint32_t m0, uint32_t n, uint32_t hh, uint32_t col0) {
    if (n >= a.N) return;
    const float bias = a.bias[col0 + n];
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const uint32_t m = m0 + (uint32_t)rowmap(r, (int)hh);
        if (m >= a.M) continue;
        const size_t at = (size_t)m * a.ldc + col0 + n;
        float v = acc[r] + bias;
        if (a.gelu) v = gelu_erf(v);
        if (a.res) v += a.res[at];
        a.C[at] = v;
    }
}

__global__ void __launch_bounds__(256) k_gemm(GemmArgs a) {
    __shared__ __attribute__((aligned(16))) float As[kBK * kLd], Bs[kBK * kLd];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, j = lane & 31u, hh = lane >> 5;
    const uint32_t wm = wave >> 1, wn = wave & 1u;
    const uint32_t bm = blockIdx.y * kBM, bn = blockIdx.x * kBN, z = blockIdx.z;
    const float *A = a.A + z * a.a_group, *W = a.W + z * a.w_group;

    // this thread's two float4 of the A tile (row, four k) and of the W tile (k, four n)
    const float *arow[2];
    uint32_t a_r[2], a_k[2], w_k[2], w_n[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const uint32_t idx = tid + 256u * (uint32_t)i;
        a_r[i] = idx >> 2; a_k[i] = (idx & 3u) * 4u;
        const uint32_t m = bm + a_r[i];
        if (m < a.M) {
            const uint32_t b = m / a.rows_per_batch, t = m - b * a.rows_per_batch;
            arow[i] = A + b * a.a_batch + t * a.a_row;
        } else {
            arow[i] = nullptr;
        }
        w_k[i] = idx >> 5; w_n[i] = (idx & 31u) * 4u;
    }
    float4 ra[2], rw[2];
    auto fetch = [&](uint32_t k0) {
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const uint32_t k = k0 + a_k[i];
            ra[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (arow[i] && k < a.K) {
                const uint32_t seg = k / a.seg_len;
                ra[i] = *reinterpret_cast<const float4 *>(arow[i] + (size_t)seg * a.seg_stride + (k - seg * a.seg_len));
            }
            const uint32_t kw = k0 + w_k[i], n = bn + w_n[i];
            rw[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (kw < a.K && n < a.ldw) rw[i] = *reinterpret_cast<const float4 *>(W + (size_t)kw * a.ldw + n);
        }
    };
    f32x16 acc00 = zero16(), acc01 = zero16(), acc10 = zero16(), acc11 = zero16();
    fetch(0);
    for (uint32_t k0 = 0; k0 < a.K; k0 += kBK) {
#pragma unroll
        for (int i = 0; i < 2; i++) {
            float *d = As + a_k[i] * kLd + a_r[i];
            d[0] = ra[i].x; d[kLd] = ra[i].y; d[2 * kLd] = ra[i].z; d[3 * kLd] = ra[i].w;
            *reinterpret_cast<float4 *>(Bs + w_k[i] * kLd + w_n[i]) = rw[i];
        }
        __syncthreads();
        if (k0 + kBK < a.K) fetch(k0 + kBK);
        const float *ap = As + hh * kLd + wm * 64u + j, *bp = Bs + hh * kLd + wn * 64u + j;
#pragma unroll
        for (uint32_t s = 0; s < kBK / 2u; s++) {
            const float a0 = ap[2u * s * kLd], a1 = ap[2u * s * kLd + 32u], b0 = bp[2u * s * kLd], b1 = bp[2u * s * kLd + 32u];
            acc00 = mfma32(a0, b0, acc00);
            acc01 = mfma32(a0, b1, acc01);
            acc10 = mfma32(a1, b0, acc10);
            acc11 = mfma32(a1, b1, acc11);
        }
        __syncthreads();
    }
    const uint32_t m0 = bm + wm * 64u, n0 = bn + wn * 64u + j, col0 = z * a.c_group;
    epilogue(a, acc00, m0, n0, hh, col0);
    epilogue(a, acc01, m0, n0 + 32u, hh, col0);
    epilogue(a, acc10, m0 + 32u, n0, hh, col0);
    epilogue(a, acc11, m0 + 32u, n0 + 32u, hh, col0);
}

// The 32-row tiling: a workgroup is four waves on four row tiles of one 32-column strip, a wave owns one 32 x 32 tile and walks all
// of K alone.  Lane (j, hh) holds row m0 + j of A as whole float4 along k (both lane halves load the same 16 bytes and pick the
// k's of their half) and column n0 + j of W for k = 2 s + hh.  Stages of kSK k's are fetched one stage ahead into registers.
// Every output runs the MFMA chain of k_gemm: steps s = 0 .. up16(K) / 2 - 1 from a zero accumulator, zeros past K.
constexpr uint32_t kSK = 64;

__global__ void __launch_bounds__(256) k_gemm32(GemmArgs a) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, j = lane & 31u, hh = lane >> 5;
    const uint32_t m0 = (blockIdx.y * 4u + wave) * 32u, n0 = blockIdx.x * 32u, z = blockIdx.z;
    if (m0 >= a.M) return;
    // a lane past M or past ldw, and a k past K, loads from a clamped address and drops the value: no branch sits between the loads
    const bool alive = m0 + j < a.M, wlive = n0 + j < a.ldw;
    const uint32_t m = alive ? m0 + j : a.M - 1u, b = m / a.rows_per_batch, t = m - b * a.rows_per_batch;
    const float *arow = a.A + z * a.a_group + b * a.a_batch + t * a.a_row;
    const float *wcol = a.W + z * a.w_group + (wlive ? n0 + j : 0u);
    const uint32_t Kpad = (a.K + kBK - 1u) / kBK * kBK;

    // the fetches come in order: the next k, its place in its segment and the segment's start in the row (the same in every lane)
    uint32_t fk = 0, foff = 0;
    size_t fbase = 0;
    auto fetch = [&](float4 (&ra)[kSK / 4u], float (&rw)[kSK / 2u]) {
#pragma unroll
        for (uint32_t s = 0; s < kSK / 2u; s++) {
            const uint32_t kw = fk + 2u * s + hh;
            const bool ok = kw < a.K;
            rw[s] = wcol[(size_t)(ok ? kw : 0u) * a.ldw];
        }
#pragma unroll
        for (uint32_t q = 0; q < kSK / 4u; q++) {
            const bool ok = fk < a.K;
            ra[q] = *reinterpret_cast<const float4 *>(arow + (ok ? fbase + foff : (size_t)0));
            fk += 4u; foff += 4u;
            if (foff >= a.seg_len) { foff = 0u; fbase += a.seg_stride; }
        }
    };
    f32x16 acc = zero16();
    auto compute = [&](const float4 (&ra)[kSK / 4u], const float (&rw)[kSK / 2u], uint32_t k0) {
#pragma unroll
        for (uint32_t g = 0; g < kSK / kBK; g++) {
            if (k0 + g * kBK < Kpad) {
#pragma unroll
                for (uint32_t s = g * (kBK / 2u); s < (g + 1u) * (kBK / 2u); s++) {
                    const float4 v = ra[s >> 1];
                    const uint32_t k = k0 + 2u * s + hh;        // dropped here, not at the load: the load stays in flight
                    const float av = (s & 1u) ? (hh ? v.w : v.z) : (hh ? v.y : v.x);
                    acc = mfma32((alive && k < a.K) ? av : 0.0f, (wlive && k < a.K) ? rw[s] : 0.0f, acc);
                }
            }
        }
    };
    // two register stages in turn, each fetched while the other is multiplied (a fetch past K reads the clamped address again)
    float4 ra0[kSK / 4u], ra1[kSK / 4u];
    float rw0[kSK / 2u], rw1[kSK / 2u];
    fetch(ra0, rw0);
    for (uint32_t k0 = 0; k0 < Kpad; k0 += 2u * kSK) {
        fetch(ra1, rw1);
        compute(ra0, rw0, k0);
        if (k0 + kSK >= Kpad) break;
        fetch(ra0, rw0);
        compute(ra1, rw1, k0 + kSK);
    }
    epilogue(a, acc, m0, n0 + j, hh, z * a.c_group);
}

// ------------------------------------------------------------------------------------------------------------------ rows
__global__ void __launch_bounds__(256) k_layer_norm(const float *__restrict__ in, float *__restrict__ out, const float *__restrict__ gamma,
                                                    const float *__restrict__ beta, uint32_t rows, uint32_t C, float eps, int gelu) {
    const uint32_t lane = threadIdx.x & 63u, row = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float *x = in + (size_t)row * C;
    float s = 0.0f;
    for (uint32_t c = lane; c < C; c += 64u) s += x[c];
    const float mean = wave_sum_all(s) / (float)C;
    s = 0.0f;
    for (uint32_t c = lane; c < C; c += 64u) {
        const float d = x[c] - mean;
        s += d * d;
    }
    const float inv = 1.0f / sqrtf(wave_sum_all(s) / (float)C + eps);
    float *dst = out + (size_t)row * C;
    for (uint32_t c = lane; c < C; c += 64u) {
        const float v = (x[c] - mean) * inv * gamma[c] + beta[c];
        dst[c] = gelu ? gelu_erf(v) : v;
    }
}

__global__ void __launch_bounds__(256) k_pad(const float *__restrict__ h, float *__restrict__ pad, uint32_t T, uint32_t taps, uint32_t H4,
                                             size_t total4) {
    const size_t idx = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (idx >= total4) return;
    const uint32_t c4 = (uint32_t)(idx % H4);
    const size_t row = idx / H4;
    const uint32_t r = (uint32_t)(row % (T + taps)), b = (uint32_t)(row / (T + taps));
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (r >= taps / 2u && r - taps / 2u < T) v = reinterpret_cast<const float4 *>(h)[((size_t)b * T + (r - taps / 2u)) * H4 + c4];
    reinterpret_cast<float4 *>(pad)[idx] = v;
}

// grid (heads, B).  qkv [B][T][3 H]: q | k | v, head `hd` at columns 64 hd .. 64 hd + 63 of each.  T <= kMaxT.
__global__ void __launch_bounds__(256) k_attention(const float *__restrict__ qkv, float *__restrict__ out, uint32_t T, uint32_t H, float scale) {
    __shared__ float Ks[kMaxT * (kHeadDim + 1u)], Vs[kMaxT * kHeadDim];
    const uint32_t hd = blockIdx.x, b = blockIdx.y, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const float *base = qkv + (size_t)b * T * 3u * H + hd * kHeadDim;
    for (uint32_t idx = threadIdx.x; idx < T * kHeadDim; idx += 256u) {
        const uint32_t t = idx >> 6, d = idx & 63u;
        Ks[t * (kHeadDim + 1u) + d] = base[(size_t)t * 3u * H + H + d];
        Vs[t * kHeadDim + d] = base[(size_t)t * 3u * H + 2u * H + d];
    }
    __syncthreads();
    const bool v0 = lane < T, v1 = lane + 64u < T;
    const float *k0 = Ks + (v0 ? lane : 0u) * (kHeadDim + 1u), *k1 = Ks + (v1 ? lane + 64u : 0u) * (kHeadDim + 1u);
    for (uint32_t t = wave; t < T; t += 4u) {
        const float q = base[(size_t)t * 3u * H + lane] * scale;
        float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
        for (int d = 0; d < (int)kHeadDim; d++) {
            const float qd = __shfl(q, d, 64);
            s0 = __builtin_fmaf(qd, k0[d], s0);
            s1 = __builtin_fmaf(qd, k1[d], s1);
        }
        s0 = v0 ? s0 : -INFINITY;
        s1 = v1 ? s1 : -INFINITY;
        const float mx = wave_max_all(fmaxf(s0, s1));
        const float e0 = v0 ? expf(s0 - mx) : 0.0f, e1 = v1 ? expf(s1 - mx) : 0.0f;
        const float sum = wave_sum_all(e0 + e1);
        const float p0 = e0 / sum, p1 = e1 / sum;
        float o = 0.0f;
        const uint32_t n0 = T < 64u ? T : 64u;
        for (uint32_t key = 0; key < n0; key++) o = __builtin_fmaf(__shfl(p0, (int)key, 64), Vs[key * kHeadDim + lane], o);
        for (uint32_t key = 64u; key < T; key++) o = __builtin_fmaf(__shfl(p1, (int)(key - 64u), 64), Vs[key * kHeadDim + lane], o);
        out[((size_t)b * T + t) * H + hd * kHeadDim + lane] = o;
    }
}

// ------------------------------------------------------------------------------------------------------------------ features
constexpr uint32_t kMaxSegments = 4;
struct FeatArgs {
    uint32_t first[kMaxSegments], windows[kMaxSegments], T[kMaxSegments], left[kMaxSegments], kept[kMaxSegments];
    uint32_t n, M, C, F;
};

__global__ void __launch_bounds__(256) k_features(const float *__restrict__ logits, FeatArgs a, float *__restrict__ out) {
    const size_t idx = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (idx >= (size_t)a.F * a.C * 16u) return;
    const uint32_t jj = (uint32_t)(idx & 15u), c = (uint32_t)((idx >> 4) % a.C), f = (uint32_t)((idx >> 4) / a.C);
    const int64_t i = 2 * (int64_t)f - 8 + jj;
    float v = 0.0f;
    if (i >= 0 && i < (int64_t)a.M) {
        uint32_t rest = (uint32_t)i;
        for (uint32_t s = 0; s < a.n; s++) {
            const uint32_t rows = a.windows[s] * a.kept[s];
            if (rest < rows) {
                const uint32_t w = rest / a.kept[s], r = rest - w * a.kept[s];
                v = logits[((size_t)a.first[s] + (size_t)w * a.T[s] + a.left[s] + r) * a.C + c];
                break;
            }
            rest -= rows;
        }
    }
    out[idx] = v;
}

// ------------------------------------------------------------------------------------------------------------------ live ring
// ring row (first_row + i) % ring_rows = logits row left + i for i < rows, zeros for rows <= i < rows + zero_rows
__global__ void __launch_bounds__(256) k_ring_push(const float *__restrict__ logits, uint32_t C, uint32_t left, uint32_t rows,
                                                   float *__restrict__ ring, uint32_t ring_rows, uint32_t first_row, uint32_t zero_rows) {
    const size_t idx = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (idx >= (size_t)(rows + zero_rows) * C) return;
    const uint32_t i = (uint32_t)(idx / C), c = (uint32_t)(idx - (size_t)i * C);
    const uint32_t dst = (uint32_t)(((uint64_t)first_row + i) % ring_rows);
    ring[(size_t)dst * C + c] = i < rows ? logits[(size_t)(left + i) * C + c] : 0.0f;
}

// out[e][c][t] = ring[(ring_rows - 8 + 2 s + t) % ring_rows][c] for slice s = k - 4 + e in 0 .. n_slices - 1, else 0
__global__ void __launch_bounds__(256) k_ring_window(const float *__restrict__ ring, uint32_t ring_rows, uint32_t C, uint32_t k,
                                                     uint32_t n_slices, float *__restrict__ out) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= 8u * C * 16u) return;
    const uint32_t t = idx & 15u, c = (idx >> 4) % C, e = (idx >> 4) / C;
    const int64_t s = (int64_t)k - 4 + e;
    float v = 0.0f;
    if (s >= 0 && s < (int64_t)n_slices) v = ring[(size_t)(((uint64_t)ring_rows - 8u + 2u * (uint64_t)s + t) % ring_rows) * C + c];
    out[idx] = v;
}

// ------------------------------------------------------------------------------------------------------------------ host
// one tensor [Cout][Cin][k] into columns col0 .. col0 + width - 1 of a [k * Cin][ld] matrix
static void pack_one(const float *src, float *dst, uint32_t Cout, uint32_t Cin, uint32_t k, uint32_t width, uint32_t ld, uint32_t col0,
                     uint32_t co0, const float *scale, hipStream_t st) {
    const size_t total = (size_t)k * Cin * width;
    hipLaunchKernelGGL(k_pack, dim3((uint32_t)((total + 255u) / 256u)), dim3(256), 0, st, src, dst, Cout, Cin, k, width, ld, col0, co0, scale,
                       total);
}
static void pack_mat(const float *src, float *dst, uint32_t Cout, uint32_t Cin, uint32_t k, hipStream_t st) {
    pack_one(src, dst, Cout, Cin, k, (uint32_t)up4(Cout), (uint32_t)up4(Cout), 0u, 0u, nullptr, st);
}
static void pack_vec(const float *src, float *dst, uint32_t n, hipStream_t st) { pack_mat(src, dst, n, 1u, 1u, st); }

// tile: 0 = pick_tile's choice, 32 or 128
static void gemm(const GemmArgs &a, uint32_t groups, uint32_t tile, hipStream_t st) {
    if (tile == 0) tile = pick_tile(a.M, a.N, a.K, groups, (uint32_t)num_cus());
    if (tile == 32u)
        hipLaunchKernelGGL(k_gemm32, dim3(div_up(a.N, 32u), div_up(div_up(a.M, 32u), 4u), groups), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL(k_gemm, dim3(div_up(a.N, kBN), div_up(a.M, kBM), groups), dim3(256), 0, st, a);
}
// C [M][N] = epilogue(A [M][K] W [K][up4(N)]) with plain rows
static GemmArgs dense(const float *A, const float *W, const float *bias, float *C, uint32_t M, uint32_t N, uint32_t K) {
    GemmArgs a{};
    a.A = A; a.W = W; a.bias = bias; a.C = C; a.M = M; a.N = N; a.K = K;
    a.rows_per_batch = M; a.a_batch = 0; a.a_row = K; a.seg_len = K; a.seg_stride = 0;
    a.ldw = (uint32_t)up4(N); a.ldc = N;
    return a;
}
static void layer_norm(const float *in, float *out, const float *g, const float *b, uint32_t rows, uint32_t C, float eps, int gelu,
                       hipStream_t st) {
    hipLaunchKernelGGL(k_layer_norm, dim3(div_up(rows, 4u)), dim3(256), 0, st, in, out, g, b, rows, C, eps, gelu);
}

}  // namespace asr
}  // namespace rn

using namespace rn;
using namespace rn::asr;

extern "C" {

size_t rn_asr_image_floats(const rn_asr_config_t *config) { return unsupported(config) ? 0 : image_layout(*config).total; }

int rn_asr_pack(const rn_asr_config_t *config, const float *const *tensors, uint32_t n_tensors, float *image, rn_stream_t stream) {
    const char *why = unsupported(config);
    RN_REQUIRE(!why, "asr_pack: unsupported config: %s", why);
    RN_REQUIRE(tensors && image, "asr_pack: null pointer");
    const rn_asr_config_t &c = *config;
    RN_REQUIRE(n_tensors == tensor_count(c), "asr_pack: %u tensors, this config has %u", n_tensors, tensor_count(c));
    for (uint32_t i = 0; i < n_tensors; i++) RN_REQUIRE(tensors[i], "asr_pack: tensor %u is a null pointer", i);
    RN_REQUIRE(((uintptr_t)image & 15u) == 0, "asr_pack: image must be 16-byte aligned");
    const ImageLayout L = image_layout(c);
    hipStream_t st = as_stream(stream);
    const uint32_t H = c.hidden, I = c.intermediate;
    const float *const *t = tensors;
    for (uint32_t i = 0; i < c.n_conv; i++, t += 4) {
        const uint32_t cin = i ? c.conv_dim[i - 1] : 1u, co = c.conv_dim[i];
        pack_mat(t[0], image + L.conv_w[i], co, cin, c.conv_kernel[i], st);
        pack_vec(t[1], image + L.conv_b[i], co, st); pack_vec(t[2], image + L.conv_lnw[i], co, st); pack_vec(t[3], image + L.conv_lnb[i], co, st);
    }
    const uint32_t cl = c.conv_dim[c.n_conv - 1];
    pack_vec(t[0], image + L.proj_lnw, cl, st); pack_vec(t[1], image + L.proj_lnb, cl, st);
    pack_mat(t[2], image + L.proj_w, H, cl, 1u, st); pack_vec(t[3], image + L.proj_b, H, st);
    t += 4;
    const uint32_t cg = H / c.pos_groups;
    hipLaunchKernelGGL(k_pack_norm, dim3(c.pos_taps), dim3(256), 0, st, t[0], t[1], H * cg, c.pos_taps, image + L.pos_scale);
    for (uint32_t g = 0; g < c.pos_groups; g++)
        pack_one(t[1], image + L.pos_w + (size_t)g * c.pos_taps * cg * cg, cg, cg, c.pos_taps, cg, cg, 0u, g * cg, image + L.pos_scale, st);
    pack_vec(t[2], image + L.pos_b, H, st);
    t += 3;
    pack_vec(t[0], image + L.enc_lnw, H, st); pack_vec(t[1], image + L.enc_lnb, H, st);
    t += 2;
    for (uint32_t l = 0; l < c.layers; l++, t += kLayerTensors) {
        float *y = image + L.layers + (size_t)l * L.layer.size;
        const LayerLayout &o = L.layer;
        pack_vec(t[0], y + o.ln1_w, H, st); pack_vec(t[1], y + o.ln1_b, H, st);
        for (uint32_t p = 0; p < 3u; p++) {         // q | k | v side by side: columns p H .. p H + H - 1 of [H][3 H]
            pack_one(t[2 + 2 * p], y + o.wqkv, H, H, 1u, H, 3u * H, p * H, 0u, nullptr, st);
            pack_vec(t[3 + 2 * p], y + o.bqkv + p * H, H, st);
        }
        pack_mat(t[8], y + o.wo, H, H, 1u, st); pack_vec(t[9], y + o.bo, H, st);
        pack_vec(t[10], y + o.ln2_w, H, st); pack_vec(t[11], y + o.ln2_b, H, st);
        pack_mat(t[12], y + o.w1, I, H, 1u, st); pack_vec(t[13], y + o.b1, I, st);
        pack_mat(t[14], y + o.w2, H, I, 1u, st); pack_vec(t[15], y + o.b2, H, st);
    }
    pack_mat(t[0], image + L.head_w, c.vocab, H, 1u, st); pack_vec(t[1], image + L.head_b, c.vocab, st);
    return check_launch("asr_pack");
}

size_t rn_asr_workspace(const rn_asr_config_t *config, uint32_t B, uint32_t samples) {
    return unsupported(config) ? 0 : make_plan(*config, B, samples).total * sizeof(float);
}

int rn_asr_forward(const rn_asr_config_t *config, const float *image, void *workspace, size_t workspace_bytes, const float *windows,
                   uint32_t B, uint32_t samples, float *logits, rn_stream_t stream) {
    return rn_asr_forward_tile(config, image, workspace, workspace_bytes, windows, B, samples, logits, 0u, stream);
}

int rn_asr_forward_tile(const rn_asr_config_t *config, const float *image, void *workspace, size_t workspace_bytes, const float *windows,
                        uint32_t B, uint32_t samples, float *logits, uint32_t tile, rn_stream_t stream) {
    const char *why = unsupported(config);
    RN_REQUIRE(!why, "asr_forward: unsupported config: %s", why);
    RN_REQUIRE(tile == 0u || tile == 32u || tile == 128u, "asr_forward: tile must be 0 (auto), 32 or 128, got %u", tile);
    RN_REQUIRE(image && workspace && windows && logits, "asr_forward: null pointer");
    const rn_asr_config_t &c = *config;
    const Plan pl = make_plan(c, B, samples);
    RN_REQUIRE(pl.total > 0, "asr_forward: unsupported shape B = %u, %u samples (B 1 .. 4096; at least the encoder's receptive field, at most %u "
               "output steps)", B, samples, kMaxT);
    RN_REQUIRE(workspace_bytes >= pl.total * sizeof(float), "asr_forward: workspace of %zu bytes, rn_asr_workspace asks for %zu", workspace_bytes,
               pl.total * sizeof(float));
    RN_REQUIRE(((uintptr_t)workspace & 15u) == 0 && ((uintptr_t)image & 15u) == 0, "asr_forward: workspace and image must be 16-byte aligned");
    const ImageLayout L = image_layout(c);
    hipStream_t st = as_stream(stream);
    float *ws = static_cast<float *>(workspace);
    const float eps = c.layer_norm_eps;
    const uint32_t H = c.hidden, I = c.intermediate, T = pl.Tout, rows = B * T;

    hipLaunchKernelGGL(k_normalize, dim3(B), dim3(256), 0, st, windows, ws + pl.xn, samples);
    float *cur = ws + pl.conv_a, *nxt = ws + pl.conv_b;
    hipLaunchKernelGGL(k_conv0, dim3(div_up(B * pl.T[0], 4u)), dim3(256), 0, st, ws + pl.xn, image + L.conv_w[0], image + L.conv_b[0],
                       image + L.conv_lnw[0], image + L.conv_lnb[0], cur, B * pl.T[0], pl.T[0], samples, c.conv_dim[0], c.conv_kernel[0],
                       c.conv_stride[0], eps);
    for (uint32_t i = 1; i < c.n_conv; i++) {
        const uint32_t cin = c.conv_dim[i - 1], co = c.conv_dim[i], M = B * pl.T[i];
        GemmArgs a = dense(cur, image + L.conv_w[i], image + L.conv_b[i], nxt, M, co, c.conv_kernel[i] * cin);
        a.rows_per_batch = pl.T[i]; a.a_batch = (size_t)pl.T[i - 1] * cin; a.a_row = (size_t)c.conv_stride[i] * cin;
        gemm(a, 1u, tile, st);
        layer_norm(nxt, nxt, image + L.conv_lnw[i], image + L.conv_lnb[i], M, co, eps, 1, st);
        float *tmp = cur; cur = nxt; nxt = tmp;
    }
    const uint32_t cl = c.conv_dim[c.n_conv - 1];
    float *h = ws + pl.h, *x = ws + pl.x, *qkv = ws + pl.qkv, *att = ws + pl.att, *ff = ws + pl.ff, *pad = ws + pl.pad;
    layer_norm(cur, cur, image + L.proj_lnw, image + L.proj_lnb, rows, cl, eps, 0, st);
    gemm(dense(cur, image + L.proj_w, image + L.proj_b, h, rows, H, cl), 1u, tile, st);
    {   // h += GELU(conv(h) + bias): one GEMM per group over the zero-padded copy
        const size_t total4 = (size_t)B * (T + c.pos_taps) * (H / 4u);
        hipLaunchKernelGGL(k_pad, dim3((uint32_t)((total4 + 255u) / 256u)), dim3(256), 0, st, h, pad, T, c.pos_taps, H / 4u, total4);
        const uint32_t cg = H / c.pos_groups;
        GemmArgs a = dense(pad, image + L.pos_w, image + L.pos_b, h, rows, cg, c.pos_taps * cg);
        a.rows_per_batch = T; a.a_batch = (size_t)(T + c.pos_taps) * H; a.a_row = H;
        a.seg_len = cg; a.seg_stride = H;
        a.ldw = cg; a.ldc = H; a.a_group = cg; a.w_group = (size_t)c.pos_taps * cg * cg; a.c_group = cg;
        a.res = h; a.gelu = 1;
        gemm(a, c.pos_groups, tile, st);
    }
    for (uint32_t l = 0; l < c.layers; l++) {
        const float *y = image + L.layers + (size_t)l * L.layer.size;
        const LayerLayout &o = L.layer;
        layer_norm(h, x, y + o.ln1_w, y + o.ln1_b, rows, H, eps, 0, st);
        gemm(dense(x, y + o.wqkv, y + o.bqkv, qkv, rows, 3u * H, H), 1u, tile, st);
        hipLaunchKernelGGL(k_attention, dim3(c.heads, B), dim3(256), 0, st, qkv, att, T, H, 0.125f);
        GemmArgs p = dense(att, y + o.wo, y + o.bo, h, rows, H, H);
        p.res = h;
        gemm(p, 1u, tile, st);
        layer_norm(h, x, y + o.ln2_w, y + o.ln2_b, rows, H, eps, 0, st);
        GemmArgs f1 = dense(x, y + o.w1, y + o.b1, ff, rows, I, H);
        f1.gelu = 1;
        gemm(f1, 1u, tile, st);
        GemmArgs f2 = dense(ff, y + o.w2, y + o.b2, h, rows, H, I);
        f2.res = h;
        gemm(f2, 1u, tile, st);
    }
    layer_norm(h, x, image + L.enc_lnw, image + L.enc_lnb, rows, H, eps, 0, st);
    gemm(dense(x, image + L.head_w, image + L.head_b, logits, rows, c.vocab, H), 1u, tile, st);
    return check_launch("asr_forward");
}

int rn_asr_features(const float *logits, size_t logits_rows, uint32_t C, const uint32_t *segments, uint32_t n_segments, float *features,
                    uint32_t F, rn_stream_t stream) {
    RN_REQUIRE(logits && segments && features, "asr_features: null pointer");
    RN_REQUIRE(C >= 1 && C <= 65536u, "asr_features: C must be 1 .. 65536");
    RN_REQUIRE(n_segments >= 1 && n_segments <= kMaxSegments, "asr_features: n_segments must be 1 .. %u", kMaxSegments);
    FeatArgs a{};
    size_t M = 0;
    for (uint32_t s = 0; s < n_segments; s++) {
        const uint32_t *g = segments + 5u * s;
        RN_REQUIRE(g[3] <= g[4] && g[4] <= g[2], "asr_features: segment %u keeps rows %u .. %u of %u", s, g[3], g[4], g[2]);
        RN_REQUIRE((size_t)g[0] + (size_t)g[1] * g[2] <= logits_rows, "asr_features: segment %u ends past the %zu rows of logits", s, logits_rows);
        a.first[s] = g[0]; a.windows[s] = g[1]; a.T[s] = g[2]; a.left[s] = g[3]; a.kept[s] = g[4] - g[3];
        if (a.kept[s] == 0) a.windows[s] = 0;
        M += (size_t)a.windows[s] * a.kept[s];
    }
    RN_REQUIRE(M < (1u << 30), "asr_features: %zu kept rows", M);
    RN_REQUIRE(F == (uint32_t)(M / 2u + 1u), "asr_features: F = %u, %zu kept rows unfold to %zu", F, M, M / 2u + 1u);
    RN_REQUIRE((size_t)F * C * 16u < ((size_t)1 << 40), "asr_features: output too large");
    a.n = n_segments; a.M = (uint32_t)M; a.C = C; a.F = F;
    const size_t total = (size_t)F * C * 16u;
    hipLaunchKernelGGL(k_features, dim3((uint32_t)((total + 255u) / 256u)), dim3(256), 0, as_stream(stream), logits, a, features);
    return check_launch("asr_features");
}

int rn_asr_ring_push(const float *logits, uint32_t T, uint32_t C, uint32_t left, uint32_t right, float *ring, uint32_t ring_rows,
                     uint32_t first_row, uint32_t zero_rows, rn_stream_t stream) {
    RN_REQUIRE(logits && ring, "asr_ring_push: null pointer");
    RN_REQUIRE(C >= 1 && C <= 65536u, "asr_ring_push: C must be 1 .. 65536");
    RN_REQUIRE(left <= right && right <= T, "asr_ring_push: rows %u .. %u of %u", left, right, T);
    RN_REQUIRE(ring_rows >= 16u && ring_rows <= (1u << 24), "asr_ring_push: ring_rows must be 16 .. 2^24");
    RN_REQUIRE(first_row < ring_rows, "asr_ring_push: first_row %u of %u", first_row, ring_rows);
    RN_REQUIRE((uint64_t)(right - left) + zero_rows <= ring_rows, "asr_ring_push: %u rows and %u zero rows into a ring of %u", right - left,
               zero_rows, ring_rows);
    const size_t total = (size_t)(right - left + zero_rows) * C;
    if (total == 0) return RN_OK;
    hipLaunchKernelGGL(k_ring_push, dim3((uint32_t)((total + 255u) / 256u)), dim3(256), 0, as_stream(stream), logits, C, left, right - left,
                       ring, ring_rows, first_row, zero_rows);
    return check_launch("asr_ring_push");
}

int rn_asr_ring_window(const float *ring, uint32_t ring_rows, uint32_t C, uint32_t k, uint32_t n_slices, float *out, rn_stream_t stream) {
    RN_REQUIRE(ring && out, "asr_ring_window: null pointer");
    RN_REQUIRE(C >= 1 && C <= 65536u, "asr_ring_window: C must be 1 .. 65536");
    RN_REQUIRE(ring_rows >= 16u && ring_rows <= (1u << 24), "asr_ring_window: ring_rows must be 16 .. 2^24");
    hipLaunchKernelGGL(k_ring_window, dim3(div_up(8u * C * 16u, 256u)), dim3(256), 0, as_stream(stream), ring, ring_rows, C, k, n_slices, out);
    return check_launch("asr_ring_window");
}

}  // extern "C"
