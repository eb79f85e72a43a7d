// rn_resample.hip -- any PCM audio to the mono float signal at another rate: the step the reference leaves to soundfile and
// resampy (nerf/asr.py:255-264).  See include/radnerf_fused.h for the arithmetic and rn_resample_dev.h for the tile and the table.
//
//   k_pcm_decode   one frame per thread: the first channel's bytes, one byte load each (the buffer has byte alignment only), put
//                  together and scaled
//   k_resample     one output per thread, kTile per workgroup: the workgroup's input span into LDS (zeros outside the buffer), then
//                  one fmaf chain over the taps, k ascending, from 0
//
// No float atomics, no cross-lane sums: an output's bits are a function of its index and the signal alone.
#include "rn_resample_dev.h"

namespace rn {
namespace resample {

__global__ __launch_bounds__(256) void k_pcm_decode(const uint8_t *__restrict__ raw, uint64_t n_frames, uint32_t frame_bytes, int format,
                                                    float *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_frames) return;
    const uint8_t *b = raw + i * frame_bytes;
    float v;
    switch (format) {
        case RN_PCM_U8:
            v = (float)((int32_t)b[0] - 128) * 0.0078125f;
            break;
        case RN_PCM_S16LE:
            v = (float)(int16_t)((uint32_t)b[0] | ((uint32_t)b[1] << 8)) * 0.000030517578125f;
            break;
        case RN_PCM_S24LE: {
            const uint32_t u = ((uint32_t)b[0] << 8) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 24);
            v = (float)((int32_t)u >> 8) * 1.1920928955078125e-07f;
            break;
        }
        case RN_PCM_S32LE: {
            const uint32_t u = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
            v = (float)(int32_t)u * 4.656612873077392578125e-10f;
            break;
        }
        default: {
            const uint32_t u = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
            v = __uint_as_float(u);
            break;
        }
    }
    out[i] = v;
}

__global__ __launch_bounds__(256) void k_resample(const float *__restrict__ x, int64_t n_buf, int64_t origin, const float *__restrict__ table,
                                                  uint32_t L, uint32_t M, uint32_t W, int64_t t0, int64_t n_out, uint32_t span,
                                                  float *__restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) float xs[];
    const int64_t i0 = (int64_t)blockIdx.x * kTile;
    const int64_t first = ((t0 + i0) * (int64_t)M) / (int64_t)L - (int64_t)W;      // input index of xs[0]; the same in every lane
    for (uint32_t e = threadIdx.x; e < span; e += kTile) {
        const int64_t g = first + (int64_t)e - origin;
        xs[e] = (g >= 0 && g < n_buf) ? x[g] : 0.0f;
    }
    __syncthreads();
    const int64_t i = i0 + threadIdx.x;
    if (i >= n_out) return;
    const int64_t tm = (t0 + i) * (int64_t)M;
    const int64_t n = tm / (int64_t)L;
    const uint32_t p = (uint32_t)(tm - n * (int64_t)L);
    const float *xw = xs + (uint32_t)(n - (int64_t)W - first);                        // n - W >= first; the last tap stays below span
    const float *row = table + p;
    const uint32_t taps = 2u * W + 1u;
    float acc = 0.0f;
    for (uint32_t j = 0; j < taps; j++) acc = fmaf(row[(size_t)j * L], xw[j], acc);
    y[i] = acc;
}

}  // namespace resample
}  // namespace rn

using namespace rn;
using namespace rn::resample;

extern "C" {

int rn_pcm_decode(const uint8_t *raw, size_t n_frames, uint32_t channels, int format, float *out, rn_stream_t stream) {
    const uint32_t width = sample_bytes(format);
    RN_REQUIRE(width != 0, "pcm_decode: format %d is not one of RN_PCM_U8 .. RN_PCM_F32LE", format);
    RN_REQUIRE(channels >= 1 && channels <= 4096u, "pcm_decode: channels must be 1 .. 4096, got %u", channels);
    if (n_frames == 0) return RN_OK;
    RN_REQUIRE(raw && out, "pcm_decode: null pointer");
    RN_REQUIRE(n_frames <= ((size_t)1 << 38), "pcm_decode: %zu frames", n_frames);
    const uint64_t blocks = ((uint64_t)n_frames + 255u) / 256u;
    hipLaunchKernelGGL(k_pcm_decode, dim3((uint32_t)blocks), dim3(256), 0, as_stream(stream), raw, (uint64_t)n_frames, channels * width, format,
                       out);
    return check_launch("pcm_decode");
}

int rn_resample(const float *x, size_t n_buf, int64_t origin, const float *table, uint32_t L, uint32_t M, uint32_t W, int64_t t0, size_t n_out,
                float *y, rn_stream_t stream) {
    RN_REQUIRE(L >= 1 && M >= 1 && W >= 1, "resample: L, M, W = %u, %u, %u must all be at least 1", L, M, W);
    RN_REQUIRE(L <= kMaxRatio && M <= kMaxRatio && W <= kMaxW, "resample: L, M <= %u and W <= %u, got %u, %u, %u", kMaxRatio, kMaxW, L, M, W);
    RN_REQUIRE(origin >= 0 && t0 >= 0, "resample: origin and t0 must not be negative");
    const uint64_t span = span_floats(L, M, W);
    RN_REQUIRE(span * sizeof(float) <= kMaxLdsBytes, "resample: a tile's input span of %llu floats does not fit %u bytes of LDS (M / L too large)",
               (unsigned long long)span, kMaxLdsBytes);
    if (n_out == 0) return RN_OK;
    RN_REQUIRE(table && y && (x || n_buf == 0), "resample: null pointer");
    RN_REQUIRE(n_buf <= ((size_t)1 << 40) && n_out <= ((size_t)1 << 38), "resample: n_buf = %zu, n_out = %zu", n_buf, n_out);
    RN_REQUIRE((uint64_t)t0 + n_out <= (uint64_t)INT64_MAX / M, "resample: (t0 + n_out) * M leaves int64");
    const uint64_t blocks = ((uint64_t)n_out + kTile - 1u) / kTile;
    hipLaunchKernelGGL(k_resample, dim3((uint32_t)blocks), dim3(kTile), (size_t)span * sizeof(float), as_stream(stream), x, (int64_t)n_buf, origin,
                       table, L, M, W, t0, (int64_t)n_out, (uint32_t)span, y);
    return check_launch("resample");
}

}  // extern "C"
