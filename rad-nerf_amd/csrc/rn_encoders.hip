// rn_encoders.hip -- spherical-harmonics and frequency encoders for gfx950.
//
// Behaviour: shencoder/src/shencoder.cu:28-382 and freqencoder/src/freqencoder.cu:30-94 of the
// reference.  Both are streaming kernels (12 B in / 64 B out per sample for the degree-4 SH the
// model uses): one sample per lane, the whole output row built in registers and written with
// 16-byte stores.
#include "rn_sh_dev.h"

namespace rn {

constexpr int kBlockE = 256;

template <uint32_t N>
__device__ __forceinline__ void store_f32_row(float *dst, const float *v) {
    if constexpr (N % 4 == 0) {
#pragma unroll
        for (uint32_t i = 0; i < N / 4; i++)
            reinterpret_cast<float4 *>(dst)[i] = make_float4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
    } else {
#pragma unroll
        for (uint32_t i = 0; i < N; i++) dst[i] = v[i];
    }
}

// shencoder.cu:28-355
template <uint32_t C>
__global__ void __launch_bounds__(kBlockE)
k_sh_forward(const float *__restrict__ inputs, float *__restrict__ outputs, uint32_t B, uint32_t D,
             float *__restrict__ dy_dx) {
    const uint32_t b = blockIdx.x * kBlockE + threadIdx.x;
    if (b >= B) return;
    constexpr uint32_t C2 = C * C;
    const float x = inputs[(size_t)b * D], y = inputs[(size_t)b * D + 1], z = inputs[(size_t)b * D + 2];
    float o[C2];
    sh_basis<C>(x, y, z, o);
    store_f32_row<C2>(outputs + (size_t)b * C2, o);
    if (dy_dx) {
        float *g = dy_dx + (size_t)b * D * C2;  // rows dx | dy | dz  (shencoder.cu:126-128)
        sh_jac<C, 0>(x, y, z, o); store_f32_row<C2>(g, o);
        sh_jac<C, 1>(x, y, z, o); store_f32_row<C2>(g + C2, o);
        sh_jac<C, 2>(x, y, z, o); store_f32_row<C2>(g + 2 * C2, o);
    }
}

// shencoder.cu:359-382: grad_inputs[b,d] += sum_ch grad[b,ch] * dy_dx[b,d,ch]
__global__ void __launch_bounds__(kBlockE)
k_sh_backward(const float *__restrict__ grad, uint32_t B, uint32_t D, uint32_t C2,
              const float *__restrict__ dy_dx, float *__restrict__ grad_inputs) {
    const uint32_t t = blockIdx.x * kBlockE + threadIdx.x;
    const uint32_t b = t / D;
    if (b >= B) return;
    const uint32_t d = t - b * D;
    const float *g = grad + (size_t)b * C2;
    const float *dd = dy_dx + (size_t)b * D * C2 + (size_t)d * C2;
    float acc = grad_inputs[t];
    for (uint32_t ch = 0; ch < C2; ch++) acc += g[ch] * dd[ch];
    grad_inputs[t] = acc;
}

// freqencoder.cu:30-58.  One SAMPLE per lane (the reference uses one output element per thread):
// the lane builds its C = D + 2*D*deg outputs and stores them contiguously.
__global__ void __launch_bounds__(kBlockE)
k_freq_forward(const float *__restrict__ inputs, uint32_t B, uint32_t D, uint32_t deg, uint32_t C,
               float *__restrict__ outputs) {
    const uint32_t b = blockIdx.x * kBlockE + threadIdx.x;
    if (b >= B) return;
    const float *in = inputs + (size_t)b * D;
    float *out = outputs + (size_t)b * C;
    constexpr float kHalfPi = 3.141592653589793f / 2;
    for (uint32_t d = 0; d < D; d++) {
        const float x = in[d];
        out[d] = x;
        for (uint32_t f = 0; f < deg; f++) {
            const float a = scalbnf(x, (int)f);
            out[D + (2 * f) * D + d] = sinf(a);                // col = 2f,   phase 0
            out[D + (2 * f + 1) * D + d] = sinf(a + kHalfPi);  // col = 2f+1, phase pi/2
        }
    }
}

// freqencoder.cu:63-94
__global__ void __launch_bounds__(kBlockE)
k_freq_backward(const float *__restrict__ grad, const float *__restrict__ outputs, uint32_t B, uint32_t D,
                uint32_t deg, uint32_t C, float *__restrict__ grad_inputs) {
    const uint32_t t = blockIdx.x * kBlockE + threadIdx.x;
    if (t >= B * D) return;
    const uint32_t b = t / D, d = t - b * D;
    const float *g = grad + (size_t)b * C;
    const float *o = outputs + (size_t)b * C;
    float result = g[d];
    g += D;
    o += D;
    for (uint32_t f = 0; f < deg; f++) {
        result += scalbnf(1.0f, (int)f) * (g[d] * o[D + d] - g[D + d] * o[d]);
        g += 2 * D;
        o += 2 * D;
    }
    grad_inputs[t] = result;
}

}  // namespace rn

using namespace rn;

extern "C" {

int rn_sh_encode_forward(const float *inputs, float *outputs, uint32_t B, uint32_t D, uint32_t C, float *dy_dx,
                         rn_stream_t stream) {
    if (B == 0) return RN_OK;
    RN_REQUIRE(inputs && outputs, "sh_encode_forward: null pointer");
    RN_REQUIRE(D == 3, "SH encoder only support input dim == 3");  // sphere_harmonics.py:69
    RN_REQUIRE(C >= 1 && C <= 8, "SH encoder only supports degree in [1, 8]");
    const dim3 grid(div_up(B, kBlockE)), block(kBlockE);
    hipStream_t s = as_stream(stream);
    switch (C) {
        case 1: hipLaunchKernelGGL(k_sh_forward<1>, grid, block, 0, s, inputs, outputs, B, D, dy_dx); break;
        case 2: hipLaunchKernelGGL(k_sh_forward<2>, grid, block, 0, s, inputs, outputs, B, D, dy_dx); break;
        case 3: hipLaunchKernelGGL(k_sh_forward<3>, grid, block, 0, s, inputs, outputs, B, D, dy_dx); break;
        case 4: hipLaunchKernelGGL(k_sh_forward<4>, grid, block, 0, s, inputs, outputs, B, D, dy_dx); break;
        case 5: hipLaunchKernelGGL(k_sh_forward<5>, grid, block, 0, s, inputs, outputs, B, D, dy_dx); break;
        case 6: hipLaunchKernelGGL(k_sh_forward<6>, grid, block, 0, s, inputs, outputs, B, D, dy_dx); break;
        case 7: hipLaunchKernelGGL(k_sh_forward<7>, grid, block, 0, s, inputs, outputs, B, D, dy_dx); break;
        case 8: hipLaunchKernelGGL(k_sh_forward<8>, grid, block, 0, s, inputs, outputs, B, D, dy_dx); break;
    }
    return check_launch("sh_encode_forward");
}

int rn_sh_encode_backward(const float *grad, const float *inputs, uint32_t B, uint32_t D, uint32_t C,
                          const float *dy_dx, float *grad_inputs, rn_stream_t stream) {
    if (B == 0) return RN_OK;
    (void)inputs;
    RN_REQUIRE(grad && dy_dx && grad_inputs, "sh_encode_backward: null pointer");
    RN_REQUIRE(D == 3 && C >= 1 && C <= 8, "sh_encode_backward: D must be 3 and degree in [1, 8]");
    hipLaunchKernelGGL(k_sh_backward, dim3(div_up(B * D, kBlockE)), dim3(kBlockE), 0, as_stream(stream), grad, B, D,
                       C * C, dy_dx, grad_inputs);
    return check_launch("sh_encode_backward");
}

int rn_freq_encode_forward(const float *inputs, uint32_t B, uint32_t D, uint32_t deg, uint32_t C, float *outputs,
                           rn_stream_t stream) {
    if (B == 0) return RN_OK;
    RN_REQUIRE(inputs && outputs, "freq_encode_forward: null pointer");
    RN_REQUIRE(D >= 1 && C == D + 2 * D * deg, "freq_encode_forward: output_dim must equal D + 2*D*deg");
    hipLaunchKernelGGL(k_freq_forward, dim3(div_up(B, kBlockE)), dim3(kBlockE), 0, as_stream(stream), inputs, B, D,
                       deg, C, outputs);
    return check_launch("freq_encode_forward");
}

int rn_freq_encode_backward(const float *grad, const float *outputs, uint32_t B, uint32_t D, uint32_t deg, uint32_t C,
                            float *grad_inputs, rn_stream_t stream) {
    if (B == 0) return RN_OK;
    RN_REQUIRE(grad && outputs && grad_inputs, "freq_encode_backward: null pointer");
    RN_REQUIRE(D >= 1 && C == D + 2 * D * deg, "freq_encode_backward: output_dim must equal D + 2*D*deg");
    hipLaunchKernelGGL(k_freq_backward, dim3(div_up(B * D, kBlockE)), dim3(kBlockE), 0, as_stream(stream), grad,
                       outputs, B, D, deg, C, grad_inputs);
    return check_launch("freq_encode_backward");
}

}  // extern "C"
