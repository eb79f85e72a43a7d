// rn_train_sched.hip -- what validation under the averaged weights needs besides the render (gfx950): the exchange of weights and
// shadows (torch_ema's store() + copy_to(), and restore(), without a third copy of the model) and the squared error of a frame
// (Trainer.evaluate_one_epoch's loss and PSNRMeter, nerf/utils.py:402-430, :1220-1300) summed on the device in a fixed order.
// The schedule and the EMA update themselves live in the Adam launches of rn_train.hip.
#include "rn_common.h"

#include "../../include/radnerf_train.h"

namespace rn {

constexpr int kSwapBlock = 256, kSwapPerThread = 4;
constexpr int kSwapChunk = kSwapBlock * kSwapPerThread;   // elements per workgroup
constexpr int kSwapMaxTensors = 48;                       // pointers travel as kernel arguments, as in k_adam

struct SwapArgs {
    float *a[kSwapMaxTensors], *b[kSwapMaxTensors];
    uint32_t n[kSwapMaxTensors], first_block[kSwapMaxTensors + 1];
    uint32_t count;
};

__global__ void __launch_bounds__(kSwapBlock) k_param_swap(SwapArgs s) {
    uint32_t t = 0;
    while (t + 1 < s.count && blockIdx.x >= s.first_block[t + 1]) t++;
    const uint32_t base = (blockIdx.x - s.first_block[t]) * kSwapChunk + threadIdx.x * kSwapPerThread;
    const uint32_t n = s.n[t];
    if (base >= n) return;
    float *a = s.a[t] + base, *b = s.b[t] + base;
    if (base + 4 <= n && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15u) == 0) {
        const float4 A = *reinterpret_cast<float4 *>(a), B = *reinterpret_cast<float4 *>(b);
        *reinterpret_cast<float4 *>(a) = B;
        *reinterpret_cast<float4 *>(b) = A;
    } else {
        for (uint32_t i = 0; i < 4 && base + i < n; i++) {
            const float A = a[i], B = b[i];
            a[i] = B;
            b[i] = A;
        }
    }
}

constexpr int kErrBlock = 256;
constexpr uint32_t kErrPixels = 1024;      // pixels per workgroup of the first pass

// First pass: workgroup w sums pixels [1024 w, 1024 w + 1024).  A thread adds its pixels in ascending order, the workgroup its
// threads in block_sum_first's order; part[3 w + ..] = all values | values inside the rect | how many of the latter.
__global__ void __launch_bounds__(kErrBlock) k_image_error_partial(const float *__restrict__ pred, const float *__restrict__ target,
                                                                   uint32_t n_px, uint32_t W, const int32_t *__restrict__ rect,
                                                                   double *__restrict__ part) {
    __shared__ double red_all[kErrBlock / kWave], red_in[kErrBlock / kWave], red_cnt[kErrBlock / kWave];
    int32_t xmin = 0, xmax = 0, ymin = 0, ymax = 0;          // no rect: nothing is inside
    if (rect) { xmin = rect[0]; xmax = rect[1]; ymin = rect[2]; ymax = rect[3]; }
    const uint32_t first = blockIdx.x * kErrPixels;
    const uint32_t end = n_px - first < kErrPixels ? n_px : first + kErrPixels;
    double all = 0.0, in = 0.0, cnt = 0.0;
    for (uint32_t px = first + threadIdx.x; px < end; px += kErrBlock) {
        const int32_t row = (int32_t)(px / W), col = (int32_t)(px - (uint32_t)row * W);
        const bool inside = row >= xmin && row < xmax && col >= ymin && col < ymax;
        double sq = 0.0;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float d = pred[(size_t)px * 3 + c] - target[(size_t)px * 3 + c];     // in fp32, as torch's pred - truth
            sq += (double)d * (double)d;
        }
        all += sq;
        if (inside) { in += sq; cnt += 3.0; }
    }
    const double t_all = block_sum_first<double, kErrBlock>(all, red_all);
    const double t_in = block_sum_first<double, kErrBlock>(in, red_in);
    const double t_cnt = block_sum_first<double, kErrBlock>(cnt, red_cnt);
    if (threadIdx.x == 0) {
        part[(size_t)blockIdx.x * 3] = t_all;
        part[(size_t)blockIdx.x * 3 + 1] = t_in;
        part[(size_t)blockIdx.x * 3 + 2] = t_cnt;
    }
}

// Second pass, one workgroup: thread k adds partials k, k + 256, .. in ascending order, then the same workgroup sum.
__global__ void __launch_bounds__(kErrBlock) k_image_error_final(const double *__restrict__ part, uint32_t n_part, uint32_t n_px,
                                                                 double *__restrict__ out) {
    __shared__ double red_all[kErrBlock / kWave], red_in[kErrBlock / kWave], red_cnt[kErrBlock / kWave];
    double all = 0.0, in = 0.0, cnt = 0.0;
    for (uint32_t w = threadIdx.x; w < n_part; w += kErrBlock) {
        all += part[(size_t)w * 3];
        in += part[(size_t)w * 3 + 1];
        cnt += part[(size_t)w * 3 + 2];
    }
    const double t_all = block_sum_first<double, kErrBlock>(all, red_all);
    const double t_in = block_sum_first<double, kErrBlock>(in, red_in);
    const double t_cnt = block_sum_first<double, kErrBlock>(cnt, red_cnt);
    if (threadIdx.x == 0) {
        out[0] = t_all;
        out[1] = t_in;
        out[2] = 3.0 * (double)n_px;
        out[3] = t_cnt;
    }
}

}  // namespace rn

using namespace rn;

extern "C" {

int rn_param_swap(float *const *a, float *const *b, const uint32_t *numel, uint32_t count, rn_stream_t stream) {
    if (count == 0) return RN_OK;
    RN_REQUIRE(a && b && numel, "param_swap: null pointer (tensor lists)");
    for (uint32_t i = 0; i < count; i++) {          // everything is checked before the first launch
        RN_REQUIRE(numel[i] == 0 || (a[i] && b[i]), "param_swap: null pointer in tensor %u", i);
        RN_REQUIRE(numel[i] == 0 || a[i] + numel[i] <= b[i] || b[i] + numel[i] <= a[i], "param_swap: tensor %u overlaps its partner", i);
    }
    for (uint32_t at = 0; at < count; at += kSwapMaxTensors) {
        SwapArgs s{};
        uint32_t blocks = 0, k = 0;
        for (; k < (uint32_t)kSwapMaxTensors && at + k < count; k++) {
            s.a[k] = a[at + k]; s.b[k] = b[at + k]; s.n[k] = numel[at + k];
            s.first_block[k] = blocks;
            blocks += div_up(numel[at + k], kSwapChunk);
        }
        s.first_block[k] = blocks;
        s.count = k;
        if (blocks) hipLaunchKernelGGL(k_param_swap, dim3(blocks), dim3(kSwapBlock), 0, as_stream(stream), s);
    }
    return check_launch("param_swap");
}

size_t rn_image_error_workspace(uint32_t H, uint32_t W) {
    const uint64_t n_px = (uint64_t)H * W;
    if (n_px == 0 || n_px > (1ull << 30)) return 0;
    return (size_t)div_up((uint32_t)n_px, kErrPixels) * 3 * sizeof(double);
}

int rn_image_error(const float *pred, const float *target, uint32_t H, uint32_t W, const int32_t *rect, void *workspace, double *out,
                   rn_stream_t stream) {
    RN_REQUIRE(H > 0 && W > 0 && (uint64_t)H * W <= (1ull << 30), "image_error: 0 < H * W <= 2^30 is required");
    RN_REQUIRE(pred && target && workspace && out, "image_error: null pointer");
    RN_REQUIRE(((uintptr_t)workspace & 7u) == 0 && ((uintptr_t)out & 7u) == 0, "image_error: workspace and out must be 8-byte aligned");
    const uint32_t n_px = H * W, n_part = div_up(n_px, kErrPixels);
    double *part = static_cast<double *>(workspace);
    hipLaunchKernelGGL(k_image_error_partial, dim3(n_part), dim3(kErrBlock), 0, as_stream(stream), pred, target, n_px, W, rect, part);
    hipLaunchKernelGGL(k_image_error_final, dim3(1), dim3(kErrBlock), 0, as_stream(stream), part, n_part, n_px, out);
    return check_launch("image_error");
}

}  // extern "C"
