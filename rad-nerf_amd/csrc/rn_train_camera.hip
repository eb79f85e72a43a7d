// rn_train_camera.hip -- the pose code of --train_camera around the training step (C ABI: include/radnerf_train.h).  What is
// replaced: nerf/renderer.py:170-174 under autograd -- camera_dT[index], camera_dR[index], / 180 * pi + 1e-8,
// euler_angles_to_matrix (cos, sin, ones, zeros, three stacks, two matmuls), rays_o + dT, rays_d @ R and the backward of all of it,
// which ends in two index_put passes: ~30 small launches each way for 12 numbers of real work.  Here:
//
//   k_camera_rays_forward   one lane per ray: the row's R and dT from uniform loads (every lane works out the same R: 3 sin/cos
//                           and 54 multiplies hide behind the ray's own loads), 24 B read and 24 B written per ray            1 launch
//   k_camera_rays_partial   one lane per ray: the 3 + 9 products g_o[n], d[n][i] g_d[n][j], a shuffle tree over the wave, the
//                           four waves' sums added in wave order, 12 floats per 256-ray workgroup into the workspace          1 launch
//   k_camera_rays_finish    one workgroup: the workgroups' partials summed in double in a fixed order, the closed-form angle
//                           gradient (rn_camera_dev.h), and BOTH gradient tables written whole -- zeros in every other row     1 launch
//
// No float atomics and no dependence on dispatch order: two runs give the same bits.  All three are latency-bound (~100 KB moved
// for 4096 rays); nothing here is tuned beyond coalesced 12-byte rows.  A row index outside [-n_rows, n_rows) reads and writes
// nothing outside the tables: the rays pass through unchanged and both gradients are zero everywhere.
#include "rn_common.h"

#include "rn_camera_dev.h"

#include "../../include/radnerf_train.h"

namespace rn {
namespace cam {

constexpr uint32_t kThreads = 256;   // rays per workgroup, one lane each
constexpr uint32_t kSums = 12;       // sum g_o [3] | G = d^T g_d [3][3]
constexpr uint32_t kSlices = 16;     // k_camera_rays_finish: slices of the workgroup list summed side by side, then in slice order
static_assert(kThreads == kSlices * kSlices && kSums <= kSlices, "k_camera_rays_finish: one thread per (slice, sum)");

struct f3 { float x, y, z; };
__device__ __forceinline__ f3 load3(const float *__restrict__ rows, size_t n) { return *reinterpret_cast<const f3 *>(rows + 3 * n); }
__device__ __forceinline__ void store3(float *__restrict__ rows, size_t n, f3 v) { *reinterpret_cast<f3 *>(rows + 3 * n) = v; }

// The table row of *index: negative values wrap once (as torch's indexing does); -1 = outside the table.
__device__ __forceinline__ int64_t table_row(const int64_t *__restrict__ index, uint32_t n_rows) {
    int64_t r = *index;
    if (r < 0) r += (int64_t)n_rows;
    return (r >= 0 && r < (int64_t)n_rows) ? r : -1;
}

__global__ void __launch_bounds__(kThreads)
k_camera_rays_forward(const float *__restrict__ rays_o, const float *__restrict__ rays_d, const float *__restrict__ camera_dT,
                      const float *__restrict__ camera_dR, const int64_t *__restrict__ index, uint32_t n_rows, uint32_t N,
                      float *__restrict__ out_o, float *__restrict__ out_d) {
    const uint32_t n = blockIdx.x * kThreads + threadIdx.x;
    if (n >= N) return;
    const int64_t row = table_row(index, n_rows);
    const f3 o = load3(rays_o, n), d = load3(rays_d, n);
    if (row < 0) {
        store3(out_o, n, o);
        store3(out_d, n, d);
        return;
    }
    const float *dT = camera_dT + 3 * row;
    float a[3], R[9], od[3];
    pose_angles(camera_dR + 3 * row, a);
    pose_matrix(a, R);
    const float dv[3] = {d.x, d.y, d.z};
    rotate_row(dv, R, od);
    store3(out_o, n, f3{o.x + dT[0], o.y + dT[1], o.z + dT[2]});
    store3(out_d, n, f3{od[0], od[1], od[2]});
}

__global__ void __launch_bounds__(kThreads)
k_camera_rays_partial(const float *__restrict__ grad_o, const float *__restrict__ grad_d, const float *__restrict__ rays_d, uint32_t N,
                      float *__restrict__ partial) {
    __shared__ float lds[kThreads / kWave][kSums];
    const uint32_t n = blockIdx.x * kThreads + threadIdx.x;
    float v[kSums];
#pragma unroll
    for (uint32_t q = 0; q < kSums; q++) v[q] = 0.0f;
    if (n < N) {
        const f3 go = load3(grad_o, n), gd = load3(grad_d, n), d = load3(rays_d, n);
        v[0] = go.x; v[1] = go.y; v[2] = go.z;
        v[3] = d.x * gd.x; v[4] = d.x * gd.y; v[5] = d.x * gd.z;
        v[6] = d.y * gd.x; v[7] = d.y * gd.y; v[8] = d.y * gd.z;
        v[9] = d.z * gd.x; v[10] = d.z * gd.y; v[11] = d.z * gd.z;
    }
#pragma unroll
    for (uint32_t q = 0; q < kSums; q++) {
        const float s = wave_sum(v[q]);
        if ((threadIdx.x & 63u) == 0) lds[threadIdx.x >> 6][q] = s;
    }
    __syncthreads();
    if (threadIdx.x < kSums) {
        float s = lds[0][threadIdx.x];
        for (uint32_t w = 1; w < kThreads / kWave; w++) s += lds[w][threadIdx.x];
        partial[(size_t)blockIdx.x * kSums + threadIdx.x] = s;
    }
}

__global__ void __launch_bounds__(kThreads)
k_camera_rays_finish(const float *__restrict__ partial, uint32_t n_partials, const float *__restrict__ camera_dR,
                     const int64_t *__restrict__ index, uint32_t n_rows, float *__restrict__ grad_dT, float *__restrict__ grad_dR) {
    __shared__ double slices[kSlices][kSlices];
    __shared__ float row_grads[6];
    const uint32_t q = threadIdx.x % kSlices, sl = threadIdx.x / kSlices;   // kThreads == kSlices * kSlices
    const int64_t row = table_row(index, n_rows);
    double s = 0.0;
    if (q < kSums)
        for (uint32_t b = sl; b < n_partials; b += kSlices) s += (double)partial[(size_t)b * kSums + q];
    slices[sl][q] = s;
    __syncthreads();
    if (threadIdx.x == 0 && row >= 0) {
        double sum[kSums];
        for (uint32_t k = 0; k < kSums; k++) {
            double t = slices[0][k];
            for (uint32_t i = 1; i < kSlices; i++) t += slices[i][k];
            sum[k] = t;
        }
        float a[3], ga[3];
        pose_angles(camera_dR + 3 * row, a);
        pose_angle_grads(sum + 3, a, ga);
        for (int k = 0; k < 3; k++) {
            row_grads[k] = (float)sum[k];
            row_grads[3 + k] = ga[k] * pose_angle_scale();
        }
    }
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < 3u * n_rows; e += kThreads) {
        const bool mine = row >= 0 && e / 3u == (uint32_t)row;
        grad_dT[e] = mine ? row_grads[e % 3u] : 0.0f;
        grad_dR[e] = mine ? row_grads[3u + e % 3u] : 0.0f;
    }
}

}  // namespace cam
}  // namespace rn

using namespace rn;

extern "C" {

size_t rn_camera_rays_workspace(uint32_t N) {
    const size_t blocks = div_up(N, cam::kThreads);
    return (blocks ? blocks : 1) * cam::kSums * sizeof(float);
}

int rn_camera_rays_forward(const float *rays_o, const float *rays_d, const float *camera_dT, const float *camera_dR, const int64_t *index,
                           uint32_t n_rows, uint32_t N, float *out_rays_o, float *out_rays_d, rn_stream_t stream) {
    if (N == 0) return RN_OK;
    RN_REQUIRE(rays_o && rays_d && camera_dT && camera_dR && index && out_rays_o && out_rays_d, "camera_rays_forward: null pointer");
    RN_REQUIRE(n_rows > 0, "camera_rays_forward: the pose tables have no rows");
    hipLaunchKernelGGL(cam::k_camera_rays_forward, dim3(div_up(N, cam::kThreads)), dim3(cam::kThreads), 0, as_stream(stream), rays_o, rays_d,
                       camera_dT, camera_dR, index, n_rows, N, out_rays_o, out_rays_d);
    return check_launch("camera_rays_forward");
}

int rn_camera_rays_backward(const float *grad_rays_o, const float *grad_rays_d, const float *rays_d, const float *camera_dR,
                            const int64_t *index, uint32_t n_rows, uint32_t N, float *grad_dT, float *grad_dR, void *workspace,
                            rn_stream_t stream) {
    RN_REQUIRE(camera_dR && index && grad_dT && grad_dR, "camera_rays_backward: null pointer");
    RN_REQUIRE(n_rows > 0, "camera_rays_backward: the pose tables have no rows");
    RN_REQUIRE(N == 0 || (grad_rays_o && grad_rays_d && rays_d && workspace), "camera_rays_backward: null pointer");
    RN_REQUIRE(((uintptr_t)workspace & 3u) == 0, "camera_rays_backward: the workspace must be 4-byte aligned");
    const uint32_t blocks = div_up(N, cam::kThreads);
    float *partial = static_cast<float *>(workspace);
    if (blocks)
        hipLaunchKernelGGL(cam::k_camera_rays_partial, dim3(blocks), dim3(cam::kThreads), 0, as_stream(stream), grad_rays_o, grad_rays_d, rays_d,
                           N, partial);
    hipLaunchKernelGGL(cam::k_camera_rays_finish, dim3(1), dim3(cam::kThreads), 0, as_stream(stream), partial, blocks, camera_dR, index, n_rows,
                       grad_dT, grad_dR);
    return check_launch("camera_rays_backward");
}

}  // extern "C"
