// rn_ray_dev.h -- what the ray loop does per ray around the DDA walk (rn_dda_dev.h), each piece written once: the pinhole ray of a
// pixel, its background coordinate, the pose 6-vector, the ray/box test, the order of the alive list, the reset of a ray's accumulators, the inference compositor.  Used by
// rn_rays.hip, rn_raymarching.hip (the per-operator kernels) and rn_head_loop.hip (the device-resident loop): the two engines
// produce the same bits because they run the same expressions.  -ffp-contract=off: the expressions round as written.
#pragma once

#include "rn_dda_dev.h"

#include <float.h>

namespace rn {

// get_rays (nerf/utils.py:249-333, N = -1) for pixel `ray` of a W-wide image: pose = [3,4] / [4,4] row-major cam2world.
__device__ __forceinline__ void pinhole_ray(uint32_t ray, uint32_t W, float fx, float fy, float cx, float cy,
                                            const float *__restrict__ pose, float *__restrict__ o, float *__restrict__ d) {
    const uint32_t r = ray / W, c = ray - r * W;
    // i = col + 0.5, j = row + 0.5 (:268-270); xs = (i - cx) / fx * zs, ys = (j - cy) / fy * zs, zs = 1 (:320-322)
    const float x = ((float)c + 0.5f - cx) / fx, y = ((float)r + 0.5f - cy) / fy, z = 1.0f;
    const float norm = sqrtf(x * x + y * y + z * z);  // :324
    const float ux = x / norm, uy = y / norm, uz = z / norm;
#pragma unroll
    for (int k = 0; k < 3; k++) {  // rays_d = directions @ R^T (:325): row k of R
        d[k] = ux * pose[k * 4] + uy * pose[k * 4 + 1] + uz * pose[k * 4 + 2];
        o[k] = pose[k * 4 + 3];  // :327
    }
}

// get_bg_coords (nerf/utils.py:240-245) for pixel (row r, column c): [-1, 1], component 0 along the rows -- arange / (n - 1) * 2 - 1
__device__ __forceinline__ void bg_coord_of(uint32_t r, uint32_t c, uint32_t H, uint32_t W, float &x, float &y) {
    x = (float)r / (float)(H - 1u) * 2.0f - 1.0f;
    y = (float)c / (float)(W - 1u) * 2.0f - 1.0f;
}

// convert_poses (nerf/utils.py:231-237) of one cam2world matrix m [4,4]: (XYZ euler angles of the rotation, translation);
// matrix_to_euler_angles(R, 'XYZ') (:130-169) = (atan2(-R12, R22), asin(R02), atan2(-R01, R00))
__device__ __forceinline__ void pose6_of(const float *__restrict__ m, float *__restrict__ o) {
    o[0] = atan2f(-m[1 * 4 + 2], m[2 * 4 + 2]);
    o[1] = asinf(m[0 * 4 + 2]);
    o[2] = atan2f(-m[0 * 4 + 1], m[0 * 4 + 0]);
    o[3] = m[3];
    o[4] = m[7];
    o[5] = m[11];
}

// near / far of a ray against the box  (raymarching.cu:91-145); FLT_MAX for both when the ray misses
__device__ __forceinline__ void near_far_of(const float *__restrict__ o, const float *__restrict__ d, const float *__restrict__ aabb,
                                            float min_near, float &near_out, float &far_out) {
    const float ox = o[0], oy = o[1], oz = o[2];
    const float dx = d[0], dy = d[1], dz = d[2];
    const float rdx = 1 / dx, rdy = 1 / dy, rdz = 1 / dz;

    float near = (aabb[0] - ox) * rdx, far = (aabb[3] - ox) * rdx;
    if (near > far) { float c = near; near = far; far = c; }
    float near_y = (aabb[1] - oy) * rdy, far_y = (aabb[4] - oy) * rdy;
    if (near_y > far_y) { float c = near_y; near_y = far_y; far_y = c; }

    bool miss = (near > far_y || near_y > far);
    if (!miss) {
        if (near_y > near) near = near_y;
        if (far_y < far) far = far_y;
        float near_z = (aabb[2] - oz) * rdz, far_z = (aabb[5] - oz) * rdz;
        if (near_z > far_z) { float c = near_z; near_z = far_z; far_z = c; }
        miss = (near > far_z || near_z > far);
        if (!miss) {
            if (near_z > near) near = near_z;
            if (far_z < far) far = far_z;
            if (near < min_near) near = min_near;
        }
    }
    near_out = miss ? FLT_MAX : near;
    far_out = miss ? FLT_MAX : far;
}

// Slot n of a frame's first alive list: ray n, or (order_w = image width) the rays of 8 x 8 pixel blocks together, so that the 64
// samples of a wave and the tiles of a CU cover a compact patch of the image instead of a one-pixel-high strip -- more of their
// grid rows coincide.  Rays are independent, so the order changes no pixel.
__device__ __forceinline__ uint32_t alive_order(uint32_t n, uint32_t order_w) {
    if (!order_w) return n;
    const uint32_t t = n >> 6, within = n & 63u, tiles_x = order_w >> 3;
    return ((t / tiles_x) * 8u + (within >> 3)) * order_w + (t % tiles_x) * 8u + (within & 7u);
}
// The width to launch with: the block order needs an image of whole 8 x 8 blocks, otherwise the plain order (0) is used.
static inline uint32_t usable_order_w(uint32_t order_w, uint32_t N) {
    return (order_w && (order_w % 8u || N % order_w || (N / order_w) % 8u)) ? 0u : order_w;
}

// A ray enters the loop (renderer.py:229-237): near / far, its walk starts at near, its accumulators start from zero.
__device__ __forceinline__ void begin_ray(uint32_t ray, const float *__restrict__ o, const float *__restrict__ d,
                                          const float *__restrict__ aabb, float min_near, float *__restrict__ nears,
                                          float *__restrict__ fars, float *__restrict__ rays_t, float *__restrict__ weights_sum,
                                          float *__restrict__ depth, float *__restrict__ image, float &near, float &far) {
    near_far_of(o, d, aabb, min_near, near, far);
    nears[ray] = near; fars[ray] = far;
    rays_t[ray] = near;
    weights_sum[ray] = 0.0f; depth[ray] = 0.0f;
    image[(size_t)ray * 3] = 0.0f; image[(size_t)ray * 3 + 1] = 0.0f; image[(size_t)ray * 3 + 2] = 0.0f;
}

// Inference compositor  (raymarching.cu:942-1029) for entry n of the alive list: adds the entry's n_step samples to its ray's
// accumulators; a ray that ended (an unused slot, or transmittance below T_thresh) leaves the list (entry = -1), one that
// goes on keeps its t.  Returns whether the ray survives.
__device__ __forceinline__ bool composite_ray(uint32_t n, uint32_t n_step, float T_thresh, int32_t *__restrict__ rays_alive,
                                              float *__restrict__ rays_t, const float *__restrict__ sigmas,
                                              const float *__restrict__ rgbs, const float *__restrict__ deltas,
                                              float *__restrict__ weights_sum, float *__restrict__ depth, float *__restrict__ image) {
    const int index = rays_alive[n];
    const float *sg = sigmas + (size_t)n * n_step;
    const float *rg = rgbs + (size_t)n * n_step * 3;
    const float *dl = deltas + (size_t)n * n_step * 2;

    float t = rays_t[index];
    float weight_sum = weights_sum[index];
    float d = depth[index];
    float r = image[index * 3], g = image[index * 3 + 1], b = image[index * 3 + 2];

    uint32_t step = 0;
    while (step < n_step) {
        if (dl[0] == 0) break;
        const float alpha = 1.0f - __expf(-sg[0] * dl[0]);
        const float T = 1 - weight_sum;
        const float weight = alpha * T;
        weight_sum += weight;
        t = dl[1];
        d += weight * t;
        r += weight * rg[0]; g += weight * rg[1]; b += weight * rg[2];
        if (T < T_thresh) break;
        sg++; rg += 3; dl += 2;
        step++;
    }
    const bool survive = !(step < n_step);
    if (survive) rays_t[index] = t;
    else rays_alive[n] = -1;

    weights_sum[index] = weight_sum;
    depth[index] = d;
    image[index * 3] = r; image[index * 3 + 1] = g; image[index * 3 + 2] = b;
    return survive;
}

}  // namespace rn
