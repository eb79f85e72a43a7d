// rn_camera_dev.h -- the pose arithmetic of --train_camera (nerf/renderer.py:170-174), plain functions for host and device:
// the Euler angles of a row of camera_dR, the rotation R = Rx(a0) Ry(a1) Rz(a2) of euler_angles_to_matrix (nerf/utils.py:172-227,
// radnerf/rays.py:51-62), and the gradient of the angles from G = d^T g_d.  No HIP header is needed: a host compiler that defines
// RN_HD away builds the same text (tests/test_camera_pose_abi.py does), the kernels of rn_train_camera.hip include it as it is.
//
// Every product and sum is fp32 and rounded on its own (the tree builds with -ffp-contract=off), summed left to right; only the
// contraction of G with dR/da runs in double, on the double sums the backward kernel hands it: grad_a0 is close to G[2][1] - G[1][2],
// a difference of two sums over all rays.
#pragma once

#include <math.h>

#ifndef RN_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define RN_HD __host__ __device__ inline
#else
#define RN_HD inline
#endif
#endif

namespace rn {
namespace cam {

// a[k] = camera_dR[row][k] / 180 * pi + 1e-8 (nerf/renderer.py:172), each operation rounded to fp32
RN_HD void pose_angles(const float deg[3], float a[3]) {
    for (int k = 0; k < 3; k++) a[k] = deg[k] / 180.0f * 3.14159265358979323846f + 1e-8f;
}

// out = A B, row-major 3 x 3, every entry a[i][0] b[0][j] + a[i][1] b[1][j] + a[i][2] b[2][j] from left to right
RN_HD void mat3_mul(const float A[9], const float B[9], float out[9]) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) out[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}

// The three axis rotations of rays.py:53-58 (deriv = false) or their derivatives in the angle (deriv = true), row-major.
RN_HD void axis_rot(int axis, float angle, bool deriv, float M[9]) {
    const float s0 = sinf(angle), c0 = cosf(angle);
    const float c = deriv ? -s0 : c0, s = deriv ? c0 : s0, one = deriv ? 0.0f : 1.0f;   // d/da (cos, sin, 1) = (-sin, cos, 0)
    for (int e = 0; e < 9; e++) M[e] = 0.0f;
    if (axis == 0) {           // X: (1 0 0 | 0 c -s | 0 s c)
        M[0] = one; M[4] = c; M[5] = -s; M[7] = s; M[8] = c;
    } else if (axis == 1) {    // Y: (c 0 s | 0 1 0 | -s 0 c)
        M[0] = c; M[2] = s; M[4] = one; M[6] = -s; M[8] = c;
    } else {                   // Z: (c -s 0 | s c 0 | 0 0 1)
        M[0] = c; M[1] = -s; M[3] = s; M[4] = c; M[8] = one;
    }
}

// Rx(a0) Ry(a1) Rz(a2) with the factor `which` (0, 1, 2) replaced by its derivative; which < 0: the rotation itself.
RN_HD void pose_product(const float a[3], int which, float R[9]) {
    float X[9], Y[9], Z[9], XY[9];
    axis_rot(0, a[0], which == 0, X);
    axis_rot(1, a[1], which == 1, Y);
    axis_rot(2, a[2], which == 2, Z);
    mat3_mul(X, Y, XY);
    mat3_mul(XY, Z, R);
}

RN_HD void pose_matrix(const float a[3], float R[9]) { pose_product(a, -1, R); }

// rays_d @ R: out[j] = d[0] R[0][j] + d[1] R[1][j] + d[2] R[2][j], from left to right
RN_HD void rotate_row(const float d[3], const float R[9], float out[3]) {
    for (int j = 0; j < 3; j++) out[j] = d[0] * R[j] + d[1] * R[3 + j] + d[2] * R[6 + j];
}

// grad_a[k] = sum_ij G[i][j] dR[i][j] / da_k, G[i][j] = sum_n d[n][i] g_d[n][j]: one factor of the product differentiated at a time
RN_HD void pose_angle_grads(const double G[9], const float a[3], float grad_a[3]) {
    for (int k = 0; k < 3; k++) {
        float dR[9];
        pose_product(a, k, dR);
        double s = 0.0;
        for (int e = 0; e < 9; e++) s += G[e] * (double)dR[e];
        grad_a[k] = (float)s;
    }
}

// d a / d camera_dR = pi / 180 (the chain of pose_angles)
RN_HD float pose_angle_scale() { return 3.14159265358979323846f / 180.0f; }

}  // namespace cam
}  // namespace rn
