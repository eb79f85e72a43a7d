// rn_prep_dev.h -- the conventions of the dataset-preparation kernels (rn_prep.hip): the background plate, and the gt and torso layers
// of every frame (the reference's data_utils/process.py, tasks 5 and 6).  Plain functions for host and device; see
// include/radnerf_fused.h for the entry points.
//
// Everything is integer or table-driven: a result is a function of the inputs alone, whatever the batching or the launch shape.
//   * images are uint8, row-major, RGB: frames [F,H,W,3], plate [H,W,3], gt [F,H,W,3], torso [F,H,W,4] (RGBA);
//   * labels [F,H,W] uint8: kOther 0, kHead 1, kNeck 2, kTorso 3, kBackground 4 (radnerf/prepare.py derives them from the parsing
//     PNG's colours);
//   * distances are squared Euclidean pixel distances in int32.  Sides are at most kMaxSide, so that a real distance stays below
//     kFar = 2^30, which is the distance of every pixel of a frame without a single source pixel, and a row of int32 fits 64 KiB of LDS;
//   * a distance transform is two passes.  Columns: every pixel gets the vertical distance to the nearest source of its column.
//     Rows: a workgroup stages its row of those in LDS, and every thread takes min over x' of (x - x')^2 + g^2(x'), walking outward
//     from its own x and stopping once (x - x')^2 alone can no longer win;
//   * plate: a frame replaces a pixel's (best_d2, best_id, colour) only where its d2 is strictly greater -- frames in ascending
//     order, hence np.argmax's first maximum;
//   * fill: a pixel is sure where best_d2 > thresh_d2; every other pixel copies the plate colour of its nearest sure pixel, ties
//     going to the smallest source row, then the smallest source column.  The column pass keeps, of an equidistant pair above and
//     below, the one above: the one below loses every tie it could enter;
//   * layers: per column x of a frame, in-paints go upward from the top torso pixel (9 rows) and from the pushed-down top of the
//     vertically dilated neck (53 rows) where a head pixel sits right above that top; rows above row 0 are dropped and a top at row 0
//     has no head above.  A darkened colour is uint8(trunc(double(c) * darken[k])), darken a host table of float64;
//   * blur: 5 x 5, weights kBlur[] / 256 per axis (a Gaussian of sigma 4 rounded to 1/256; they sum to 256), reflect-101 edges,
//     (sum of w_i w_j p + 32768) >> 16; it reads the in-painted image and replaces only pixels the neck in-paint marked.
#pragma once

#include <stdint.h>

#ifndef RN_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define RN_HD __host__ __device__ inline
#else
#define RN_HD inline
#endif
#endif

namespace rn {
namespace prep {

constexpr uint8_t kOther = 0, kHead = 1, kNeck = 2, kTorso = 3, kBackground = 4;
constexpr uint32_t kBlock = 256;
constexpr uint32_t kMaxSide = 16384;          // 2 * (kMaxSide - 1)^2 < kFar; kMaxSide * 4 bytes = 64 KiB of LDS
constexpr int32_t kFar = 1 << 30;
constexpr int32_t kTorsoRows = 9, kNeckRows = 53, kNeckPush = 4, kNeckDilate = 3;
constexpr uint32_t kDarken = 53;              // entries of the darken table: max(kTorsoRows, kNeckRows)
constexpr uint32_t kColumnInts = 4;           // per (frame, column): torso top, neck start (-1: no in-paint), their two colours packed

// i reflected into 0 .. n - 1 without repeating the edge (cv2.BORDER_REFLECT_101); n = 1: 0
RN_HD int32_t reflect101(int32_t i, int32_t n) {
    if (n == 1) return 0;
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i;
    return i;
}

RN_HD int32_t blur_weight(int32_t tap) {      // tap -2 .. 2
    return tap == 0 ? 54 : (tap == 1 || tap == -1) ? 53 : 48;
}

RN_HD uint32_t pack_rgb(uint32_t r, uint32_t g, uint32_t b) { return r | (g << 8) | (b << 16); }

// every channel of a packed colour times one darken entry, truncated
RN_HD uint32_t darken_rgb(uint32_t c, double s) {
    const uint32_t r = (uint32_t)(int32_t)((double)(c & 255u) * s);
    const uint32_t g = (uint32_t)(int32_t)((double)((c >> 8) & 255u) * s);
    const uint32_t b = (uint32_t)(int32_t)((double)((c >> 16) & 255u) * s);
    return pack_rgb(r & 255u, g & 255u, b & 255u);
}

// bytes of scratch for F frames: the larger of the plate's int32 [F,H,W] and the layers' int32 [F,W,kColumnInts]; 16-byte aligned
static inline uint64_t workspace_bytes(uint64_t F, uint64_t H, uint64_t W) {
    const uint64_t a = F * H * W * 4ull, b = F * W * kColumnInts * 4ull;
    return ((a > b ? a : b) + 15ull) / 16ull * 16ull;
}

}  // namespace prep
}  // namespace rn
