// rn_prep.hip -- a dataset directory's image files from the video's frames and their parsing labels: the background plate and the gt
// and torso layers (the reference's data_utils/process.py:63-237, there a k-d tree per frame and lexsort / unique index arithmetic
// on the host).  See rn_prep_dev.h for every convention and include/radnerf_fused.h for the entry points.
//
//   k_plate_columns   one (frame, column) per thread: two sweeps leave the squared vertical distance to the column's nearest
//                     foreground pixel (kFar: none)
//   k_plate_rows      one row per workgroup slice: per frame of the batch, in order, the row's column distances go to LDS, every
//                     thread takes its exact squared distance and keeps the frame where it is strictly greater
//   k_fill_columns    one column per thread: the row of the nearest sure pixel of the column (-1: none), and the count of sure pixels
//   k_fill_rows       one row per workgroup slice: a pixel that is not sure copies its nearest sure pixel's colour
//   k_layer_columns   one (frame, column) per thread: where the two in-paints start and with which colour
//   k_layer_pixels    one pixel per thread: gt, the in-painted and blurred torso colour, alpha
//
// Integer arithmetic and one table of doubles; no float atomics.  The one atomic is the integer count of sure pixels.
#include "rn_common.h"

#include "rn_prep_dev.h"

#include "../../include/radnerf_fused.h"

namespace rn {
namespace prep {

__global__ __launch_bounds__(kBlock) void k_plate_columns(const uint8_t *__restrict__ labels, uint32_t F, uint32_t H, uint32_t W,
                                                          int32_t *__restrict__ g2) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= F * W) return;
    const uint32_t f = i / W, x = i - f * W;
    const size_t base = (size_t)f * H * W + x;
    const uint8_t *L = labels + base;
    int32_t *G = g2 + base;
    int32_t d = -1;                                             // rows since the last foreground pixel; -1: none yet
    for (uint32_t y = 0; y < H; y++) {
        d = L[(size_t)y * W] != kBackground ? 0 : (d >= 0 ? d + 1 : -1);
        G[(size_t)y * W] = d;
    }
    d = -1;
    for (uint32_t y = H; y-- > 0;) {
        d = L[(size_t)y * W] != kBackground ? 0 : (d >= 0 ? d + 1 : -1);
        const int32_t up = G[(size_t)y * W];
        const int32_t m = (d >= 0 && (up < 0 || d < up)) ? d : up;
        G[(size_t)y * W] = m < 0 ? kFar : m * m;
    }
}

__global__ __launch_bounds__(kBlock) void k_plate_rows(const uint8_t *__restrict__ frames, const int32_t *__restrict__ g2, uint32_t F,
                                                       uint32_t H, uint32_t W, uint32_t frame0, int32_t *__restrict__ best_d2,
                                                       int32_t *__restrict__ best_id, uint8_t *__restrict__ plate) {
    extern __shared__ __attribute__((aligned(16))) int32_t row[];
    const uint32_t y = blockIdx.y, x = blockIdx.x * kBlock + threadIdx.x;
    const bool live = x < W;
    const size_t p = (size_t)y * W + x;
    int32_t bd = 0, bi = 0;
    uint32_t colour = 0;
    bool changed = false;
    if (live) {
        bd = best_d2[p];
        bi = best_id[p];
    }
    for (uint32_t f = 0; f < F; f++) {
        const size_t at = ((size_t)f * H + y) * W;
        __syncthreads();                                        // the last frame's readers are done with the row
        for (uint32_t e = threadIdx.x; e < W; e += kBlock) row[e] = g2[at + e];
        __syncthreads();
        if (!live) continue;
        int32_t best = row[x];
        for (uint32_t dx = 1;; dx++) {
            const int32_t dx2 = (int32_t)(dx * dx);             // dx2 < best <= kFar before anything is added to it
            const bool left = x >= dx, right = x + dx < W;
            if (dx2 >= best || !(left || right)) break;
            if (left) best = min(best, dx2 + row[x - dx]);
            if (right) best = min(best, dx2 + row[x + dx]);
        }
        best = min(best, kFar);
        if (best > bd) {
            const uint8_t *c = frames + (at + x) * 3;
            bd = best;
            bi = (int32_t)(frame0 + f);
            colour = pack_rgb(c[0], c[1], c[2]);
            changed = true;
        }
    }
    if (live && changed) {
        best_d2[p] = bd;
        best_id[p] = bi;
        plate[p * 3 + 0] = (uint8_t)(colour & 255u);
        plate[p * 3 + 1] = (uint8_t)((colour >> 8) & 255u);
        plate[p * 3 + 2] = (uint8_t)((colour >> 16) & 255u);
    }
}

__global__ __launch_bounds__(kBlock) void k_fill_columns(const int32_t *__restrict__ best_d2, uint32_t H, uint32_t W, int32_t thresh,
                                                         int32_t *__restrict__ src_row, uint32_t *__restrict__ n_sure) {
    const uint32_t x = blockIdx.x * kBlock + threadIdx.x;
    if (x >= W) return;
    int32_t s = -1;
    uint32_t count = 0;
    for (uint32_t y = 0; y < H; y++) {
        if (best_d2[(size_t)y * W + x] > thresh) {
            s = (int32_t)y;
            count++;
        }
        src_row[(size_t)y * W + x] = s;
    }
    s = -1;
    for (uint32_t y = H; y-- > 0;) {
        if (best_d2[(size_t)y * W + x] > thresh) s = (int32_t)y;
        const int32_t above = src_row[(size_t)y * W + x];
        // of an equidistant pair the one above stays: the smaller source row
        const bool take_below = s >= 0 && (above < 0 || s - (int32_t)y < (int32_t)y - above);
        src_row[(size_t)y * W + x] = take_below ? s : above;
    }
    if (count) atomicAdd(n_sure, count);
}

__global__ __launch_bounds__(kBlock) void k_fill_rows(const int32_t *__restrict__ best_d2, const int32_t *__restrict__ src_row, uint32_t H,
                                                      uint32_t W, int32_t thresh, uint8_t *plate) {
    extern __shared__ __attribute__((aligned(16))) int32_t row[];
    const uint32_t y = blockIdx.y, x = blockIdx.x * kBlock + threadIdx.x;
    for (uint32_t e = threadIdx.x; e < W; e += kBlock) row[e] = src_row[(size_t)y * W + e];
    __syncthreads();
    if (x >= W) return;
    const size_t p = (size_t)y * W + x;
    if (best_d2[p] > thresh) return;                            // sure: keeps its colour, and nothing writes it
    int32_t best = INT32_MAX, by = -1, bx = -1;
    auto consider = [&](uint32_t xs, int32_t dx2) {
        const int32_t s = row[xs];
        if (s < 0) return;
        const int32_t dy = (int32_t)y - s, c = dx2 + dy * dy;
        if (c < best || (c == best && (s < by || (s == by && (int32_t)xs < bx)))) {
            best = c;
            by = s;
            bx = (int32_t)xs;
        }
    };
    consider(x, 0);
    for (uint32_t dx = 1;; dx++) {
        const int32_t dx2 = (int32_t)(dx * dx);
        const bool left = x >= dx, right = x + dx < W;
        if (dx2 > best || !(left || right)) break;              // a source at dx2 == best can still win the tie
        if (left) consider(x - dx, dx2);
        if (right) consider(x + dx, dx2);
    }
    if (bx < 0) return;                                         // no sure pixel anywhere: *n_sure is 0, the caller's to refuse
    const size_t q = (size_t)by * W + (uint32_t)bx;
    plate[p * 3 + 0] = plate[q * 3 + 0];
    plate[p * 3 + 1] = plate[q * 3 + 1];
    plate[p * 3 + 2] = plate[q * 3 + 2];
}

// gt: the frame, the plate where the label says background
__device__ __forceinline__ uint32_t gt_rgb(const uint8_t *__restrict__ frames, const uint8_t *__restrict__ plate, size_t frame_px, size_t px,
                                           uint8_t label) {
    const uint8_t *c = label == kBackground ? plate + px * 3 : frames + frame_px * 3;
    return pack_rgb(c[0], c[1], c[2]);
}

__global__ __launch_bounds__(kBlock) void k_layer_columns(const uint8_t *__restrict__ frames, const uint8_t *__restrict__ labels,
                                                          const uint8_t *__restrict__ plate, uint32_t F, uint32_t H, uint32_t W,
                                                          int32_t *__restrict__ cols) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= F * W) return;
    const uint32_t f = i / W, x = i - f * W;
    const size_t base = (size_t)f * H * W + x;
    const uint8_t *L = labels + base;
    int32_t torso_top = -1, neck_first = -1, covered = 0, n = 0;    // covered: first row the dilated neck has not reached yet
    for (int32_t y = 0; y < (int32_t)H; y++) {
        const uint8_t l = L[(size_t)y * W];
        if (l == kTorso && torso_top < 0) torso_top = y;
        if (l == kNeck) {
            if (neck_first < 0) neck_first = y;
            const int32_t lo = max(max(y - kNeckDilate, 0), covered), hi = min(y + kNeckDilate, (int32_t)H - 1) + 1;
            if (hi > lo) {
                n += hi - lo;
                covered = hi;
            }
        }
    }
    int32_t tt = -1, ns = -1;
    uint32_t ct = 0, cn = 0;
    if (torso_top >= 1 && L[(size_t)(torso_top - 1) * W] == kHead) {
        tt = torso_top;
        ct = gt_rgb(frames, plate, base + (size_t)tt * W, (size_t)tt * W + x, kTorso);
    }
    if (neck_first >= 0) {
        const int32_t t = max(neck_first - kNeckDilate, 0);
        if (t >= 1 && L[(size_t)(t - 1) * W] == kHead) {
            ns = t + min(n - 1, kNeckPush);                     // stays inside the top run of the dilated neck, hence below H
            cn = gt_rgb(frames, plate, base + (size_t)ns * W, (size_t)ns * W + x, L[(size_t)ns * W]);
        }
    }
    int32_t *out = cols + (size_t)i * kColumnInts;
    out[0] = tt;
    out[1] = ns;
    out[2] = (int32_t)ct;
    out[3] = (int32_t)cn;
}

// the torso image before the blur at (y, x) of frame f: neck in-paint over torso in-paint over gt with the plate under the head
__device__ __forceinline__ uint32_t pre_blur(const uint8_t *__restrict__ frames, const uint8_t *__restrict__ labels,
                                             const uint8_t *__restrict__ plate, const double *__restrict__ darken,
                                             const int32_t *__restrict__ cols, uint32_t f, int32_t y, int32_t x, uint32_t H, uint32_t W) {
    const int32_t *c = cols + ((size_t)f * W + (uint32_t)x) * kColumnInts;
    const int32_t tt = c[0], ns = c[1];
    if (ns >= 0 && y <= ns && y > ns - kNeckRows) return darken_rgb((uint32_t)c[3], darken[ns - y]);
    if (tt >= 0 && y <= tt && y > tt - kTorsoRows) return darken_rgb((uint32_t)c[2], darken[tt - y]);
    const size_t px = (size_t)y * W + (uint32_t)x, fpx = (size_t)f * H * W + px;
    const uint8_t l = labels[fpx];
    return gt_rgb(frames, plate, fpx, px, l == kHead ? kBackground : l);
}

__global__ __launch_bounds__(kBlock) void k_layer_pixels(const uint8_t *__restrict__ frames, const uint8_t *__restrict__ labels,
                                                         const uint8_t *__restrict__ plate, const double *__restrict__ darken,
                                                         const int32_t *__restrict__ cols, uint32_t F, uint32_t H, uint32_t W,
                                                         uint8_t *__restrict__ gt, uint8_t *__restrict__ torso) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;      // F H W < 2^31
    if (i >= F * H * W) return;
    const uint32_t f = i / (H * W), px = i - f * (H * W);
    const int32_t y = (int32_t)(px / W), x = (int32_t)(px - (uint32_t)y * W);
    const uint8_t l = labels[i];
    const uint32_t g = gt_rgb(frames, plate, i, px, l);
    gt[(size_t)i * 3 + 0] = (uint8_t)(g & 255u);
    gt[(size_t)i * 3 + 1] = (uint8_t)((g >> 8) & 255u);
    gt[(size_t)i * 3 + 2] = (uint8_t)((g >> 16) & 255u);

    const int32_t *c = cols + ((size_t)f * W + (uint32_t)x) * kColumnInts;
    const int32_t tt = c[0], ns = c[1];
    const bool in_torso = tt >= 0 && y <= tt && y > tt - kTorsoRows, in_neck = ns >= 0 && y <= ns && y > ns - kNeckRows;
    bool neck_d = false;
    for (int32_t dy = -kNeckDilate; dy <= kNeckDilate; dy++) {
        const int32_t yy = y + dy;
        if (yy >= 0 && yy < (int32_t)H) neck_d |= labels[(size_t)f * H * W + (size_t)yy * W + (uint32_t)x] == kNeck;
    }
    uint32_t out = 0;                                           // RGBA, all zero where alpha is
    if (neck_d || l == kTorso || in_torso || in_neck) {
        uint32_t rgb;
        if (in_neck) {
            uint32_t sr = 32768u, sg = 32768u, sb = 32768u;
            for (int32_t j = -2; j <= 2; j++) {
                const int32_t yy = reflect101(y + j, (int32_t)H);
                for (int32_t k = -2; k <= 2; k++) {
                    const uint32_t w = (uint32_t)(blur_weight(j) * blur_weight(k));
                    const uint32_t v = pre_blur(frames, labels, plate, darken, cols, f, yy, reflect101(x + k, (int32_t)W), H, W);
                    sr += w * (v & 255u);
                    sg += w * ((v >> 8) & 255u);
                    sb += w * ((v >> 16) & 255u);
                }
            }
            rgb = pack_rgb(sr >> 16, sg >> 16, sb >> 16);
        } else {
            rgb = pre_blur(frames, labels, plate, darken, cols, f, y, x, H, W);
        }
        out = rgb | 0xff000000u;
    }
    torso[(size_t)i * 4 + 0] = (uint8_t)(out & 255u);
    torso[(size_t)i * 4 + 1] = (uint8_t)((out >> 8) & 255u);
    torso[(size_t)i * 4 + 2] = (uint8_t)((out >> 16) & 255u);
    torso[(size_t)i * 4 + 3] = (uint8_t)(out >> 24);
}

static bool shape_ok(uint64_t F, uint64_t H, uint64_t W) {
    return F >= 1 && H >= 1 && W >= 1 && H <= kMaxSide && W <= kMaxSide && F * H * W < (1ull << 31);
}

}  // namespace prep
}  // namespace rn

using namespace rn;
using namespace rn::prep;

#define RN_PREP_SHAPE(what, F, H, W)                                                                                              \
    RN_REQUIRE(shape_ok(F, H, W), what ": F, H, W >= 1, sides <= %u and F * H * W < 2^31, got F = %u, H = %u, W = %u", kMaxSide, \
               (uint32_t)(F), (uint32_t)(H), (uint32_t)(W))

extern "C" {

size_t rn_prep_workspace(uint32_t F, uint32_t H, uint32_t W) {
    return shape_ok(F, H, W) ? (size_t)workspace_bytes(F, H, W) : 0;
}

int rn_prep_plate_accumulate(const uint8_t *frames, const uint8_t *labels, uint32_t F, uint32_t H, uint32_t W, uint32_t frame0,
                             int32_t *best_d2, int32_t *best_id, uint8_t *plate, void *workspace, rn_stream_t stream) {
    RN_PREP_SHAPE("prep_plate_accumulate", F, H, W);
    RN_REQUIRE((uint64_t)frame0 + F <= (uint64_t)INT32_MAX, "prep_plate_accumulate: frame0 + F = %llu leaves int32",
               (unsigned long long)frame0 + F);
    RN_REQUIRE(frames && labels && best_d2 && best_id && plate && workspace, "prep_plate_accumulate: null pointer");
    int32_t *g2 = static_cast<int32_t *>(workspace);
    hipLaunchKernelGGL(k_plate_columns, dim3(div_up(F * W, kBlock)), dim3(kBlock), 0, as_stream(stream), labels, F, H, W, g2);
    hipLaunchKernelGGL(k_plate_rows, dim3(div_up(W, kBlock), H), dim3(kBlock), (size_t)W * sizeof(int32_t), as_stream(stream), frames, g2, F, H,
                       W, frame0, best_d2, best_id, plate);
    return check_launch("prep_plate_accumulate");
}

int rn_prep_plate_fill(const int32_t *best_d2, uint8_t *plate, uint32_t H, uint32_t W, int32_t thresh_d2, uint32_t *n_sure, void *workspace,
                       rn_stream_t stream) {
    RN_PREP_SHAPE("prep_plate_fill", 1u, H, W);
    RN_REQUIRE(best_d2 && plate && n_sure && workspace, "prep_plate_fill: null pointer");
    int32_t *src_row = static_cast<int32_t *>(workspace);
    if (hipMemsetAsync(n_sure, 0, sizeof(uint32_t), as_stream(stream)) != hipSuccess) return check_launch("prep_plate_fill");
    hipLaunchKernelGGL(k_fill_columns, dim3(div_up(W, kBlock)), dim3(kBlock), 0, as_stream(stream), best_d2, H, W, thresh_d2, src_row, n_sure);
    hipLaunchKernelGGL(k_fill_rows, dim3(div_up(W, kBlock), H), dim3(kBlock), (size_t)W * sizeof(int32_t), as_stream(stream), best_d2, src_row, H,
                       W, thresh_d2, plate);
    return check_launch("prep_plate_fill");
}

int rn_prep_layers(const uint8_t *frames, const uint8_t *labels, const uint8_t *plate, const double *darken, uint32_t F, uint32_t H, uint32_t W,
                   uint8_t *gt, uint8_t *torso, void *workspace, rn_stream_t stream) {
    RN_PREP_SHAPE("prep_layers", F, H, W);
    RN_REQUIRE(frames && labels && plate && darken && gt && torso && workspace, "prep_layers: null pointer");
    int32_t *cols = static_cast<int32_t *>(workspace);
    hipLaunchKernelGGL(k_layer_columns, dim3(div_up(F * W, kBlock)), dim3(kBlock), 0, as_stream(stream), frames, labels, plate, F, H, W, cols);
    hipLaunchKernelGGL(k_layer_pixels, dim3(div_up(F * H * W, kBlock)), dim3(kBlock), 0, as_stream(stream), frames, labels, plate, darken, cols, F,
                       H, W, gt, torso);
    return check_launch("prep_layers");
}

}  // extern "C"
