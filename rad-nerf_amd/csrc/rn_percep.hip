// rn_percep.hip -- the perceptual term of lip fine-tuning (LPIPS, net = 'alex', eval mode): forward and the gradient with
// respect to the prediction.  See include/radnerf_train.h for the arithmetic and rn_percep_dev.h for the layouts.
//
//   k_pack          the five weight tensors -> forward images Wt[k][co] and data-gradient images Wb[k][ci], biases, lin   1 launch
//   k_gemm<..>      one layer as an implicit GEMM on v_mfma_f32_32x32x2_f32: a wave owns a 32 x 32 tile of [M = channels] x
//                   [N = images x positions] over one slice of K and writes it as a partial tile; the gather builds the B
//                   operand in registers (conv1: the caller's tensor through its strides, shift / scale folded in; conv2, conv3:
//                   the 3 x 3 / stride 2 max of the tap before; data gradient: the ReLU-masked gradient at y + pad - ky)
//   k_epi_fwd       bias + partial tiles in slice order, ReLU -> tap
//   k_distance      per tap, image and 32 positions: normalise both halves, weighted squared difference, ordered sums, and
//                   d value / d tap of the pred half in the same pass
//   k_value         the workgroups' sums in order -> the five taps' values -> value_out[P]
//   k_epi_bwd       partial tiles in slice order (+ the tap's own distance gradient) -> gradient of the tap before
//   k_pool_route    gradient of a pooled map back to the first maximum of every window, as a gather (no atomics)
//   k_conv1_bwd     conv1's data gradient, direct (3 channels, stride 4), through the caller's strides, scaled
//
// fp32 throughout; no float atomics, every sum in one fixed order.
#include "rn_percep_dev.h"
#include "rn_tile32_dev.h"

#include "../../include/radnerf_train.h"

namespace rn {
namespace percep {

constexpr ImageLayout kImg = image_layout();

// ------------------------------------------------------------------------------------------------------------------ pack
struct PackArgs {
    const float *w[kLayers], *b[kLayers], *lin[kLayers], *ss;
};

__global__ void __launch_bounds__(256) k_pack(PackArgs a, float *__restrict__ image) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= kImg.total) return;
    float v = 0.0f;
    if (idx < kImg.bias) {
        bool bwd = idx >= kImg.bwd[0];
        int l = bwd ? 1 : 0;
        const uint32_t *start = bwd ? kImg.bwd : kImg.fwd;
        for (int i = l + 1; i < kLayers; i++)
            if (idx >= start[i]) l = i;
        const uint32_t rel = idx - start[l], kk2 = kKern[l] * kKern[l], cin = kCin[l], cout = kCout[l];
        if (!bwd) {                                   // Wt[(ci, t)][co] = W[co][ci][t]
            const uint32_t k = rel / cout, co = rel - k * cout;
            if (k < cin * kk2) v = a.w[l][co * cin * kk2 + k];
        } else {                                      // Wb[(co, t)][ci] = W[co][ci][t]
            const uint32_t k = rel / cin, ci = rel - k * cin, co = k / kk2, t = k - co * kk2;
            v = a.w[l][(co * cin + ci) * kk2 + t];
        }
    } else if (idx < kImg.ss) {
        const bool is_lin = idx >= kImg.lin;
        const uint32_t rel = idx - (is_lin ? kImg.lin : kImg.bias);
        int l = 0;
        for (int i = 1; i < kLayers; i++)
            if (rel >= channel_offset(i)) l = i;
        v = (is_lin ? a.lin[l] : a.b[l])[rel - channel_offset(l)];
    } else if (idx < kImg.ss + 6u) {
        v = a.ss[idx - kImg.ss];
    }
    image[idx] = v;
}

// ------------------------------------------------------------------------------------------------------------------ GEMM
enum Mode { kModeImage, kModeTap, kModeTapPooled, kModeGrad };

struct GemmArgs {
    const float *wt;        // [Kpad][M]
    const float *src;       // kModeTap*: the tap before, [Cin][src_row]; kModeGrad: gradient of this tap, [Cout][src_row]
    const float *mask;      // kModeGrad: this tap, [Cout][mask_row] (pred half first)
    float *part;            // [S][M][N]
    uint32_t M, K, N, len, steps, S, mt, nt;
    uint32_t oh, ow;        // spatial size of the output (per image)
    uint32_t sh, sw;        // spatial size of src per image (before the pool)
    uint32_t ih, iw;        // spatial size of the convolution's input (after the pool; kModeImage: h, w)
    uint32_t src_row, mask_row;
    // kModeImage
    const float *pred, *target, *ss;
    int64_t p_img, p_pix, p_ch, t_img, t_pix, t_ch;
    uint32_t P;
    int normalize;
};

template <int KK, int MODE>
__device__ __forceinline__ float gather(const GemmArgs &a, uint32_t k, bool valid, uint32_t img, int oy, int ox) {
    constexpr int PAD = MODE == kModeImage ? 2 : KK / 2;
    if (!valid || k >= a.K) return 0.0f;
    const uint32_t c = k / (uint32_t)(KK * KK), r = k - c * (uint32_t)(KK * KK);
    const int ky = (int)(r / (uint32_t)KK), kx = (int)(r - (uint32_t)ky * (uint32_t)KK);
    if (MODE == kModeImage) {
        const int iy = oy * 4 - PAD + ky, ix = ox * 4 - PAD + kx;
        if (iy < 0 || ix < 0 || iy >= (int)a.ih || ix >= (int)a.iw) return 0.0f;
        const bool is_pred = img < a.P;
        const float *base = is_pred ? a.pred + (int64_t)img * a.p_img : a.target + (int64_t)(img - a.P) * a.t_img;
        const int64_t pix = (int64_t)iy * a.iw + ix;
        float v = is_pred ? base[pix * a.p_pix + (int64_t)c * a.p_ch] : base[pix * a.t_pix + (int64_t)c * a.t_ch];
        if (a.normalize) v = 2.0f * v - 1.0f;
        return (v - a.ss[c]) / a.ss[3 + c];
    } else if (MODE == kModeGrad) {
        const int iy = oy + PAD - ky, ix = ox + PAD - kx;
        if (iy < 0 || ix < 0 || iy >= (int)a.ih || ix >= (int)a.iw) return 0.0f;
        const uint32_t at = img * a.ih * a.iw + (uint32_t)iy * a.iw + (uint32_t)ix;
        return a.mask[c * a.mask_row + at] > 0.0f ? a.src[c * a.src_row + at] : 0.0f;
    } else {
        const int iy = oy - PAD + ky, ix = ox - PAD + kx;
        if (iy < 0 || ix < 0 || iy >= (int)a.ih || ix >= (int)a.iw) return 0.0f;
        const float *s = a.src + c * a.src_row + img * a.sh * a.sw;
        if (MODE == kModeTap) return s[(uint32_t)iy * a.sw + (uint32_t)ix];
        // the window (2 iy .. 2 iy + 2) x (2 ix .. 2 ix + 2) lies inside the map: ih = (sh - 3) / 2 + 1
        s += (uint32_t)(2 * iy) * a.sw + (uint32_t)(2 * ix);
        float m = s[0];
#pragma unroll
        for (int dy = 0; dy < 3; dy++)
#pragma unroll
            for (int dx = 0; dx < 3; dx++) m = fmaxf(m, s[dy * (int)a.sw + dx]);
        return m;
    }
}

// one wave per workgroup: the work items (slice, tile m, tile n) are few and latency-bound, so they are spread over as many
// compute units as there are
template <int KK, int MODE>
__global__ void __launch_bounds__(64) k_gemm(GemmArgs a) {
    const uint32_t lane = threadIdx.x, item = blockIdx.x;
    const uint32_t tiles = a.mt * a.nt;
    const uint32_t s = item / tiles, t = item - s * tiles, tm = t / a.nt, tn = t - tm * a.nt;
    const uint32_t j = lane & 31u, hh = lane >> 5;
    const uint32_t n = tn * 32u + j;
    const bool valid = n < a.N;
    const uint32_t hw = a.oh * a.ow, img = valid ? n / hw : 0u, rem = valid ? n - img * hw : 0u;
    const int oy = (int)(rem / a.ow), ox = (int)(rem - (uint32_t)oy * a.ow);
    const float *wcol = a.wt + tm * 32u + j;
    f32x16 acc = zero16();
    const uint32_t s0 = s * a.len, s1 = min(s0 + a.len, a.steps);
    uint32_t st = s0;
    for (; st + 4u <= s1; st += 4u) {                          // four steps' loads in flight before the first product
        float wv[4], bv[4];
#pragma unroll
        for (uint32_t u = 0; u < 4u; u++) {
            const uint32_t k = 2u * (st + u) + hh;             // < Kpad: the image has a zero row past K
            wv[u] = wcol[k * a.M];
            bv[u] = gather<KK, MODE>(a, k, valid, img, oy, ox);
        }
#pragma unroll
        for (uint32_t u = 0; u < 4u; u++) acc = mfma32(wv[u], bv[u], acc);
    }
    for (; st < s1; st++) {
        const uint32_t k = 2u * st + hh;
        acc = mfma32(wcol[k * a.M], gather<KK, MODE>(a, k, valid, img, oy, ox), acc);
    }
    if (valid) {
        float *dst = a.part + (s * a.M + tm * 32u) * a.N + n;
#pragma unroll
        for (int r = 0; r < 16; r++) dst[(uint32_t)rowmap(r, (int)hh) * a.N] = acc[r];
    }
}

__global__ void __launch_bounds__(256) k_epi_fwd(const float *__restrict__ part, uint32_t S, uint32_t M, uint32_t N,
                                                 const float *__restrict__ bias, float *__restrict__ out) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x, MN = M * N;
    if (idx >= MN) return;
    float v = bias[idx / N];
    for (uint32_t s = 0; s < S; s++) v += part[s * MN + idx];
    out[idx] = fmaxf(v, 0.0f);
}

__global__ void __launch_bounds__(256) k_epi_bwd(const float *__restrict__ part, uint32_t S, uint32_t MN,
                                                 const float *__restrict__ add, float *__restrict__ out) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= MN) return;
    float v = part[idx];
    for (uint32_t s = 1; s < S; s++) v += part[s * MN + idx];
    out[idx] = add ? add[idx] + v : v;
}

// ------------------------------------------------------------------------------------------------------------------ distance
constexpr uint32_t kDistSlices = 8;       // channel slices per position (kDistPos positions per workgroup)

struct DistArgs {
    const float *tap[kLayers], *lin[kLayers];
    float *dgrad[kLayers];
    float *part;            // per tap, image and workgroup: the sum of d over the workgroup's positions
    float *vals;            // [5][P] per-tap values
    uint32_t hw[kLayers], part_off[kLayers], P;
};

// Sum over the channel slices of one position, the same for all eight threads of the position: slice order.
__device__ __forceinline__ float slice_sum(float (*s)[kDistPos], uint32_t j) {
    float t = s[0][j];
#pragma unroll
    for (uint32_t i = 1; i < kDistSlices; i++) t += s[i][j];
    return t;
}

// grid (workgroups of the largest tap, P, 5).  Thread (slice, j) of a workgroup owns position 32 blockIdx.x + j and the channels
// slice, slice + 8, ...: for a fixed channel the 32 positions are one 128-byte line.  Three passes over the channels (norms;
// distance and u . x; gradient), the slices' partial sums meeting in LDS in slice order.
__global__ void __launch_bounds__(256) k_distance(DistArgs a) {
    __shared__ float sa[kDistSlices][kDistPos], sb[kDistSlices][kDistPos];
    const uint32_t l = blockIdx.z, p = blockIdx.y, hw = a.hw[l], nblk = (hw + kDistPos - 1u) / kDistPos;
    if (blockIdx.x >= nblk) return;
    const uint32_t j = threadIdx.x & (kDistPos - 1u), cs = threadIdx.x / kDistPos, q = blockIdx.x * kDistPos + j;
    const bool live = q < hw;
    const uint32_t C = kCout[l], row = 2u * a.P * hw, grow = a.P * hw;
    const float *lin = a.lin[l];
    const float *x = a.tap[l] + p * hw + (live ? q : 0u), *y = x + a.P * hw;
    const float inv_hw = 1.0f / (float)hw;
    float sx = 0.0f, sy = 0.0f;
    if (live)
        for (uint32_t c = cs; c < C; c += kDistSlices) {
            const float xv = x[c * row], yv = y[c * row];
            sx += xv * xv;
            sy += yv * yv;
        }
    sa[cs][j] = sx; sb[cs][j] = sy;
    __syncthreads();
    sx = slice_sum(sa, j); sy = slice_sum(sb, j);
    __syncthreads();
    const float nx = sqrtf(sx), ny = sqrtf(sy), dx = nx + 1e-10f, dy = ny + 1e-10f;
    float d = 0.0f, dot = 0.0f;                       // dot = sum_c u_c x_c, u_c = d value / d n(x)_c
    if (live)
        for (uint32_t c = cs; c < C; c += kDistSlices) {
            const float xv = x[c * row], diff = xv / dx - y[c * row] / dy;
            d += lin[c] * (diff * diff);
            dot += (2.0f * lin[c] * diff * inv_hw) * xv;
        }
    sa[cs][j] = d; sb[cs][j] = dot;
    __syncthreads();
    d = slice_sum(sa, j); dot = slice_sum(sb, j);
    __syncthreads();
    // d n(x)_c / d x_j = delta_cj / (|x| + eps) - x_c x_j / ((|x| + eps)^2 |x|); at |x| = 0 the second term is taken as 0
    const float back = nx > 0.0f ? dot / (dx * dx * nx) : 0.0f;
    if (live) {
        float *g = a.dgrad[l] + p * hw + q;
        for (uint32_t c = cs; c < C; c += kDistSlices) {
            const float xv = x[c * row], diff = xv / dx - y[c * row] / dy;
            g[c * grow] = (2.0f * lin[c] * diff * inv_hw) / dx - xv * back;
        }
    }
    if (cs == 0) sa[0][j] = live ? d : 0.0f;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = sa[0][0];
        for (uint32_t i = 1; i < kDistPos; i++) t += sa[0][i];
        a.part[a.part_off[l] + p * nblk + blockIdx.x] = t;
    }
}

// value of tap l = (the workgroups' sums in workgroup order) / positions; value_out = the five values in tap order
__global__ void k_value(DistArgs a, float *__restrict__ out) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.P) return;
    float total = 0.0f;
    for (int l = 0; l < kLayers; l++) {
        const uint32_t nblk = (a.hw[l] + kDistPos - 1u) / kDistPos;
        const float *part = a.part + a.part_off[l] + p * nblk;
        float t = part[0];
        for (uint32_t i = 1; i < nblk; i++) t += part[i];
        const float v = t / (float)a.hw[l];
        a.vals[l * a.P + p] = v;
        total = l == 0 ? v : total + v;
    }
    out[p] = total;
}

// ------------------------------------------------------------------------------------------------------------------ backward
// out[c][p][y][x] = dgrad[c][p][y][x] + sum of pooled[c][p][py][px] over the windows (py, px) that hold (y, x) and whose first
// maximum in row-major order is (y, x).  tap: [C][2P][sh][sw], pred half first.
__global__ void __launch_bounds__(256) k_pool_route(const float *__restrict__ pooled, const float *__restrict__ dgrad,
                                                    const float *__restrict__ tap, float *__restrict__ out, uint32_t C, uint32_t P,
                                                    uint32_t sh, uint32_t sw, uint32_t ph, uint32_t pw) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x, hw = sh * sw;
    if (idx >= C * P * hw) return;
    const uint32_t c = idx / (P * hw), r = idx - c * P * hw, p = r / hw, q = r - p * hw;
    const int y = (int)(q / sw), x = (int)(q - (uint32_t)y * sw);
    const float *t = tap + c * 2u * P * hw + p * hw;
    const float *g = pooled + (c * P + p) * ph * pw;
    float v = dgrad[idx];
    const int py0 = y >= 2 ? (y - 1) / 2 : 0, py1 = min(y / 2, (int)ph - 1);
    const int px0 = x >= 2 ? (x - 1) / 2 : 0, px1 = min(x / 2, (int)pw - 1);
    for (int py = py0; py <= py1; py++)
        for (int px = px0; px <= px1; px++) {
            int by = 0, bx = 0;
            float best = t[(uint32_t)(2 * py) * sw + (uint32_t)(2 * px)];
            for (int dy = 0; dy < 3; dy++)
                for (int dx = 0; dx < 3; dx++) {
                    const float tv = t[(uint32_t)(2 * py + dy) * sw + (uint32_t)(2 * px + dx)];
                    if (tv > best) { best = tv; by = dy; bx = dx; }
                }
            if (2 * py + by == y && 2 * px + bx == x) v += g[(uint32_t)py * pw + (uint32_t)px];
        }
    out[idx] = v;
}

struct Conv1BwdArgs {
    const float *wt;            // conv1's forward image [364][64]
    const float *grad, *tap;    // [64][P][oh][ow], [64][2P][oh][ow]
    const float *ss, *upstream;
    float *g_pred;
    int64_t g_img, g_pix, g_ch;
    uint32_t P, h, w, oh, ow, upstream_stride;
    int normalize;
};

// Eight lanes per pixel of a pred image, eight of conv1's 64 output channels each, over the (at most 3 x 3) windows that hold the
// pixel; the eight partial sums meet in a shuffle butterfly (the same bits in every lane, whatever the order of a + b).
constexpr uint32_t kC1Parts = 8;
__global__ void __launch_bounds__(256) k_conv1_bwd(Conv1BwdArgs a) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x, npx = a.h * a.w, part = idx & (kC1Parts - 1u);
    const bool live = idx / kC1Parts < a.P * npx;               // a dead lane goes through the shuffles with zeros
    const uint32_t pix = live ? idx / kC1Parts : 0u, p = pix / npx, q = pix - p * npx;
    const int y = (int)(q / a.w), x = (int)(q - (uint32_t)y * a.w);
    const uint32_t hw = a.oh * a.ow;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (int ky = (y + 2) & 3; ky < 11 && live; ky += 4) {
        const int oy = (y + 2 - ky) / 4;
        if (y + 2 - ky < 0 || oy >= (int)a.oh) continue;
        for (int kx = (x + 2) & 3; kx < 11; kx += 4) {
            const int ox = (x + 2 - kx) / 4;
            if (x + 2 - kx < 0 || ox >= (int)a.ow) continue;
            const uint32_t at = p * hw + (uint32_t)oy * a.ow + (uint32_t)ox;
            const float *wk = a.wt + (uint32_t)(ky * 11 + kx) * 64u;
#pragma unroll
            for (uint32_t i = 0; i < 64u / kC1Parts; i++) {
                const uint32_t co = part * (64u / kC1Parts) + i;
                const float dz = a.tap[co * 2u * a.P * hw + at] > 0.0f ? a.grad[co * a.P * hw + at] : 0.0f;
#pragma unroll
                for (int c = 0; c < 3; c++) acc[c] += wk[(uint32_t)c * 121u * 64u + co] * dz;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int m = 1; m < (int)kC1Parts; m <<= 1) acc[c] += __shfl_xor(acc[c], m, 64);
    if (!live || part != 0u) return;
    const float up = a.upstream[p * a.upstream_stride];
    float *dst = a.g_pred + (int64_t)p * a.g_img + (int64_t)q * a.g_pix;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float v = acc[c] / a.ss[3 + c];
        if (a.normalize) v = 2.0f * v;
        dst[(int64_t)c * a.g_ch] = v * up;
    }
}

// ------------------------------------------------------------------------------------------------------------------ host
template <int KK, int MODE>
static void launch_gemm(const GemmArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL((k_gemm<KK, MODE>), dim3(a.mt * a.nt * a.S), dim3(kWave), 0, stream, a);
}

static void set_split(GemmArgs &a, uint32_t M, uint32_t K, uint32_t Kpad, uint32_t N) {
    const Split s = split_rule(M, N, Kpad);
    a.M = M; a.K = K; a.N = N; a.len = s.len; a.steps = s.steps; a.S = s.S; a.mt = s.mt; a.nt = s.nt;
}

}  // namespace percep
}  // namespace rn

using namespace rn;
using namespace rn::percep;

extern "C" {

size_t rn_percep_image_floats(void) { return (size_t)kImg.total; }

int rn_percep_pack(const float *const *weights, const float *const *biases, const float *const *lins, const float *shift_scale,
                   float *image, rn_stream_t stream) {
    RN_REQUIRE(weights && biases && lins && shift_scale && image, "percep_pack: null pointer");
    PackArgs a{};
    for (int l = 0; l < kLayers; l++) {
        RN_REQUIRE(weights[l] && biases[l] && lins[l], "percep_pack: null pointer in layer %d", l + 1);
        a.w[l] = weights[l]; a.b[l] = biases[l]; a.lin[l] = lins[l];
    }
    a.ss = shift_scale;
    hipLaunchKernelGGL(k_pack, dim3(div_up(kImg.total, 256u)), dim3(256), 0, as_stream(stream), a, image);
    return check_launch("percep_pack");
}

size_t rn_percep_workspace(uint32_t P, uint32_t h, uint32_t w) { return (size_t)make_plan(P, h, w).total * sizeof(float); }

int rn_percep_tap(uint32_t P, uint32_t h, uint32_t w, uint32_t layer, size_t *offset_floats, uint32_t *channels, uint32_t *oh,
                  uint32_t *ow) {
    RN_REQUIRE(offset_floats && channels && oh && ow, "percep_tap: null pointer");
    RN_REQUIRE(layer < (uint32_t)kLayers, "percep_tap: layer must be 0..4");
    const Plan pl = make_plan(P, h, w);
    RN_REQUIRE(pl.total > 0, "percep_tap: unsupported shape P = %u, %u x %u (P >= 1, h, w >= 31)", P, h, w);
    *offset_floats = pl.tap[layer]; *channels = kCout[layer]; *oh = pl.oh[layer]; *ow = pl.ow[layer];
    return RN_OK;
}

int rn_percep_tap_values(uint32_t P, uint32_t h, uint32_t w, size_t *offset_floats) {
    RN_REQUIRE(offset_floats, "percep_tap_values: null pointer");
    const Plan pl = make_plan(P, h, w);
    RN_REQUIRE(pl.total > 0, "percep_tap_values: unsupported shape P = %u, %u x %u (P >= 1, h, w >= 31)", P, h, w);
    *offset_floats = pl.vals;
    return RN_OK;
}

int rn_percep_forward(const float *image, void *workspace, size_t workspace_bytes, const float *pred, int64_t pred_image_stride,
                      int64_t pred_pixel_stride, int64_t pred_channel_stride, const float *target, int64_t target_image_stride,
                      int64_t target_pixel_stride, int64_t target_channel_stride, uint32_t P, uint32_t h, uint32_t w, int normalize,
                      float *value_out, rn_stream_t stream) {
    RN_REQUIRE(P > 0, "percep_forward: P must be positive");
    RN_REQUIRE(h >= kMinSide && w >= kMinSide, "percep_forward: %u x %u is below the smallest image, 31 x 31", h, w);
    RN_REQUIRE(image && workspace && pred && target && value_out, "percep_forward: null pointer");
    const Plan pl = make_plan(P, h, w);
    RN_REQUIRE(pl.total > 0, "percep_forward: unsupported shape P = %u, %u x %u", P, h, w);
    RN_REQUIRE(workspace_bytes >= pl.total * sizeof(float), "percep_forward: workspace of %zu bytes, rn_percep_workspace asks for %zu",
               workspace_bytes, (size_t)pl.total * sizeof(float));
    RN_REQUIRE(((uintptr_t)workspace & 15u) == 0, "percep_forward: workspace must be 16-byte aligned");
    hipStream_t st = as_stream(stream);
    float *ws = static_cast<float *>(workspace);
    for (int l = 0; l < kLayers; l++) {
        GemmArgs a{};
        const uint32_t N = 2u * P * pl.oh[l] * pl.ow[l];
        set_split(a, kCout[l], k_fwd(l), k_fwd_pad(l), N);
        a.wt = image + kImg.fwd[l];
        a.part = ws + pl.part;
        a.oh = pl.oh[l]; a.ow = pl.ow[l];
        if (l == 0) {
            a.ih = h; a.iw = w;
            a.pred = pred; a.target = target; a.ss = image + kImg.ss;
            a.p_img = pred_image_stride; a.p_pix = pred_pixel_stride; a.p_ch = pred_channel_stride;
            a.t_img = target_image_stride; a.t_pix = target_pixel_stride; a.t_ch = target_channel_stride;
            a.P = P; a.normalize = normalize;
            launch_gemm<11, kModeImage>(a, st);
        } else {
            a.src = ws + pl.tap[l - 1];
            a.sh = pl.oh[l - 1]; a.sw = pl.ow[l - 1];
            a.src_row = 2u * P * a.sh * a.sw;
            a.ih = pl.oh[l]; a.iw = pl.ow[l];           // stride 1, "same" padding: the input has the output's size
            if (l == 1) launch_gemm<5, kModeTapPooled>(a, st);
            else if (l == 2) launch_gemm<3, kModeTapPooled>(a, st);
            else launch_gemm<3, kModeTap>(a, st);
        }
        hipLaunchKernelGGL(k_epi_fwd, dim3(div_up(a.M * a.N, 256u)), dim3(256), 0, st, ws + pl.part, a.S, a.M, a.N,
                           image + kImg.bias + channel_offset(l), ws + pl.tap[l]);
    }
    DistArgs d{};
    for (int l = 0; l < kLayers; l++) {
        d.tap[l] = ws + pl.tap[l]; d.lin[l] = image + kImg.lin + channel_offset(l); d.dgrad[l] = ws + pl.dgrad[l];
        d.hw[l] = pl.oh[l] * pl.ow[l];
    }
    uint32_t part_at = 0;
    for (int l = 0; l < kLayers; l++) {
        d.part_off[l] = part_at;
        part_at += P * div_up(d.hw[l], kDistPos);
    }
    d.part = ws + pl.dist_part; d.vals = ws + pl.vals; d.P = P;
    hipLaunchKernelGGL(k_distance, dim3(div_up(d.hw[0], kDistPos), P, kLayers), dim3(256), 0, st, d);
    hipLaunchKernelGGL(k_value, dim3(div_up(P, 256u)), dim3(256), 0, st, d, value_out);
    return check_launch("percep_forward");
}

int rn_percep_backward(const float *image, void *workspace, size_t workspace_bytes, const float *upstream, uint32_t upstream_stride,
                       float *g_pred, int64_t g_image_stride, int64_t g_pixel_stride, int64_t g_channel_stride, uint32_t P,
                       uint32_t h, uint32_t w, int normalize, float *const *keep, rn_stream_t stream) {
    RN_REQUIRE(P > 0, "percep_backward: P must be positive");
    RN_REQUIRE(h >= kMinSide && w >= kMinSide, "percep_backward: %u x %u is below the smallest image, 31 x 31", h, w);
    RN_REQUIRE(image && workspace && upstream && g_pred, "percep_backward: null pointer");
    RN_REQUIRE(upstream_stride <= 1u, "percep_backward: upstream_stride must be 0 or 1");
    const Plan pl = make_plan(P, h, w);
    RN_REQUIRE(pl.total > 0, "percep_backward: unsupported shape P = %u, %u x %u", P, h, w);
    RN_REQUIRE(workspace_bytes >= pl.total * sizeof(float), "percep_backward: workspace of %zu bytes, rn_percep_workspace asks for %zu",
               workspace_bytes, (size_t)pl.total * sizeof(float));
    RN_REQUIRE(((uintptr_t)workspace & 15u) == 0, "percep_backward: workspace must be 16-byte aligned");
    hipStream_t st = as_stream(stream);
    float *ws = static_cast<float *>(workspace);
    for (int l = kLayers - 1; l >= 1; l--) {
        // gradient of conv l's input from the ReLU-masked gradient of tap l
        GemmArgs a{};
        const uint32_t hw = pl.oh[l] * pl.ow[l], N = P * hw;
        set_split(a, kCin[l], k_bwd(l), k_bwd(l), N);
        a.wt = image + kImg.bwd[l];
        a.part = ws + pl.part;
        a.src = ws + pl.grad[l]; a.mask = ws + pl.tap[l];
        a.src_row = N; a.mask_row = 2u * N;
        a.oh = a.ih = pl.oh[l]; a.ow = a.iw = pl.ow[l];
        if (l == 1) launch_gemm<5, kModeGrad>(a, st);
        else launch_gemm<3, kModeGrad>(a, st);
        const uint32_t MN = a.M * N;
        if (l >= 3) {
            hipLaunchKernelGGL(k_epi_bwd, dim3(div_up(MN, 256u)), dim3(256), 0, st, ws + pl.part, a.S, MN, ws + pl.dgrad[l - 1],
                               ws + pl.grad[l - 1]);
        } else {
            hipLaunchKernelGGL(k_epi_bwd, dim3(div_up(MN, 256u)), dim3(256), 0, st, ws + pl.part, a.S, MN, (const float *)nullptr,
                               ws + pl.pooled);
            const uint32_t sh = pl.oh[l - 1], sw = pl.ow[l - 1], n = kCout[l - 1] * P * sh * sw;
            hipLaunchKernelGGL(k_pool_route, dim3(div_up(n, 256u)), dim3(256), 0, st, ws + pl.pooled, ws + pl.dgrad[l - 1],
                               ws + pl.tap[l - 1], ws + pl.grad[l - 1], kCout[l - 1], P, sh, sw, pl.oh[l], pl.ow[l]);
        }
    }
    Conv1BwdArgs c{};
    c.wt = image + kImg.fwd[0]; c.grad = ws + pl.grad[0]; c.tap = ws + pl.tap[0]; c.ss = image + kImg.ss; c.upstream = upstream;
    c.g_pred = g_pred; c.g_img = g_image_stride; c.g_pix = g_pixel_stride; c.g_ch = g_channel_stride;
    c.P = P; c.h = h; c.w = w; c.oh = pl.oh[0]; c.ow = pl.ow[0]; c.upstream_stride = upstream_stride; c.normalize = normalize;
    hipLaunchKernelGGL(k_conv1_bwd, dim3(div_up(P * h * w * kC1Parts, 256u)), dim3(256), 0, st, c);
    if (keep)
        for (int l = 0; l < kLayers; l++)
            if (keep[l])
                (void)hipMemcpyAsync(keep[l], ws + pl.grad[l], (size_t)kCout[l] * P * pl.oh[l] * pl.ow[l] * sizeof(float),
                                     hipMemcpyDeviceToDevice, st);
    return check_launch("percep_backward");
}

}  // extern "C"
