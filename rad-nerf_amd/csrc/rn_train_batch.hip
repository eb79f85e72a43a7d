// rn_train_batch.hip -- the training step's input stage for a data set resident in device memory (C ABI: include/radnerf_train.h,
// rn_train_set_t).  What is computed: NeRFDataset.collate (nerf/provider.py:625-714) for one frame -- the torso-over-background
// blend, get_rays with N random pixels (nerf/utils.py:249-333), the face-rect mask, the gathers of bg_color / images / bg_coords,
// get_audio_features (:42-72) and convert_poses (:231-237): ~30 torch launches over the FULL frame there, ONE launch over the n
// picked pixels here.  The ray, the background coordinate and the pose 6-vector are the functions of rn_ray_dev.h that the frame
// prologue, rn_get_rays, rn_get_bg_coords and rn_convert_poses run, so the batch and a rendered frame agree bit for bit.
//
// Layout: one thread per picked pixel; its 3- and 2-float rows go out as one 12- / 8-byte store per lane, lane k at row k of the
// section, so a wave writes one contiguous span per section.  Which pixel a ray is comes from an index list, the kernel's own draw,
// a rect or a set of square patches (rn_train_set_batch / _rect / _patch: lip fine-tuning samples the last two,
// nerf/utils.py:277-303); everything after that is one body.  The reads are a coalesced int64 index, uniform (scalar) loads of the
// pose / rect, and three byte gathers of 3, 4 and 3 bytes per pixel, which the data layout makes inherent.  One extra workgroup
// writes the per-call outputs.  No LDS, no scratch, nothing that depends on the wave's width.
#include "rn_ray_dev.h"

#include "../../include/radnerf_train.h"

namespace rn {
namespace ts {

struct Out {
    float *packed;
    int64_t *inds_out;
    float *poses6, *pose_matrix, *eye, *auds;
    uint32_t *bad;
};

struct f3 { float x, y, z; };   // a row of a [n,3] section: one 12-byte store per lane
__device__ __forceinline__ void put3(float *__restrict__ section, size_t row, float x, float y, float z) {
    *reinterpret_cast<f3 *>(section + row * 3) = f3{x, y, z};
}

// np.float32(v) / np.float32(255): the loader's `astype(np.float32) / 255` (provider.py:671, 694), correctly rounded
__device__ __forceinline__ float decode(uint32_t v) { return __fdiv_rn((float)v, 255.0f); }
// provider.py:673: t * a + bg * (1 - a) as torch's three elementwise kernels round it (no contraction into an FMA)
__device__ __forceinline__ float over(float t, float a, float bg) {
    return __fadd_rn(__fmul_rn(t, a), __fmul_rn(bg, __fsub_rn(1.0f, a)));
}

// Pixel k of draw `draw` of stream `seed`: uniform in [0, HW) from the 32-bit mix of rn_common.h (multiply-high maps the 32 random
// bits onto the range; its bias is below HW / 2^32).  A function of (seed, draw, k) alone.
__host__ __device__ inline uint32_t drawn_pixel(uint32_t seed, uint32_t draw, uint32_t k, uint32_t HW) {
    const uint32_t h = mix32(mix32(mix32(k) ^ draw) ^ seed);
    return (uint32_t)(((uint64_t)h * HW) >> 32);
}

// poses6, the pose matrix, the eye value and the audio window (get_audio_features, nerf/utils.py:42-72; Fa >= 8 is checked on the
// host, so the reference's pads are plain zero rows)
__device__ __forceinline__ void per_call(const rn_train_set_t &s, uint32_t frame, uint32_t aud_frame, const Out &o) {
    const uint32_t t = threadIdx.x;
    const float *m = s.poses + (size_t)frame * 16;
    if (t < 16) o.pose_matrix[t] = m[t];
    if (t == 16) pose6_of(m, o.poses6);
    if (t == 17 && s.eye && o.eye) o.eye[0] = s.eye[frame];
    const uint32_t rows = s.att == 0 ? 1u : 8u, row_floats = s.C * 16u;
    const int32_t first = (int32_t)aud_frame - (s.att == 0 ? 0 : s.att == 1 ? 8 : 4);
    for (uint32_t e = t; e < rows * row_floats; e += blockDim.x) {
        const uint32_t row = e / row_floats;
        const int32_t src = first + (int32_t)row;
        o.auds[e] = (src >= 0 && src < (int32_t)s.Fa) ? s.auds[(size_t)src * row_floats + (e - row * row_floats)] : 0.0f;
    }
}

// Which pixel is ray k: the four instantiations of the kernel differ in nothing else.
//   kBatch  inds[k], or the draw above (get_rays' randint, nerf/utils.py:306)
//   kFrame  the evaluation form -- pixel k is ray k, no face section, target = images in both modes (provider.py:681-702 with
//           training = False)
//   kRect   every pixel of a rect in ascending order (torch.where of the rect's mask, nerf/utils.py:297-303)
//   kPatch  P square patches, each in meshgrid 'ij' order (nerf/utils.py:281-292)
enum Mode { kBatch = 0, kFrame = 1, kRect = 2, kPatch = 3 };
struct NoPick {};
struct RectPick { uint32_t xmin, ymin, w; };                        // x along the ROWS; w = ymax - ymin
struct PatchPick { const int32_t *corners; uint32_t patch, area; };  // corners [P,2] = (x0, y0) or null: drawn; area = patch^2
template <int MODE> struct PickOf { typedef NoPick type; };
template <> struct PickOf<kRect> { typedef RectPick type; };
template <> struct PickOf<kPatch> { typedef PatchPick type; };

// Top-left corner of patch q: explicit (clamped into the range the draw covers, counted in *bad by the patch's first ray), or
// drawn like a pixel -- x0 from element 2q, y0 from element 2q + 1 of (seed, draw).  The ranges are randint's of
// nerf/utils.py:282-283, [0, H - patch) and [0, W - patch): the last row and column of start positions are never drawn.
__device__ __forceinline__ void patch_corner(const PatchPick &pk, const rn_train_set_t &s, uint32_t q, bool first, uint32_t seed,
                                             uint32_t draw, uint32_t *bad, uint32_t &x0, uint32_t &y0) {
    const uint32_t nx = s.H - pk.patch, ny = s.W - pk.patch;
    if (pk.corners) {
        const int32_t x = pk.corners[2 * (size_t)q], y = pk.corners[2 * (size_t)q + 1];
        const bool out = x < 0 || x >= (int32_t)nx || y < 0 || y >= (int32_t)ny;
        if (out && first) atomicAdd(bad, 1u);
        x0 = x < 0 ? 0u : x >= (int32_t)nx ? nx - 1 : (uint32_t)x;
        y0 = y < 0 ? 0u : y >= (int32_t)ny ? ny - 1 : (uint32_t)y;
    } else {
        x0 = drawn_pixel(seed, draw, 2 * q, nx);
        y0 = drawn_pixel(seed, draw, 2 * q + 1, ny);
    }
}

template <int MODE>
__global__ void __launch_bounds__(256)
k_train_set(rn_train_set_t s, uint32_t frame, uint32_t aud_frame, const int64_t *__restrict__ inds, uint32_t n, uint32_t seed,
            uint32_t draw, Out o, typename PickOf<MODE>::type pick) {
    constexpr bool FRAME = MODE == kFrame;
    if (blockIdx.x == gridDim.x - 1) {   // the workgroup past the rays
        per_call(s, frame, aud_frame, o);
        return;
    }
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const uint32_t HW = s.H * s.W;
    uint32_t p;
    if (FRAME) {
        p = k;
    } else if constexpr (MODE == kRect) {
        const uint32_t i = k / pick.w;
        p = (pick.xmin + i) * s.W + pick.ymin + (k - i * pick.w);
        if (o.inds_out) o.inds_out[k] = (int64_t)p;
    } else if constexpr (MODE == kPatch) {
        const uint32_t q = k / pick.area, off = k - q * pick.area, i = off / pick.patch;
        uint32_t x0, y0;
        patch_corner(pick, s, q, off == 0, seed, draw, o.bad, x0, y0);
        p = (x0 + i) * s.W + y0 + (off - i * pick.patch);
        if (o.inds_out) o.inds_out[k] = (int64_t)p;
    } else {
        if (inds) {
            int64_t v = inds[k];
            if (v < 0 || v >= (int64_t)HW) {
                atomicAdd(o.bad, 1u);
                v = v < 0 ? 0 : (int64_t)HW - 1;
            }
            p = (uint32_t)v;
        } else {
            p = drawn_pixel(seed, draw, k, HW);
        }
        if (o.inds_out) o.inds_out[k] = (int64_t)p;
    }
    const uint32_t r = p / s.W, c = p - r * s.W;
    const size_t N = n;
    float *rays_o = o.packed, *rays_d = o.packed + 3 * N, *bg_coords = o.packed + 6 * N, *bg_color = o.packed + 8 * N,
          *target = o.packed + 11 * N;

    float ro[3], rd[3];
    pinhole_ray(p, s.W, s.fx, s.fy, s.cx, s.cy, s.poses + (size_t)frame * 16, ro, rd);
    put3(rays_o, k, ro[0], ro[1], ro[2]);
    put3(rays_d, k, rd[0], rd[1], rd[2]);
    float2 bc;
    bg_coord_of(r, c, s.H, s.W, bc.x, bc.y);
    *reinterpret_cast<float2 *>(bg_coords + 2 * (size_t)k) = bc;   // 8-byte aligned: the section starts 24 n bytes into `packed`

    const size_t px = (size_t)frame * HW + p;
    const uchar4 t = *reinterpret_cast<const uchar4 *>(s.torso + px * 4);
    const uint8_t *b = s.bg + (size_t)p * 3;
    const float a = decode(t.w), b0 = decode(b[0]), b1 = decode(b[1]), b2 = decode(b[2]);
    const float m0 = over(decode(t.x), a, b0), m1 = over(decode(t.y), a, b1), m2 = over(decode(t.z), a, b2);
    if (FRAME || !s.torso_mode) {
        const uint8_t *im = s.images + px * 3;
        put3(target, k, decode(im[0]), decode(im[1]), decode(im[2]));
    } else {
        put3(target, k, m0, m1, m2);   // the loader's bg_torso_color (provider.py:686-688)
    }
    if (s.torso_mode) put3(bg_color, k, b0, b1, b2);
    else put3(bg_color, k, m0, m1, m2);
    if (!FRAME) {
        const int32_t *rect = s.face_rect + (size_t)frame * 4;   // (xmin, xmax, ymin, ymax), x along the rows (provider.py:657-658)
        const int32_t ri = (int32_t)r, ci = (int32_t)c;
        o.packed[14 * N + k] = (rect[0] <= ri && ri < rect[1] && rect[2] <= ci && ci < rect[3]) ? 1.0f : 0.0f;
    }
}

static int check_set(const rn_train_set_t *s, uint32_t frame, uint32_t aud_frame) {
    RN_REQUIRE(s, "train_set: null descriptor");
    RN_REQUIRE(s->images && s->torso && s->bg && s->poses && s->face_rect && s->auds, "train_set: null pointer in the descriptor");
    RN_REQUIRE(((uintptr_t)s->torso & 3u) == 0, "train_set: the torso RGBA array must be 4-byte aligned");
    RN_REQUIRE(s->H >= 2 && s->W >= 2 && (uint64_t)s->H * s->W < (1ull << 31), "train_set: H, W >= 2 and H * W < 2^31 are required");
    RN_REQUIRE(s->fx != 0.0f && s->fy != 0.0f, "train_set: bad intrinsics");
    RN_REQUIRE(s->att <= 2 && s->torso_mode <= 1, "train_set: att must be 0, 1 or 2 and torso_mode 0 or 1");
    RN_REQUIRE(s->C >= 1 && s->C <= (1u << 20), "train_set: audio feature channels out of range");
    RN_REQUIRE(s->Fa >= 8, "train_set: Fa = %u audio frames; at least 8 are required (the window's padding below that is not restated)", s->Fa);
    RN_REQUIRE(frame < s->F, "train_set: frame %u is outside the %u frames of the set", frame, s->F);
    RN_REQUIRE(aud_frame < s->Fa, "train_set: audio frame %u is outside the %u audio frames of the set", aud_frame, s->Fa);
    return RN_OK;
}

}  // namespace ts
}  // namespace rn

using namespace rn;
using namespace rn::ts;

extern "C" int rn_train_set_batch(const rn_train_set_t *set, uint32_t frame, uint32_t aud_frame, const int64_t *inds, uint32_t n,
                                  uint32_t seed, uint32_t draw, float *packed, int64_t *inds_out, float *poses6, float *pose_matrix,
                                  float *eye, float *auds_out, uint32_t *bad, rn_stream_t stream) {
    if (n == 0) return RN_OK;
    if (int rc = check_set(set, frame, aud_frame)) return rc;
    RN_REQUIRE(packed && poses6 && pose_matrix && auds_out && bad, "train_set_batch: null pointer");
    RN_REQUIRE(((uintptr_t)packed & 7u) == 0, "train_set_batch: packed must be 8-byte aligned");
    RN_REQUIRE(n < (1u << 31), "train_set_batch: n must be below 2^31");
    const Out o{packed, inds_out, poses6, pose_matrix, eye, auds_out, bad};
    hipLaunchKernelGGL(k_train_set<kBatch>, dim3(div_up(n, 256) + 1), dim3(256), 0, as_stream(stream), *set, frame, aud_frame, inds, n,
                       seed, draw, o, NoPick{});
    return check_launch("train_set_batch");
}

extern "C" int rn_train_set_batch_rect(const rn_train_set_t *set, uint32_t frame, uint32_t aud_frame, int32_t xmin, int32_t xmax,
                                       int32_t ymin, int32_t ymax, float *packed, int64_t *inds_out, float *poses6,
                                       float *pose_matrix, float *eye, float *auds_out, rn_stream_t stream) {
    if (int rc = check_set(set, frame, aud_frame)) return rc;
    RN_REQUIRE(0 <= xmin && xmin < xmax && xmax <= (int32_t)set->H && 0 <= ymin && ymin < ymax && ymax <= (int32_t)set->W,
               "train_set_batch_rect: rect (%d, %d, %d, %d) is empty or outside the %u x %u image (0 <= xmin < xmax <= H and "
               "0 <= ymin < ymax <= W are required)", xmin, xmax, ymin, ymax, set->H, set->W);
    RN_REQUIRE(packed && poses6 && pose_matrix && auds_out, "train_set_batch_rect: null pointer");
    RN_REQUIRE(((uintptr_t)packed & 7u) == 0, "train_set_batch_rect: packed must be 8-byte aligned");
    const uint32_t w = (uint32_t)(ymax - ymin), n = (uint32_t)(xmax - xmin) * w;   // <= H * W < 2^31 (check_set)
    const Out o{packed, inds_out, poses6, pose_matrix, eye, auds_out, nullptr};
    hipLaunchKernelGGL(k_train_set<kRect>, dim3(div_up(n, 256) + 1), dim3(256), 0, as_stream(stream), *set, frame, aud_frame,
                       (const int64_t *)nullptr, n, 0u, 0u, o, RectPick{(uint32_t)xmin, (uint32_t)ymin, w});
    return check_launch("train_set_batch_rect");
}

extern "C" int rn_train_set_batch_patch(const rn_train_set_t *set, uint32_t frame, uint32_t aud_frame, const int32_t *corners,
                                        uint32_t P, uint32_t patch, uint32_t seed, uint32_t draw, float *packed, int64_t *inds_out,
                                        float *poses6, float *pose_matrix, float *eye, float *auds_out, uint32_t *bad,
                                        rn_stream_t stream) {
    if (int rc = check_set(set, frame, aud_frame)) return rc;
    RN_REQUIRE(patch >= 2 && patch < set->H && patch < set->W, "train_set_batch_patch: patch = %u; 2 <= patch < H and patch < W are required "
               "(H = %u, W = %u)", patch, set->H, set->W);
    RN_REQUIRE(P >= 1, "train_set_batch_patch: P >= 1 patches are required");
    RN_REQUIRE((uint64_t)P * patch * patch < (1ull << 31), "train_set_batch_patch: P * patch^2 must be below 2^31");
    RN_REQUIRE(packed && poses6 && pose_matrix && auds_out && bad, "train_set_batch_patch: null pointer");
    RN_REQUIRE(((uintptr_t)packed & 7u) == 0, "train_set_batch_patch: packed must be 8-byte aligned");
    const uint32_t area = patch * patch, n = P * area;
    const Out o{packed, inds_out, poses6, pose_matrix, eye, auds_out, bad};
    hipLaunchKernelGGL(k_train_set<kPatch>, dim3(div_up(n, 256) + 1), dim3(256), 0, as_stream(stream), *set, frame, aud_frame,
                       (const int64_t *)nullptr, n, seed, draw, o, PatchPick{corners, patch, area});
    return check_launch("train_set_batch_patch");
}

extern "C" int rn_train_set_frame(const rn_train_set_t *set, uint32_t frame, uint32_t aud_frame, float *packed, float *poses6,
                                  float *pose_matrix, float *eye, float *auds_out, rn_stream_t stream) {
    if (int rc = check_set(set, frame, aud_frame)) return rc;
    RN_REQUIRE(packed && poses6 && pose_matrix && auds_out, "train_set_frame: null pointer");
    RN_REQUIRE(((uintptr_t)packed & 7u) == 0, "train_set_frame: packed must be 8-byte aligned");
    const uint32_t n = set->H * set->W;
    const Out o{packed, nullptr, poses6, pose_matrix, eye, auds_out, nullptr};
    hipLaunchKernelGGL(k_train_set<kFrame>, dim3(div_up(n, 256) + 1), dim3(256), 0, as_stream(stream), *set, frame, aud_frame,
                       (const int64_t *)nullptr, n, 0u, 0u, o, NoPick{});
    return check_launch("train_set_frame");
}
