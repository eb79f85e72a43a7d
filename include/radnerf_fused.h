/*
 * radnerf_fused.h -- C ABI of the MI355X-native fused render path of libradnerf_hip.so.
 *
 * These entry points have no single counterpart among the reference's pybind functions: they replace
 * whole stretches of its Python hot loop with a handful of gfx950 kernels, while computing exactly what
 * that loop computes:
 *
 *   rn_nerf_fused_forward   NeRFNetwork.forward (nerf/network.py:222-283): xyz grid -> [enc_x | enc_a] ->
 *                           ambient MLP -> tanh -> ambient grid -> [enc_x | enc_w | eye] -> sigma MLP ->
 *                           exp, SH(d) -> [enc_d | geo | ind] -> color MLP -> sigmoid, per sample, as ONE
 *                           kernel: hash/tiled-grid gathers + fp32 MFMA (v_mfma_f32_32x32x2_f32) tiles with the
 *                           weights resident in LDS; the broadcast inputs (audio code, eye, individual code)
 *                           are folded into per-frame bias vectors (rn_nerf_frame_bias).
 *   rn_head_begin /         the inference branch of NeRFRenderer.run_cuda (nerf/renderer.py:183, 225-262):
 *   rn_head_iterate         near/far, then the <= max_steps loop {march, network, composite, compact}.  The
 *                           live-ray count, the n_step policy max(min(N // n_alive, 8), 1) and the loop
 *                           condition live in device memory, so the host enqueues the loop without reading
 *                           anything back; compaction is a stable wavefront ballot/prefix-sum scatter.
 *   rn_torso_fused          the torso pass (nerf/renderer.py:269-299 + nerf/network.py:188-219): bilinear
 *                           occupancy test, deformation MLP, 2-D grid, torso MLP, blend over the background.
 *   rn_blend_frame          image + (1 - weights_sum) * bg, clamp, depth normalisation (renderer.py:306-311).
 *
 * Conventions are those of radnerf_hip.h (device pointers, caller allocates, explicit stream, int status).
 * Supported network shape (validated; anything else returns RN_ERR_INVALID_ARG and the caller must use the
 * per-operator path): grids L=16, C=2 (xyz D=3, ambient/torso D=2), hidden width 64, geo_feat 64, SH degree
 * 4, ambient_dim 2; audio_dim, eye and individual-code widths are free (they only enter the bias vectors).
 */
#ifndef RADNERF_FUSED_H
#define RADNERF_FUSED_H

#include "radnerf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One multiresolution grid as GridEncoder holds it (gridencoder/grid.py:96-161). */
typedef struct {
    const void *embeddings;  /* [rows, 2], float32 or float16 */
    const int32_t *offsets;  /* [L+1] */
    uint32_t D, L, H;        /* input dim, levels (16), base resolution */
    float S;                 /* log2(per_level_scale) */
    uint32_t gridtype;       /* 0 hash, 1 tiled */
    int dtype;               /* RN_F32 / RN_F16 */
} rn_grid_t;

/* Raw nn.Linear weights ([out, in] row-major, bias-free) of the per-sample MLPs (nerf/network.py:140-167). */
typedef struct {
    const float *amb_w0, *amb_w1, *amb_w2; /* ambient_net: [64, 32+audio_dim] [64,64] [2,64]      */
    const float *sig_w0, *sig_w1, *sig_w2; /* sigma_net:   [64, 64+has_eye]   [64,64] [65,64]     */
    const float *col_w0, *col_w1;          /* color_net:   [64, 80+ind_dim]   [3,64]              */
    uint32_t audio_dim, has_eye, ind_dim;
} rn_nerf_weights_t;

/* Number of floats of the packed (MFMA-ordered) weight image / of the per-frame bias block. */
size_t rn_nerf_packed_floats(void);
/* Opt-in 16-bit matrix-core variant (mlp_dtype = RN_F16 below): weights and per-sample activations are rounded to fp16
 * where they enter the f16 matrix instruction (v_mfma_f32_32x32x8f16), accumulation stays fp32 -- the arithmetic of the reference's `-O`
 * (autocast) mode, nerf/utils.py:944.  Grid interpolation, per-frame bias vectors, the narrow output layers and the
 * activations stay fp32.  Its weight image has its own size and packer; `packed` passed to rn_nerf_fused_forward /
 * rn_head_iterate must be the image that matches `mlp_dtype` (RN_F32: rn_nerf_pack_weights). */
size_t rn_nerf_packed_floats_h16(void);
int rn_nerf_pack_weights_h16(const rn_nerf_weights_t *w, float *packed, rn_stream_t stream);
/* Split-precision variant (mlp_dtype = RN_F32_SPLIT): fp32-grade contractions on the 16-bit matrix cores.  Every operand
 * is carried as two fp16 numbers (hi = fp16(v), lo = fp16(v - hi): 22 significant bits) and a product is evaluated as
 * hi*hi + hi*lo + lo*hi with fp32 accumulation on v_mfma_f32_32x32x8f16 (~3e-7 relative per product).  It meets the
 * tolerances of the fp32-MFMA kernel against the fp32 oracle; it is NOT bit-identical to it. */
#define RN_F32_SPLIT 2
size_t rn_nerf_packed_floats_split(void);
int rn_nerf_pack_weights_split(const rn_nerf_weights_t *w, float *packed, rn_stream_t stream);
size_t rn_nerf_bias_floats(void);
/* Re-order the raw weights into the image the fused kernel stages into LDS (call when weights change).  The fp32 and the
 * split image hold color_net's geo_feat columns already multiplied by sigma_net's geo_feat rows (one 64 x 64 product,
 * summed in double): those kernels feed the colour net from the sigma net's last hidden layer and never form geo_feat. */
int rn_nerf_pack_weights(const rn_nerf_weights_t *w, float *packed, rn_stream_t stream);
/* Per-frame bias vectors: W0_amb[:,32:] enc_a | W0_sig[:,64] eye | W0_col[:,80:] ind_code  (3 x 64). */
int rn_nerf_frame_bias(const rn_nerf_weights_t *w, const float *enc_a, const float *eye, const float *ind_code,
                       float *bias, rn_stream_t stream);
/* The same for n frames at once: enc_a [n, audio_dim] -> bias [n, rn_nerf_bias_floats()] (eye / ind_code shared). */
int rn_nerf_frame_bias_batch(const rn_nerf_weights_t *w, const float *enc_a, uint32_t n, const float *eye, const float *ind_code,
                             float *bias, rn_stream_t stream);

/* NeRFNetwork.forward for M sample slots.  deltas (nullable): when given, slots with deltas[2*i] == 0 are
 * dead (raymarching.cu:982) and skipped -- their outputs are left untouched.  m_dev (nullable): device
 * count of slots, overrides M (M is then only the launch bound).  ambient (nullable): [M,2] output.
 * rgbs == NULL (dirs may then be NULL too): density query -- NeRFNetwork.density (nerf/network.py:286-325), sigma only; the
 * fp32 kernel then skips the SH basis and the colour network (a quarter of its matrix instructions). */
int rn_nerf_fused_forward(const float *xyzs, const float *dirs, const float *deltas, uint32_t M,
                          const int32_t *m_dev, const rn_grid_t *grid_xyz, const rn_grid_t *grid_amb,
                          const float *packed, const float *bias, float bound, float *sigmas, float *rgbs,
                          float *ambient, int mlp_dtype, rn_stream_t stream);

/* ---- dense image of a hash grid's coarser levels (inference) ------------------------------------------------------
 * A hashed level spreads the corners of neighbouring cells over its whole slice of the table.  While the table does not change
 * the level can be stored once as its whole lattice instead,
 *     image[image_offsets[l] + x + y (R+1) + z (R+1)^2] = table[offsets[l] + hash(x, y, z) % size_l],      x, y, z in 0..R,
 * and a descriptor {embeddings = image, offsets = image_offsets, everything else as in `grid`} then takes every kernel that
 * reads an rn_grid_t down the dense path it has for the coarse levels: a level is dense when its slice holds (R+1)^3 rows,
 * which is decided from the offsets alone.  Same rows, blended in the same order: the features are bit-identical.
 *
 * rn_grid_dense_plan (host only, launches nothing): which levels to store that way.  Hashed levels are taken in ascending
 * order while the whole image stays within budget_bytes, below 4 GiB (the kernels form 32-bit byte offsets) and below 2^31
 * rows; a taken level gets (R+1)^3 rows rounded up to a multiple of 8, every other level keeps its size and its rows.
 * Writes image_offsets [L+1] (host, in rows), *levels (bit l: level l is taken) and *image_bytes.  Returns 1, or 0 = "no
 * image" (tiled grid, D != 3, or no hashed level fits: keep the table; nothing is written), or a negative error.
 * rn_grid_dense_build: fills `image` (image_bytes from the plan, 16-byte aligned) from the table, one launch per level;
 * the rows of a taken level past (R+1)^3 are zero.  offsets_host / image_offsets are host arrays. */
int rn_grid_dense_plan(const rn_grid_t *grid, const int32_t *offsets_host, size_t budget_bytes, int32_t *image_offsets,
                       uint32_t *levels, size_t *image_bytes);
int rn_grid_dense_build(const rn_grid_t *grid, const int32_t *offsets_host, const int32_t *image_offsets, uint32_t levels,
                        void *image, size_t image_bytes, rn_stream_t stream);

/* ---- device-side inference loop ------------------------------------------------------------------ */
#define RN_HEAD_STATE_INTS 64 /* int32 words of loop state the caller provides (zeroed once before first use) */

typedef struct {
    /* inputs */
    const float *rays_o, *rays_d; /* [N,3] */
    uint32_t N;
    const float *aabb;            /* [6] */
    float min_near;
    const uint8_t *bitfield;
    float bound, dt_gamma;
    uint32_t max_steps, cascade, grid_size;
    float T_thresh;
    /* outputs */
    float *nears, *fars;                  /* [N] */
    float *weights_sum, *depth, *image;   /* [N] [N] [N,3] (zeroed by rn_head_begin) */
    /* scratch, caller-allocated: N slots are always enough (n_alive * n_step <= N) */
    int32_t *rays_alive_a, *rays_alive_b; /* [N] each */
    float *rays_t;                        /* [N] */
    float *xyzs, *dirs, *deltas;          /* [N,3] [N,3] [N,2] */
    float *sigmas, *rgbs;                 /* [N] [N,3] */
    int32_t *state;                       /* [RN_HEAD_STATE_INTS] */
    uint32_t *block_counts;               /* [3 * (ceil(N/256) + 1)]: survivor counts | live-sample partial sums x 2; zeroed once
                                             before first use when RN_LOOP_COOP is used */
    int32_t *live_slots;                  /* [N] or NULL.  Scratch for the list of live sample slots of an iteration: the
                                             marchers write it and the network kernel then runs over st[6] live samples
                                             instead of all n_alive * n_step slots (rays that end in the middle of their
                                             n_step samples leave dead slots: 16 % of the benchmark stream).  NULL: the
                                             network visits every slot and skips the dead ones.  Same pixels either way. */
    uint32_t order_w;                     /* 0: alive list starts in ray order.  Image width W (rays are row-major pixels,
                                             W % 8 == 0, N % W == 0, (N / W) % 8 == 0; otherwise treated as 0): the list
                                             starts in 8 x 8 pixel blocks, so neighbouring samples share more grid rows.
                                             Speed only -- rays are independent, every pixel is unchanged. */
    const int32_t *occ_box;               /* [8] as rn_occ_box wrote it for THIS bitfield, or NULL.  With one cascade and a constant
                                             step, a ray steps over the lattice points in front of the box around the set bits
                                             without looking their cells up and ends its walk where it leaves that box, instead of
                                             testing every cell up to `far`.  Speed only: no set bit lies outside the box, so the
                                             samples are the same, bit for bit.  NULL (and every other configuration): the full walk. */
    float *dir_term;                      /* [N][64], 16-byte aligned (N <= 2^24), or NULL.  Scratch, never zeroed: the colour net's
                                             first layer starts from a term that depends on the ray's direction and the frame's
                                             bias only (bias + 8 MFMA steps over SH(dir)), the same for every sample of a ray.  The
                                             fp32 network launch of loop iteration 0 stores it from every live sample's own
                                             accumulators, the launches of iterations >= 1 load it instead of recomputing it (a ray
                                             that reaches iteration 1 had a live sample in iteration 0).  Speed only: the loaded
                                             term is the value the sample would compute, bit for bit.  NULL (and RN_F16 /
                                             RN_F32_SPLIT): every sample computes its own.  rn_head_iterate_ex decides by the
                                             iteration number, so a loop enqueued over several calls works the same; a frame's loop
                                             starts at iteration 0. */
} rn_head_t;

/* near/far + loop initialisation (rays_alive = arange(N), rays_t = nears, accumulators = 0, step = 0). */
int rn_head_begin(const rn_head_t *h, rn_stream_t stream);
/* Enqueue loop iterations first_iter .. first_iter + n_iters - 1.  Iterations past the end of the loop
 * (step >= max_steps or no ray alive) are no-ops decided on the device.  Kernels per call: march(first_iter), then per
 * iteration {fused network, composite, compaction}; inside a call the compaction kernel also marches the next iteration
 * (3 launches per iteration), the last compaction of a call does not -- so a loop enqueued one iteration per call is the
 * plain four-kernel sequence and its schedule may be adjusted between calls (rn_head_reschedule).  mlp_dtype selects the
 * arithmetic variant of the network kernel (RN_F32 / RN_F32_SPLIT / RN_F16) and must match the packed image. */
int rn_head_iterate(const rn_head_t *h, const rn_grid_t *grid_xyz, const rn_grid_t *grid_amb, const float *packed,
                    const float *bias, uint32_t first_iter, uint32_t n_iters, int mlp_dtype, rn_stream_t stream);
/* The same loop with options (flags):
 *   RN_LOOP_FIRST_MARCHED  iteration first_iter has been marched already (rn_frame_begin marches iteration 0 inside the prologue
 *                          kernel), so the call starts with the network launch;
 *   RN_LOOP_CLOSE_FRAME    the call's last compaction is the frame's last: it also does what rn_head_check_done does (flags the
 *                          frame in state[RN_HEAD_ST_UNFINISHED] when the loop was still active) and leaves both live-sample
 *                          counters (state[6], state[14]) at zero, which rn_frame_begin relies on;
 *   RN_LOOP_COOP           compositor + compaction (+ next march) of an iteration run as ONE launch with a grid-wide barrier inside
 *                          (2 launches per iteration instead of 3; same results; slower than the split form: 2 % with a plain launch, 15 % with the
 *                          cooperative launch it now uses for the residency guarantee).  The launch
 *                          needs its <= 512 workgroups of 256 threads resident together: it is a COOPERATIVE launch
 *                          (hipLaunchCooperativeKernel), which the runtime places whole or refuses -- a refusal comes back as
 *                          RN_ERR_INVALID_ARG and the caller falls back to the split loop.  Should a workgroup ever give up waiting
 *                          at the barrier, state[RN_HEAD_ST_STALLED] counts it AND the frame is flagged in
 *                          state[RN_HEAD_ST_UNFINISHED] like a frame whose loop was cut short: it must be rendered again. */
#define RN_LOOP_FIRST_MARCHED 1u
#define RN_LOOP_CLOSE_FRAME 2u
#define RN_LOOP_COOP 4u
int rn_head_iterate_ex(const rn_head_t *h, const rn_grid_t *grid_xyz, const rn_grid_t *grid_amb, const float *packed,
                       const float *bias, uint32_t first_iter, uint32_t n_iters, int mlp_dtype, uint32_t flags,
                       rn_stream_t stream);
/* Frame prologue in ONE launch: ray generation (pose != NULL: get_rays with N = -1, nerf/utils.py:249-333, written to
 * h->rays_o / h->rays_d, which must then be writable; pose: device pointer to a row-major [3,4] / [4,4] cam2world matrix, W =
 * image width) + near/far + loop initialisation (= rn_head_begin) + the march of iteration 0 (n_step = 1).  Follow with
 * rn_head_iterate_ex(..., first_iter = 0, flags = RN_LOOP_FIRST_MARCHED | RN_LOOP_CLOSE_FRAME).  h->state[6] must be zero on
 * entry (a zeroed state block on first use; afterwards RN_LOOP_CLOSE_FRAME keeps it so). */
int rn_frame_begin(const rn_head_t *h, const float *pose, float fx, float fy, float cx, float cy, uint32_t W,
                   rn_stream_t stream);
/* Step schedule of a SHARD of a frame (tile-parallel rendering, BASELINE config 4).  The reference's policy
 * n_step = max(min(N // n_alive, 8), 1) (nerf/renderer.py:249) uses the ray count and the live count of the whole
 * call; a rank that renders only a band of the image reproduces the whole-frame schedule (and so the whole-frame
 * pixels: `step += n_step` may overshoot max_steps, so the schedule is visible in the image) by calling this after
 * iteration `iter_done` with schedule_N = rays of the whole frame and *alive_total = live rays of the whole frame
 * for the coming iteration (the all-reduced sum of each rank's state[((iter_done + 1) & 1) * 8 + 0]).  Only
 * n_step and the slot count of the coming iteration are rewritten; everything stays on the device. */
int rn_head_reschedule(const rn_head_t *h, uint32_t iter_done, uint32_t schedule_N, const int32_t *alive_total,
                       rn_stream_t stream);
/* Layout of h->state (int32 words).  Words 0..15 are the loop state, reset by rn_head_begin; words 16.. are
 * statistics that ACCUMULATE across frames (wrapping int32; the caller zeroes them when it wants to). */
#define RN_HEAD_ST_ACTIVE 4      /* state[(iter & 1) * 8 + 4]: 1 while the loop wants another iteration */
#define RN_HEAD_ST_ITERS 16      /* iterations that did work */
#define RN_HEAD_ST_LIVE 17       /* live samples evaluated */
#define RN_HEAD_ST_SLOTS 18      /* sample slots n_alive * n_step summed over iterations */
#define RN_HEAD_ST_UNFINISHED 19 /* frames whose loop was still active when rn_head_check_done looked (see below) */
#define RN_HEAD_ST_BARRIER 20    /* launch counter of the RN_LOOP_COOP kernels (tags the survivor counts of a launch; never reset) */
#define RN_HEAD_ST_STALLED 22    /* RN_LOOP_COOP: workgroups that gave up waiting at the in-launch barrier (must stay 0; a frame
                                    rendered while it moved is invalid and has to be rendered again without RN_LOOP_COOP) */
#define RN_HEAD_ST_HIST 32       /* state[32 + i], i = 0 .. max_steps (<= 31): live rays entering loop iteration i of the frame in
                                    flight (0 once the loop is over).  A shard of a frame publishes these so the ranks can verify,
                                    after the fact, that their band-local step schedules were the whole frame's (radnerf/parallel.py) */
/* Speculative loop length.  A caller that knows how many iterations frames of this stream need (device counters of
 * earlier frames) may enqueue fewer than max_steps iterations and skip the no-op launches behind them; this entry point
 * then records, on the device, whether the loop really was over after iteration iters_done - 1: if it was not,
 * state[RN_HEAD_ST_UNFINISHED] is incremented and the caller must render that frame again with more iterations (the
 * count is checked whenever the caller synchronises anyway).  Never needed when all max_steps iterations are enqueued. */
int rn_head_check_done(const rn_head_t *h, uint32_t iters_done, rn_stream_t stream);

/* ---- torso + blend ----------------------------------------------------------------------------------- */
typedef struct {
    const float *def_w0, *def_w1, *def_w2; /* torso_deform_net: [64, 96+ind] [64,64] [2,64]  */
    const float *tor_w0, *tor_w1, *tor_w2; /* torso_net:        [32, 128+ind] [32,32] [4,32] */
    uint32_t ind_dim;
} rn_torso_weights_t;

size_t rn_torso_packed_floats(void);
int rn_torso_pack_weights(const rn_torso_weights_t *w, float *packed, rn_stream_t stream);
/* bg_out[i] = torso_color * alpha + bg_in[i] * (1 - alpha) for pixels whose bilinear torso occupancy exceeds
 * `thresh`, else bg_in[i].  bg_in may be NULL (= white, the reference's `bg_color = 1`).
 * torso_alpha (nullable) [N], deform (nullable) [N,2] receive the per-pixel values (0 where masked out). */
int rn_torso_fused(const float *bg_coords, uint32_t N, const float *density_grid_torso, uint32_t grid_size,
                   float thresh, const float *poses6, const float *ind_code, float torso_shrink,
                   const rn_torso_weights_t *w, const float *packed, const rn_grid_t *grid_torso,
                   const float *bg_in, float *bg_out, float *torso_alpha, float *deform, rn_stream_t stream);

/* rn_torso_fused + rn_blend_frame in one pass over the pixels (frame epilogue): the blended background never goes to
 * memory unless bg_out is given (nullable, like torso_alpha). */
int rn_torso_blend_frame(const float *bg_coords, uint32_t N, const float *density_grid_torso, uint32_t grid_size,
                         float thresh, const float *poses6, const float *ind_code, float torso_shrink,
                         const rn_torso_weights_t *w, const float *packed, const rn_grid_t *grid_torso, const float *bg_in,
                         float *bg_out, float *torso_alpha, float *image, const float *weights_sum, float *depth,
                         const float *nears, const float *fars, uint8_t *image_u8, rn_stream_t stream);

/* ---- torso plan: the frame-invariant half of rn_torso_blend_frame, built once per view ---------------------
 * Of the torso pass, the occupancy test and enc_x = freq(x * shrink, 10) -- 40 sines and cosines per covered pixel, two
 * thirds of the pass's vector instructions -- depend only on (bg_coords, density_grid_torso, thresh, torso_shrink): a
 * renderer hands the same pixel grid to every frame, and only the pose and the individual code change.  A plan keeps the
 * covered pixels (ascending), a per-pixel flag and enc_x of the covered pixels as matrix operands, 168 B per covered pixel;
 * the planned frame call runs the covered pixels as dense 32-pixel tiles and blends the rest.  Its outputs equal
 * rn_torso_blend_frame's bit for bit (the same products summed in the same order).  A plan is valid for exactly the inputs
 * it was built from; the caller rebuilds it when one of them changes.
 *
 *   rn_torso_plan_bytes   bytes of a plan of N pixels of which n_on are covered (n_on = 0: the part every build needs).
 *   rn_torso_plan_build   `plan` (device, 256-byte aligned, plan_bytes >= rn_torso_plan_bytes(N, 0)).  Finds the covered
 *                         pixels, waits for the stream and stores their count in *n_on; writes enc_x when plan_bytes
 *                         >= rn_torso_plan_bytes(N, *n_on) -- otherwise the caller allocates that much and calls again.
 *                         An error while the stream is capturing.
 *   rn_torso_blend_frame_planned   rn_torso_blend_frame over a complete plan (n_on as the build returned it); `deform`
 *                         (nullable) [N,2] as rn_torso_fused writes it.  One launch. */
/* 256 MiB: callers keep to rn_torso_blend_frame where a plan would be larger */
#define RN_TORSO_PLAN_MAX_BYTES 268435456
size_t rn_torso_plan_bytes(uint32_t N, uint32_t n_on);
int rn_torso_plan_build(const float *bg_coords, uint32_t N, const float *density_grid_torso, uint32_t grid_size, float thresh,
                        float torso_shrink, void *plan, size_t plan_bytes, uint32_t *n_on, rn_stream_t stream);
int rn_torso_blend_frame_planned(const void *plan, size_t plan_bytes, uint32_t N, uint32_t n_on, const float *poses6,
                                 const float *ind_code, float torso_shrink, const rn_torso_weights_t *w, const float *packed,
                                 const rn_grid_t *grid_torso, const float *bg_in, float *bg_out, float *torso_alpha,
                                 float *deform, float *image, const float *weights_sum, float *depth, const float *nears,
                                 const float *fars, uint8_t *image_u8, rn_stream_t stream);

/* mask[i] = 1 where the bilinear torso occupancy at bg_coords[i] exceeds `thresh` (F.grid_sample(bilinear, zeros,
 * align_corners=True) > thresh, nerf/renderer.py:281-283) -- the test rn_torso_fused applies per pixel, exposed for the
 * differentiable training formulation that gathers those pixels. */
int rn_torso_mask(const float *bg_coords, uint32_t N, const float *density_grid_torso, uint32_t grid_size, float thresh,
                  uint8_t *mask, rn_stream_t stream);

/* image = clamp(image + (1 - weights_sum) * bg, 0, 1); depth = max(depth - near, 0) / (far - near);
 * optional uint8 quantisation of the frame (image_u8 nullable): floor(image * 255). */
int rn_blend_frame(float *image, const float *weights_sum, const float *bg, float *depth, const float *nears,
                   const float *fars, uint32_t N, uint8_t *image_u8, rn_stream_t stream);

/* ---- occupancy-grid maintenance -------------------------------------------------------------------
 * NeRFRenderer.update_extra_state (nerf/renderer.py:383-499) and mark_untrained_grid (:318-379) without the Python block
 * loops: the cells are enumerated in MORTON order (element i of cascade c = the cell with morton code i), so the sample
 * buffer of the density query and the density grid share their indexing and nothing is ever scattered.
 *
 *   rn_occupancy_points      xyzs[C*H^3, 3]: cell centre (2 c / (H-1) - 1) * (bound_c - bound_c / H) + (u * 2 - 1) * bound_c / H
 *                            with u from `noise` ([C*H^3, 3] uniform [0,1), torch.rand_like in the reference) or, noise ==
 *                            NULL, from a counter-based hash of (seed, element index) -- rn_hash_u01_bits() * 2^-24.
 *   (density query)          rn_nerf_fused_forward(xyzs, NULL, NULL, C*H^3, ..., sigmas, rgbs = NULL, ...): sigma only.
 *   rn_occupancy_update      tmp = sigmas * density_scale; 6-neighbour max in morton space (raymarching.cu:304-341); where
 *                            grid >= 0 and tmp >= 0: grid = max(grid * decay, tmp); stats[0] = mean(max(grid, 0)) (summed in
 *                            double), stats[1] = min(stats[0], density_thresh); bitfield = packbits(grid, stats[1]).
 *                            workspace: rn_occupancy_workspace(C, H) bytes (per-workgroup partial sums; a one-workgroup
 *                            launch adds them up).  Nothing is read back by the host.
 *   rn_mark_untrained_grid   grid[c, cell] = -1 for cells no camera sees: poses [n, 4, 4] (pose_stride = 16 floats) or
 *                            [n, 3, 4] (12) cam2world, intrinsics as the Python floats fx, fy, cx, cy.
 *   rn_torso_grid_points     xys[H*H, 2] for element i = (column i % H, row i / H) (the transposed index of renderer.py:472);
 *   rn_torso_grid_update     5 x 5 max pool (-inf padding) of the H*H alphas, grid = max(grid * decay, pooled),
 *                            stats[0] = mean(grid).  The alphas come from rn_torso_fused(xys, ..., thresh = -1, ...). */
size_t rn_occupancy_workspace(uint32_t C, uint32_t H);
int rn_occupancy_points(uint32_t C, uint32_t H, float bound, const float *noise, uint32_t seed, float *xyzs, rn_stream_t stream);
int rn_occupancy_update(const float *sigmas, float density_scale, float *density_grid, uint32_t C, uint32_t H, float decay,
                        float density_thresh, uint8_t *bitfield, float *stats, void *workspace, rn_stream_t stream);
int rn_mark_untrained_grid(const float *poses, uint32_t n_poses, uint32_t pose_stride, double fx, double fy, double cx, double cy,
                           uint32_t C, uint32_t H, float bound, float *density_grid, rn_stream_t stream);
int rn_torso_grid_points(uint32_t H, const float *noise, uint32_t seed, float *xys, rn_stream_t stream);
int rn_torso_grid_update(const float *alphas, float *density_grid_torso, uint32_t H, float decay, float *stats, rn_stream_t stream);
/* The box around the set bits of cascade 0 of a bitfield ([cascade * H^3 / 8] bytes, morton order), in cell coordinates:
 * box[0..2] = the lowest x, y, z of a set cell, box[3..5] = the highest, box[6] = box[7] = 0; no bit set: box[0..2] = H,
 * box[3..5] = -1 (lo > hi).  Stays on the device (rn_head_t.occ_box reads it); valid until the bitfield changes.  Two launches. */
int rn_occ_box(const uint8_t *bitfield, uint32_t cascade, uint32_t grid_size, int32_t *box, rn_stream_t stream);
uint32_t rn_hash_u01_bits(uint32_t seed, uint32_t idx);   /* the 24 random bits behind the built-in jitter (host-callable) */

/* ---- audio code ------------------------------------------------------------------------------
 * NeRFNetwork.encode_audio (nerf/network.py:170-185) = AudioNet (nerf/network.py:41-67: 4 x Conv1d(k3, s2, p1) +
 * LeakyReLU(0.02) over the 16-sample window, Linear-LeakyReLU-Linear) on each of the 8 frames of the attention window,
 * then AudioAttNet (nerf/network.py:10-37: 5 x Conv1d(k3, s1, p1) + LeakyReLU(0.02) over the 8 codes, Linear(8,8),
 * softmax, weighted sum) -- ~45 tiny PyTorch launches per frame in the reference; here one workgroup per (window, frame)
 * for AudioNet and one per window for the attention: two launches for any number of windows.
 * All weights are the modules' own tensors (Conv1d [cout, cin, 3] + bias, Linear [out, in] + bias), fp32. */
typedef struct {
    const float *conv_w[4], *conv_b[4];         /* audio_net.encoder_conv.{0,2,4,6}: dim_in->32->32->64->64 */
    const float *fc_w[2], *fc_b[2];             /* audio_net.encoder_fc1.{0,2}: 64->64->dim_aud */
    const float *att_conv_w[5], *att_conv_b[5]; /* audio_att_net.attentionConvNet.{0,2,4,6,8}: dim_aud->16->8->4->2->1 */
    const float *att_fc_w, *att_fc_b;           /* audio_att_net.attentionNet.0: [8,8], [8] */
    uint32_t dim_in, dim_aud, has_att;          /* has_att = 0: one frame per window, no attention (opt.att == 0) */
} rn_audio_weights_t;
#define RN_AUDIO_SEQ 8   /* frames per attention window */
#define RN_AUDIO_WIN 16  /* feature samples per frame */
/* enc[i, :] = encode_audio(auds[i]) for n windows; auds: [n, (has_att ? 8 : 1), dim_in, 16] as NeRFRenderer.run_cuda
 * receives them (nerf/renderer.py:186).  workspace: n * 8 * dim_aud floats of scratch for the per-frame codes (caller-
 * allocated like every buffer; may be NULL when has_att == 0). */
int rn_audio_encode_windows(const rn_audio_weights_t *w, const float *auds, uint32_t n, float *enc, float *workspace,
                            rn_stream_t stream);
/* Backward of rn_audio_encode_windows for the training step: given grad_enc [n, dim_aud] (and `codes`, the forward's
 * workspace with the per-frame codes), ADDS the gradients of every AudioNet / AudioAttNet parameter to the buffers of
 * `grads` (same shapes as the weights; zero them first for a plain gradient).  grad_codes: n * 8 * dim_aud floats of scratch
 * (has_att).  The input features receive no gradient (they are data). */
typedef struct {
    float *conv_w[4], *conv_b[4], *fc_w[2], *fc_b[2], *att_conv_w[5], *att_conv_b[5], *att_fc_w, *att_fc_b;
} rn_audio_grads_t;
int rn_audio_encode_windows_backward(const rn_audio_weights_t *w, const float *auds, uint32_t n, const float *codes,
                                     const float *grad_enc, const rn_audio_grads_t *grads, float *grad_codes,
                                     rn_stream_t stream);
/* The pair a training step uses: the forward keeps every AudioNet layer's output of every frame in `acts`
 * (rn_audio_train_acts_floats(n, has_att) floats), the backward starts from them instead of running the forward again
 * (five weight stagings and layer passes of a latency-bound kernel).  Same results as the pair above, bit for bit. */
size_t rn_audio_train_acts_floats(uint32_t n, int has_att);
int rn_audio_encode_windows_train(const rn_audio_weights_t *w, const float *auds, uint32_t n, float *enc, float *workspace,
                                  float *acts, rn_stream_t stream);
int rn_audio_encode_windows_backward_acts(const rn_audio_weights_t *w, const float *auds, uint32_t n, const float *codes,
                                          const float *grad_enc, const rn_audio_grads_t *grads, float *grad_codes,
                                          const float *acts, rn_stream_t stream);
/* The same backward without a float atomic (opt-in, RN_TRAIN_DETERMINISTIC=1): every workgroup STORES its contributions to the
 * parameter gradients into its own slice of `partials` (rn_audio_backward_partials_floats(n, has_att) floats, sized for dim_in
 * = dim_aud = 64; needs no initialisation), and one reduction launch computes per element acc = p[0]; acc = acc + p[k] in
 * ascending workgroup order -- (window, frame) row-major for AudioNet, window for AudioAttNet -- and then grads[e] = grads[e] +
 * acc: like the entries above it ADDS to `grads`.  The per-workgroup arithmetic is that of the entries above; two calls give
 * the same bits. */
size_t rn_audio_backward_partials_floats(uint32_t n, int has_att);
int rn_audio_encode_windows_backward_ordered(const rn_audio_weights_t *w, const float *auds, uint32_t n, const float *codes,
                                             const float *grad_enc, const rn_audio_grads_t *grads, float *grad_codes,
                                             const float *acts, float *partials, rn_stream_t stream);
/* The same for n consecutive frames (first + i) mod T of a feature stream feats [T, dim_in, 16]: the windows are cut on
 * the device exactly as get_audio_features(att_mode=2) does (nerf/utils.py:56-72: frames index-4 .. index+3, zero rows
 * outside the stream).  Needs T >= 8 and has_att. */
int rn_audio_encode_stream(const rn_audio_weights_t *w, const float *feats, uint32_t T, uint32_t first, uint32_t n,
                           float *enc, float *workspace, rn_stream_t stream);
/* Lip smoothing (nerf/renderer.py:190-194) folded over n codes in order:
 * state = state_valid ? lambda * state + (1 - lambda) * enc[i] : enc[i]; state [dim] is updated in place. */
int rn_audio_smooth(const float *enc, uint32_t n, uint32_t dim, float lambda, float *state, int state_valid,
                    rn_stream_t stream);

/* The smoothing recurrence with every intermediate state kept: out[i] = state after folding enc[i] (n x dim), `state` is
 * updated to out[n-1].  Lets a renderer that knows the next n frames' audio compute all their codes in one go. */
int rn_audio_smooth_seq(const float *enc, uint32_t n, uint32_t dim, float lambda, float *state, int state_valid, float *out,
                        rn_stream_t stream);

/* ---- ray generation -----------------------------------------------------------------------
 * get_rays for the full image (nerf/utils.py:249-333, N = -1 branch): pixel (row r, column c) -> ray r * W + c with
 * centre (c + 0.5, r + 0.5); dir = normalize(((c + 0.5) - cx) / fx, ((r + 0.5) - cy) / fy, 1); rays_d = dir @ R^T,
 * rays_o = pose[:3, 3].  ~12 PyTorch launches and two [N,3] round trips in the reference, one kernel here.
 * pose: device pointer to a row-major [4,4] (or [3,4]: row stride 4) cam2world matrix. */
int rn_get_rays(const float *pose, float fx, float fy, float cx, float cy, uint32_t H, uint32_t W, float *rays_o,
                float *rays_d, rn_stream_t stream);
/* get_bg_coords (nerf/utils.py:240-245): bg_coords [H*W, 2] in [-1, 1], component 0 along the image rows.
 * convert_poses (nerf/utils.py:231-237): n cam2world matrices [n, 4, 4] (row-major) -> poses6 [n, 6] = XYZ euler angles of the
 * rotation (matrix_to_euler_angles, :130-169) | translation -- the other two inputs of the torso pass, one launch each. */
int rn_get_bg_coords(uint32_t H, uint32_t W, float *bg_coords, rn_stream_t stream);
int rn_convert_poses(const float *poses, uint32_t n, float *poses6, rn_stream_t stream);

/* ---- the per-sample MLPs in training --------------------------------------------------------
 * nerf/network.py:69-88 (`MLP`: bias-free nn.Linear stack, ReLU between layers) with its autograd, for the shapes of the
 * path: hidden width 64, n_layers 2 or 3, in_dim <= 96, out_dim <= 4 (narrow) or 64 .. 68 (64 wide rows preceded by
 * out_dim - 64 narrow ones, as sigma_net's [sigma | geo_feat]).  x and grad_x are row-major [M, in_pad] with in_pad =
 * in_dim rounded up to a multiple of 4 (pad columns of x are read: keep them zero); out / grad_out are [M, out_dim].
 * Hidden activations h0 (h1: 3 layers) and pre-activation gradients dz0 (dz1) are opaque tile buffers of
 * rn_mlp64_tile_floats(M) floats each, written by forward / backward and read by backward / weight_grads.  `image` holds
 * rn_mlp64_image_floats() floats (16-byte aligned) and is rebuilt by rn_mlp64_pack whenever a weight changes (w0 [64,in_dim],
 * w1 [64,64] (3 layers, else NULL), w_last [out_dim,64]: the nn.Linear weights).  Weight gradients are written (not
 * accumulated) in the nn.Linear layout; `workspace` needs rn_mlp64_wgrad_workspace(n_layers) bytes.  fp32 MFMA throughout:
 * equal to torch up to summation order.
 * Constant input columns (the audio code, eye value, individual code: the same for every sample of a call) need not be
 * materialised: the MLP then reads only the first in_dim columns of a wider w0 (`ld0` = its row stride; gw0 is written with
 * the same stride, columns in_dim .. ld0-1 untouched) and the constants enter as bias0 [64] = w0[:, in_dim:] . constants, added
 * to the first layer's pre-activation; grad_bias0 [64] (nullable; needs in_dim <= 92) receives its gradient, from which the
 * caller derives the gradients of w0[:, in_dim:] (outer product with the constants) and of the constants. */
size_t rn_mlp64_image_floats(uint32_t in_dim, uint32_t out_dim, uint32_t n_layers);
size_t rn_mlp64_tile_floats(uint32_t M);
size_t rn_mlp64_wgrad_workspace(uint32_t n_layers);
int rn_mlp64_pack(const float *w0, uint32_t ld0, const float *w1, const float *w_last, uint32_t in_dim, uint32_t out_dim,
                  uint32_t n_layers, float *image, rn_stream_t stream);
int rn_mlp64_forward(const float *x, uint32_t M, const float *image, const float *bias0, uint32_t in_dim, uint32_t out_dim,
                     uint32_t n_layers, float *out, float *h0, float *h1, rn_stream_t stream);
int rn_mlp64_backward(const float *grad_out, uint32_t M, const float *image, uint32_t in_dim, uint32_t out_dim, uint32_t n_layers,
                      const float *h0, const float *h1, float *grad_x, float *dz0, float *dz1, rn_stream_t stream);
int rn_mlp64_weight_grads(const float *x, const float *grad_out, uint32_t M, uint32_t in_dim, uint32_t out_dim, uint32_t n_layers,
                          const float *h0, const float *h1, const float *dz0, const float *dz1, float *gw0, uint32_t ld0,
                          float *gw1, float *gw_last, float *grad_bias0, void *workspace, rn_stream_t stream);

/* ---- elementwise glue of the training step (one kernel per direction where PyTorch takes 3 - 15) -------------------------
 * rn_head_mid_*: between sigma_net and color_net (nerf/network.py:266-276): sigma = trunc_exp(h[:, 0]) (activation.py:5-17),
 * x_color [M, n_sh + 64] = cat[enc_d [M, n_sh], h[:, 1:65]]; backward assembles grad_h [M, 65] from grad_sigma and the geo_feat
 * columns of grad_x_color.  rn_abs_sum2_*: ambient.abs().sum(-1) for [M, 2] (nerf/renderer.py:216).
 * rn_train_loss: the head's training loss (nerf/utils.py:772-803: mean squared error + 1e-4 mean binary entropy of
 * clamp(weights_sum, 1e-5, 1 - 1e-5) + *w_amb * mean(ambient * (1 - face))) over N rays and its gradients with respect to
 * pred [N, 3], weights_sum [N], ambient [N] in one launch; face [N] is the 0 / 1 face mask as floats, w_amb a device scalar. */
int rn_head_mid_forward(const float *h, const float *enc_d, uint32_t M, uint32_t n_sh, float *sigma, float *x_color, rn_stream_t stream);
int rn_head_mid_backward(const float *h, const float *grad_sigma, const float *grad_x_color, uint32_t M, uint32_t n_sh, float *grad_h,
                         rn_stream_t stream);
int rn_abs_sum2_forward(const float *a, uint32_t M, float *out, rn_stream_t stream);
int rn_abs_sum2_backward(const float *a, const float *grad_out, uint32_t M, float *grad_a, rn_stream_t stream);
int rn_train_loss(const float *pred, const float *target, const float *weights_sum, const float *ambient, const float *face,
                  const float *w_amb, uint32_t N, float *loss, float *grad_pred, float *grad_weights_sum, float *grad_ambient,
                  rn_stream_t stream);

/* ---- optimizer update of the training step ------------------------------------------------------------------------
 * torch.optim.Adam as main.py:204 configures it (betas, eps; no weight decay, no amsgrad) for `count` tensors in ONE
 * launch (+ a one-thread launch that advances *step and computes the bias corrections in double, as Python does):
 *   m = m + (g - m)(1 - beta1);  v = beta2 v + (1 - beta2) g^2;  p -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 * `tensors` is a HOST array (the pointers travel as kernel arguments, 48 tensors per launch); *step (device int32) counts
 * the steps taken, corr is a 2-float device scratch.  Enqueue-only, capturable in a hipGraph. */
typedef struct {
    float *param;
    const float *grad;
    float *exp_avg, *exp_avg_sq;
    uint32_t numel;
    float lr;
} rn_adam_tensor_t;
int rn_adam_step(const rn_adam_tensor_t *tensors, uint32_t count, float beta1, float beta2, float eps, int32_t *step, float *corr,
                 rn_stream_t stream);
/* The same with the learning rates read from device memory at run time (lr_dev [count] floats, one per tensor; NULL = the
 * `lr` fields): a launch captured in a hipGraph then follows the reference's schedule (main.py:219: LambdaLR over the
 * optimizer's param_groups) -- the host refreshes lr_dev between replays instead of re-capturing. */
int rn_adam_step_lr(const rn_adam_tensor_t *tensors, uint32_t count, float beta1, float beta2, float eps, int32_t *step, float *corr,
                    const float *lr_dev, rn_stream_t stream);

/* ---- mesh export (nerf/utils.py:369-399, 871-891) ------------------------------------------------------------------
 * The density lattice of Trainer.save_mesh and its isosurface, on the device.  The reference queries 256^3 points in 128^3
 * blocks, reads each back and runs mcubes on the CPU; here the lattice points are generated by range, the density query is
 * rn_nerf_fused_forward's sigma branch, and the surface is marching tetrahedra on the Kuhn subdivision (six tetrahedra per
 * cell, one per permutation of the axes; csrc/rn_mesh_dev.h states every convention) with a specified, reproducible order.
 * A lattice is [X, Y, Z] fp32 in C order, every axis >= 2 and 12 (X-1)(Y-1)(Z-1) < 2^31, 7 X Y Z < 2^31 (so that every count and
 * index fits an int32); anything else is RN_ERR_INVALID_ARG (rn_mesh_workspace: 0).  `box`: DEVICE pointer to
 * {min x, y, z, max x, y, z}.
 *
 *   rn_mesh_lattice_points   points[n, 3] = lattice points first .. first + n - 1 (C order) of torch.linspace(min, max, R) per
 *                            axis through meshgrid(indexing = 'ij'): step = (max - min) / (R - 1) in fp32, the lower half
 *                            min + i * step, the upper half max - (R - 1 - i) * step, each as ONE fused multiply-add -- what
 *                            torch's own kernels compute, bit for bit.
 *   rn_mesh_count            pass 1 .. 3: a code byte per point (which of its seven owned edges cross the surface, and whether it is
 *                            inside: u > threshold), per-chunk sums of vertices and triangles, their exclusive scan;
 *                            totals[0] = V, totals[1] = T (device int32).  workspace: rn_mesh_workspace(X, Y, Z) bytes, 16-byte
 *                            aligned; about 5 bytes per point (code | int32 base index).
 *   rn_mesh_emit             after the host has read the totals and allocated vertices [V, 3] fp32 and triangles [T, 3] int32:
 *                            vertices ordered by owning point (C order), then edge kind; triangles by cell (C order), then
 *                            tetrahedron, then position in the split; winding: (v1 - v0) x (v2 - v0) points from inside to
 *                            outside.  box = NULL: lattice units, else v / (R - 1) * (max - min) + min per axis.  The same
 *                            field, threshold and workspace as rn_mesh_count.  No atomic decides an index: two runs, same bytes.
 *   rn_mesh_tet_case         host-callable: the triangles of a tetrahedron (not a mirror image) whose corner l is inside iff bit l
 *                            of mask, as local edge numbers 0 .. 5 = (c0,c1) (c0,c2) (c0,c3) (c1,c2) (c1,c3) (c2,c3):
 *                            *n_triangles = 0, 1 or 2, edges[3 * t + c]. */
size_t rn_mesh_workspace(uint32_t X, uint32_t Y, uint32_t Z);
int rn_mesh_lattice_points(uint32_t X, uint32_t Y, uint32_t Z, const float *box, uint32_t first, uint32_t n, float *points,
                           rn_stream_t stream);
int rn_mesh_count(const float *field, uint32_t X, uint32_t Y, uint32_t Z, float threshold, void *workspace, int32_t *totals,
                  rn_stream_t stream);
int rn_mesh_emit(const float *field, uint32_t X, uint32_t Y, uint32_t Z, float threshold, const float *box, void *workspace,
                 uint32_t n_vertices, uint32_t n_triangles, float *vertices, int32_t *triangles, rn_stream_t stream);
int rn_mesh_tet_case(uint32_t mask, int32_t *n_triangles, int32_t *edges);

/* ---- video write-out: Motion-JPEG on the device (nerf/utils.py:971 hands the frames to an encoder on the host) -------
 * A batch of finished frames [F, H, W, 3] uint8 (device) becomes one baseline JPEG scan per frame: JFIF YCbCr, subsampling 420
 * (MCU 16 x 16) or 444 (MCU 8 x 8), the Annex K quantisation tables under the IJG quality rule and the four Annex K Huffman tables;
 * csrc/rn_jpeg_dev.h states every convention.  The host writes SOI .. SOS before a scan and EOI after it (radnerf/video.py).
 * F, H, W >= 1, sides <= 65535, subsampling 420 or 444, quality 1 .. 100, a frame's worst-case stream below 2^31 bits; anything
 * else is RN_ERR_INVALID_ARG before a launch (the three size functions: 0).
 *
 *   rn_jpeg_blocks           8 x 8 blocks of one frame, in MCU-interleaved scan order (420: Y Y Y Y Cb Cr per MCU; 444: Y Cb Cr).
 *   rn_jpeg_stream_capacity  bytes no frame's scan can exceed: 416 per block = twice the 208 that hold the longest coded block
 *                            (22 bits of DC, 63 x 26 of AC), byte stuffing at most doubling it.
 *   rn_jpeg_workspace        bytes of scratch rn_jpeg_entropy needs for F frames (16-byte aligned).
 *   rn_jpeg_coefficients     coefficients[F, blocks, 64] int16: quantised, zigzag order.
 *   rn_jpeg_entropy          streams = the scans of frames 0 .. F - 1 one behind the other (0xFF stuffed with 0x00, the last byte of
 *                            each padded with 1-bits), sizes[f] (device uint32) the byte count of frame f; capacity: bytes of
 *                            `streams`, >= F * rn_jpeg_stream_capacity and that product < 2^31.  The bytes are a function
 *                            of the coefficients alone: two runs, the same bytes.  A coefficient beyond the invariants of the
 *                            coefficient pass (|DC difference| <= 2047, |AC| <= 1023) is coded as the nearest value within them. */
size_t rn_jpeg_blocks(uint32_t H, uint32_t W, uint32_t subsampling);
size_t rn_jpeg_stream_capacity(uint32_t H, uint32_t W, uint32_t subsampling);
size_t rn_jpeg_workspace(uint32_t F, uint32_t H, uint32_t W, uint32_t subsampling);
int rn_jpeg_coefficients(const uint8_t *frames, uint32_t F, uint32_t H, uint32_t W, uint32_t subsampling, uint32_t quality,
                         int16_t *coefficients, rn_stream_t stream);
int rn_jpeg_entropy(const int16_t *coefficients, uint32_t F, uint32_t H, uint32_t W, uint32_t subsampling, void *workspace,
                    uint8_t *streams, size_t capacity, uint32_t *sizes, rn_stream_t stream);

/* ---- audio features from samples: the wav2vec2 CTC model of nerf/asr.py, file mode -------------------------------------
 * The `Wav2Vec2ForCTC` variant with feat_extract_norm = "layer", conv_bias, do_stable_layer_norm, in eval mode without an
 * attention mask, fp32 throughout, no float atomics and no split of K chosen from the batch: a window's logits do not depend on
 * which other windows share the call, and two calls give the same bits.
 *
 *   input       per window of `samples` floats: (x - mean) / sqrt(var + 1e-7), population variance
 *   encoder     n_conv layers: Conv1d(conv_dim[i-1] -> conv_dim[i], conv_kernel[i], conv_stride[i], no padding) + bias,
 *               LayerNorm over the channels, exact (erf) GELU; layer 0 has one input channel
 *   projection  LayerNorm over conv_dim[n_conv-1], Linear -> hidden
 *   position    h += GELU(conv(h)): pos_taps taps (even), pos_groups groups, padding pos_taps / 2, last output step dropped;
 *               the weight norm (over dims 0, 1 for each tap) is folded into the image by the pack
 *   layers      h += out_proj(attention(LN(h))), queries scaled by 64^-1/2, softmax(Q K^T) V per head of 64 features;
 *               h += W2 GELU(W1 LN(h))
 *   output      LayerNorm, lm_head -> logits [B, T, vocab], T = steps after the last conv layer (at most 96)
 *
 * rn_asr_config_t: hidden = 64 * heads; conv_dim, intermediate and hidden / pos_groups multiples of 4.  Anything else is
 * RN_ERR_INVALID_ARG naming the field, before any launch (the size functions: 0).
 *
 *   rn_asr_image_floats  floats of the packed weight image.
 *   rn_asr_pack          tensors: host array of n_tensors DEVICE pointers, fp32, contiguous, in the layout of the model's state
 *                        dict: per conv layer {conv.weight [Cout,Cin,k], conv.bias, layer_norm.weight, .bias}; projection
 *                        {layer_norm.weight, .bias, projection.weight [H,C], .bias}; position {g [taps], v [H, H/groups, taps],
 *                        bias}; encoder layer_norm {weight, bias}; per layer {layer_norm, q_proj, k_proj, v_proj, out_proj,
 *                        final_layer_norm, intermediate_dense, output_dense} x {weight, bias}; lm_head {weight, bias}:
 *                        4 n_conv + 11 + 16 layers pointers.
 *   rn_asr_workspace     bytes of scratch for B windows of `samples` samples (16-byte aligned); 0: unsupported.
 *   rn_asr_forward       windows [B, samples] -> logits [B, T, vocab].
 *   rn_asr_features      the cut and the unfold of asr.py:331-338, 238-243 in one launch.  `logits`: logits_rows rows of C
 *                        floats; segments: HOST array [n_segments <= 4][5] = {first row, windows, T, left, right}: `windows`
 *                        windows of T rows one behind the other from `first row`, rows left .. right - 1 of each kept.  The M
 *                        kept rows, in order, are unfolded (window 16, padding 8, stride 2) into features [F, C, 16],
 *                        F = M / 2 + 1: features[f][c][j] = kept[2 f - 8 + j][c], 0 outside.
 *   rn_asr_forward_tile  rn_asr_forward with the tiling of its matrix products named: tile = 0 (per product, a function of the
 *                        product's shape and the device's compute-unit count alone), 32 (one wave per 32 x 32 tile, for the few
 *                        rows of one window) or 128 (128 x 128 tiles through LDS).  Both tilings run the same chain over k for
 *                        every output: the logits have the same bits under every value, only the time differs.
 *
 * Live mode (nerf/asr.py:160-224): the logits of one window at a time go into a ring of ring_rows rows of C floats, and every
 * video frame reads its attention window out of it.  Pure copies; the host passes every scalar, nothing is read back.
 *   rn_asr_ring_push     rows left .. right - 1 of logits [T, C] -> ring rows (first_row + i) % ring_rows, then zero_rows rows of
 *                        zeros behind them (0 while streaming; 16 behind the terminal window).  right - left + zero_rows <=
 *                        ring_rows, ring_rows >= 16.
 *   rn_asr_ring_window   frame k's window out [8, C, 16]: entry e is slice s = k - 4 + e, all zeros when s < 0 or s >= n_slices
 *                        (UINT32_MAX while the stream is open), else out[e][c][t] = ring[(ring_rows - 8 + 2 s + t) % ring_rows][c]. */
typedef struct {
    uint32_t n_conv, conv_dim[8], conv_kernel[8], conv_stride[8];
    uint32_t hidden, heads, intermediate, layers, pos_taps, pos_groups, vocab;
    float layer_norm_eps;
} rn_asr_config_t;
size_t rn_asr_image_floats(const rn_asr_config_t *config);
int rn_asr_pack(const rn_asr_config_t *config, const float *const *tensors, uint32_t n_tensors, float *image, rn_stream_t stream);
size_t rn_asr_workspace(const rn_asr_config_t *config, uint32_t B, uint32_t samples);
int rn_asr_forward(const rn_asr_config_t *config, const float *image, void *workspace, size_t workspace_bytes, const float *windows,
                   uint32_t B, uint32_t samples, float *logits, rn_stream_t stream);
int rn_asr_forward_tile(const rn_asr_config_t *config, const float *image, void *workspace, size_t workspace_bytes, const float *windows,
                        uint32_t B, uint32_t samples, float *logits, uint32_t tile, rn_stream_t stream);
int rn_asr_features(const float *logits, size_t logits_rows, uint32_t C, const uint32_t *segments, uint32_t n_segments,
                    float *features, uint32_t F, rn_stream_t stream);
int rn_asr_ring_push(const float *logits, uint32_t T, uint32_t C, uint32_t left, uint32_t right, float *ring, uint32_t ring_rows,
                     uint32_t first_row, uint32_t zero_rows, rn_stream_t stream);
int rn_asr_ring_window(const float *ring, uint32_t ring_rows, uint32_t C, uint32_t k, uint32_t n_slices, float *out, rn_stream_t stream);

/* ---- any PCM audio -> the 16 kHz mono float signal the wav2vec2 path takes (csrc/rn_resample.hip, radnerf/resample.py) ------------
 *   rn_pcm_decode  n_frames interleaved frames of `channels` samples in `format` -> out[i] = the FIRST channel of frame i as float:
 *                  RN_PCM_U8 (v - 128) / 128, RN_PCM_S16LE v / 2^15, RN_PCM_S24LE v / 2^23, RN_PCM_S32LE float(v) * 2^-31 (the
 *                  conversion rounds to nearest even, the scaling is exact), RN_PCM_F32LE the four bytes as they are.  `raw` needs
 *                  byte alignment only.  n_frames = 0: RN_OK, no launch.
 *   rn_resample    band-limited interpolation by a rational ratio L / M (output rate / input rate, in lowest terms) with a table
 *                  of 2 W + 1 taps per phase.  Output t sits at input time n + p / L, n = (t M) / L, p = (t M) % L in int64:
 *                      y[t - t0] = sum over k = -W .. W of table[(k + W) * L + p] * X(n + k),   t = t0 .. t0 + n_out - 1
 *                  one fmaf chain over k ascending from an accumulator of 0.  X(j) = x[j - origin] where 0 <= j - origin < n_buf,
 *                  else 0: element 0 of the buffer holds input index `origin`.  `table` is TAP-major, [2 W + 1][L] floats (the
 *                  transpose of resample.phase_table's array).  A sample's bits do not depend on t0, origin, n_out or the tiling.
 *                  n_out = 0: RN_OK, no launch.  The staged input span of one tile, 255 M / L + 2 W + 2 floats, must fit 64 KiB. */
#define RN_PCM_U8 0
#define RN_PCM_S16LE 1
#define RN_PCM_S24LE 2
#define RN_PCM_S32LE 3
#define RN_PCM_F32LE 4
int rn_pcm_decode(const uint8_t *raw, size_t n_frames, uint32_t channels, int format, float *out, rn_stream_t stream);
int rn_resample(const float *x, size_t n_buf, int64_t origin, const float *table, uint32_t L, uint32_t M, uint32_t W, int64_t t0,
                size_t n_out, float *y, rn_stream_t stream);

/* ---- a dataset directory's image files: background plate, gt and torso layers (data_utils/process.py:63-237) ---------------------
 * Integer and table-driven throughout, csrc/rn_prep_dev.h states every convention: a result is a function of the inputs alone.
 * Images are uint8 RGB(A), row-major; labels [F,H,W] uint8: 0 other, 1 head, 2 neck, 3 torso, 4 background.  F, H, W >= 1, sides
 * <= 16384 and F * H * W < 2^31; anything else, or a null pointer, is RN_ERR_INVALID_ARG before a launch (rn_prep_workspace: 0).
 *
 *   rn_prep_workspace         bytes of scratch any of the three calls needs for F frames (fill: F = 1); 16-byte aligned.
 *   rn_prep_plate_accumulate  per frame d2 = the exact squared distance of every pixel to the nearest pixel whose label is not 4
 *                             (2^30 everywhere in a frame without one).  Frames in order: where d2 > best_d2 [H,W], best_d2 = d2,
 *                             best_id [H,W] = frame0 + f and plate [H,W,3] = the frame's pixel.  The caller sets best_d2 to -1 before
 *                             the first batch; any split of the frames into batches gives the same three arrays.
 *   rn_prep_plate_fill        sure = best_d2 > thresh_d2.  *n_sure (device) = the number of sure pixels; every other pixel of
 *                             `plate` takes the colour of its nearest sure pixel -- of equidistant ones the smallest row, then the
 *                             smallest column.  n_sure = 0: plate is left as it is.
 *   rn_prep_layers            gt [F,H,W,3] = the frame with the plate where the label is 4.  torso [F,H,W,4] = gt with the plate under
 *                             the head, the two vertical in-paints darkened by darken[k] (53 doubles from the host:
 *                             0.98 ** k), the 5 x 5 blur on the neck in-paint's pixels, alpha 255 on the dilated neck, the torso and
 *                             both in-paints, RGBA = 0 elsewhere. */
size_t rn_prep_workspace(uint32_t F, uint32_t H, uint32_t W);
int rn_prep_plate_accumulate(const uint8_t *frames, const uint8_t *labels, uint32_t F, uint32_t H, uint32_t W, uint32_t frame0,
                             int32_t *best_d2, int32_t *best_id, uint8_t *plate, void *workspace, rn_stream_t stream);
int rn_prep_plate_fill(const int32_t *best_d2, uint8_t *plate, uint32_t H, uint32_t W, int32_t thresh_d2, uint32_t *n_sure, void *workspace,
                       rn_stream_t stream);
int rn_prep_layers(const uint8_t *frames, const uint8_t *labels, const uint8_t *plate, const double *darken, uint32_t F, uint32_t H, uint32_t W,
                   uint8_t *gt, uint8_t *torso, void *workspace, rn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RADNERF_FUSED_H */
