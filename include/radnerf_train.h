/*
 * radnerf_train.h -- C ABI of the fused TRAINING pass of the per-sample network (libradnerf_hip.so, gfx950).
 *
 * What is replaced: NeRFNetwork.forward (nerf/network.py:222-283) under autograd in the train branch of
 * NeRFRenderer.run_cuda (nerf/renderer.py:206-223), i.e. per training step of Trainer.train_step (nerf/utils.py:718-806):
 * two grid encodes with their backward (gridencoder/grid.py:24-89, gridencoder.cu:87-368), the SH encode, eight bias-free
 * nn.Linear layers with ReLU / tanh / trunc_exp / sigmoid (nerf/network.py:69-88, activation.py:5-17), three `repeat` + `cat`
 * of per-call constants, and the autograd of all of it -- ~130 launches in stock PyTorch.  Here:
 *
 *   rn_train_head_pack       weight images (forward + transposed) and the three first-layer bias vectors    1 launch
 *   rn_train_head_forward    xyz grid -> ambient net -> tanh -> ambient grid (+ d/dx) -> sigma net -> exp,
 *                            SH -> colour net -> sigmoid, per 32-sample tile on fp32 MFMA, saving every hidden
 *                            activation in the matrix-core register layout                                    1 launch
 *   rn_train_head_backward   the same tile walked back: pre-activation gradients of all eight layers, the
 *                            gradient of the ambient coordinates through the 2-D grid, and the feature
 *                            gradients of both grids in level-major [L, M, 2] layout                          1 launch
 *   rn_train_head_input_grads    only with --train_camera: d/d xyzs (the corners of the xyz grid gathered again, DYDX
 *                            blend) and d/d dirs (W_col0[:, 0:16]^T dZ_col0 through the SH Jacobian); zero rows past
 *                            the live count                                                                    1 launch
 *   rn_train_head_weight_grads   dW = dZ X^T for all eight layers in one launch (+ one reduction launch, + one
 *                            launch for the constant columns: audio code / eye / individual code and their
 *                            weight columns)                                                                   3 launches
 *   rn_grid_scatter_lbc      table gradient: scatter-add of the level-major feature gradients, merged per
 *                            64-byte line of the table in LDS before anything goes to memory                   1 launch per grid
 *
 * Conventions are those of radnerf_hip.h (device pointers, caller allocates, explicit stream, int status).  Supported
 * network shape = rn_nerf_fused_forward's (radnerf_fused.h): grids L = 16, C = 2 (xyz D = 3, ambient D = 2), hidden width 64,
 * geo_feat 64, SH degree 4, ambient_dim 2, fp32 tables.  Sample rows at index >= the live count (m_dev, nullable) receive
 * no output and contribute no gradient, exactly like the zero rows past the marcher's counter in the reference
 * (raymarching/raymarching.py:231-257).
 */
#ifndef RADNERF_TRAIN_H
#define RADNERF_TRAIN_H

#include "radnerf_fused.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Floats of the packed image rn_train_head_pack writes: forward image | transposed image | bias [192]. */
size_t rn_train_head_image_floats(void);
/* Floats of the activation / gradient workspace for a capacity of M sample rows (opaque; written by forward and
 * backward, read by backward and weight_grads). */
size_t rn_train_head_workspace_floats(uint32_t M);
/* Bytes of the weight-gradient workspace (partial sums of the reduction over the samples). */
size_t rn_train_head_wgrad_workspace(void);

/* Pack the weights (call once per step: the optimizer changed them) and fold the per-call constants into the first-layer
 * biases: W_amb0[:, 32:] enc_a | W_sig0[:, 64] eye | W_col0[:, 80:] ind_code (nerf/network.py:236, 262, 274). */
int rn_train_head_pack(const rn_nerf_weights_t *w, const float *enc_a, const float *eye, const float *ind_code, float *image,
                       rn_stream_t stream);
/* The same with the individual code picked on the device: ind_table = individual_codes [rows, ind_dim], *ind_index (int64 device
 * scalar) the row -- nerf/renderer.py:199's `self.individual_codes[index]` without an index_select launch. */
int rn_train_head_pack_row(const rn_nerf_weights_t *w, const float *enc_a, const float *eye, const float *ind_table,
                           const int64_t *ind_index, float *image, rn_stream_t stream);

/* Forward for M sample rows (m_dev: device int32 live count, clipped to M; NULL = M).  xyzs in [-bound, bound], dirs unit
 * vectors.  Outputs: sigmas [M], rgbs [M,3], ambient [M,2] (after tanh), ambient_abs [M] (|a0| + |a1|, nerf/renderer.py:216;
 * nullable).  xn [M,3] / wn [M,2]: the normalised grid inputs (x + bound) / (2 bound) and (ambient + 1) / 2 as the grid
 * kernels see them (gridencoder/grid.py:151), kept for the table scatter. */
int rn_train_head_forward(const float *xyzs, const float *dirs, uint32_t M, const int32_t *m_dev, const rn_grid_t *grid_xyz,
                          const rn_grid_t *grid_amb, const float *image, float bound, float *sigmas, float *rgbs,
                          float *ambient, float *ambient_abs, float *xn, float *wn, float *workspace, rn_stream_t stream);

/* Backward.  grad_sigmas [M], grad_rgbs [M,3], grad_ambient [M,2] (nullable), grad_ambient_abs [M] (nullable) are the
 * gradients of the forward's outputs; sigmas / rgbs / ambient its saved outputs.  Writes the feature gradients of the two
 * grids level-major: grad_enc_x [16, M, 2], grad_enc_w [16, M, 2] (rows >= live count are not written: the scatter takes
 * the same m_dev), and the pre-activation gradients into the workspace. */
int rn_train_head_backward(const float *grad_sigmas, const float *grad_rgbs, const float *grad_ambient,
                           const float *grad_ambient_abs, const float *rgbs, const float *ambient, uint32_t M,
                           const int32_t *m_dev, const float *image, float *workspace, float *grad_enc_x, float *grad_enc_w,
                           rn_stream_t stream);

/* Gradients of the sample positions and directions (only a caller that trains the camera pose needs them; call after
 * rn_train_head_backward, before the tables or the weights change).  xn [M,3]: the forward's normalised positions; dirs [M,3]:
 * the forward's directions; grad_enc_x [16, M, 2]: the backward's feature gradients of the xyz grid (ambient-net + sigma-net
 * paths already summed); image / workspace: the forward's and backward's.  The table corners are gathered again:
 *   grad_xyzs[b, d] = 1 / (2 bound) * sum_l sum_c grad_enc_x[l, b, c] * dy_dx[b, l, d, c]   (gridencoder.cu:189-240, 342-368;
 *                     exactly 0 for a sample whose normalised position lies outside [0, 1])
 *   grad_dirs[b, :] = J_SH(dirs[b])^T g_sh[b],  g_sh[b, k] = sum_o W_col0[o][k] dZ_col0[b, o], k < 16   (shencoder.cu:359-382)
 * Rows b >= live count of both outputs are written as zeros.  fp32 table, D = 3, C = 2, align_corners = false, linear. */
int rn_train_head_input_grads(const float *xn, const float *dirs, const float *grad_enc_x, uint32_t M, const int32_t *m_dev,
                              const rn_grid_t *grid_xyz, const float *image, const float *workspace, float bound,
                              float *grad_xyzs, float *grad_dirs, rn_stream_t stream);

/* Gradients of the eight weight matrices in the nn.Linear layout (written, not accumulated; the full [64, 32 + audio_dim]
 * etc. shapes including the constant columns) and of the constants: grad_enc_a [audio_dim], grad_eye [1] (nullable when
 * has_eye == 0), grad_ind_code [ind_dim] (nullable when ind_dim == 0). */
typedef struct {
    float *amb_w0, *amb_w1, *amb_w2, *sig_w0, *sig_w1, *sig_w2, *col_w0, *col_w1;
    float *enc_a, *eye, *ind_code;
} rn_train_head_grads_t;
int rn_train_head_weight_grads(const rn_nerf_weights_t *w, const float *enc_a, const float *eye, const float *ind_code,
                               uint32_t M, const int32_t *m_dev, const float *workspace, const rn_train_head_grads_t *grads,
                               void *wgrad_workspace, rn_stream_t stream);
/* Row form (see rn_train_head_pack_row): ind_table / g->ind_code are [ind_rows, ind_dim]; the launch that writes the constants'
 * gradients writes the picked row of g->ind_code and zeros everywhere else -- the whole gradient of individual_codes, which
 * index_select's backward builds with a memset and an index_add. */
int rn_train_head_weight_grads_row(const rn_nerf_weights_t *w, const float *enc_a, const float *eye, const float *ind_table,
                                   const int64_t *ind_index, uint32_t ind_rows, uint32_t M, const int32_t *m_dev, const float *workspace,
                                   const rn_train_head_grads_t *g, void *wgrad_workspace, rn_stream_t stream);

/* ---- 16-bit matrix products (opt-in; csrc/rn_train_head_f16.hip) ----------------------------------------------------------
 * The arithmetic of the reference's `-O` runs for its eight nn.Linear layers (nerf/utils.py:1168-1172): 16-bit operands, fp32
 * sums.  Same arguments, same outputs, same workspace (rn_train_head_workspace_floats) as the fp32 namesakes; only the image
 * is longer.  rn_train_head_input_grads, rn_train_head_weight_grads(_row) and the table scatters are called as they are:
 * they read the fp32 part of the image and the fp32 workspace.
 *   rounded to half (nearest even), once, by the pack kernel: the weights of every 64-row contraction -- W_amb0[:, 0:32],
 *     W_amb1, W_sig0[:, 0:64], W_sig1, W_sig2[1:65], W_col0[:, 0:80] -- and their transposes;
 *   rounded to half where it enters a contraction: a layer's input (grid features, SH basis, the previous layer's fp32
 *     accumulators after the activation) in the forward, and dY in the backward after the per-tile scaling below;
 *   products are exact, sums are fp32 (v_mfma_f32_32x32x8f16);
 *   per-tile scaling: for each 32-sample tile and each product dX = W^T dY, dY is multiplied by the power of two that
 *     brings its largest magnitude in the tile into [2^14, 2^15) before it is rounded, and the fp32 sums by the inverse
 *     power; a tile whose dY is all zero skips the products (its dX is zero).  No state, nothing to tune: a gradient 2^-20
 *     times smaller gives 2^-20 times the same bits;
 *   fp32 throughout: grid gathers and interpolation, d enc_w / d ambient, SH, tanh / trunc_exp / sigmoid and their
 *     derivatives, the narrow layers (W_amb2, W_sig2[0], W_col1), the first-layer biases of the per-call constants, every
 *     saved tile and pre-activation gradient of the workspace (so dW = dZ X^T sees unrounded X and dZ), the level-major
 *     feature gradients.
 * No float atomics: two calls on the same inputs give the same bits. */
/* Floats of the image rn_train_head_pack_h16 writes: the fp32 image of rn_train_head_pack | 16-bit forward image | 16-bit
 * transposed image. */
size_t rn_train_head_image_floats_h16(void);
int rn_train_head_pack_h16(const rn_nerf_weights_t *w, const float *enc_a, const float *eye, const float *ind_code, float *image,
                           rn_stream_t stream);
int rn_train_head_pack_row_h16(const rn_nerf_weights_t *w, const float *enc_a, const float *eye, const float *ind_table,
                               const int64_t *ind_index, float *image, rn_stream_t stream);
int rn_train_head_forward_h16(const float *xyzs, const float *dirs, uint32_t M, const int32_t *m_dev, const rn_grid_t *grid_xyz,
                              const rn_grid_t *grid_amb, const float *image, float bound, float *sigmas, float *rgbs,
                              float *ambient, float *ambient_abs, float *xn, float *wn, float *workspace, rn_stream_t stream);
int rn_train_head_backward_h16(const float *grad_sigmas, const float *grad_rgbs, const float *grad_ambient,
                               const float *grad_ambient_abs, const float *rgbs, const float *ambient, uint32_t M,
                               const int32_t *m_dev, const float *image, float *workspace, float *grad_enc_x, float *grad_enc_w,
                               rn_stream_t stream);

/* Table gradient of one grid from level-major feature gradients: grad_table[row(l, corner)] += w_corner * grad[l, b, :]
 * (kernel_grid_backward, gridencoder.cu:247-339) for b < live count; inputs [M, D] normalised coordinates (rows outside
 * [0, 1] contribute nothing, gridencoder.cu:275-280).  grad_table [rows, 2] fp32 must be zeroed by the caller.  D = 2 / 3,
 * C = 2, fp32, align_corners = false, linear interpolation.  One workgroup merges the rows of 64 (D = 3) / 128 (D = 2) samples of one level per
 * 64-byte line of the table in LDS and issues one atomic request per touched line. */
int rn_grid_scatter_lbc(const float *grad, const float *inputs, uint32_t M, const int32_t *m_dev, const rn_grid_t *grid,
                        float *grad_table, rn_stream_t stream);

/* The same gradient with the large levels summed by TABLE REGION instead of by workgroup (two launches).  A level with at least
 * 16 buckets of 4096 rows that is HASHED is "binned": the first kernel appends its (row, w g) entries to the bucket that
 * owns the row, the second has one workgroup per bucket add them in LDS and update the region with plain loads and stores -- no
 * global float atomic on those levels (the hashed levels of a T = 2^19 table are touched ~5 times per launch, but never twice by
 * one workgroup, so a per-workgroup merge leaves one memory-side request per corner pair there).  The other levels go through
 * the LDS line merge of rn_grid_scatter_lbc inside the same first launch.  offsets_host: host copy of grid->offsets [L + 1];
 * workspace: rn_grid_scatter_workspace() bytes, 256-byte aligned, ZEROED once by the caller before first use (bucket cursors
 * live at its start and are left zero by every call).  Same results up to summation order.  The rows of a BINNED level are
 * WRITTEN (each by the one workgroup that owns its region), not accumulated: the caller need not zero them, and must not
 * expect earlier contents to survive; rows of the other levels are accumulated into (zero them first). */
size_t rn_grid_scatter_workspace(uint32_t M, const rn_grid_t *grid, const int32_t *offsets_host);
/* Bit l set: level l of this grid is binned (its rows of grad_table are written, not accumulated into). */
uint32_t rn_grid_scatter_binned_levels(const rn_grid_t *grid, const int32_t *offsets_host);
/* One or two grids at once -- what the training step calls for its xyz and ambient grids: the line-merged levels of both grids
 * share ONE launch, job 0's binned levels (offsets_host + workspace given) take the two bucket launches.  3 launches in all. */
typedef struct {
    const float *grad, *inputs;      /* [L, M, 2] level-major feature gradients, [M, D] normalised coordinates */
    const rn_grid_t *grid;
    const int32_t *offsets_host;     /* host copy of grid->offsets (nullable).  With it the library knows which levels are hashed:
                                        large hashed levels skip the LDS merge (a workgroup never touches one of their lines twice)
                                        and send each x-pair's four floats from four adjacent lanes -- one request per pair; job 0's
                                        may additionally be binned when a workspace is given */
    float *grad_table;
} rn_scatter_job_t;
int rn_grid_scatter_jobs(const rn_scatter_job_t *jobs, uint32_t n_jobs, uint32_t M, const int32_t *m_dev, void *workspace,
                         size_t workspace_bytes, rn_stream_t stream);
int rn_grid_scatter_binned(const float *grad, const float *inputs, uint32_t M, const int32_t *m_dev, const rn_grid_t *grid,
                           const int32_t *offsets_host, float *grad_table, void *workspace, size_t workspace_bytes, rn_stream_t stream);

/* The same gradient summed in ONE fixed order, without a float atomic (csrc/rn_grid_scatter_ordered.hip; opt-in,
 * RN_TRAIN_DETERMINISTIC=1).  Same jobs, M, m_dev and zeroed grad_table as rn_grid_scatter_jobs.  Every row of grad_table starts
 * at +0.0f and receives its contributions level by level, samples ascending, corners ascending, with sequential fp32 adds; a
 * contribution is w * g with w = 1; w *= (bit d of the corner ? pos[d] : 1 - pos[d]) for d = 0 .. D-1, every operation rounded
 * on its own -- the order and the arithmetic of the CPU oracle's loops, so the result equals orc_grid_encode_backward's bit for
 * bit, and two calls give the same bits.  A sample with a coordinate outside [0, 1] contributes nothing; rows of `grad` and
 * `inputs` at or past the live count are not read; table rows nothing contributes to are not written.  Per job: one launch that
 * writes a key (the table row) per (level, sample, corner), a stable radix sort of (key, item), one launch that walks every
 * row's run.  The jobs run one after the other and share the workspace: rn_grid_scatter_ordered_workspace() bytes (0: a job is
 * out of range), 256-byte aligned, needs no initialisation; it is sized from the capacity M alone, never from the device count.
 * offsets_host (nullable) lets the sort stop at the table's top row bit instead of bit 31.  L * M * 2^D must stay below 2^31. */
size_t rn_grid_scatter_ordered_workspace(const rn_scatter_job_t *jobs, uint32_t n_jobs, uint32_t M);
int rn_grid_scatter_ordered(const rn_scatter_job_t *jobs, uint32_t n_jobs, uint32_t M, const int32_t *m_dev, void *workspace,
                            size_t workspace_bytes, rn_stream_t stream);

/* Head loss of the training step on the composited rays (nerf/renderer.py:306 + nerf/utils.py:772-803):
 *   pred = clamp(image + (1 - weights_sum) * bg, 0, 1);
 *   loss = mean_n mean_c (pred - target)^2 + 1e-4 mean_n H(clamp(ws, 1e-5, 1 - 1e-5)) + *w_amb mean_n (ambient_n (1 - face_n))
 * and its gradients with respect to image [N,3], weights_sum [N], ambient [N] in one launch.  pred (nullable) receives the
 * blended prediction.  Row strides (floats) of bg / target / face let them be columns of one packed batch table. */
int rn_train_head_loss(const float *image, const float *weights_sum, const float *ambient, const float *bg, uint32_t bg_stride,
                       const float *target, uint32_t target_stride, const float *face, uint32_t face_stride, const float *w_amb,
                       uint32_t N, float *loss, float *pred, float *grad_image, float *grad_weights_sum, float *grad_ambient,
                       rn_stream_t stream);
/* A further term on pred that the caller computed (the patch / lips term of nerf/utils.py:757-781) joins that loss: g_pred [N,3] =
 * d term / d pred goes back through the clamp and the blend, in one launch with one thread per ray.  Per channel c = 0, 1, 2:
 * raw = image + (1 - ws) * bg as above, pass = raw in [0, 1], grad_image += pass ? g_pred : 0, grad_weights_sum -= (pass ? g_pred
 * : 0) * bg; and loss[0] += term[0].  grad_image / grad_weights_sum / loss: what rn_train_head_loss wrote, updated in place. */
int rn_train_head_loss_chain(const float *image, const float *weights_sum, const float *bg, uint32_t bg_stride, const float *g_pred,
                             uint32_t N, const float *term, float *loss, float *grad_image, float *grad_weights_sum,
                             rn_stream_t stream);

/* A training batch from a per-pixel table: out = [n, widths[0]] | [n, widths[1]] | ... (each section contiguous), section s
 * holding columns (widths[0] + .. + widths[s-1]) .. of the rows table[idx[i], :] (idx: int64 device array, row_floats = sum of
 * the <= 8 widths, given as a HOST array).  One launch where indexing + making each strided column block contiguous takes one
 * gather and one copy per section (the loader side of nerf/provider.py:588-690 for rays that are already on the device). */
int rn_train_batch_gather(const float *table, uint32_t row_floats, const int64_t *idx, uint32_t n, const uint32_t *widths,
                          uint32_t sections, float *out, rn_stream_t stream);

/*
 * The pose code of --train_camera (nerf/renderer.py:170-174) around the step: the frame's row of camera_dT [n_rows,3] added to
 * the ray origins, the ray directions turned by R = Rx(a0) Ry(a1) Rz(a2) (euler_angles_to_matrix, nerf/utils.py:172-227) with
 * a[k] = camera_dR[row][k] / 180 * pi + 1e-8 -- and the gradients of both tables.  Opt-in (RN_TRAIN_CAMERA=fused,
 * radnerf/train_camera.py); one launch forward, two backward, where autograd over the torch operators takes ~30 each way.
 *
 * index: int64 device scalar, the frame's row.  A negative value wraps once (row + n_rows).  A row outside the tables reads and
 * writes nothing outside them: the forward copies the rays unchanged, the backward writes zeros everywhere.
 */
/* out_rays_o[n] = rays_o[n] + camera_dT[row];  out_rays_d[n][j] = d[n][0] R[0][j] + d[n][1] R[1][j] + d[n][2] R[2][j].  All of it
 * fp32, every operation rounded on its own, sums from left to right (csrc/rn_camera_dev.h).  rays / outputs: [N,3].  N == 0:
 * nothing is launched. */
int rn_camera_rays_forward(const float *rays_o, const float *rays_d, const float *camera_dT, const float *camera_dR,
                           const int64_t *index, uint32_t n_rows, uint32_t N, float *out_rays_o, float *out_rays_d,
                           rn_stream_t stream);
/* Bytes of the backward's workspace for N rays (12 partial sums per 256 rays; opaque, needs no initialisation). */
size_t rn_camera_rays_workspace(uint32_t N);
/* grad_rays_o / grad_rays_d [N,3]: the gradients of the forward's outputs (what rn_march_rays_train_backward wrote); rays_d: the
 * forward's UNTRANSFORMED directions.  grad_dT [n_rows,3] and grad_dR [n_rows,3] are written whole:
 *   grad_dT[row] = sum_n g_o[n];   grad_dR[row][k] = pi / 180 * sum_ij G[i][j] dR[i][j] / da_k,  G[i][j] = sum_n d[n][i] g_d[n][j],
 * zeros in every other row -- the dense gradient index_put's backward builds with a memset and a scatter.  The sums run over a
 * shuffle tree per wave, the waves of a workgroup in order, the workgroups' partials in double in a fixed order: no float
 * atomics, two calls give the same bits.  N == 0: both tables are written as zeros. */
int rn_camera_rays_backward(const float *grad_rays_o, const float *grad_rays_d, const float *rays_d, const float *camera_dR,
                            const int64_t *index, uint32_t n_rows, uint32_t N, float *grad_dT, float *grad_dR, void *workspace,
                            rn_stream_t stream);

/*
 * The torso layer under autograd: NeRFNetwork.forward_torso (nerf/network.py:188-219) per covered pixel -- two frequency
 * encodings, the deformation net (104 + ind -> 64 -> 64 -> 2), x = clamp(x + dx, -1, 1), the 2-D grid (L = 16, C = 2, fp32,
 * bound 1) with dy_dx, the torso net (136 + ind -> 32 -> 32 -> 4), sigmoid -- and the gradients of the six weight matrices, the
 * table and the individual code.  Eight launches for a forward + backward:
 *
 *   rn_train_torso_pack          weight images (forward + transposed), enc_pose = freq(poses6, 4) and the first-layer biases
 *                                W_def0[:, 42:] [enc_pose | c], W_tor0[:, 74:] [enc_pose | c]                         1 launch
 *   rn_train_torso_forward       per 32-pixel tile on fp32 MFMA, the torso net at its true width of 32 rows         1 launch
 *   rn_train_torso_backward      the tile walked back; feature gradients of the grid level-major [16, P, 2]         1 launch
 *   rn_train_torso_weight_grads  the six dW = dZ X^T in one launch, a reduction, the constant columns and the code  3 launches
 *   rn_grid_scatter_jobs         the table gradient (one D = 2 job) after a memset of grad_table                    1 + 1
 *
 * p_dev: device int32 live count, clipped to P; NULL = P.  Pixel rows at or past it are neither read nor written and
 * contribute to no gradient.  P == 0: nothing is launched.  No gradient is returned for the pixel coordinates.
 */
/* Floats of the image rn_train_torso_pack writes: forward image | transposed image | biases [96] and enc_pose [54]. */
size_t rn_train_torso_image_floats(void);
/* Floats of the activation / gradient workspace for a capacity of P pixel rows (opaque; written by forward and backward,
 * read by backward and weight_grads). */
size_t rn_train_torso_workspace_floats(uint32_t P);
/* Bytes of the weight-gradient workspace (partial sums of the reduction over the pixels). */
size_t rn_train_torso_wgrad_workspace(void);

/* Pack the weights (once per step: the optimizer changed them) and fold the per-call constants -- poses6 [6] and the
 * individual code [w->ind_dim] (nullable when ind_dim == 0) -- into the first-layer biases. */
int rn_train_torso_pack(const rn_torso_weights_t *w, const float *poses6, const float *ind_code, float *image,
                        rn_stream_t stream);

/* Forward for P pixels.  xy [P,2] in [-1, 1] (before torso_shrink).  Outputs: alpha [P,1] and color [P,3] after the sigmoid,
 * dx [P,2] the deformation, wn [P,2] = (clamp(xy * torso_shrink + dx, -1, 1) + 1) / 2, the grid's normalised input, kept for
 * the table scatter. */
int rn_train_torso_forward(const float *xy, uint32_t P, const int32_t *p_dev, float torso_shrink, const rn_grid_t *grid_torso,
                           const float *image, float *alpha, float *color, float *dx, float *wn, float *workspace,
                           rn_stream_t stream);

/* Backward.  grad_alpha [P,1], grad_color [P,3], grad_dx [P,2]: gradients of the forward's outputs, each nullable (= zeros);
 * alpha / color: its saved outputs.  Writes grad_feat [16, P, 2], the level-major feature gradients of the grid (rows >= live
 * count are not written: the scatter takes the same p_dev), and the pre-activation gradients into the workspace. */
int rn_train_torso_backward(const float *grad_alpha, const float *grad_color, const float *grad_dx, const float *alpha,
                            const float *color, uint32_t P, const int32_t *p_dev, const float *image, float *workspace,
                            float *grad_feat, rn_stream_t stream);

/* Gradients of the six weight matrices in the nn.Linear layout at full shape ([64, 96 + ind_dim], [64, 64], [2, 64],
 * [32, 128 + ind_dim], [32, 32], [4, 32]; written, not accumulated) and of the individual code [ind_dim] (nullable when
 * ind_dim == 0).  xy / torso_shrink / ind_code / image: the forward's. */
typedef struct {
    float *def_w0, *def_w1, *def_w2, *tor_w0, *tor_w1, *tor_w2;
    float *ind_code;
} rn_train_torso_grads_t;
int rn_train_torso_weight_grads(const rn_torso_weights_t *w, const float *xy, float torso_shrink, const float *ind_code, uint32_t P,
                                const int32_t *p_dev, const float *image, const float *workspace,
                                const rn_train_torso_grads_t *grads, void *wgrad_workspace, rn_stream_t stream);

/*
 * A torso step that never tells the host how many pixels are covered (opt-in RN_TORSO_TRAIN=fused, radnerf/train_torso.py).  The
 * launches of the torso part of such a step, forward + backward, ten in all:
 *
 *   rn_torso_select              covered pixels of the batch, compacted in ascending order, and their count            1 launch
 *   rn_train_torso_pack / _forward   on the compact rows at capacity N with p_dev = the count                          2 launches
 *   rn_train_torso_loss          scatter-back, blend over the background, MSE + entropy, their gradients               1 launch
 *   rn_train_torso_backward, _weight_grads, a memset and rn_grid_scatter_jobs, all with the same p_dev               1 + 3 + 1 + 1
 *
 * Nothing in it depends on the count on the host side, so the step can be captured in a graph and replayed.
 */
/* Pixels the torso layer covers, as rn_torso_mask decides it (bilinear occupancy of density_grid_torso [G * G] at bg_coords [N,2]
 * strictly above the threshold), compacted: covered [N] int32 receives their indices in ascending order, xy_c [N,2] their
 * coordinates in the same order, count [1] how many there are; rows at or past the count of both are not written.  The
 * threshold is min(density_thresh, *mean_density_dev), the device float read when the kernel runs (nerf/renderer.py:281:
 * min(density_thresh_torso, mean_density_torso)); mean_density_dev == NULL: density_thresh alone.  One workgroup walks the pixels
 * (a training batch: 4 096 .. 65 536); N == 0 sets *count = 0 and launches nothing. */
int rn_torso_select(const float *bg_coords, uint32_t N, const float *density_grid_torso, uint32_t grid_size, float density_thresh,
                    const float *mean_density_dev, int32_t *covered, float *xy_c, int32_t *count, rn_stream_t stream);

/* Loss of a torso step (nerf/renderer.py:286-302, nerf/utils.py:749, 783-791) from the compact rows of the layer:
 *   a[n] = alpha_c[i], c[n] = color_c[i] where covered[i] == n for an i < live count (p_dev clipped to P; NULL = P), a[n] = 0 elsewhere;
 *   pred[n] = c[n] a[n] + bg[n] (1 - a[n])   (= bg[n] bit for bit on uncovered pixels);
 *   loss = mean_n mean_c (pred - target)^2 + 1e-4 mean_n H(clamp(a[n], 1e-5, 1 - 1e-5)),  H the binary entropy in log2,
 * uncovered pixels included in both means.  covered [P] must be ascending over its live rows (rn_torso_select's order).
 * Outputs: loss [1], pred [N,3], alpha_full [N,1], and for live rows only grad_alpha_c [P,1], grad_color_c [P,3] = d loss / d
 * (alpha_c, color_c).  No gradient for bg.  bg / target: [N,3] with row strides in floats (columns of one packed batch table).
 * One launch, one workgroup, sums in double in a fixed order.  N == 0: nothing is launched. */
int rn_train_torso_loss(const float *alpha_c, const float *color_c, const int32_t *covered, uint32_t P, const int32_t *p_dev,
                        const float *bg, uint32_t bg_stride, const float *target, uint32_t target_stride, uint32_t N, float *loss,
                        float *pred, float *alpha_full, float *grad_alpha_c, float *grad_color_c, rn_stream_t stream);

/*
 * The training step's input stage for a data set that already lives in device memory: the loader's batch of one frame
 * (NeRFDataset.collate, nerf/provider.py:625-714, with get_rays / get_audio_features / convert_poses of nerf/utils.py) in ONE
 * launch that touches only the n picked pixels.  The arrays stay as decoded: uint8 images, 7 bytes per pixel and frame.
 *
 *   images [F,H,W,3] u8, torso [F,H,W,4] u8 (RGBA, 4-byte aligned), bg [H,W,3] u8, poses [F,4,4] f32 cam2world,
 *   face_rect [F,4] i32 (xmin, xmax, ymin, ymax; x indexes ROWS, provider.py:657-658), eye [F] f32 (nullable),
 *   auds [Fa,C,16] f32; att 0 / 1 / 2 = get_audio_features' mode; torso_mode = opt.torso.
 */
typedef struct {
    const uint8_t *images, *torso, *bg;
    const float *poses;
    const int32_t *face_rect;
    const float *eye, *auds;
    float fx, fy, cx, cy;
    uint32_t H, W, F, Fa, C, att, torso_mode;
} rn_train_set_t;

/* One training batch of `n` pixels of frame `frame` (audio window around `aud_frame`).  inds: int64 [n] pixel indices r * W + c;
 * a value outside [0, H*W) is clamped into it and counted in *bad (device word, added to, never reset here).  inds == NULL: the
 * kernel draws them, n independent uniform integers from a counter-based generator keyed by (seed, draw, k) -- duplicates
 * allowed, no state in device memory, the same (seed, draw) gives the same batch.  inds_out (nullable) receives the pixels used.
 * packed: rays_o [n,3] | rays_d [n,3] | bg_coords [n,2] | bg_color [n,3] | target [n,3] | face [n], each section contiguous, 15 n
 * floats.  Decoded values are float(u8) / 255 correctly rounded; blend = t_rgb * a + bg * (1 - a), every operation rounded on its
 * own.  Head mode: bg_color = blend, target = images.  Torso mode: bg_color = bg, target = blend.  face = 1 inside the frame's
 * rect, else 0.  Per call: poses6 [6] (rn_convert_poses), pose_matrix [16], eye [1] = set->eye[frame] (both nullable together
 * with set->eye), auds_out = the audio window ([1,C,16] for att 0; [8,C,16]: frames [i-8, i) for att 1, [i-4, i+4) for att 2, rows
 * outside [0, Fa) zero).  n == 0: RN_OK, nothing launched. */
int rn_train_set_batch(const rn_train_set_t *set, uint32_t frame, uint32_t aud_frame, const int64_t *inds, uint32_t n,
                       uint32_t seed, uint32_t draw, float *packed, int64_t *inds_out, float *poses6, float *pose_matrix,
                       float *eye, float *auds_out, uint32_t *bad, rn_stream_t stream);
/* The loader's evaluation form (training = False): every pixel in order, no face section, target = images in both modes.
 * packed: rays_o | rays_d | bg_coords | bg_color | images over H*W pixels, 14 H W floats.  Same kernel, same per-call outputs. */
int rn_train_set_frame(const rn_train_set_t *set, uint32_t frame, uint32_t aud_frame, float *packed, float *poses6,
                       float *pose_matrix, float *eye, float *auds_out, rn_stream_t stream);
/* The two samplings of lip fine-tuning (nerf/utils.py:277-303) as further instantiations of the same kernel: only "which pixel
 * is ray k" differs, every output is written as rn_train_set_batch writes it.
 * _rect: the n = (xmax - xmin) * (ymax - ymin) pixels of a rect in ascending order (torch.where of its mask, :297-303): ray k is
 * pixel (xmin + k / w) * W + (ymin + k % w), w = ymax - ymin, x along the ROWS.  0 <= xmin < xmax <= H and 0 <= ymin < ymax <= W
 * are required (the reference's slice would clamp silently).
 * _patch: n = P * patch^2 rays; ray k is offset o = k % patch^2 of patch q = k / patch^2, pixel (x0 + o / patch) * W + (y0 + o %
 * patch) (:281-292, an 'ij' meshgrid).  corners: int32 [P,2] = (x0, y0) on the device; a corner outside [0, H - patch) x [0, W -
 * patch) is clamped into it and counted once in *bad.  corners == NULL: drawn from (seed, draw) as rn_train_set_batch draws
 * pixels, x0 from element 2q onto [0, H - patch), y0 from element 2q + 1 onto [0, W - patch) -- randint's exclusive upper end
 * (:282-283), so the last row and column of start positions are never drawn.  2 <= patch < min(H, W), P >= 1, n < 2^31. */
int rn_train_set_batch_rect(const rn_train_set_t *set, uint32_t frame, uint32_t aud_frame, int32_t xmin, int32_t xmax, int32_t ymin,
                            int32_t ymax, float *packed, int64_t *inds_out, float *poses6, float *pose_matrix, float *eye,
                            float *auds_out, rn_stream_t stream);
int rn_train_set_batch_patch(const rn_train_set_t *set, uint32_t frame, uint32_t aud_frame, const int32_t *corners, uint32_t P,
                             uint32_t patch, uint32_t seed, uint32_t draw, float *packed, int64_t *inds_out, float *poses6,
                             float *pose_matrix, float *eye, float *auds_out, uint32_t *bad, rn_stream_t stream);

/*
 * What the reference wraps around the training step (main.py:204-224, nerf/utils.py:1018, :1220-1300), keyed on the optimizer's
 * device-side step counter: the learning-rate schedule and the EMA of the weights inside the Adam launches, a swap of weights and
 * shadows, and the squared error of a rendered frame.  The arithmetic of the schedule and of the decay is csrc/rn_optim_dev.h.
 */
/* One tensor of rn_adam_step_sched: rn_adam_tensor_t with the shadow (EMA) array (nullable: no average is kept) and lr0, the rate
 * before any decay.  grad == NULL: a tensor the optimizer holds that has no gradient this step -- no Adam update (exp_avg /
 * exp_avg_sq are then not touched and may be NULL), but its shadow is averaged on update steps. */
typedef struct {
    float *param;
    const float *grad;
    float *exp_avg, *exp_avg_sq, *shadow;
    uint32_t numel;
    float lr0;
} rn_sched_tensor_t;
/* rn_adam_step_lr's update with the schedule and the EMA inside the same launches.  With s = *step after this call's increment:
 *   lr_dev[t] = (float)((double)lr0_t * pow(gamma, (double)(s - 1) / (double)iters))   -- LambdaLR as Trainer.train_one_epoch drives
 *     it (main.py:219, scheduler_update_every_step): step s uses the rate after s - 1 scheduler steps.  gamma == 1: lr0_t.  Written
 *     by the begin kernel (one per 48 tensors), read by the update kernel, and left in lr_dev [count] for the caller to read back.
 *   EMA (decay > 0): on steps with s % interval == 0 the begin kernel does *num_updates += 1 and
 *     omd = (float)(1.0 - min(decay, (1.0 + *num_updates) / (10.0 + *num_updates))), in double; every tensor with a shadow then does
 *     tmp = shadow - p_new; tmp *= omd; shadow -= tmp -- three separately rounded fp32 operations on the value this step wrote
 *     (torch_ema's update with use_num_updates).  On every other step no shadow is read or written.
 * corr: 4 floats of scratch (bias corrections, omd, the update flag).  num_updates: device int32, nullable when decay == 0.
 * Enqueue-only, capturable.  Refused before any launch: decay > 0 with interval == 0, decay outside [0, 1], gamma != 1 with
 * iters == 0, gamma <= 0, null pointers. */
int rn_adam_step_sched(const rn_sched_tensor_t *tensors, uint32_t count, float beta1, float beta2, float eps, double gamma,
                       uint32_t iters, double decay, uint32_t interval, int32_t *step, float *corr, float *lr_dev,
                       int32_t *num_updates, rn_stream_t stream);
/* Exchange a[i][0 .. numel[i]) with b[i][0 .. numel[i]) for `count` tensors (a, b, numel: HOST arrays) in one launch per 48:
 * weights <-> shadows is torch_ema's store() + copy_to(), the same call again its restore().  float4 accesses where both
 * pointers are 16-byte aligned, scalar ones elsewhere.  a[i] and b[i] must not overlap. */
int rn_param_swap(float *const *a, float *const *b, const uint32_t *numel, uint32_t count, rn_stream_t stream);
/* Squared error of one frame: pred, target [H*W, 3] fp32.  out [4] doubles: sum over all values of ((double)(pred - target))^2 with
 * the difference taken in fp32 | the same sum over the pixels inside rect | the number of values | the number inside rect.
 * rect: device int32 [4] = (xmin, xmax, ymin, ymax), xmin <= row < xmax, ymin <= col < ymax (rn_train_set_t's face_rect), NULL =
 * no rect (both rect entries 0).  Per-workgroup partials in `workspace` (rn_image_error_workspace(H, W) bytes, 8-byte aligned, no
 * initialisation), then one ordered pass: no float atomics, the same bits on every run.  H * W <= 2^30. */
size_t rn_image_error_workspace(uint32_t H, uint32_t W);
int rn_image_error(const float *pred, const float *target, uint32_t H, uint32_t W, const int32_t *rect, void *workspace,
                   double *out, rn_stream_t stream);

/*
 * The perceptual term of lip fine-tuning: lpips.LPIPS(net='alex') in eval mode (nerf/utils.py:649-650, 766, 781; LPIPSMeter
 * :438-466), forward and the gradient with respect to the prediction (csrc/rn_percep.hip).  The weights are frozen: there is no
 * weight gradient, and none with respect to the target.
 *   x' = (x - shift) / scale per channel (normalize != 0: x = 2 x - 1 first);
 *   five convolutions with bias and ReLU -- 3 -> 64 k 11 s 4 p 2 | 64 -> 192 k 5 p 2 | 192 -> 384 k 3 p 1 | 384 -> 256 k 3 p 1 |
 *   256 -> 256 k 3 p 1 -- conv2 and conv3 on the 3 x 3 / stride 2 max-pool (no padding, floor) of the tap before them;
 *   per tap: n(x) = x / (sqrt(sum_c x^2) + 1e-10), d = sum_c lin[c] (n(x) - n(y))^2, mean over the positions; value = sum of the five.
 * Decisions: at a position whose channels are all zero d|x| / dx is taken as 0 (torch's sqrt backward gives NaN there); the
 * gradient of a pool window goes to its first maximum in row-major order (torch's choice).
 * Every layer is an implicit GEMM on the fp32 matrix cores, pred and target as one batch of 2P images, K split over the
 * workgroups and the partial tiles summed in slice order (the split depends on the shape alone).  No float atomics: two calls on
 * the same inputs give the same bits.  pred, target and g_pred are read and written through element strides
 * (image, pixel, channel; a row is `w` pixels), so [P,3,h,w] and the [n,3] rows of train_step both go in without a copy.
 * Nothing is allocated, read back or synchronised inside a call (capturable).  h, w >= 31.
 */
/* Floats of the packed image: forward images of the five layers | data-gradient images of conv2..5 | biases | lin | shift, scale. */
size_t rn_percep_image_floats(void);
/* weights, biases, lins: HOST arrays of five device pointers -- conv weights [Cout,Cin,k,k], biases [Cout], lin [Cout]; shift_scale:
 * device [6] = shift[3] | scale[3].  One launch. */
int rn_percep_pack(const float *const *weights, const float *const *biases, const float *const *lins, const float *shift_scale,
                   float *image, rn_stream_t stream);
/* Bytes of the workspace for P image pairs of h x w (taps, gradient maps, split-K partials); 0 for a shape that is refused. */
size_t rn_percep_workspace(uint32_t P, uint32_t h, uint32_t w);
/* Where tap `layer` (0..4) of a forward lives: offset in floats into the workspace and its [channels][2P][oh][ow] dimensions
 * (images 0..P-1 are pred, P..2P-1 target). */
int rn_percep_tap(uint32_t P, uint32_t h, uint32_t w, uint32_t layer, size_t *offset_floats, uint32_t *channels, uint32_t *oh,
                  uint32_t *ow);
/* Where the five per-tap values of a forward live, [5][P] floats (value_out[p] is their sum over the taps, in tap order). */
int rn_percep_tap_values(uint32_t P, uint32_t h, uint32_t w, size_t *offset_floats);
/* value_out [P].  Leaves the taps and d value[p] / d tap (pred half) in the workspace for rn_percep_backward. */
int rn_percep_forward(const float *image, void *workspace, size_t workspace_bytes, const float *pred, int64_t pred_image_stride,
                      int64_t pred_pixel_stride, int64_t pred_channel_stride, const float *target, int64_t target_image_stride,
                      int64_t target_pixel_stride, int64_t target_channel_stride, uint32_t P, uint32_t h, uint32_t w, int normalize,
                      float *value_out, rn_stream_t stream);
/* g_pred[p] = upstream[p * upstream_stride] * d value[p] / d pred[p] (upstream: device floats, stride 0 = one factor for all
 * images; the factor is the last fp32 multiply), every element written -- a pixel no conv1 window covers gets 0.  Same P, h, w,
 * normalize and workspace as the forward before it.  keep: NULL, or a HOST array of five device pointers (each nullable) that
 * receive the gradient of `value` with respect to the pred half of each tap, [channels][P][oh][ow] (before the upstream factor). */
int rn_percep_backward(const float *image, void *workspace, size_t workspace_bytes, const float *upstream, uint32_t upstream_stride,
                       float *g_pred, int64_t g_image_stride, int64_t g_pixel_stride, int64_t g_channel_stride, uint32_t P,
                       uint32_t h, uint32_t w, int normalize, float *const *keep, rn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RADNERF_TRAIN_H */
