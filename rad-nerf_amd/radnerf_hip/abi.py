"""The Python mirror of the C ABI (include/radnerf_hip.h, radnerf_fused.h, radnerf_train.h): every struct, the constants the
Python side uses, and the signature of every exported function -- in header order, grouped by header, and nowhere else.

A call into the library passes raw device pointers and sizes positionally, so a wrong entry here is not an exception but a
kernel launched with a float where a pointer belongs.  tests/test_abi.py therefore checks ALL of this file against the headers
(names both ways, every parameter and return type, struct layouts against the C compiler, constants).  To add an entry point:
declare it in the header, add its line to FUNCTIONS below; the test names whatever was forgotten.

ctypes only -- nothing here needs torch or a device.  The table is written out by hand on purpose: the installed package
does not read include/ at run time.
"""
import ctypes as C

_int, _u32, _f32, _f64, _sz, _ptr, _P = C.c_int, C.c_uint32, C.c_float, C.c_double, C.c_size_t, C.c_void_p, C.POINTER
_i64 = C.c_int64

# ====================================================================================================== radnerf_hip.h
RN_F32, RN_F16 = 0, 1
RN_LAYOUT_LBC, RN_LAYOUT_BLC, RN_LAYOUT_BLC_LEVELMAJOR = 0, 1, 2

# ==================================================================================================== radnerf_fused.h
RN_F32_SPLIT = 2
RN_HEAD_STATE_INTS = 64
RN_TORSO_PLAN_MAX_BYTES = 256 << 20
RN_LOOP_FIRST_MARCHED, RN_LOOP_CLOSE_FRAME, RN_LOOP_COOP = 1, 2, 4
RN_HEAD_ST_ACTIVE, RN_HEAD_ST_ITERS, RN_HEAD_ST_LIVE, RN_HEAD_ST_SLOTS = 4, 16, 17, 18
RN_HEAD_ST_UNFINISHED, RN_HEAD_ST_STALLED, RN_HEAD_ST_HIST = 19, 22, 32
RN_PCM_U8, RN_PCM_S16LE, RN_PCM_S24LE, RN_PCM_S32LE, RN_PCM_F32LE = 0, 1, 2, 3, 4


class GridT(C.Structure):
    c_name = "rn_grid_t"
    _fields_ = [("embeddings", _ptr), ("offsets", _ptr), ("D", _u32), ("L", _u32), ("H", _u32), ("S", _f32),
                ("gridtype", _u32), ("dtype", _int)]


class NerfWeightsT(C.Structure):
    c_name = "rn_nerf_weights_t"
    _fields_ = [("amb_w0", _ptr), ("amb_w1", _ptr), ("amb_w2", _ptr), ("sig_w0", _ptr), ("sig_w1", _ptr),
                ("sig_w2", _ptr), ("col_w0", _ptr), ("col_w1", _ptr), ("audio_dim", _u32), ("has_eye", _u32),
                ("ind_dim", _u32)]


class HeadT(C.Structure):
    c_name = "rn_head_t"
    _fields_ = [("rays_o", _ptr), ("rays_d", _ptr), ("N", _u32), ("aabb", _ptr), ("min_near", _f32),
                ("bitfield", _ptr), ("bound", _f32), ("dt_gamma", _f32), ("max_steps", _u32), ("cascade", _u32),
                ("grid_size", _u32), ("T_thresh", _f32), ("nears", _ptr), ("fars", _ptr), ("weights_sum", _ptr),
                ("depth", _ptr), ("image", _ptr), ("rays_alive_a", _ptr), ("rays_alive_b", _ptr), ("rays_t", _ptr),
                ("xyzs", _ptr), ("dirs", _ptr), ("deltas", _ptr), ("sigmas", _ptr), ("rgbs", _ptr), ("state", _ptr),
                ("block_counts", _ptr), ("live_slots", _ptr), ("order_w", _u32), ("occ_box", _ptr),
                ("dir_term", _ptr)]


class TorsoWeightsT(C.Structure):
    c_name = "rn_torso_weights_t"
    _fields_ = [("def_w0", _ptr), ("def_w1", _ptr), ("def_w2", _ptr), ("tor_w0", _ptr), ("tor_w1", _ptr),
                ("tor_w2", _ptr), ("ind_dim", _u32)]


class AudioWeightsT(C.Structure):
    c_name = "rn_audio_weights_t"
    _fields_ = [("conv_w", _ptr * 4), ("conv_b", _ptr * 4), ("fc_w", _ptr * 2), ("fc_b", _ptr * 2),
                ("att_conv_w", _ptr * 5), ("att_conv_b", _ptr * 5), ("att_fc_w", _ptr), ("att_fc_b", _ptr),
                ("dim_in", _u32), ("dim_aud", _u32), ("has_att", _u32)]


class AudioGradsT(C.Structure):
    c_name = "rn_audio_grads_t"
    _fields_ = [("conv_w", _ptr * 4), ("conv_b", _ptr * 4), ("fc_w", _ptr * 2), ("fc_b", _ptr * 2),
                ("att_conv_w", _ptr * 5), ("att_conv_b", _ptr * 5), ("att_fc_w", _ptr), ("att_fc_b", _ptr)]


class AdamTensorT(C.Structure):
    c_name = "rn_adam_tensor_t"
    _fields_ = [("param", _ptr), ("grad", _ptr), ("exp_avg", _ptr), ("exp_avg_sq", _ptr), ("numel", _u32), ("lr", _f32)]


class AsrConfigT(C.Structure):
    c_name = "rn_asr_config_t"
    _fields_ = [("n_conv", _u32), ("conv_dim", _u32 * 8), ("conv_kernel", _u32 * 8), ("conv_stride", _u32 * 8), ("hidden", _u32),
                ("heads", _u32), ("intermediate", _u32), ("layers", _u32), ("pos_taps", _u32), ("pos_groups", _u32), ("vocab", _u32),
                ("layer_norm_eps", _f32)]


# ==================================================================================================== radnerf_train.h
class HeadGradsT(C.Structure):
    c_name = "rn_train_head_grads_t"
    _fields_ = [(n, _ptr) for n in ("amb_w0", "amb_w1", "amb_w2", "sig_w0", "sig_w1", "sig_w2", "col_w0", "col_w1",
                                    "enc_a", "eye", "ind_code")]


class ScatterJobT(C.Structure):
    c_name = "rn_scatter_job_t"
    _fields_ = [("grad", _ptr), ("inputs", _ptr), ("grid", _P(GridT)), ("offsets_host", _ptr), ("grad_table", _ptr)]


class TorsoGradsT(C.Structure):
    c_name = "rn_train_torso_grads_t"
    _fields_ = [(n, _ptr) for n in ("def_w0", "def_w1", "def_w2", "tor_w0", "tor_w1", "tor_w2", "ind_code")]


class TrainSetT(C.Structure):
    c_name = "rn_train_set_t"
    _fields_ = [("images", _ptr), ("torso", _ptr), ("bg", _ptr), ("poses", _ptr), ("face_rect", _ptr), ("eye", _ptr),
                ("auds", _ptr), ("fx", _f32), ("fy", _f32), ("cx", _f32), ("cy", _f32), ("H", _u32), ("W", _u32), ("F", _u32),
                ("Fa", _u32), ("C", _u32), ("att", _u32), ("torso_mode", _u32)]


class SchedTensorT(C.Structure):
    c_name = "rn_sched_tensor_t"
    _fields_ = [("param", _ptr), ("grad", _ptr), ("exp_avg", _ptr), ("exp_avg_sq", _ptr), ("shadow", _ptr), ("numel", _u32),
                ("lr0", _f32)]


# name -> (restype, argtypes).  rn_stream_t and pointers to device or host buffers are void *; pointers to the structs above
# are typed, as are the few host arrays the callers hand over as ctypes objects.
FUNCTIONS = {
    # ---- include/radnerf_hip.h
    "rn_last_error": (C.c_char_p, []),
    "rn_version": (_int, []),
    "rn_device_count": (_int, []),
    "rn_prof_enable": (_int, [_int]),
    "rn_prof_pause": (_int, [_int]),
    "rn_prof_collect": (_int, [C.POINTER(_u32), C.POINTER(_f32)]),
    "rn_prof_durations": (_int, [C.POINTER(_f32), _u32]),
    "rn_near_far_from_aabb": (_int, [_ptr, _ptr, _ptr, _u32, _f32, _ptr, _ptr, _ptr]),
    "rn_sph_from_ray": (_int, [_ptr, _ptr, _f32, _u32, _ptr, _ptr]),
    "rn_morton3D": (_int, [_ptr, _u32, _ptr, _ptr]),
    "rn_morton3D_invert": (_int, [_ptr, _u32, _ptr, _ptr]),
    "rn_packbits": (_int, [_ptr, _u32, _f32, _ptr, _ptr]),
    "rn_morton3D_dilation": (_int, [_ptr, _u32, _u32, _ptr, _ptr]),
    "rn_march_rays_train_workspace": (_sz, [_u32]),
    "rn_march_rays_train": (_int, [_ptr, _ptr, _ptr, _f32, _f32, _u32, _u32, _u32, _u32, _u32, _ptr, _ptr, _ptr, _ptr, _ptr,
                                   _ptr, _ptr, _ptr, _ptr, _ptr]),
    "rn_march_rays_train_budget": (_int, [_ptr, _ptr, _ptr, _f32, _f32, _u32, _u32, _u32, _u32, _u32, _ptr, _ptr, _ptr, _ptr,
                                          _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "rn_march_rays_train_step_state": (_sz, [_u32]),
    "rn_march_rays_train_step": (_int, [_ptr, _ptr, _ptr, _ptr, _f32, _f32, _f32, _u32, _u32, _u32, _u32, _u32, _ptr, _ptr,
                                        _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _u32, _ptr]),
    "rn_march_rays_train_backward": (_int, [_ptr, _ptr, _ptr, _ptr, _u32, _u32, _ptr, _ptr, _ptr]),
    "rn_composite_rays_train_forward": (_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _u32, _u32, _f32, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "rn_composite_rays_train_backward": (_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _u32, _u32,
                                                _f32, _ptr, _ptr, _ptr, _ptr]),
    "rn_march_rays": (_int, [_u32, _u32, _ptr, _ptr, _ptr, _ptr, _f32, _f32, _u32, _u32, _u32, _ptr, _ptr, _ptr, _ptr, _ptr,
                             _ptr, _ptr, _ptr, _ptr]),
    "rn_composite_rays": (_int, [_u32, _u32, _f32, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "rn_compact_rays_workspace": (_sz, [_u32]),
    "rn_compact_rays": (_int, [_ptr, _u32, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "rn_grid_encode_forward": (_int, [_ptr, _ptr, _ptr, _ptr, _u32, _u32, _u32, _u32, _f32, _u32, _ptr, _u32, _int, _u32, _int,
                                      _int, _ptr]),
    "rn_grid_encode_forward_workspace": (_sz, [_u32, _u32, _u32, _int]),
    "rn_grid_encode_forward_ws": (_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _u32, _u32, _u32, _u32, _f32, _u32, _ptr, _u32, _int,
                                         _u32, _int, _int, _ptr, _sz, _ptr]),
    "rn_grid_encode_forward_bound": (_int, [_ptr, _f32, _ptr, _ptr, _ptr, _ptr, _u32, _u32, _u32, _u32, _f32, _u32, _u32, _int,
                                            _int, _ptr, _sz, _ptr]),
    "rn_grid_encode_backward": (_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _u32, _u32, _u32, _u32, _f32, _u32, _ptr, _ptr, _u32, _int,
                                       _u32, _int, _int, _ptr]),
    "rn_grad_total_variation": (_int, [_ptr, _ptr, _ptr, _ptr, _f32, _u32, _u32, _u32, _u32, _f32, _u32, _u32, _int, _ptr]),
    "rn_sh_encode_forward": (_int, [_ptr, _ptr, _u32, _u32, _u32, _ptr, _ptr]),
    "rn_sh_encode_backward": (_int, [_ptr, _ptr, _u32, _u32, _u32, _ptr, _ptr, _ptr]),
    "rn_freq_encode_forward": (_int, [_ptr, _u32, _u32, _u32, _u32, _ptr, _ptr]),
    "rn_freq_encode_backward": (_int, [_ptr, _ptr, _u32, _u32, _u32, _u32, _ptr, _ptr]),
    # ---- include/radnerf_fused.h
    "rn_nerf_packed_floats": (_sz, []),
    "rn_nerf_packed_floats_h16": (_sz, []),
    "rn_nerf_pack_weights_h16": (_int, [_P(NerfWeightsT), _ptr, _ptr]),
    "rn_nerf_packed_floats_split": (_sz, []),
    "rn_nerf_pack_weights_split": (_int, [_P(NerfWeightsT), _ptr, _ptr]),
    "rn_nerf_bias_floats": (_sz, []),
    "rn_nerf_pack_weights": (_int, [_P(NerfWeightsT), _ptr, _ptr]),
    "rn_nerf_frame_bias": (_int, [_P(NerfWeightsT), _ptr, _ptr, _ptr, _ptr, _ptr]),
    "rn_nerf_frame_bias_batch": (_int, [_P(NerfWeightsT), _ptr, _u32, _ptr, _ptr, _ptr, _ptr]),
    "rn_nerf_fused_forward": (_int, [_ptr, _ptr, _ptr, _u32, _ptr, _P(GridT), _P(GridT), _ptr, _ptr, _f32, _ptr, _ptr, _ptr,
                                     _int, _ptr]),
    "rn_grid_dense_plan": (_int, [_P(GridT), _ptr, _sz, _ptr, _P(_u32), _P(_sz)]),
    "rn_grid_dense_build": (_int, [_P(GridT), _ptr, _ptr, _u32, _ptr, _sz, _ptr]),
    "rn_head_begin": (_int, [_P(HeadT), _ptr]),
    "rn_head_iterate": (_int, [_P(HeadT), _P(GridT), _P(GridT), _ptr, _ptr, _u32, _u32, _int, _ptr]),
    "rn_head_iterate_ex": (_int, [_P(HeadT), _P(GridT), _P(GridT), _ptr, _ptr, _u32, _u32, _int, _u32, _ptr]),
    "rn_frame_begin": (_int, [_P(HeadT), _ptr, _f32, _f32, _f32, _f32, _u32, _ptr]),
    "rn_head_reschedule": (_int, [_P(HeadT), _u32, _u32, _ptr, _ptr]),
    "rn_head_check_done": (_int, [_P(HeadT), _u32, _ptr]),
    "rn_torso_packed_floats": (_sz, []),
    "rn_torso_pack_weights": (_int, [_P(TorsoWeightsT), _ptr, _ptr]),
    "rn_torso_fused": (_int, [_ptr, _u32, _ptr, _u32, _f32, _ptr, _ptr, _f32, _P(TorsoWeightsT), _ptr, _P(GridT), _ptr, _ptr,
                              _ptr, _ptr, _ptr]),
    "rn_torso_blend_frame": (_int, [_ptr, _u32, _ptr, _u32, _f32, _ptr, _ptr, _f32, _P(TorsoWeightsT), _ptr, _P(GridT), _ptr,
                                    _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "rn_torso_plan_bytes": (_sz, [_u32, _u32]),
    "rn_torso_plan_build": (_int, [_ptr, _u32, _ptr, _u32, _f32, _f32, _ptr, _sz, C.POINTER(_u32), _ptr]),
    "rn_torso_blend_frame_planned": (_int, [_ptr, _sz, _u32, _u32, _ptr, _ptr, _f32, _P(TorsoWeightsT), _ptr, _P(GridT), _ptr, _ptr,
                                            _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "rn_torso_mask": (_int, [_ptr, _u32, _ptr, _u32, _f32, _ptr, _ptr]),
    "rn_blend_frame": (_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _u32, _ptr, _ptr]),
    "rn_occupancy_workspace": (_sz, [_u32, _u32]),
    "rn_occupancy_points": (_int, [_u32, _u32, _f32, _ptr, _u32, _ptr, _ptr]),
    "rn_occupancy_update": (_int, [_ptr, _f32, _ptr, _u32, _u32, _f32, _f32, _ptr, _ptr, _ptr, _ptr]),
    "rn_mark_untrained_grid": (_int, [_ptr, _u32, _u32, _f64, _f64, _f64, _f64, _u32, _u32, _f32, _ptr, _ptr]),
    "rn_torso_grid_points": (_int, [_u32, _ptr, _u32, _ptr, _ptr]),
    "rn_torso_grid_update": (_int, [_ptr, _ptr, _u32, _f32, _ptr, _ptr]),
    "rn_occ_box": (_int, [_ptr, _u32, _u32, _ptr, _ptr]),
    "rn_hash_u01_bits": (_u32, [_u32, _u32]),
    "rn_audio_encode_windows": (_int, [_P(AudioWeightsT), _ptr, _u32, _ptr, _ptr, _ptr]),
    "rn_audio_encode_windows_backward": (_int, [_P(AudioWeightsT), _ptr, _u32, _ptr, _ptr, _P(AudioGradsT), _ptr, _ptr]),
    "rn_audio_train_acts_floats": (_sz, [_u32, _int]),
    "rn_audio_encode_windows_train": (_int, [_P(AudioWeightsT), _ptr, _u32, _ptr, _ptr, _ptr, _ptr]),
    "rn_audio_encode_windows_backward_acts": (_int, [_P(AudioWeightsT), _ptr, _u32, _ptr, _ptr, _P(AudioGradsT), _ptr, _ptr,
                                                     _ptr]),
    "rn_audio_backward_partials_floats": (_sz, [_u32, _int]),
    "rn_audio_encode_windows_backward_ordered": (_int, [_P(AudioWeightsT), _ptr, _u32, _ptr, _ptr, _P(AudioGradsT), _ptr, _ptr,
                                                        _ptr, _ptr]),
    "rn_audio_encode_stream": (_int, [_P(AudioWeightsT), _ptr, _u32, _u32, _u32, _ptr, _ptr, _ptr]),
    "rn_audio_smooth": (_int, [_ptr, _u32, _u32, _f32, _ptr, _int, _ptr]),
    "rn_audio_smooth_seq": (_int, [_ptr, _u32, _u32, _f32, _ptr, _int, _ptr, _ptr]),
    "rn_get_rays": (_int, [_ptr, _f32, _f32, _f32, _f32, _u32, _u32, _ptr, _ptr, _ptr]),
    "rn_get_bg_coords": (_int, [_u32, _u32, _ptr, _ptr]),
    "rn_convert_poses": (_int, [_ptr, _u32, _ptr, _ptr]),
    "rn_mlp64_image_floats": (_sz, [_u32, _u32, _u32]),
    "rn_mlp64_tile_floats": (_sz, [_u32]),
    "rn_mlp64_wgrad_workspace": (_sz, [_u32]),
    "rn_mlp64_pack": (_int, [_ptr, _u32, _ptr, _ptr, _u32, _u32, _u32, _ptr, _ptr]),
    "rn_mlp64_forward": (_int, [_ptr, _u32, _ptr, _ptr, _u32, _u32, _u32, _ptr, _ptr, _ptr, _ptr]),
    "rn_mlp64_backward": (_int, [_ptr, _u32, _ptr, _u32, _u32, _u32, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "rn_mlp64_weight_grads": (_int, [_ptr, _ptr, _u32, _u32, _u32, _u32, _ptr, _ptr, _ptr, _ptr, _ptr, _u32, _ptr, _ptr, _ptr,
                                     _ptr, _ptr]),
    "rn_head_mid_forward": (_int, [_ptr, _ptr, _u32, _u32, _ptr, _ptr, _ptr]),
    "rn_head_mid_backward": (_int, [_ptr, _ptr, _ptr, _u32, _u32, _ptr, _ptr]),
    "rn_abs_sum2_forward": (_int, [_ptr, _u32, _ptr, _ptr]),
    "rn_abs_sum2_backward": (_int, [_ptr, _ptr, _u32, _ptr, _ptr]),
    "rn_train_loss": (_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _u32, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "rn_adam_step": (_int, [_P(AdamTensorT), _u32, _f32, _f32, _f32, _ptr, _ptr, _ptr]),
    "rn_adam_step_lr": (_int, [_P(AdamTensorT), _u32, _f32, _f32, _f32, _ptr, _ptr, _ptr, _ptr]),
    "rn_mesh_workspace": (_sz, [_u32, _u32, _u32]),
    "rn_mesh_lattice_points": (_int, [_u32, _u32, _u32, _ptr, _u32, _u32, _ptr, _ptr]),
    "rn_mesh_count": (_int, [_ptr, _u32, _u32, _u32, _f32, _ptr, _ptr, _ptr]),
    "rn_mesh_emit": (_int, [_ptr, _u32, _u32, _u32, _f32, _ptr, _ptr, _u32, _u32, _ptr, _ptr, _ptr]),
    "rn_mesh_tet_case": (_int, [_u32, _P(C.c_int32), _P(C.c_int32)]),
    "rn_jpeg_blocks": (_sz, [_u32, _u32, _u32]),
    "rn_jpeg_stream_capacity": (_sz, [_u32, _u32, _u32]),
    "rn_jpeg_workspace": (_sz, [_u32, _u32, _u32, _u32]),
    "rn_jpeg_coefficients": (_int, [_ptr, _u32, _u32, _u32, _u32, _u32, _ptr, _ptr]),
    "rn_jpeg_entropy": (_int, [_ptr, _u32, _u32, _u32, _u32, _ptr, _ptr, _sz, _ptr, _ptr]),
    "rn_asr_image_floats": (_sz, [_P(AsrConfigT)]),
    "rn_asr_pack": (_int, [_P(AsrConfigT), _ptr, _u32, _ptr, _ptr]),
    "rn_asr_workspace": (_sz, [_P(AsrConfigT), _u32, _u32]),
    "rn_asr_forward": (_int, [_P(AsrConfigT), _ptr, _ptr, _sz, _ptr, _u32, _u32, _ptr, _ptr]),
    "rn_asr_forward_tile": (_int, [_P(AsrConfigT), _ptr, _ptr, _sz, _ptr, _u32, _u32, _ptr, _u32, _ptr]),
    "rn_asr_features": (_int, [_ptr, _sz, _u32, _P(_u32), _u32, _ptr, _u32, _ptr]),
    "rn_asr_ring_push": (_int, [_ptr, _u32, _u32, _u32, _u32, _ptr, _u32, _u32, _u32, _ptr]),
    "rn_asr_ring_window": (_int, [_ptr, _u32, _u32, _u32, _u32, _ptr, _ptr]),
    "rn_pcm_decode": (_int, [_ptr, _sz, _u32, _int, _ptr, _ptr]),
    "rn_resample": (_int, [_ptr, _sz, _i64, _ptr, _u32, _u32, _u32, _i64, _sz, _ptr, _ptr]),
    "rn_prep_workspace": (_sz, [_u32, _u32, _u32]),
    "rn_prep_plate_accumulate": (_int, [_ptr, _ptr, _u32, _u32, _u32, _u32, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "rn_prep_plate_fill": (_int, [_ptr, _ptr, _u32, _u32, C.c_int32, _ptr, _ptr, _ptr]),
    "rn_prep_layers": (_int, [_ptr, _ptr, _ptr, _ptr, _u32, _u32, _u32, _ptr, _ptr, _ptr, _ptr]),
    # ---- include/radnerf_train.h
    "rn_train_head_image_floats": (_sz, []),
    "rn_train_head_workspace_floats": (_sz, [_u32]),
    "rn_train_head_wgrad_workspace": (_sz, []),
    "rn_train_head_pack": (_int, [_P(NerfWeightsT), _ptr, _ptr, _ptr, _ptr, _ptr]),
    "rn_train_head_pack_row": (_int, [_P(NerfWeightsT), _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "rn_train_head_forward": (_int, [_ptr, _ptr, _u32, _ptr, _P(GridT), _P(GridT), _ptr, _f32, _ptr, _ptr, _ptr, _ptr, _ptr,
                                     _ptr, _ptr, _ptr]),
    "rn_train_head_backward": (_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _u32, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "rn_train_head_input_grads": (_int, [_ptr, _ptr, _ptr, _u32, _ptr, _P(GridT), _ptr, _ptr, _f32, _ptr, _ptr, _ptr]),
    "rn_train_head_weight_grads": (_int, [_P(NerfWeightsT), _ptr, _ptr, _ptr, _u32, _ptr, _ptr, _P(HeadGradsT), _ptr, _ptr]),
    "rn_train_head_weight_grads_row": (_int, [_P(NerfWeightsT), _ptr, _ptr, _ptr, _ptr, _u32, _u32, _ptr, _ptr, _P(HeadGradsT),
                                              _ptr, _ptr]),
    "rn_train_head_image_floats_h16": (_sz, []),
    "rn_train_head_pack_h16": (_int, [_P(NerfWeightsT), _ptr, _ptr, _ptr, _ptr, _ptr]),
    "rn_train_head_pack_row_h16": (_int, [_P(NerfWeightsT), _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "rn_train_head_forward_h16": (_int, [_ptr, _ptr, _u32, _ptr, _P(GridT), _P(GridT), _ptr, _f32, _ptr, _ptr, _ptr, _ptr, _ptr,
                                         _ptr, _ptr, _ptr]),
    "rn_train_head_backward_h16": (_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _u32, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "rn_grid_scatter_lbc": (_int, [_ptr, _ptr, _u32, _ptr, _P(GridT), _ptr, _ptr]),
    "rn_grid_scatter_workspace": (_sz, [_u32, _P(GridT), _ptr]),
    "rn_grid_scatter_binned_levels": (_u32, [_P(GridT), _ptr]),
    "rn_grid_scatter_jobs": (_int, [_P(ScatterJobT), _u32, _u32, _ptr, _ptr, _sz, _ptr]),
    "rn_grid_scatter_binned": (_int, [_ptr, _ptr, _u32, _ptr, _P(GridT), _ptr, _ptr, _ptr, _sz, _ptr]),
    "rn_grid_scatter_ordered_workspace": (_sz, [_P(ScatterJobT), _u32, _u32]),
    "rn_grid_scatter_ordered": (_int, [_P(ScatterJobT), _u32, _u32, _ptr, _ptr, _sz, _ptr]),
    "rn_train_head_loss": (_int, [_ptr, _ptr, _ptr, _ptr, _u32, _ptr, _u32, _ptr, _u32, _ptr, _u32, _ptr, _ptr, _ptr, _ptr,
                                  _ptr, _ptr]),
    "rn_train_head_loss_chain": (_int, [_ptr, _ptr, _ptr, _u32, _ptr, _u32, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "rn_train_batch_gather": (_int, [_ptr, _u32, _ptr, _u32, C.POINTER(_u32), _u32, _ptr, _ptr]),
    "rn_camera_rays_forward": (_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _u32, _u32, _ptr, _ptr, _ptr]),
    "rn_camera_rays_workspace": (_sz, [_u32]),
    "rn_camera_rays_backward": (_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _u32, _u32, _ptr, _ptr, _ptr, _ptr]),
    "rn_train_torso_image_floats": (_sz, []),
    "rn_train_torso_workspace_floats": (_sz, [_u32]),
    "rn_train_torso_wgrad_workspace": (_sz, []),
    "rn_train_torso_pack": (_int, [_P(TorsoWeightsT), _ptr, _ptr, _ptr, _ptr]),
    "rn_train_torso_forward": (_int, [_ptr, _u32, _ptr, _f32, _P(GridT), _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "rn_train_torso_backward": (_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _u32, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "rn_train_torso_weight_grads": (_int, [_P(TorsoWeightsT), _ptr, _f32, _ptr, _u32, _ptr, _ptr, _ptr, _P(TorsoGradsT), _ptr,
                                           _ptr]),
    "rn_torso_select": (_int, [_ptr, _u32, _ptr, _u32, _f32, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "rn_train_torso_loss": (_int, [_ptr, _ptr, _ptr, _u32, _ptr, _ptr, _u32, _ptr, _u32, _u32, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "rn_train_set_batch": (_int, [_P(TrainSetT), _u32, _u32, _ptr, _u32, _u32, _u32, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr,
                                  _ptr]),
    "rn_train_set_frame": (_int, [_P(TrainSetT), _u32, _u32, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "rn_train_set_batch_rect": (_int, [_P(TrainSetT), _u32, _u32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _ptr, _ptr, _ptr, _ptr,
                                       _ptr, _ptr, _ptr]),
    "rn_train_set_batch_patch": (_int, [_P(TrainSetT), _u32, _u32, _ptr, _u32, _u32, _u32, _u32, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr,
                                        _ptr, _ptr]),
    "rn_adam_step_sched": (_int, [_P(SchedTensorT), _u32, _f32, _f32, _f32, _f64, _u32, _f64, _u32, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "rn_param_swap": (_int, [_ptr, _ptr, _P(_u32), _u32, _ptr]),
    "rn_image_error_workspace": (_sz, [_u32, _u32]),
    "rn_image_error": (_int, [_ptr, _ptr, _u32, _u32, _ptr, _ptr, _ptr, _ptr]),
    "rn_percep_image_floats": (_sz, []),
    "rn_percep_pack": (_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "rn_percep_workspace": (_sz, [_u32, _u32, _u32]),
    "rn_percep_tap": (_int, [_u32, _u32, _u32, _u32, _P(_sz), _P(_u32), _P(_u32), _P(_u32)]),
    "rn_percep_tap_values": (_int, [_u32, _u32, _u32, _P(_sz)]),
    "rn_percep_forward": (_int, [_ptr, _ptr, _sz, _ptr, _i64, _i64, _i64, _ptr, _i64, _i64, _i64, _u32, _u32, _u32, _int, _ptr, _ptr]),
    "rn_percep_backward": (_int, [_ptr, _ptr, _sz, _ptr, _u32, _ptr, _i64, _i64, _i64, _u32, _u32, _u32, _int, _ptr, _ptr]),
}


def bind(lib):
    """Declare every function of the ABI on the loaded library; a symbol the library lacks is an AttributeError here."""
    for name, (restype, argtypes) in FUNCTIONS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
