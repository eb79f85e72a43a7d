"""Fused inference engine: NeRFRenderer.run_cuda's inference branch on the MI355X-native C ABI
(include/radnerf_fused.h).

Per frame the host enqueues, on torch's current stream and without reading anything back first:

    rn_nerf_frame_bias   broadcast inputs (audio code, eye, individual code) -> 3 x 64 bias values
    rn_head_begin        near/far + loop state
    rn_head_iterate      max_steps x {march, fused network (grid gathers + fp32 MFMA MLPs), composite, stable
                         compaction}; iterations after the loop has ended are device-side no-ops
    rn_torso_fused       torso occupancy test + deformation / torso MLPs + blend over the background
    rn_blend_frame       image + (1 - weights_sum) * bg, clamp, depth normalisation [, uint8]

(a whole-frame render folds the last two into rn_torso_blend_frame, and from the second frame of a view on into
rn_torso_blend_frame_planned over the view's torso plan, see FusedState.torso_plan).

Results equal the per-operator engine's (same DDA samples, same grid features, fp32 MLPs; parity tests in
tests/test_gpu_fused.py).
"""
import ctypes as C

import numpy as np
import torch

import radnerf_hip as hip
from radnerf_hip.abi import (RN_F16, RN_F32, RN_F32_SPLIT, RN_HEAD_ST_HIST, RN_HEAD_ST_ITERS, RN_HEAD_ST_SLOTS, RN_HEAD_ST_STALLED,
                             RN_HEAD_ST_UNFINISHED, RN_HEAD_STATE_INTS, RN_LOOP_CLOSE_FRAME, RN_LOOP_COOP, RN_LOOP_FIRST_MARCHED,
                             RN_TORSO_PLAN_MAX_BYTES, GridT, HeadT, NerfWeightsT, TorsoWeightsT)

from . import switches
from .frame_cache import FrameCaches, LoopStats

_lib = hip._lib

DIR_TERM_MAX_RAYS = 1 << 20     # rays per frame up to which a FusedState keeps direction terms (256 bytes each)


def _grid_desc(enc, table):
    g = GridT()
    g.embeddings, g.offsets = table.data_ptr(), enc.offsets.data_ptr()
    g.D, g.L, g.H = enc.input_dim, enc.num_levels, enc.base_resolution
    g.S = float(np.log2(enc.per_level_scale))
    g.gridtype = enc.gridtype_id
    g.dtype = RN_F16 if table.dtype == torch.float16 else RN_F32
    return g


def _image_desc(g, image, offsets):
    """The descriptor `g` over a dense image of its table (rn_grid_dense_build): same lattice, the image's rows and offsets."""
    d = GridT()
    C.pointer(d)[0] = g
    d.embeddings, d.offsets = image.data_ptr(), offsets.data_ptr()
    return d


def head_weights(model):
    """The eight nn.Linear weights of the per-sample MLPs, in the order of rn_nerf_weights_t."""
    return [l.weight for l in model.ambient_net.net] + [l.weight for l in model.sigma_net.net] + [l.weight for l in model.color_net.net]


def weights_desc(ws, audio_dim, has_eye, ind_dim):
    nw = NerfWeightsT()
    (nw.amb_w0, nw.amb_w1, nw.amb_w2, nw.sig_w0, nw.sig_w1, nw.sig_w2, nw.col_w0, nw.col_w1) = [w.data_ptr() for w in ws]
    nw.audio_dim, nw.has_eye, nw.ind_dim = audio_dim, has_eye, ind_dim
    return nw


def torso_weights(model):
    """The six nn.Linear weights of the torso layer, in the order of rn_torso_weights_t."""
    return [l.weight for l in model.torso_deform_net.net] + [l.weight for l in model.torso_net.net]


def torso_weights_desc(ws, ind_dim):
    assert tuple(ws[0].shape) == (64, 96 + ind_dim) and tuple(ws[3].shape) == (32, 128 + ind_dim)
    tw = TorsoWeightsT()
    (tw.def_w0, tw.def_w1, tw.def_w2, tw.tor_w0, tw.tor_w1, tw.tor_w2) = [w.data_ptr() for w in ws]
    tw.ind_dim = ind_dim
    return tw


def torso_constants(poses, ind_code):
    """The constant inputs of the torso layer as the kernels read them: (poses6 [6], individual code [ind_dim] or None)."""
    return (poses.detach().reshape(-1).contiguous().float(),
            ind_code.detach().reshape(-1).contiguous().float() if ind_code is not None else None)


def supported(model):
    """True when the model has the shape the fused kernels are built for (else: use the 'ops' engine)."""
    try:
        ok = (model.encoder.num_levels == 16 and model.encoder.level_dim == 2 and model.encoder.input_dim == 3
              and model.encoder_ambient.num_levels == 16 and model.encoder_ambient.level_dim == 2
              and model.encoder_ambient.input_dim == 2 and model.hidden_dim == 64 and model.geo_feat_dim == 64
              and model.hidden_dim_ambient == 64 and model.hidden_dim_color == 64 and model.num_layers == 3
              and model.num_layers_ambient == 3 and model.num_layers_color == 2 and model.ambient_dim == 2
              and model.encoder_dir.degree == 4 and not model.encoder.align_corners and model.encoder.interp_id == 0)
        if model.torso:
            ok = ok and (model.torso_encoder.num_levels == 16 and model.torso_encoder.level_dim == 2
                         and model.torso_deform_net.dim_hidden == 64 and model.torso_net.dim_hidden == 32
                         and model.torso_deform_in_dim == 42 and model.pose_in_dim == 54)
        return bool(ok)
    except AttributeError:
        return False


def _caches(model):
    """The model's FrameCaches, made on first use.  The one engine attribute on the module, besides _fused_loop_hint."""
    if getattr(model, "_fused_cache", None) is None:
        object.__setattr__(model, "_fused_cache", FrameCaches())
    return model._fused_cache


class FusedState:
    """Device-side constants + scratch of one model on one stream: packed weights (re-packed when parameters change), grid
    descriptors, per-frame bias block, loop scratch for N rays, the occupied box.  `cache` is the model's FrameCaches: the torso
    plan and the dense image of the xyz table live in its slots, shared with the model's other streams (`plan_builds`,
    `dense_builds`: the records those slots have made)."""

    def __init__(self, model):
        if not supported(model):
            raise RuntimeError("fused engine: unsupported network shape; use engine='ops'")
        self.model, self.cache = model, _caches(model)
        self.dev = model.density_bitfield.device
        n_packed = max(int(_lib.rn_nerf_packed_floats()), int(_lib.rn_nerf_packed_floats_h16()),
                       int(_lib.rn_nerf_packed_floats_split()))
        self.packed = torch.empty(n_packed, dtype=torch.float32, device=self.dev)
        self.mlp_dtype = RN_F32
        self.bias = torch.empty(int(_lib.rn_nerf_bias_floats()), dtype=torch.float32, device=self.dev)
        self.tpacked = (torch.empty(int(_lib.rn_torso_packed_floats()), dtype=torch.float32, device=self.dev)
                        if model.torso else None)
        self._versions = None
        self._N = 0
        self._zero_eye = torch.zeros(1, dtype=torch.float32, device=self.dev)
        self.box = None
        self._box_key = None
        self.box_builds = 0

    loop_hint = property(lambda self: self.cache.loop_hint)
    plan_builds = property(lambda self: self.cache.plan.builds)
    dense_builds = property(lambda self: self.cache.image.builds)

    # -- what is built once and reused across frames --------------------------------------------------
    def _cached(self, slot, key, refs, build):
        """The slot's record for `key` with the current stream ordered behind its build, or None (frame_cache.Slot.get)."""
        rec = slot.get(key, refs, build, torch.cuda.is_current_stream_capturing())
        if rec is not None:
            rec.order(torch.cuda.current_stream())
        return rec

    def _built(self, slot, key, refs, tensors, **payload):
        """A record of what was just enqueued on the current stream."""
        event = torch.cuda.Event()
        event.record()
        return slot.record(key, refs, tensors, event, torch.cuda.current_stream().cuda_stream, **payload)

    # -- dense image of the xyz table -----------------------------------------------------------------
    def frame_grid(self):
        """grid_xyz of this frame's loop: the descriptor of the table (`gx`), or of its dense image -- the coarser hashed
        levels stored once as whole lattices (rn_grid_dense_plan / rn_grid_dense_build; same rows, same features), which the
        network kernels then walk as dense levels.  The key is the table's (address, version, dtype) and the budget, the
        lifetime frame_cache's rule: training moves the version with every step, so validation renders between steps never
        pay for a build.  Only the frame loop asks: density() and network_forward() keep the table.  RN_DENSE_LEVELS=0:
        always the table; the budget is `opt.dense_budget_mb` or RN_DENSE_BUDGET_MB, in MiB."""
        if not switches.on("RN_DENSE_LEVELS"):
            return self.gx
        m = self.model
        table = self.tables[0]
        mb = getattr(getattr(m, "opt", None), "dense_budget_mb", None)
        budget = int(switches.get("RN_DENSE_BUDGET_MB") if mb is None else mb) << 20
        key = (table.data_ptr(), m.encoder.embeddings._version, table.dtype, budget)
        img = self._cached(self.cache.image, key, [table], lambda: self._build_dense(key, table, budget))
        return self.gx if img is None else img.gx

    def _build_dense(self, key, table, budget):
        """-> the record of one dense image: `buf` holds it (None: the planner found no level within the budget, or the
        allocation failed), `offsets` its level offsets on the device, `gx` its descriptor, `levels` the de-hashed levels' mask."""
        enc = self.model.encoder
        oh = hip.host_offsets(enc.offsets)
        new_off = (C.c_int32 * (enc.num_levels + 1))()
        levels, nbytes = C.c_uint32(0), C.c_size_t(0)
        rc = _lib.rn_grid_dense_plan(C.byref(self.gx), oh, budget, new_off, C.byref(levels), C.byref(nbytes))
        if rc < 0:
            raise RuntimeError(f"rn_grid_dense_plan failed ({rc}): {hip.last_error()}")
        buf = offsets = gx = None
        if rc == 1:
            try:
                buf = torch.empty(nbytes.value, dtype=torch.uint8, device=self.dev)
                offsets = torch.tensor(list(new_off), dtype=torch.int32, device=self.dev)
            except torch.cuda.OutOfMemoryError:       # no room for the image: the frames stay on the table
                buf = None
        if buf is not None:
            hip.call("rn_grid_dense_build", C.byref(self.gx), oh, new_off, levels.value, hip.ptr(buf), nbytes.value, hip.stream())
            gx = _image_desc(self.gx, buf, offsets)
        return self._built(self.cache.image, key, [table], [] if buf is None else [buf, offsets], buf=buf, offsets=offsets, gx=gx,
                           levels=levels.value)

    # -- occupied box ---------------------------------------------------------------------------------
    def occ_box(self):
        """The box around the set bits of the model's bitfield (rn_occ_box: 8 int32 on the device, never read back) for
        rn_head_t.occ_box, or None with RN_OCC_BOX=0.  Built on the current stream when the bitfield's address or version, the
        cascade count or the grid size differ from the last build's -- a grid refresh (update_extra_state) and an in-place edit
        both move the version -- so a stream of frames over one grid builds it once."""
        if not switches.on("RN_OCC_BOX"):
            return None
        m = self.model
        bits = m.density_bitfield
        key = (bits.data_ptr(), bits._version, int(m.cascade), int(m.grid_size))
        if key != self._box_key:
            if self.box is None:
                self.box = torch.zeros(8, dtype=torch.int32, device=self.dev)
            hip.call("rn_occ_box", hip.ptr(bits), int(m.cascade), int(m.grid_size), hip.ptr(self.box), hip.stream())
            self._box_key = key
            self.box_builds += 1
        return self.box

    # -- weights --------------------------------------------------------------------------------------
    def _weights(self):
        m = self.model
        ws = head_weights(m)
        if m.torso:
            ws += torso_weights(m)
        return ws

    def refresh(self):
        ws = self._weights()
        tables = [self.model.encoder.embeddings, self.model.encoder_ambient.embeddings]
        if self.model.torso:
            tables.append(self.model.torso_encoder.embeddings)
        # opt.mlp_dtype = "f16": contractions on the 16-bit matrix cores (fp32 accumulate), the reference's -O arithmetic
        # "f32x2": fp32-grade products from two fp16 halves per operand on the same matrix cores (include/radnerf_fused.h)
        mlp = {"f32": RN_F32, "f16": RN_F16, "f32x2": RN_F32_SPLIT}[
            getattr(getattr(self.model, "opt", None), "mlp_dtype", "f32")]
        # opt.half_tables (load_checkpoint(half_tables=True) sets it): the kernels read persistent fp16 copies of the grid tables
        # (GridEncoder.half_table, re-cast only when the parameter changes) -- the reference's -O mode casts every table on every
        # call (gridencoder/grid.py:43-44: 7.2 + 4.4 + 4.4 MB per loop iteration)
        half = bool(getattr(getattr(self.model, "opt", None), "half_tables", False))
        versions = tuple((w._version, w.data_ptr()) for w in ws + tables) + (mlp, half)
        if versions == self._versions:
            return
        m = self.model
        for w in ws:
            if w.dtype != torch.float32 or not w.is_contiguous():
                raise RuntimeError("fused engine: MLP weights must be contiguous float32")
        self.nw = weights_desc(ws[:8], m.audio_dim, int(m.exp_eye), m.individual_dim)
        assert tuple(ws[0].shape) == (64, 32 + m.audio_dim) and tuple(ws[3].shape) == (64, 64 + int(m.exp_eye))
        assert tuple(ws[5].shape) == (65, 64) and tuple(ws[6].shape) == (64, 80 + m.individual_dim)
        self.mlp_dtype = mlp
        packer = {RN_F32: "rn_nerf_pack_weights", RN_F16: "rn_nerf_pack_weights_h16",
                  RN_F32_SPLIT: "rn_nerf_pack_weights_split"}[mlp]
        hip.call(packer, C.byref(self.nw), hip.ptr(self.packed), hip.stream())
        if m.torso:
            self.tw = torso_weights_desc(ws[8:14], m.individual_dim_torso)
            hip.call("rn_torso_pack_weights", C.byref(self.tw), hip.ptr(self.tpacked), hip.stream())
        # tables: fp32 parameters are read in place; with opt.half_tables their persistent fp16 copies
        if half:
            encs = [m.encoder, m.encoder_ambient] + ([m.torso_encoder] if m.torso else [])
            self.tables = [hip.aligned(e.half_table()) for e in encs]
        else:
            self.tables = [hip.aligned(t.detach()) for t in tables]
        self.gx = _grid_desc(m.encoder, self.tables[0])
        self.gw = _grid_desc(m.encoder_ambient, self.tables[1])
        self.gt = _grid_desc(m.torso_encoder, self.tables[2]) if m.torso else None
        self._versions = versions

    # -- torso plan -----------------------------------------------------------------------------------
    def torso_plan(self, bg_coords, coords, thresh):
        """The plan for this frame's torso pass, or None (the frame then runs rn_torso_blend_frame).  `bg_coords` is the
        caller's tensor, `coords` its contiguous fp32 form.  The key is (address, version, shape) of the coordinates and of the
        occupancy grid, thresh and shrink, the lifetime frame_cache's rule: a caller whose coordinates change with every call
        (patch batches, validation renders during training) never pays for a build.  (The weights, the grid table and the
        pose reach a planned frame as they reach any other: nothing of them is in the plan.)"""
        if not switches.on("RN_TORSO_PLAN"):
            return None
        m = self.model
        refs = [bg_coords, m.density_grid_torso]
        key = (tuple((t.data_ptr(), t._version, tuple(t.shape), tuple(t.stride()), t.dtype) for t in refs),
               float(thresh), float(m.opt.torso_shrink))
        return self._cached(self.cache.plan, key, refs, lambda: self._build_plan(key, refs, coords, thresh))

    def _build_plan(self, key, refs, coords, thresh):
        """-> the record of one torso plan: `buf` (None: larger than RN_TORSO_PLAN_MAX_BYTES) and `n_on`, its covered pixels."""
        m = self.model
        N = int(coords.shape[0])
        n_on = C.c_uint32(0)
        nbytes = int(_lib.rn_torso_plan_bytes(N, 0))
        for _ in range(2):      # the first call finds the covered count, the second has room for its tiles
            buf = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
            hip.call("rn_torso_plan_build", hip.ptr(coords), N, hip.ptr(m.density_grid_torso), int(m.grid_size), float(thresh),
                     float(m.opt.torso_shrink), hip.ptr(buf), nbytes, C.byref(n_on), hip.stream())
            need = int(_lib.rn_torso_plan_bytes(N, n_on.value))
            if need <= nbytes:
                break
            if need > RN_TORSO_PLAN_MAX_BYTES:
                buf = None
                break
            nbytes = need
        return self._built(self.cache.plan, key, refs, [] if buf is None else [buf], buf=buf, n_on=int(n_on.value))

    # -- scratch --------------------------------------------------------------------------------------
    def scratch(self, N):
        if N == self._N:
            return
        d, f32, i32 = self.dev, torch.float32, torch.int32
        self.nears = torch.empty(N, dtype=f32, device=d)
        self.fars = torch.empty(N, dtype=f32, device=d)
        self.rays_alive = torch.empty(2, N, dtype=i32, device=d)
        self.rays_t = torch.empty(N, dtype=f32, device=d)
        self.samples = torch.empty(N * 8, dtype=f32, device=d)   # xyzs | dirs | deltas
        self.sigmas = torch.empty(N, dtype=f32, device=d)
        self.rgbs = torch.empty(N, 3, dtype=f32, device=d)
        self.state = torch.zeros(RN_HEAD_STATE_INTS, dtype=i32, device=d)
        self.stats_prev = [0, 0, 0]
        self.block_counts = torch.zeros(3 * ((N + 255) // 256 + 1), dtype=i32, device=d)
        self.live_slots = torch.empty(N, dtype=i32, device=d)   # live-sample list of the iteration in flight
        self.dir_term, self._dir_term_tried = None, False      # dir_terms() allocates on first use
        self._N = N

    def dir_terms(self):
        """The rays' direction terms for rn_head_t.dir_term, [N, 64] fp32, or None: RN_DIR_TERM=0 (nothing is allocated for a
        process that never switches it on), more than 2^20 rays, or no memory for it.  Written by every frame's first loop
        iteration before anything reads it, so never zeroed; 256 bytes per ray (64 MiB at 512 x 512), one buffer per state.
        The allocation is tried once per scratch(N): a failure is held, a frame never tries again."""
        if not switches.on("RN_DIR_TERM"):
            return None
        if not self._dir_term_tried:
            self._dir_term_tried = True
            if self._N <= DIR_TERM_MAX_RAYS:
                try:
                    self.dir_term = torch.empty(self._N, 64, dtype=torch.float32, device=self.dev)
                except torch.cuda.OutOfMemoryError:
                    pass
        return self.dir_term

    def read_loop_stats(self):
        """The frame just enqueued, for LoopStats: the device counters accumulate across frames, a frame's numbers are the
        difference to the previous read.  Synchronises."""
        cur = self.state[RN_HEAD_ST_ITERS:RN_HEAD_ST_SLOTS + 1].cpu().tolist()
        prev, self.stats_prev = self.stats_prev, cur
        return dict(zip(("iterations", "live_samples", "sample_slots"), ((c - p) & 0xFFFFFFFF for c, p in zip(cur, prev))))

    def head(self, rays_o, rays_d, dt_gamma, max_steps, T_thresh, weights_sum, depth, image):
        """rn_head_t of one frame over this state's scratch (scratch(N) has been called) and the caller's rays and outputs."""
        model, N = self.model, rays_o.shape[0]
        h = HeadT()
        h.rays_o, h.rays_d, h.N = rays_o.data_ptr(), rays_d.data_ptr(), N
        h.aabb, h.min_near = model.aabb_infer.data_ptr(), float(model.min_near)
        h.bitfield, h.bound, h.dt_gamma = model.density_bitfield.data_ptr(), float(model.bound), float(dt_gamma)
        h.max_steps, h.cascade, h.grid_size, h.T_thresh = int(max_steps), int(model.cascade), int(model.grid_size), float(T_thresh)
        h.nears, h.fars = self.nears.data_ptr(), self.fars.data_ptr()
        h.weights_sum, h.depth, h.image = weights_sum.data_ptr(), depth.data_ptr(), image.data_ptr()
        h.rays_alive_a, h.rays_alive_b = self.rays_alive[0].data_ptr(), self.rays_alive[1].data_ptr()
        h.rays_t, h.xyzs = self.rays_t.data_ptr(), self.samples.data_ptr()
        h.dirs, h.deltas = self.samples.data_ptr() + N * 3 * 4, self.samples.data_ptr() + N * 6 * 4
        h.sigmas, h.rgbs = self.sigmas.data_ptr(), self.rgbs.data_ptr()
        h.state, h.block_counts = self.state.data_ptr(), self.block_counts.data_ptr()
        h.live_slots = self.live_slots.data_ptr() if (getattr(model.opt, "live_list", True) and switches.on("RN_LIVE_LIST")) else None
        # image width, if the caller said the rays are the row-major pixels of an image (SyntheticScene does): the loop then
        # walks the rays in 8 x 8 pixel blocks (more shared grid rows per wave; no pixel changes)
        h.order_w = int(getattr(model, "ray_order_width", 0) or 0)
        h.occ_box = hip.ptr(self.occ_box())
        h.dir_term = hip.ptr(self.dir_terms())
        return h


def _all_states(model):
    """Every FusedState of the model that has rendered a frame: one per HIP stream frames are enqueued on."""
    return [st for st in _caches(model).states.values() if st._N]


def loop_counters(model):
    """Cumulative device-side loop counters (iterations, live samples, sample slots), summed over the model's streams;
    synchronises."""
    states = _all_states(model)
    if not states:
        return None
    tot = [0, 0, 0]
    for st in states:
        cur = st.state[RN_HEAD_ST_ITERS:RN_HEAD_ST_SLOTS + 1].cpu().tolist()
        tot = [(a + b) & 0xFFFFFFFF for a, b in zip(tot, cur)]
    return tot


def loop_history(model, n):
    """Device view of the live-ray count entering each of the first n loop iterations of the frame just enqueued (0 once the
    loop is over); see RN_HEAD_ST_HIST."""
    st = _state(model)
    return st.state[RN_HEAD_ST_HIST:RN_HEAD_ST_HIST + n]


def unfinished_frames(model):
    """Frames (cumulative) whose loop was cut short by a speculative iteration count (set_loop_hint); synchronises."""
    return sum(int(st.state[RN_HEAD_ST_UNFINISHED].item()) for st in _all_states(model))


def stalled_workgroups(model):
    """Workgroups (cumulative) that gave up at the in-launch barrier of the one-launch loop step (RN_LOOP_COOP); must be 0 --
    a frame rendered while this moved is invalid.  Synchronises."""
    return sum(int(st.state[RN_HEAD_ST_STALLED].item()) for st in _all_states(model))


def loop_flags(model):
    """Flags of rn_head_iterate_ex for this model: `opt.loop_launch` = "split" (default: a launch each for the compositor and
    for compaction + next march, 3 launches per iteration) or "coop" (both in one launch with a grid-wide barrier inside, 2
    launches per iteration; measured 2 % SLOWER on MI355X -- the barrier costs more than the kernel boundary it replaces,
    DESIGN.md section 3 -- and limited to three streams per device, see RN_LOOP_COOP in radnerf_fused.h)."""
    coop = getattr(model.opt, "loop_launch", "split") == "coop"
    return RN_LOOP_COOP if coop else 0


def set_loop_hint(model, iterations):
    """Enqueue only `iterations` loop iterations per frame from now on (None: all max_steps, the default).  The device
    records frames for which that was not enough (unfinished_frames); the caller checks it where it synchronises and
    renders those frames again.  Meant for streams whose iteration count is known from earlier frames."""
    hint = None if iterations is None else max(1, int(iterations))
    _caches(model).loop_hint = hint
    object.__setattr__(model, "_fused_loop_hint", hint)      # bench.py reads the hint by this name


def _state(model):
    """The model's state for the CURRENT stream (created on first use)."""
    states = _caches(model).states
    key = torch.cuda.current_stream().cuda_stream if torch.cuda.is_available() else 0
    if key not in states:
        states[key] = FusedState(model)
    return states[key]


def _frame_bias(st, enc_a, eye, ind_code, batch=False):
    """Fold the broadcast inputs (audio code, eye or the zero eye, individual code or NULL) into the first-layer biases:
    rn_nerf_frame_bias into st.bias for one code, or -- batch -- rn_nerf_frame_bias_batch into a new [n, 192] block for the n
    rows of enc_a [n, audio_dim]."""
    eye_t = eye.reshape(-1).contiguous().float() if eye is not None else st._zero_eye
    ind = ind_code.detach().reshape(-1).contiguous().float() if ind_code is not None else None
    if batch:
        codes = enc_a.contiguous().float()
        n = codes.shape[0]
        out = torch.empty(n, st.bias.numel(), dtype=torch.float32, device=codes.device)
        hip.call("rn_nerf_frame_bias_batch", C.byref(st.nw), hip.ptr(codes), n, hip.ptr(eye_t), hip.ptr(ind), hip.ptr(out), hip.stream())
        return out
    enc_a = enc_a.reshape(-1).contiguous().float()
    hip.call("rn_nerf_frame_bias", C.byref(st.nw), hip.ptr(enc_a), hip.ptr(eye_t), hip.ptr(ind), hip.ptr(st.bias), hip.stream())
    return st.bias


def network_forward(model, xyzs, dirs, enc_a, ind_code, eye, deltas=None, want_ambient=True):
    """NeRFNetwork.forward through the fused kernel: (sigma [M], color [M,3], ambient [M,2])."""
    st = _state(model)
    st.refresh()
    xyzs, dirs = xyzs.contiguous().float(), dirs.contiguous().float()
    M = xyzs.shape[0]
    _frame_bias(st, enc_a, eye, ind_code)
    sigmas = torch.empty(M, dtype=torch.float32, device=xyzs.device)
    rgbs = torch.empty(M, 3, dtype=torch.float32, device=xyzs.device)
    ambient = torch.empty(M, 2, dtype=torch.float32, device=xyzs.device) if want_ambient else None
    if deltas is not None:
        deltas = deltas.contiguous()
    hip.call("rn_nerf_fused_forward", hip.ptr(xyzs), hip.ptr(dirs), hip.ptr(deltas), M, None, C.byref(st.gx), C.byref(st.gw),
             hip.ptr(st.packed), hip.ptr(st.bias), float(model.bound), hip.ptr(sigmas), hip.ptr(rgbs), hip.ptr(ambient),
             st.mlp_dtype, hip.stream())
    return sigmas, rgbs, ambient


def density_forward(model, xyzs, enc_a, eye, out=None):
    """NeRFNetwork.density (nerf/network.py:286-325) through the fused kernel's sigma branch: no geo_feat layer, no SH, no
    colour network.  xyzs [M,3] -> sigma [M] (written into `out` when given)."""
    st = _state(model)
    st.refresh()
    xyzs = xyzs.contiguous().float()
    M = xyzs.shape[0]
    _frame_bias(st, enc_a, eye, model.individual_codes[0] if model.individual_dim > 0 else None)
    sigmas = out if out is not None else torch.empty(M, dtype=torch.float32, device=xyzs.device)
    hip.call("rn_nerf_fused_forward", hip.ptr(xyzs), None, None, M, None, C.byref(st.gx), C.byref(st.gw), hip.ptr(st.packed),
             hip.ptr(st.bias), float(model.bound), hip.ptr(sigmas), None, None, st.mlp_dtype, hip.stream())
    return sigmas


def torso_forward(model, bg_coords, poses6, ind_code_torso, thresh, bg_in=None, bg_out=None, alpha_out=None, deform_out=None):
    """The torso layer over N pixels (nerf/renderer.py:269-299 + nerf/network.py:188-219): occupancy test against `thresh`,
    deformation / torso networks, blend over bg_in (None = white).  Returns (bg_out [N,3], alpha_out [N,1])."""
    st = _state(model)
    st.refresh()
    N = bg_coords.shape[0]
    dev = bg_coords.device
    bg_coords = bg_coords.contiguous().float()
    poses6, ict = torso_constants(poses6, ind_code_torso)
    if bg_out is None:
        bg_out = torch.empty(N, 3, dtype=torch.float32, device=dev)
    if alpha_out is None:
        alpha_out = torch.empty(N, 1, dtype=torch.float32, device=dev)
    hip.call("rn_torso_fused", hip.ptr(bg_coords), N, hip.ptr(model.density_grid_torso), int(model.grid_size), float(thresh),
             hip.ptr(poses6), hip.ptr(ict), float(model.opt.torso_shrink), C.byref(st.tw), hip.ptr(st.tpacked), C.byref(st.gt),
             hip.ptr(bg_in), hip.ptr(bg_out), hip.ptr(alpha_out), hip.ptr(deform_out), hip.stream())
    return bg_out, alpha_out


def frame_bias_batch(model, codes, eye, ind_code):
    """Per-frame bias blocks of n consecutive frames' audio codes [n, audio_dim] -> [n, 192] (one launch)."""
    st = _state(model)
    st.refresh()
    return _frame_bias(st, codes, eye, ind_code, batch=True)


def render_frame(model, rays_o, rays_d, enc_a, ind_code, eye, bg_coords, poses, ind_code_torso, bg_color, dt_gamma,
                 max_steps, T_thresh, want_u8=False, ray_source=None, frame_bias=None):
    """Inference frame: returns dict(image [N,3], depth [N], weights_sum [N], nears, fars[, image_u8]).

    Launches per frame (whole-frame renders): ONE prologue (rays from `ray_source` = (pose [4,4] on the device, intrinsics,
    W) when given -- rays_o / rays_d are then output buffers --, near/far, loop initialisation, march of iteration 0), per
    loop iteration {network, composite, compaction + next march}, ONE epilogue (torso pass + blend [+ uint8]); plus the
    per-frame bias fold unless the caller hands in `frame_bias` (frame_bias_batch)."""
    st = _state(model)
    st.refresh()
    N = rays_o.shape[0]
    st.scratch(N)
    dev = rays_o.device
    s = hip.stream()

    if frame_bias is None:
        bias = _frame_bias(st, enc_a, eye, ind_code)
    else:
        bias = frame_bias.reshape(-1)
        assert bias.numel() == st.bias.numel() and bias.is_contiguous() and bias.dtype == torch.float32

    weights_sum = torch.empty(N, dtype=torch.float32, device=dev)
    depth = torch.empty(N, dtype=torch.float32, device=dev)
    image = torch.empty(N, 3, dtype=torch.float32, device=dev)

    h = st.head(rays_o, rays_d, dt_gamma, max_steps, T_thresh, weights_sum, depth, image)

    # The whole <= max_steps loop is enqueued without reading anything back: iterations past the end of the loop
    # are no-ops decided on the device (a few microseconds each), so the host can run ahead of the GPU.
    shard = getattr(model, "shard_schedule", None)
    merged = shard is None and getattr(model.opt, "frame_kernels", "merged") == "merged"
    n_iters = int(max_steps) if st.loop_hint is None else min(int(max_steps), st.loop_hint)
    gx = st.frame_grid()      # the xyz table, or its dense image (same features)
    pose, cam, W = None, (0.0, 0.0, 0.0, 0.0), 0
    if ray_source is not None:
        pose, cam, W = ray_source
        pose, cam, W = pose.reshape(-1, 4)[:4].contiguous().float(), tuple(float(v) for v in cam), int(W)
    if merged:
        hip.call("rn_frame_begin", C.byref(h), hip.ptr(pose), *cam, W, s)
        hip.call("rn_head_iterate_ex", C.byref(h), C.byref(gx), C.byref(st.gw), hip.ptr(st.packed), hip.ptr(bias), 0, n_iters,
                 st.mlp_dtype, RN_LOOP_FIRST_MARCHED | RN_LOOP_CLOSE_FRAME | loop_flags(model), s)
    else:
        if ray_source is not None:
            hip.call("rn_get_rays", hip.ptr(pose), *cam, N // W, W, hip.ptr(rays_o), hip.ptr(rays_d), s)
        hip.call("rn_head_begin", C.byref(h), s)
        if shard is None:
            hip.call("rn_head_iterate_ex", C.byref(h), C.byref(gx), C.byref(st.gw), hip.ptr(st.packed), hip.ptr(bias), 0,
                     n_iters, st.mlp_dtype, loop_flags(model), s)
        else:
            # This call renders a shard of a frame (tile-parallel): the step schedule must be the whole frame's, so the
            # live-ray counts are summed over the ranks between iterations -- still without the host reading anything.
            group, n_total = shard
            total = torch.empty(1, dtype=torch.int32, device=dev)
            for it in range(n_iters):
                hip.call("rn_head_iterate_ex", C.byref(h), C.byref(gx), C.byref(st.gw), hip.ptr(st.packed), hip.ptr(bias),
                         it, 1, st.mlp_dtype, loop_flags(model), s)
                bank = ((it + 1) & 1) * 8
                total.copy_(st.state[bank:bank + 1])
                group.all_reduce(total)
                hip.call("rn_head_reschedule", C.byref(h), it, int(n_total), hip.ptr(total), hip.stream())
        if n_iters < int(max_steps):
            hip.call("rn_head_check_done", C.byref(h), n_iters, s)

    # torso layer over the background, final blend
    bg_in = None
    if torch.is_tensor(bg_color):
        bg_in = bg_color.reshape(-1, 3).contiguous().float()
        if bg_in.shape[0] != N:
            bg_in = bg_in.expand(N, 3).contiguous()
    elif bg_color is not None and float(bg_color) != 1.0:
        bg_in = torch.full((N, 3), float(bg_color), dtype=torch.float32, device=dev)
    results = {}
    model.last_stats = LoopStats(st)
    u8 = torch.empty(N, 3, dtype=torch.uint8, device=dev) if want_u8 else None
    if model.torso and merged:
        thresh = min(model.density_thresh_torso, model.mean_density_torso)
        keep = getattr(model.opt, "keep_torso_layer", True)      # results["torso_color"] / ["torso_alpha"] (the reference returns them)
        talpha = torch.empty(N, 1, dtype=torch.float32, device=dev) if keep else None
        bg_final = torch.empty(N, 3, dtype=torch.float32, device=dev) if keep else None
        coords = bg_coords.contiguous().float()
        p6, ict = torso_constants(poses, ind_code_torso)
        plan = st.torso_plan(bg_coords, coords, thresh)
        if plan is not None:
            hip.call("rn_torso_blend_frame_planned", hip.ptr(plan.buf), plan.buf.numel(), N, plan.n_on, hip.ptr(p6), hip.ptr(ict),
                     float(model.opt.torso_shrink), C.byref(st.tw), hip.ptr(st.tpacked), C.byref(st.gt), hip.ptr(bg_in),
                     hip.ptr(bg_final), hip.ptr(talpha), None, hip.ptr(image), hip.ptr(weights_sum), hip.ptr(depth),
                     hip.ptr(st.nears), hip.ptr(st.fars), hip.ptr(u8), s)
        else:
            hip.call("rn_torso_blend_frame", hip.ptr(coords), N, hip.ptr(model.density_grid_torso), int(model.grid_size), float(thresh),
                     hip.ptr(p6), hip.ptr(ict), float(model.opt.torso_shrink), C.byref(st.tw), hip.ptr(st.tpacked), C.byref(st.gt),
                     hip.ptr(bg_in), hip.ptr(bg_final), hip.ptr(talpha), hip.ptr(image), hip.ptr(weights_sum), hip.ptr(depth),
                     hip.ptr(st.nears), hip.ptr(st.fars), hip.ptr(u8), s)
        if keep:
            results["torso_alpha"], results["torso_color"] = talpha, bg_final
    else:
        bg_final = bg_in
        if model.torso:
            thresh = min(model.density_thresh_torso, model.mean_density_torso)
            bg_final, talpha = torso_forward(model, bg_coords, poses, ind_code_torso, thresh, bg_in=bg_in)
            results["torso_alpha"], results["torso_color"] = talpha, bg_final
        hip.call("rn_blend_frame", hip.ptr(image), hip.ptr(weights_sum), hip.ptr(bg_final), hip.ptr(depth), hip.ptr(st.nears),
                 hip.ptr(st.fars), N, hip.ptr(u8), s)
    results.update(image=image, depth=depth, weights_sum=weights_sum, nears=st.nears, fars=st.fars)
    if want_u8:
        results["image_u8"] = u8
    return results


def get_rays(pose, intrinsics, H, W):
    """Full-image rays of one cam2world pose [4,4] (or [1,4,4]) on the device: dict(rays_o, rays_d) of shape [1, H*W, 3]
    (get_rays with N = -1, nerf/utils.py:249-333) in one launch."""
    pose = pose.reshape(-1, 4)[:4].contiguous().float()
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    rays_o = torch.empty(1, H * W, 3, dtype=torch.float32, device=pose.device)
    rays_d = torch.empty(1, H * W, 3, dtype=torch.float32, device=pose.device)
    hip.call("rn_get_rays", hip.ptr(pose), fx, fy, cx, cy, int(H), int(W), hip.ptr(rays_o), hip.ptr(rays_d), hip.stream())
    return {"rays_o": rays_o, "rays_d": rays_d}


def get_bg_coords(H, W, device):
    """[1, H*W, 2] (nerf/utils.py:240-245) in one launch."""
    out = torch.empty(1, int(H) * int(W), 2, dtype=torch.float32, device=device)
    hip.call("rn_get_bg_coords", int(H), int(W), hip.ptr(out), hip.stream())
    return out


def convert_poses(poses):
    """[B, 4, 4] cam2world -> [B, 6] (nerf/utils.py:231-237) in one launch."""
    p = poses.contiguous().float()
    out = torch.empty(p.shape[0], 6, dtype=torch.float32, device=p.device)
    hip.call("rn_convert_poses", hip.ptr(p), p.shape[0], hip.ptr(out), hip.stream())
    return out
