"""One training step of the render path (BASELINE config 2): the train branch of run_cuda
(march_rays_train -> NeRFNetwork.forward -> composite_rays_train, all over the HIP operators and their
backward kernels), the reference's loss and its Adam parameter groups.

Reference: Trainer.train_step (nerf/utils.py:718-806) for the loss, Trainer.train_one_epoch (:1003-1040) for
the order zero_grad -> step -> backward -> optimizer and the `update_extra_state` cadence
(`--update_extra_interval 16`, main.py:31), main.py:204 for Adam(betas=(0.9, 0.99), eps=1e-15) over
NeRFNetwork.get_params(lr, lr_net) (nerf/network.py:328-357).  The data loader, LPIPS and GradScaler are outside the path
(out of scope) and are not rebuilt.  What main.py:204-224 wraps around the step is opt-in by argument: the LambdaLR
decay (lr_gamma), the EMA of the weights (ema_decay, ema_update_interval; radnerf/ema.py) -- on the GPU both inside the Adam
launches, keyed on the optimizer's device-side step counter (rn_adam_step_sched) -- and Trainer.evaluate, the validation loss and
PSNR of nerf/utils.py:1220-1300 under the averaged weights with one read-back.
"""
import contextlib

import torch

# by the package's name: this file is also loaded on its own (tests/test_train_host.py)
from radnerf import route, switches
from radnerf.optim import HipAdam, make_optimizer      # both stay part of this module's surface
from radnerf.step_graphs import GraphCache, HeldScalar, StaticInputs


def entropy_of(alphas):
    """nerf/utils.py:785-794: binary entropy that pushes an opacity towards 0 or 1."""
    a = alphas.clamp(1e-5, 1 - 1e-5)
    return -a * torch.log2(a) - (1 - a) * torch.log2(1 - a)


def _patch_views(data, n):
    """(weight, (P, h, w), force_all_rays) of a lip fine-tuning batch, or None for a plain one: a `rect` batch is ONE h x w image
    at weight 0.01 (nerf/utils.py:757-766), a `patch_size` > 1 batch P = n / patch_size^2 square patches at weight 0.001
    (:773-781) -- and only the latter marches all rays (:741)."""
    rect, ps = data.get("rect"), int(data.get("patch_size") or 1)
    if rect is not None and ps > 1:
        raise ValueError("train_step: a batch is sampled by `rect` or by `patch_size`, not both")
    if rect is not None:
        xmin, xmax, ymin, ymax = rect
        if (xmax - xmin) * (ymax - ymin) != n:
            raise ValueError(f"train_step: rect {tuple(rect)} does not hold the batch's {n} rays")
        return 0.01, (1, xmax - xmin, ymax - ymin), False
    if ps > 1:
        if n % (ps * ps):
            raise ValueError(f"train_step: {n} rays are no multiple of patch_size^2 = {ps * ps}")
        return 0.001, (n // (ps * ps), ps, ps), True
    return None


def _patch_term(criterion, weight, shape, pred, rgb):
    """weight * criterion(pred patches, target patches).mean() with both as [P,3,h,w] (nerf/utils.py:759-760, 774-775)."""
    P, h, w = shape
    nchw = lambda t: t.reshape(P, h, w, 3).permute(0, 3, 1, 2).contiguous()
    return weight * criterion(nchw(pred), nchw(rgb)).mean()


def train_step(model, data, opt, global_step=0, iters=200000, lambda_amb=0.1, amb_weight=None, patch_criterion=None):
    """-> (pred_rgb, target_rgb, loss); `data` has the keys of the reference's loader batch
    (nerf/provider.py:588-690): rays_o, rays_d [B,N,3], bg_coords [1,N,2], poses [B,6], face_mask [B,N],
    eye [B,1], auds, index, bg_color [B,N,3], images (head) or bg_torso_color (torso) [B,N,3].

    Lip fine-tuning (DeviceTrainSet.batch_rect / batch_patch): a batch with `rect`, or with `patch_size` > 1, adds
    weight * patch_criterion(pred, target).mean() on [P,3,h,w] views -- weight 0.01 and one h x w view for a rect, 0.001 and
    [P,3,ps,ps] for patches (which also march all rays).  patch_criterion is the caller's perceptual function (the reference's
    LPIPS); it returns [P,1,1,1], or anything `.mean()` reduces.  The value is nerf/utils.py:757-783's: there the [P,1,1,1] term
    is broadcast onto the [B,N] squared errors before the mean, which is mean(mse) + weight * mean(term).  Without a criterion
    such a batch trains as a plain one.  On the fused loss route the term's gradient reaches the ready-made gradients through
    train_head.head_loss_chain."""
    torso = bool(opt.torso)
    rgb = data["bg_torso_color"] if torso else data["images"]
    views = _patch_views(data, int(rgb.reshape(-1, 3).shape[0]))
    force_all = views is not None and views[2]
    term_of = None
    if views is not None and patch_criterion is not None:
        term_of = lambda pred: _patch_term(patch_criterion, views[0], views[1], pred, rgb)
    fused_loss = (not torso and rgb.is_cuda and rgb.dtype == torch.float32 and switches.get("RN_TRAIN_LOSS") == "fused"
                  and torch.is_tensor(data.get("bg_color")) and data["bg_color"].dtype == torch.float32)
    # opt-in: a torso step that stays on the device (covered pixels compacted there, blend + loss in one kernel).  Asked for here
    # when the target can feed the loss kernel; the renderer decides (train_torso.step_usable, once per step) and answers with
    # the compact pieces, or with today's results
    torso_direct = (torso and term_of is None and rgb.is_cuda and rgb.dtype == torch.float32 and torch.is_tensor(data.get("bg_color"))
                    and route.kernels("train_torso").step_enabled())
    out = model.render(data["rays_o"], data["rays_d"], data["auds"], data["bg_coords"], data["poses"], eye=data["eye"],
                       index=data["index"], staged=False, bg_color=data["bg_color"], perturb=True, force_all_rays=force_all,
                       dt_gamma=opt.dt_gamma, max_steps=opt.max_steps, defer_blend=fused_loss or torso_direct)
    if "torso_alpha_c" in out:
        from . import train_torso
        loss, pred, alpha_full = train_torso.torso_loss(out["torso_alpha_c"], out["torso_color_c"], out["torso_covered"], out["torso_count"],
                                                        out["background"], rgb)
        out["torso_color"], out["torso_alpha"] = pred, alpha_full
        return pred, rgb, loss
    if "head_image" in out:
        # blend over the background (nerf/renderer.py:306), clamp and the loss below with their gradients: ONE kernel
        from . import train_head
        face = data["face_mask"]
        face = face if face.dtype == torch.float32 else face.float()
        w = amb_weight if amb_weight is not None else torch.full((1,), min(global_step / iters, 1.0) * lambda_amb, device=rgb.device)
        loss, pred = train_head.head_loss(out["head_image"], out["weights_sum"], out["ambient"], out["background"], rgb, face, w)
        if term_of is not None:
            own = list(patch_criterion.parameters()) if isinstance(patch_criterion, torch.nn.Module) else []
            loss = train_head.head_loss_chain(loss, pred, out["background"], term_of, own)
        return pred.view(rgb.shape), rgb, loss
    pred = out["torso_color"] if torso else out["image"]
    if not torso and pred.is_cuda:
        from . import train_glue
        face = data["face_mask"].reshape(-1)
        if train_glue.enabled(pred, rgb, out["weights_sum"], out["ambient"]):
            w = amb_weight if amb_weight is not None else torch.full((1,), min(global_step / iters, 1.0) * lambda_amb, device=pred.device)
            loss = train_glue.train_loss(pred, rgb, out["weights_sum"], out["ambient"], face if face.dtype == torch.float32 else face.float(), w)
            return pred, rgb, loss if term_of is None else loss + term_of(pred)
    # the torso prediction is [n, 3], its target [1, n, 3]: the same values without the broadcast (and its warning); a target
    # of another size is an error (reshape raises), not something to broadcast
    target = rgb.reshape(pred.shape) if torso else rgb
    loss = torch.nn.functional.mse_loss(pred, target, reduction="none").mean(-1).mean()
    if torso:
        loss = loss + 1e-4 * entropy_of(out["torso_alpha"]).mean()
    else:
        loss = loss + 1e-4 * entropy_of(out["weights_sum"]).mean()
        # ambient coordinates should stay put outside the face (nerf/utils.py:796-803), weight ramped over `iters`
        face = data["face_mask"].reshape(-1)
        loss_amb = (out["ambient"] * ((~face) if face.dtype == torch.bool else (1.0 - face))).mean()   # a 0/1 float mask is the same product
        # amb_weight: the same factor as a device scalar (a captured step reads it instead of baking the Python float in)
        loss = loss + (amb_weight if amb_weight is not None else min(global_step / iters, 1.0) * lambda_amb) * loss_amb
    if term_of is not None:
        loss = loss + term_of(pred)
    return pred, rgb, loss


def lips_schedule(train_set, index, step):
    """The batch of step `step` of lip fine-tuning: the frame's lips rect on even steps, a plain batch of random pixels on odd
    ones -- the `flip_finetune_lips` alternation of nerf/utils.py:769-770, which starts on the rect."""
    return train_set.batch_rect(index) if step % 2 == 0 else train_set.batch(index)


def _backward(loss):
    """loss.backward(); a loss of the fused head-loss kernel hands its ready-made input gradients to autograd directly."""
    if getattr(loss, "_rn_direct", None) is not None:
        from . import train_head
        train_head.backward(loss)
    else:
        loss.backward()


class SyntheticTrainStream:
    """Batches of `n_rays` random pixels of a SyntheticScene frame with the scene's own frozen render as target
    (SURVEY 8(d) config 2); everything stays on the device."""

    def __init__(self, scene, n_rays=4096, frame=0, seed=0):
        self.scene, self.n_rays, self.frame = scene, n_rays, frame
        self.gen = torch.Generator(device=scene.device).manual_seed(seed)
        m = scene.model
        was_training = m.training
        m.eval()
        with torch.no_grad():
            out = scene.render(frame)
        m.train(was_training)
        self.f = scene.frame(frame)
        self.target = out["image"].reshape(1, -1, 3).clamp(0, 1).detach().clone()
        # "face" = pixels the head layer changed (the loader's face_mask comes from a parsing net, provider.py:199-215)
        self.face_mask = (self.target - self.f["bg_color"].reshape(1, -1, 3)).abs().sum(-1) > 1e-3
        # what update_extra_state samples from (main.py:183-186 hands the loader's arrays to the model)
        m.aud_features, m.poses = scene.aud_features, scene.poses
        m.eye_area = torch.full((scene.n_frames, 1), 0.25, device=scene.device)
        self._table = None

    def batch(self):
        """One gather for the whole batch: the per-pixel arrays are kept side by side in one [n_px, 15] table, the batch's
        tensors are views of the gathered rows (key `_packed`: GraphedTrainer copies that one tensor into its static input)."""
        f, n_px = self.f, self.target.shape[1]
        if self._table is None:
            cols = [f["rays_o"][0], f["rays_d"][0], f["bg_coords"][0], f["bg_color"][0], self.target[0], self.face_mask[0].float().unsqueeze(-1)]
            self._table = torch.cat([c.reshape(n_px, -1).float() for c in cols], dim=1).contiguous()
        idx = torch.randint(0, n_px, (self.n_rays,), device=self.target.device, generator=self.gen)
        packed = switches.on("RN_TRAIN_PACKED")
        if self._table.is_cuda and packed:
            # one kernel: the picked rows, every column section written as its own contiguous array of one flat buffer
            from . import train_head
            flat, _ = train_head.batch_gather(self._table, idx, self._WIDTHS)
            return self.unpack(flat)
        rows = self._table.index_select(0, idx)
        flat = torch.cat([rows[:, a:a + w].reshape(-1) for a, w in zip(self._COL0, self._WIDTHS)])
        out = self.unpack(flat)
        if not packed:                                          # experiment switch: separate tensors, as a generic loader would hand over
            out = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in out.items() if not k.startswith("_")}
        return out

    _WIDTHS = (3, 3, 2, 3, 3, 1)          # rays_o | rays_d | bg_coords | bg_color | target | face: the table's column sections
    _COL0 = (0, 3, 6, 8, 11, 14)

    def unpack(self, flat):
        """Batch dict over the sections of `flat` ([n, 3] rays_o | [n, 3] rays_d | [n, 2] bg_coords | [n, 3] bg_color | [n, 3] target |
        [n] face, each contiguous): every per-ray entry is a VIEW (face_mask stays 0/1 floats), so refreshing `flat` in place
        refreshes the batch."""
        n = flat.numel() // sum(self._WIDTHS)
        sec, at = [], 0
        for w in self._WIDTHS:
            sec.append(flat[at:at + n * w].view(1, n, w))
            at += n * w
        f = self.f
        return dict(rays_o=sec[0], rays_d=sec[1], bg_coords=sec[2], poses=f["poses"], face_mask=sec[5].view(1, n),
                    eye=f["eye"], auds=f["auds"], index=[self.frame], bg_color=sec[3], images=sec[4],
                    bg_torso_color=sec[4], _packed=flat, _unpack=self.unpack)


class Trainer:
    """zero_grad -> train_step -> backward -> Adam, with the occupancy grid refreshed every
    `update_extra_interval` steps as the reference's loop does under --cuda_ray (nerf/utils.py:1015-1018)."""

    # the perceptual term of a lip fine-tuning batch (train_step).  A class default, so that a trainer assembled without
    # __init__ around another trainer's state (bench.py's eager probe) steps as it did before the term existed
    patch_criterion = None
    # the same for the schedule around the step: such a trainer has no EMA and a constant rate
    ema = lr_gamma = None
    _device_schedule = False
    # and for the device copy of the sample budget, made at the first step that has one
    _budget = None

    def __init__(self, model, opt, lr=5e-3, lr_net=5e-4, update_extra_interval=16, iters=200000, lambda_amb=0.1,
                 prefer_rocblas=True, capturable=False, patch_criterion=None, ema_decay=None, ema_update_interval=1000, lr_gamma=None):
        # The weight gradients of the 64-wide MLPs are [64 x ~40 000] x [~40 000 x 96] products: all reduction, almost
        # no output.  On this stack hipBLASLt runs them without a K split (132 us each, measured), rocBLAS in 37 us;
        # eight of them per step make that the largest single item of the step.
        if prefer_rocblas and torch.cuda.is_available() and getattr(torch.version, "hip", None):
            torch.backends.cuda.preferred_blas_library("cublas")      # "cublas" selects rocBLAS on ROCm builds
        self.model, self.opt = model, opt
        # the reference's schedule around the step (main.py:204-224), both opt-in: ema_decay (0.95 there) keeps averaged weights,
        # updated when the step count is a multiple of ema_update_interval; lr_gamma (0.1; 0.05 for --finetune_lips) decays every
        # group's rate by lr_gamma ** (step / iters).  HipAdam carries both on the device; another optimizer gets them from the host
        self.ema = self.lr_gamma = None
        if ema_decay is not None:
            from radnerf.ema import ParamEma
            self.ema = ParamEma(model.parameters(), ema_decay, ema_update_interval)
        if lr_gamma is not None:
            self.lr_gamma = float(lr_gamma)
            if not self.lr_gamma > 0 or iters <= 0:
                raise ValueError("Trainer: lr_gamma needs lr_gamma > 0 and iters > 0")
        schedule = None if self.lr_gamma is None else (self.lr_gamma, iters)
        self.optimizer = make_optimizer(model, lr, lr_net, capturable=capturable, schedule=schedule, ema=self.ema)
        if schedule is not None:
            for g in self.optimizer.param_groups:
                g.setdefault("initial_lr", g["lr"])      # the host route's base rate (HipAdam sets it itself)
        self._device_schedule = isinstance(self.optimizer, HipAdam) and self.optimizer._sched
        self.update_extra_interval, self.iters, self.lambda_amb = update_extra_interval, iters, lambda_amb
        self.patch_criterion = patch_criterion
        self.global_step = 0

    def _host_schedule(self):
        """After a step of an optimizer that does not carry the schedule itself (the CPU route, RN_ADAM=torch): the rate of the
        next step (LambdaLR.step()) and the EMA update on its cadence (nerf/utils.py:1018, 1030-1034)."""
        if self._device_schedule:
            return
        if self.lr_gamma is not None:
            for g in self.optimizer.param_groups:
                g["lr"] = g["initial_lr"] * self.lr_gamma ** (self.global_step / self.iters)
        if self.ema is not None and self.global_step % self.ema.update_interval == 0:
            self.ema.update()

    @contextlib.contextmanager
    def ema_scope(self):
        """The model under its averaged weights (ema.store(); ema.copy_to() ... ema.restore(), nerf/utils.py:1233-1235, 1297-1298);
        the trained weights come back on exit, also on an exception.  On the GPU one launch exchanges weights and shadows
        (rn_param_swap) -- no third copy of the model -- and the tensors' versions are bumped, so caches of packed weights
        (FusedState) re-pack.  Without an EMA: nothing happens."""
        ema = self.ema
        if ema is None:
            yield
            return
        pairs = ema.pairs()
        if pairs and pairs[0][0].is_cuda:
            import ctypes
            import radnerf_hip as hip
            n = len(pairs)
            a = (ctypes.c_void_p * n)(*[p.data_ptr() for p, _ in pairs])
            b = (ctypes.c_void_p * n)(*[s.data_ptr() for _, s in pairs])
            numel = (ctypes.c_uint32 * n)(*[p.numel() for p, _ in pairs])
            if any(not p.is_contiguous() or p.dtype != torch.float32 for p, _ in pairs):
                raise RuntimeError("ema_scope: parameters must be contiguous fp32")

            def swap():
                hip.call("rn_param_swap", a, b, numel, n, hip.stream())
                hip.mark_written([p for p, _ in pairs])
            swap()
            try:
                yield
            finally:
                swap()
        else:
            ema.store()
            ema.copy_to()
            try:
                yield
            finally:
                ema.restore()

    @contextlib.contextmanager
    def eval_scope(self):
        """What evaluate() and save_mesh() run under: eval mode, no_grad, the averaged weights when there is an EMA; the mode the
        model was in comes back on exit, also on an exception."""
        m = self.model
        was_training = m.training
        m.eval()
        try:
            with torch.no_grad(), self.ema_scope():
                yield
        finally:
            m.train(was_training)

    def evaluate(self, train_set, indices, rect=None, perceptual=None):
        """Validation over the frames `indices` of a DeviceTrainSet, as Trainer.evaluate_one_epoch does it (nerf/utils.py:1220-1300):
        eval mode, the averaged weights when there is an EMA, no_grad; per frame train_set.frame(i), model.render as eval_step
        calls it (:810-838) and the frame's squared error summed on the device (rn_image_error) into row i of one array -- ONE
        read-back after the last frame where the reference reads every frame back twice.
        rect: None, "face" / "lips" (the set's rect of each frame), an [F,4] or [4] integer array (xmin, xmax, ymin, ymax; x along
        the ROWS).  -> dict(loss = mean over frames of the MSE, psnr = mean over frames of -10 log10(mse_f) (PSNRMeter's averaging),
        per_frame = [(mse, psnr)], rect_psnr = the same mean over the rect's pixels, None without a rect).
        perceptual: a criterion such as percep.PerceptualAlex; the dict then also has lpips = mean over frames of
        perceptual(truth, pred, normalize=True) on [1,3,H,W] views (LPIPSMeter's argument order and averaging, nerf/utils.py:438-466)
        and lpips_per_frame; the values stay on the device until the same single read-back."""
        import numpy as np
        m = self.model
        indices = [int(i) for i in indices]
        if not indices:
            raise ValueError("evaluate: no frames")
        dev = next(m.parameters()).device
        on_gpu = dev.type == "cuda"
        rects = _eval_rects(train_set, rect, dev)
        H, W = train_set.H, train_set.W
        sums = torch.zeros(len(indices), 5 if perceptual is not None else 4, dtype=torch.float64, device=dev)
        if on_gpu:
            import radnerf_hip as hip
            ws = hip.persistent_buffer("image_error", int(hip._lib.rn_image_error_workspace(H, W)), dev)
        with self.eval_scope():
            for k, i in enumerate(indices):
                f = train_set.frame(i)
                out = m.render(f["rays_o"], f["rays_d"], f["auds"], f["bg_coords"], f["poses"], eye=f["eye"], index=f["index"],
                               staged=True, bg_color=f["bg_color"], perturb=False, dt_gamma=self.opt.dt_gamma,
                               max_steps=self.opt.max_steps)
                pred = out["image"].reshape(H * W, 3)
                truth = f["images"].reshape(H * W, 3)
                r = None if rects is None else (rects if rects.dim() == 1 else rects[f["index"][0]])
                if on_gpu:
                    pred = pred if pred.dtype == torch.float32 and pred.is_contiguous() else pred.float().contiguous()
                    hip.call("rn_image_error", hip.ptr(pred), hip.ptr(truth), H, W, hip.ptr(r), hip.ptr(ws), hip.ptr(sums[k]), hip.stream())
                else:
                    sums[k, :4] = _image_error_host(pred, truth, H, W, r)
                if perceptual is not None:
                    nchw = lambda t: t.reshape(1, H, W, 3).permute(0, 3, 1, 2)
                    sums[k, 4] = perceptual(nchw(truth.float()), nchw(pred.float()), normalize=True).reshape(())
        s = sums.cpu().numpy()                                   # the one read-back
        mse = s[:, 0] / s[:, 2]
        psnr = -10.0 * np.log10(mse)
        res = dict(loss=float(mse.mean()), psnr=float(psnr.mean()), per_frame=[(float(a), float(b)) for a, b in zip(mse, psnr)],
                   rect_psnr=None)
        if rects is not None:
            with np.errstate(divide="ignore", invalid="ignore"):
                res["rect_psnr"] = float((-10.0 * np.log10(s[:, 1] / s[:, 3])).mean())
        if perceptual is not None:
            res["lpips"], res["lpips_per_frame"] = float(s[:, 4].mean()), [float(v) for v in s[:, 4]]
        return res

    def save_mesh(self, path, resolution=256, threshold=10, auds=None, enc_a=None, eye=None):
        """The head's surface sigma = threshold inside aabb_infer as a binary PLY (Trainer.save_mesh, nerf/utils.py:871-891), on
        the device (radnerf/mesh.py): eval mode, no_grad, the averaged weights when there is an EMA, as evaluate().  The geometry
        depends on the audio and the eye, so exactly one of auds (a window [8, audio_in_dim, 16], encoded with
        model.encode_audio) and enc_a (an audio code) is given, and eye ([1,1]) on a model with exp_eye.
        -> (vertices, triangles), the device tensors that were written."""
        import os
        from radnerf import mesh
        m = self.model
        if (auds is None) == (enc_a is None):
            raise ValueError("save_mesh: give exactly one of auds (an audio window) and enc_a (an audio code)")
        if eye is None and getattr(m, "exp_eye", False):
            raise ValueError("save_mesh: the model has exp_eye, so the export needs an eye value")
        with self.eval_scope():
            if enc_a is None:
                enc_a = m.encode_audio(auds)
            vertices, triangles = mesh.extract_geometry(m, resolution, threshold, enc_a, eye)
        if os.path.dirname(path):
            os.makedirs(os.path.dirname(path), exist_ok=True)
        mesh.write_ply(path, vertices, triangles)
        return vertices, triangles

    def _begin_step(self):
        """What comes before every step: train mode, the occupancy refresh on its cadence, the step count."""
        m = self.model
        m.train()
        if self.update_extra_interval and self.global_step % self.update_extra_interval == 0:
            with torch.no_grad():
                m.update_extra_state()
        self.global_step += 1
        return m

    def _forward_backward_update(self, data, budget, amb_weight=None):
        """zero_grad -> train_step -> backward -> optimizer.step with `budget` as the renderer's sample budget (device int32 budget,
        row capacity; None: the marcher of the first window); returns the loss with its graph."""
        m = self.model
        self.optimizer.zero_grad(set_to_none=True)
        m._sample_budget = budget
        try:
            with _join_in_optimizer(self.optimizer):
                _, _, loss = train_step(m, data, self.opt, self.global_step, self.iters, self.lambda_amb, amb_weight,
                                        self.patch_criterion)
                _backward(loss)
                self.optimizer.step()
        finally:
            m._sample_budget = None
        return loss

    def step(self, data):
        m = self._begin_step()
        loss = self._forward_backward_update(data, self._device_budget(m)).detach()
        self._host_schedule()
        return loss

    def _device_budget(self, m):
        """(device int32 budget, row capacity) for the renderer's one-launch marcher, or None (first window, CPU).  The budget is
        raymarching.py:226-229's aligned running average; the device copy is rewritten only when it moves (every 16 steps)."""
        dev = next(m.parameters()).device
        if m.mean_count <= 0 or dev.type != "cuda":
            return None
        budget = _aligned_budget(m.mean_count)
        if self._budget is None or self._budget.tensor.device != dev:
            self._budget = HeldScalar(1, torch.int32, dev)
        return self._budget.set(budget), budget


def _eval_rects(train_set, rect, dev):
    """evaluate()'s `rect` as an int32 tensor on `dev`: [F,4] (one row per frame), [4] (the same for every frame) or None."""
    if rect is None:
        return None
    if isinstance(rect, str):
        if rect == "face":
            return train_set.face_rect.to(dev)
        if rect == "lips":
            if train_set.lips_rect is None:
                raise ValueError("evaluate: the set has no lips rects")
            held = getattr(train_set, "_lips_dev", None)
            if held is None or held.device != dev:
                held = train_set._lips_dev = torch.tensor(train_set.lips_rect, dtype=torch.int32, device=dev)
            return held
        raise ValueError(f"evaluate: rect={rect!r} (None, 'face', 'lips' or an integer array)")
    r = torch.as_tensor(rect).to(dev, torch.int32).contiguous()
    if r.shape != (4,) and (r.dim() != 2 or r.shape[1] != 4):
        raise ValueError("evaluate: rect must be [4] or [F,4] = (xmin, xmax, ymin, ymax)")
    return r


def _image_error_host(pred, truth, H, W, rect):
    """rn_image_error's four numbers with torch operators (the CPU route): the difference in fp32, squares and sums in double."""
    sq = (pred.float() - truth.float()).double().square().reshape(H, W, 3)
    out = torch.zeros(4, dtype=torch.float64, device=pred.device)
    out[0], out[2] = sq.sum(), sq.numel()
    if rect is not None:
        xmin, xmax, ymin, ymax = (int(v) for v in rect.tolist())
        inside = sq[max(xmin, 0):max(xmax, 0), max(ymin, 0):max(ymax, 0)]
        out[1], out[3] = inside.sum(), inside.numel()
    return out


def _aligned_budget(mean_count):
    """raymarching.py:226-229: the running average of the sample count, rounded up past the next multiple of 128."""
    budget = int(mean_count)
    return budget + 128 - budget % 128


def _join_in_optimizer(optimizer):
    """HipAdam.step waits for the table-gradient scatter the backward pass left on a side stream (route.deferred_join); any other
    optimizer gets gradients that are complete when backward() returns."""
    return route.deferred_join() if isinstance(optimizer, HipAdam) and torch.cuda.is_available() else contextlib.nullcontext()


class GraphedTrainer(Trainer):
    """Trainer.step with the steady-state step replayed from a hipGraph (torch.cuda.CUDAGraph): forward, loss, backward and the
    fused Adam update are ~320 launches whose enqueue costs the host more than the GPU needs to run them; replaying them as
    one graph makes the step GPU-bound and its duration repeatable.

    What stays outside the graph: the occupancy refresh every `update_extra_interval` steps, the batch (copied into the
    graph's static input buffers), the ring of per-step sample counters (the captured step counts into one static pair,
    copied to the ring afterwards) and the first window, whose marcher reads back its sample count (raymarching.py:249-255)
    and therefore runs eagerly.  The refresh changes `mean_count`, the marcher's sample budget M (raymarching.py:226-229): the
    graph is captured for a row CAPACITY (the budget rounded up to a multiple of `capacity_step`, kept while the budget stays
    within it) and the budget itself is a device scalar the marcher reads (rn_march_rays_train_budget), so a refresh changes a
    number, not the graph; rows between budget and capacity stay zero and belong to no ray.  A new graph is captured only
    when the budget leaves the capacity window for a capacity not seen before (the last `max_graphs` graphs are kept: the
    budget of a model whose density depends on the audio swings by +-20 % between refreshes).  Same arithmetic as Trainer.step.

    Lip fine-tuning batches (`rect` / `patch_size`, DeviceTrainSet.batch_rect / batch_patch) are refused by default: their ray
    count follows the frame.  lips_graphs = G > 0 opts in: such a batch is captured at its first occurrence after the first window
    and replayed like a plain one, ONE GRAPH PER SHAPE.  A rect batch is keyed by the row capacity, the rays' shape and the rect's
    (h, w) -- not by its position or frame, so another frame's rect of the same shape replays the same graph, while 32 x 40 and
    40 x 32 (the same rays, other perceptual views) do not share one.  A patch batch has one key, ("patch", n, patch_size),
    whatever the running budget: it marches every ray, which the one-launch marcher does under a device budget of n * max_steps
    rows (aligned as the running budget is) at a capacity of the same size -- no ray can need more, and nothing is read back.
    Every ray layout, a plain one too, has static inputs of its own; the lips graphs live in a least-recently-used cache of G
    entries, the plain graphs in another of `max_graphs` (step_graphs.GraphCache; size G from DeviceTrainSet.lips_shapes(): the
    shapes times the two or three capacities a run
    visits), each graph with its private memory pool, and an evicted graph takes its static inputs with it when no other graph
    uses them.  The patch_criterion runs inside the capture: PerceptualAlex's weight image is packed before it begins, and a
    criterion that cannot be captured (one that asks the host for a value, say) fails with torch's own capture error.  The first
    window and a CPU model take the eager step for these batches too; without a patch_criterion such a batch trains as a plain
    one (train_step's rule), under its own key."""

    # no lips graphs: a trainer assembled without __init__ (bench.py's) refuses lip fine-tuning batches as it always did
    lips_graphs = 0

    def __init__(self, model, opt, capacity_step=4096, max_graphs=8, lips_graphs=0, **kw):
        if int(lips_graphs) < 0:
            raise ValueError(f"GraphedTrainer: lips_graphs = {lips_graphs} (0: lip fine-tuning batches are refused; G > 0: up to G "
                             "captured lips graphs are kept)")
        # a CPU model only ever takes the eager step, and torch's Adam refuses capturable=True for parameters off the device
        super().__init__(model, opt, capturable=next(model.parameters()).is_cuda, **kw)
        if (self.ema is not None or self.lr_gamma is not None) and not self._device_schedule and next(model.parameters()).is_cuda:
            raise ValueError("GraphedTrainer: ema_decay / lr_gamma ride inside HipAdam's launches; a captured step of another "
                             "optimizer (RN_ADAM=torch) cannot carry them")
        self.capacity_step = int(capacity_step)
        self.max_graphs = int(max_graphs)
        self.lips_graphs = int(lips_graphs)
        self._capacity = 0
        # the captured steps of plain and of lips batches, least recently used first over static inputs per ray layout (keys:
        # _step_key): a budget that comes back to an earlier capacity replays that graph
        self._plain, self._lips = GraphCache(max_graphs), GraphCache(lips_graphs)
        dev = next(model.parameters()).device
        self._amb_weight = HeldScalar((), torch.float32, dev)
        self._counter = torch.zeros(2, dtype=torch.int32, device=dev)
        self.captures = self.replays = self.lips_captures = 0
        self.capture_log = []          # (step, budget, capacity) of every capture of a plain batch
        self.lips_capture_log = []     # (step, budget, capacity, "rect" | "patch", (h, w) | (P, ps, ps)) of every lips capture

    def _record(self, static, budget):
        """Capture one step over `static` with `budget` = (device int32 budget, row capacity[, True]) as the renderer's sample
        budget; what the step would create lazily is created first.  -> (graph, loss)."""
        m = self.model
        from raymarching.ops import step_marcher_prepare, step_marcher_supported
        n_rays = int(static["rays_o"].reshape(-1, 3).shape[0])
        if step_marcher_supported(n_rays, self._counter.device):
            step_marcher_prepare(n_rays, self._counter.device)       # persistent state: must not be born inside the capture
        if self._torso_route():
            route.kernels("train_torso").prepare(m, n_rays)          # the same for the torso route: pinned mean density, workspaces
        elif not self.opt.torso and route.kernels("train_head").supported(m):
            # RN_TRAIN_DETERMINISTIC=1: the ordered table scatter's workspace at this graph's row capacity
            route.kernels("train_head").prepare_scatter((m.encoder, m.encoder_ambient), budget[1], self._counter.device)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        self.optimizer.zero_grad(set_to_none=True)            # gradients of earlier steps go before the capture begins
        m._static_counter = self._counter                     # renderer._head_training counts into this pair while captured
        try:
            with torch.cuda.graph(g):                         # a private memory pool per graph: cached graphs never alias each other
                loss = self._forward_backward_update(static, budget, self._amb_weight.tensor)
        finally:
            m._static_counter = None
        m.local_step -= 1                                     # the capture pass went through the Python bookkeeping once
        return g, loss

    def _step_key(self, data):
        """-> (cache, key, layout, kind, shape) of a batch after the first window.  A plain batch (kind None) is keyed by the row
        capacity and the rays' shape.  A rect batch by those, "rect" and the rect's (h, w); a patch batch by ("patch", n,
        patch_size) whatever the capacity: it marches under a budget of its own.  The layout is the key without the capacity."""
        rays = tuple(data["rays_o"].shape)
        if data.get("rect") is None and int(data.get("patch_size") or 1) <= 1:
            return self._plain, (self._capacity, rays), ("plain", rays), None, None
        rgb = data["bg_torso_color"] if self.opt.torso else data["images"]
        n = int(rgb.reshape(-1, 3).shape[0])
        shape = _patch_views(data, n)[1]                       # (P, h, w); also refuses views that do not hold the batch's rays
        if data.get("rect") is not None:
            layout = (rays, "rect", shape[1:])
            return self._lips, (self._capacity,) + layout, layout, "rect", shape[1:]
        key = ("patch", n, int(data["patch_size"]))
        return self._lips, key, key, "patch", shape

    def _capture(self, data, kind, shape, inputs):
        """The graph of a key seen for the first time (or evicted since), over `inputs` -- or, where that is None, over new static
        inputs of the batch's ray layout.  -> (graph, loss, inputs), GraphCache.get's capture."""
        if inputs is None:
            budget = None
            if kind == "patch":
                # every sample of every ray: none takes more than max_steps, so this budget drops no ray (force_all_rays)
                rows = _aligned_budget(shape[0] * shape[1] * shape[2] * int(self.opt.max_steps))
                budget = (torch.full((1,), rows, dtype=torch.int32, device=self._counter.device), rows, True)
            inputs = StaticInputs(data, self._counter.device, budget)
            if kind == "rect":
                inputs.static["rect"] = tuple(int(v) for v in data["rect"])      # train_step reads (h, w) off it, nothing else
            elif kind == "patch":
                inputs.static["patch_size"] = int(data["patch_size"])
        if kind is not None and hasattr(self.patch_criterion, "packed_image"):
            self.patch_criterion.packed_image()                # PerceptualAlex's weight image: packed before the capture begins
        budget = inputs.budget if inputs.budget is not None else (self._budget.tensor, self._capacity)
        g, loss = self._record(inputs.static, budget)
        self.captures += 1
        row = (self.global_step, int(budget[0].item()), budget[1])
        if kind is None:
            self.capture_log.append(row)
        else:
            self.lips_captures += 1
            self.lips_capture_log.append(row + (kind, shape))
        return g, loss, inputs

    def _torso_route(self):
        """A torso step can be captured only on the device-resident route (opt-in RN_TORSO_TRAIN=fused, radnerf/train_torso.py):
        the default one asks the host for the covered pixels."""
        return bool(self.opt.torso) and next(self.model.parameters()).is_cuda and route.kernels("train_torso").step_enabled()

    def step(self, data):
        lips = data.get("rect") is not None or int(data.get("patch_size") or 1) > 1
        if lips and self.lips_graphs <= 0:
            raise ValueError("GraphedTrainer: a lip fine-tuning batch (`rect` / `patch_size`) cannot be replayed from a captured "
                             "step -- its ray count follows the frame's rect; take such steps with Trainer")
        m = self._begin_step()
        if self._torso_route():
            route.kernels("train_torso").pin_mean(m)   # a mean set from the host since the last step goes into the scalar the graph reads
        running = self._device_budget(m)               # the device scalar every graph of a running budget reads
        if running is None:                            # first window / CPU: the eager step
            loss = self._forward_backward_update(data, None).detach()
            self._host_schedule()
            return loss
        budget, step = running[1], self.capacity_step
        if not (budget <= self._capacity <= budget + 2 * step):         # keep the capacity while the budget stays inside its window
            self._capacity = -(-(budget + step // 4) // step) * step
        cache, key, layout, kind, shape = self._step_key(data)
        graph, loss, inputs = cache.get(key, layout, lambda held: self._capture(data, kind, shape, held))
        inputs.feed(data)
        self._amb_weight.set(min(self.global_step / self.iters, 1.0) * self.lambda_amb)
        if isinstance(self.optimizer, HipAdam):
            self.optimizer.refresh_lr()             # a schedule may have rewritten param_groups[i]["lr"] since the last step
        graph.replay()
        if isinstance(self.optimizer, HipAdam):
            self.optimizer.replayed()
        m.step_counter[m.local_step % 16].copy_(self._counter)
        m.local_step += 1
        self.replays += 1
        return loss.detach()
