"""The reference's Adam over NeRFNetwork.get_params (main.py:204, nerf/network.py:328-357): make_optimizer picks the implementation,
HipAdam is the one-kernel update on the GPU with the LambdaLR decay and the EMA of the weights inside its launches
(rn_adam_step_lr / rn_adam_step_sched, csrc/rn_train.hip).  radnerf/train.py drives them."""
import torch

from radnerf import route, switches


def make_optimizer(model, lr=5e-3, lr_net=5e-4, fused=None, capturable=False, kernel=None, schedule=None, ema=None):
    """main.py:204; lr for the grid tables, lr_net for the MLPs / audio nets / individual codes.  On the GPU the update runs
    as ONE kernel over all tensors (HipAdam; `kernel="torch"` or RN_ADAM=torch: torch's fused Adam, one launch per parameter
    group) -- the 49 MB table is read and written once per step either way; same arithmetic as the default implementation.
    schedule = (gamma, iters) / ema = ParamEma: HipAdam carries them inside its launches; any other optimizer ignores them here
    (Trainer then applies both from the host after each step)."""
    on_gpu = next(model.parameters()).is_cuda
    if kernel is None:
        kernel = switches.get("RN_ADAM") if on_gpu else "torch"
    if kernel == "hip" and on_gpu:
        return HipAdam(model.get_params(lr, lr_net), schedule=schedule, ema=ema)
    if fused is None:
        fused = on_gpu
    return torch.optim.Adam(model.get_params(lr, lr_net), betas=(0.9, 0.99), eps=1e-15, fused=bool(fused),
                            capturable=bool(capturable))


class HipAdam:
    """torch.optim.Adam(betas, eps, weight_decay=0) over the model's parameter groups with ONE update kernel for all
    tensors (C ABI rn_adam_step, csrc/rn_train.hip) -- the table, its moments and its gradient stream through HBM once.
    Same interface as far as Trainer needs it (param_groups, zero_grad, step, state_dict / load_state_dict in
    torch.optim.Adam's format, so reference checkpoints carry over); the step counter lives on the device, so a step is
    capturable in a hipGraph.

    schedule = (gamma, iters) and / or ema = ParamEma select rn_adam_step_sched: every tensor's rate is lr0 * gamma ** ((s - 1) / iters)
    at step s (LambdaLR as the reference drives it, main.py:219), computed by the begin kernel from the device-side step counter,
    and on steps with s % ema.update_interval == 0 the same launches fold the new weights into the shadows (which stay in the
    ParamEma; its update counter moves to the device).  Nothing is uploaded per step on that route: refresh_lr() is a no-op,
    current_lr() is a host mirror for logging, and param_groups[i]["lr"] is only rewritten by state_dict()."""

    # what torch.optim.Adam keeps in every param_group (torch/optim/adam.py): a state dict written here loads into the
    # reference's torch.optim.Adam (nerf/utils.py:1302-1426 saves / restores optimizer.state_dict())
    _TORCH_ADAM_DEFAULTS = dict(weight_decay=0, amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False,
                                fused=None, decoupled_weight_decay=False)

    def __init__(self, params, betas=(0.9, 0.99), eps=1e-15, schedule=None, ema=None):
        import radnerf_hip as hip
        self._hip = hip
        self.param_groups = []
        for g in params:
            g = dict(g)
            g["params"] = [g["params"]] if torch.is_tensor(g["params"]) else list(g["params"])    # a bare tensor is one parameter
            if g.get("weight_decay", 0):
                raise ValueError("HipAdam: weight decay is not part of the reference's configuration (main.py:204) and not implemented")
            g.setdefault("betas", betas)
            g.setdefault("eps", eps)
            for k, v in self._TORCH_ADAM_DEFAULTS.items():
                g.setdefault(k, v)
            g.setdefault("initial_lr", g["lr"])      # what torch's LR schedulers look for (LambdaLR, main.py:219)
            self.param_groups.append(g)
        self.betas, self.eps = betas, eps
        self.defaults = dict(lr=self.param_groups[0]["lr"], betas=betas, eps=eps, **self._TORCH_ADAM_DEFAULTS)
        dev = self.param_groups[0]["params"][0].device
        self.state = {p: {"exp_avg": torch.zeros_like(p, memory_format=torch.contiguous_format),
                          "exp_avg_sq": torch.zeros_like(p, memory_format=torch.contiguous_format)}
                      for g in self.param_groups for p in g["params"]}
        self._step = torch.zeros(1, dtype=torch.int32, device=dev)
        self._corr = torch.zeros(2, dtype=torch.float32, device=dev)
        n = sum(len(g["params"]) for g in self.param_groups)
        # learning rates live on the device, one per updated tensor in the order of the last step(): a captured step reads
        # them at run time, so a schedule that rewrites param_groups[i]["lr"] is followed by every replay (refresh_lr())
        self._lr_dev = torch.zeros(max(n, 1), dtype=torch.float32, device=dev)
        self._lr_groups, self._lr_sent, self._written = [], None, []
        self._sched = schedule is not None or ema is not None
        self.ema, self._host_step, self.uploads = ema, 0, 0       # uploads: host -> device copies refresh_lr() made
        self.gamma, self.sched_iters = (float(schedule[0]), int(schedule[1])) if schedule is not None else (1.0, 0)
        if self._sched:
            if not self.gamma > 0 or (self.gamma != 1.0 and self.sched_iters <= 0):
                raise ValueError("HipAdam: schedule=(gamma, iters) needs gamma > 0, and iters > 0 unless gamma == 1")
            self._corr = torch.zeros(4, dtype=torch.float32, device=dev)
            if ema is not None:
                ema.restrict([p for g in self.param_groups for p in g["params"]])
                if ema.device_num_updates is None:
                    ema.device_num_updates = torch.full((1,), ema._num_updates, dtype=torch.int32, device=dev)

    def current_lr(self):
        """Per group, the rate the NEXT step uses -- what param_groups[i]["lr"] shows in the reference once its scheduler has
        stepped.  A host mirror (initial_lr, gamma and the number of steps taken); nothing is read from the device."""
        if not self._sched:
            return [float(g["lr"]) for g in self.param_groups]
        f = 1.0 if self.gamma == 1.0 else self.gamma ** (self._host_step / self.sched_iters)
        return [float(g["initial_lr"]) * f for g in self.param_groups]

    def note_replayed(self, n=1):
        """A captured step was replayed n times: the device-side counter advanced, the host mirror follows."""
        self._host_step += int(n)

    def zero_grad(self, set_to_none=True):
        for g in self.param_groups:
            for p in g["params"]:
                if set_to_none:
                    p.grad = None
                elif p.grad is not None:
                    p.grad.zero_()

    def refresh_lr(self):
        """Upload the groups' current learning rates when they changed since the last upload (call outside a capture; a
        GraphedTrainer does so before every replay).  With a device-side schedule there is nothing to upload."""
        if self._sched:
            return
        lrs = [float(self.param_groups[gi]["lr"]) for gi in self._lr_groups]
        if lrs and lrs != self._lr_sent:
            self._lr_dev[:len(lrs)].copy_(torch.tensor(lrs, dtype=torch.float32))
            self._lr_sent = lrs
            self.uploads += 1

    @torch.no_grad()
    def step(self):
        pending = route.take_pending_events()    # table-gradient scatters still running on the side stream (route.deferred_join)
        if pending:
            held = {p.grad.data_ptr() for g in self.param_groups for p in g["params"] if p.grad is not None}
            for ev, *ptrs in pending:
                torch.cuda.current_stream().wait_event(ev)
                if not all(q in held for q in ptrs):
                    # autograd copied a table gradient instead of keeping the buffer the scatter writes (a parameter that
                    # already had a .grad): that copy raced with the side stream
                    raise RuntimeError("HipAdam: a table gradient was copied before its scatter had finished; use "
                                       "zero_grad(set_to_none=True) or RN_TRAIN_OVERLAP=0")
        if self._sched:
            return self._step_sched()
        rows = list(self._tensors())              # held until the launch is enqueued: a gradient made contiguous lives only here
        arr = (self._hip.abi.AdamTensorT * max(len(rows), 1))()
        for i, (gi, p, grad, st) in enumerate(rows):
            arr[i].param, arr[i].grad, arr[i].exp_avg, arr[i].exp_avg_sq = p.data_ptr(), grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
            arr[i].numel, arr[i].lr = p.numel(), float(self.param_groups[gi]["lr"])
        groups = [gi for gi, _, _, _ in rows]
        if groups != self._lr_groups:
            self._lr_groups, self._lr_sent = groups, None
        if not torch.cuda.is_current_stream_capturing():
            self.refresh_lr()
        elif self._lr_sent is None:
            raise RuntimeError("HipAdam: take one eager step (or call refresh_lr()) before capturing a step in a graph")
        self._hip.call("rn_adam_step_lr", arr, len(rows), float(self.betas[0]), float(self.betas[1]), float(self.eps),
                       self._hip.ptr(self._step), self._hip.ptr(self._corr), self._hip.ptr(self._lr_dev), self._hip.stream())
        self._wrote(rows)

    def _tensors(self, riders=()):
        """(group index, parameter, contiguous gradient or None, state) of every tensor a step takes, in the groups' order: those
        with a gradient, and of the parameters whose id() is in `riders` also those without one."""
        for gi, g in enumerate(self.param_groups):
            for p in g["params"]:
                grad = p.grad
                if grad is None and id(p) not in riders:
                    continue
                if grad is not None and not grad.is_contiguous():
                    grad = grad.contiguous()
                if not p.is_contiguous() or p.dtype != torch.float32 or (grad is not None and grad.dtype != torch.float32):
                    raise RuntimeError("HipAdam: parameters and gradients must be contiguous fp32")
                yield gi, p, grad, self.state[p]

    def _wrote(self, rows):
        """The launch over `rows` wrote through raw pointers: caches keyed on tensor versions must see it (and replayed(), later)."""
        self._written = [p for _, p, grad, _ in rows if grad is not None]
        self._hip.mark_written(self._written)

    def replayed(self, n=1):
        """A captured step was replayed n times: its update went through the same raw pointers, and the device-side counter advanced."""
        self._hip.mark_written(self._written)
        self.note_replayed(n)

    def _step_sched(self):
        """The same update through rn_adam_step_sched: rates and the EMA decision come from the device-side step counter.  A
        parameter without a gradient this step still rides along when it has a shadow (torch_ema averages every parameter)."""
        hip, ema = self._hip, self.ema
        shadows = {id(p): s for p, s in ema.pairs()} if ema is not None else {}
        rows = list(self._tensors(riders=shadows))
        arr = (hip.abi.SchedTensorT * max(len(rows), 1))()
        for i, (gi, p, grad, st) in enumerate(rows):
            arr[i].param, arr[i].grad, arr[i].exp_avg, arr[i].exp_avg_sq = p.data_ptr(), hip.ptr(grad), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
            arr[i].shadow, arr[i].numel, arr[i].lr0 = hip.ptr(shadows.get(id(p))), p.numel(), float(self.param_groups[gi]["initial_lr"])
        if len(rows) > self._lr_dev.numel():
            raise RuntimeError("HipAdam: more tensors than learning-rate slots")
        decay, interval = (ema.decay, ema.update_interval) if ema is not None else (0.0, 0)
        hip.call("rn_adam_step_sched", arr, len(rows), float(self.betas[0]), float(self.betas[1]), float(self.eps), self.gamma,
                 self.sched_iters, float(decay), int(interval), hip.ptr(self._step), hip.ptr(self._corr), hip.ptr(self._lr_dev),
                 hip.ptr(ema.device_num_updates) if ema is not None else None, hip.stream())
        if not torch.cuda.is_current_stream_capturing():
            self._host_step += 1
        self._wrote(rows)

    def state_dict(self):
        """torch.optim.Adam's layout: state by running parameter index, one `step` per tensor.  With a device-side schedule the
        groups' `lr` is the rate the next step uses, as the reference's scheduler leaves it."""
        if self._sched:
            for g, lr in zip(self.param_groups, self.current_lr()):
                g["lr"] = lr
        step = self._step.to(torch.float32).reshape(()).clone()
        state, groups, at = {}, [], 0
        for g in self.param_groups:
            ids = []
            for p in g["params"]:
                state[at] = {"step": step.clone(), "exp_avg": self.state[p]["exp_avg"], "exp_avg_sq": self.state[p]["exp_avg_sq"]}
                ids.append(at)
                at += 1
            groups.append({**{k: v for k, v in g.items() if k != "params"}, "params": ids})
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        params = [p for g in self.param_groups for p in g["params"]]
        steps = []
        for i, p in enumerate(params):
            st = sd["state"].get(i)
            if st is None:
                continue
            self.state[p]["exp_avg"].copy_(st["exp_avg"])
            self.state[p]["exp_avg_sq"].copy_(st["exp_avg_sq"])
            steps.append(int(st["step"]))
        if steps:
            self._step.fill_(max(steps))
            self._host_step = max(steps)
        for g, sg in zip(self.param_groups, sd["param_groups"]):
            g["lr"] = sg.get("lr", g["lr"])
