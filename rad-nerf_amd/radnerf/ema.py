"""The averaged weights the reference evaluates, tests and saves "best" checkpoints under (nerf/utils.py:1069-1080, :1233-1298,
:1346-1358): torch_ema.ExponentialMovingAverage(model.parameters(), decay=0.95) with use_num_updates=True, updated when
global_step % ema_update_interval == 0 (:1018).

ParamEma restates that class in plain torch (torch_ema is not a dependency; the update rule and the state_dict's keys are
restated from torch_ema 0.3 -- see DESIGN).  It is the CPU route, the holder of the shadow tensors on every route, and the oracle of
the tests.  On the GPU route the update itself runs inside the Adam launches (HipAdam(..., ema=), C ABI rn_adam_step_sched): the
shadows stay here, the update counter moves to the device.
"""
import torch


class ParamEma:
    """Shadows of `parameters` in their order (model.parameters(): the order the reference's checkpoints use).

    update():   num_updates += 1; d = min(decay, (1 + num_updates) / (10 + num_updates));
                per tensor  tmp = shadow - param;  tmp *= 1 - d;  shadow -= tmp        (three roundings, as torch_ema does them)
    store() / copy_to() / restore(): the weights put aside, the shadows copied into the model, the weights brought back.
    update_interval is carried for the caller that owns the step count (Trainer, HipAdam); update() itself always updates."""

    def __init__(self, parameters, decay, update_interval=1):
        if not 0.0 <= decay <= 1.0:
            raise ValueError("ParamEma: decay must be between 0 and 1")
        if int(update_interval) < 1:
            raise ValueError("ParamEma: update_interval must be at least 1")
        self.params = list(parameters)
        self.decay, self.update_interval = float(decay), int(update_interval)
        self._num_updates = 0
        self.device_num_updates = None          # int32 device scalar once an optimizer updates on the device (HipAdam)
        self.shadow_params = [p.detach().clone(memory_format=torch.contiguous_format) for p in self.params]
        self.collected_params = None

    # ---- the update count: a host integer, or the device word the optimizer's begin kernel advances
    @property
    def num_updates(self):
        if self.device_num_updates is not None:
            return int(self.device_num_updates.item())
        return self._num_updates

    @num_updates.setter
    def num_updates(self, n):
        self._num_updates = int(n)
        if self.device_num_updates is not None:
            self.device_num_updates.fill_(int(n))

    def restrict(self, held):
        """Keep shadows only for the parameters in `held` (what an optimizer updates).  Any other parameter never changes, so its
        shadow equals the weight by construction: none is stored, state_dict() writes a clone of the weight."""
        held = {id(p) for p in held}
        for i, p in enumerate(self.params):
            if id(p) not in held:
                self.shadow_params[i] = None

    def shadow_of(self, p):
        for q, s in zip(self.params, self.shadow_params):
            if q is p:
                return s
        return None

    def pairs(self):
        """(parameter, shadow) of every parameter that has a stored shadow."""
        return [(p, s) for p, s in zip(self.params, self.shadow_params) if s is not None]

    @torch.no_grad()
    def update(self):
        n = self.num_updates + 1
        self.num_updates = n
        one_minus_decay = 1.0 - min(self.decay, (1 + n) / (10 + n))
        for p, s in self.pairs():
            tmp = s - p
            tmp.mul_(one_minus_decay)
            s.sub_(tmp)

    @torch.no_grad()
    def store(self):
        self.collected_params = [p.detach().clone() if s is not None else None for p, s in zip(self.params, self.shadow_params)]

    @torch.no_grad()
    def copy_to(self):
        for p, s in self.pairs():
            p.copy_(s)

    @torch.no_grad()
    def restore(self):
        if self.collected_params is None:
            raise RuntimeError("ParamEma: restore() without a store()")
        for p, c in zip(self.params, self.collected_params):
            if c is not None:
                p.copy_(c)
        self.collected_params = None

    def state_dict(self):
        """torch_ema's four keys; the shadows in model.parameters() order -- the `ema` entry of a reference checkpoint
        (nerf/utils.py:1327-1328, read back at :1388-1389)."""
        shadows = [(s if s is not None else p.detach()).clone() for p, s in zip(self.params, self.shadow_params)]
        collected = None
        if self.collected_params is not None:
            collected = [(c if c is not None else p.detach()).clone() for p, c in zip(self.params, self.collected_params)]
        return {"decay": self.decay, "num_updates": self.num_updates, "shadow_params": shadows, "collected_params": collected}

    @torch.no_grad()
    def load_state_dict(self, sd):
        shadows = sd["shadow_params"]
        if len(shadows) != len(self.params) or any(tuple(a.shape) != tuple(p.shape) for a, p in zip(shadows, self.params)):
            raise ValueError("ParamEma: shadow_params do not match the parameters")
        self.decay = float(sd["decay"])
        if not 0.0 <= self.decay <= 1.0:
            raise ValueError("ParamEma: decay must be between 0 and 1")
        self.num_updates = 0 if sd.get("num_updates") is None else int(sd["num_updates"])
        for s, a in zip(self.shadow_params, shadows):
            if s is not None:
                s.copy_(a)
        collected = sd.get("collected_params")
        if collected is not None:
            self.collected_params = [c.to(p.device, p.dtype).clone() if s is not None else None
                                     for p, s, c in zip(self.params, self.shadow_params, collected)]
        else:
            self.collected_params = None

    @torch.no_grad()
    def reset_to_weights(self):
        """Shadows = the current weights (after loading a checkpoint that carries no average)."""
        for p, s in self.pairs():
            s.copy_(p)
