"""radnerf/ema.py on CPU tensors: ParamEma against a float64 restatement of torch_ema's update, its state dict, the store / copy_to /
restore cycle, the checkpoint's `ema` entry, and the Trainer's cadence on a CPU model.  No GPU anywhere in this file."""
import os
import types

import numpy as np
import torch


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(*s, generator=g)) for s in ((5,), (3, 4), (1,), (2, 3, 2))]


def test_update_matches_a_float64_restatement():
    """Five updates with new weights before each: shadow -= (1 - d) (shadow - p), d = min(0.95, (1 + n) / (10 + n)), in float64 on
    the same fp32 weights.  Bar: 1e-6 relative to the largest shadow -- three fp32 roundings (6e-8 each) per update, five updates."""
    from radnerf.ema import ParamEma
    ps = _params()
    ema = ParamEma(ps, 0.95, update_interval=3)
    ref = [p.detach().double().clone() for p in ps]
    g = torch.Generator().manual_seed(1)
    for n in range(1, 6):
        with torch.no_grad():
            for p in ps:
                p.add_(0.3 * torch.randn(p.shape, generator=g))
        ema.update()
        d = min(0.95, (1 + n) / (10 + n))
        ref = [s - (1 - d) * (s - p.detach().double()) for s, p in zip(ref, ps)]
    assert ema.num_updates == 5 and ema.update_interval == 3
    for s, r in zip(ema.shadow_params, ref):
        assert float((s.double() - r).abs().max()) <= 1e-6 * float(r.abs().max()), (s, r)
        assert s.dtype == torch.float32


def test_state_dict_keys_and_round_trip():
    from radnerf.ema import ParamEma
    ps = _params()
    ema = ParamEma(ps, 0.95)
    with torch.no_grad():
        for p in ps:
            p.mul_(1.5)
    ema.update()
    ema.update()
    sd = ema.state_dict()
    assert list(sd) == ["decay", "num_updates", "shadow_params", "collected_params"]                 # torch_ema's four keys
    assert sd["decay"] == 0.95 and sd["num_updates"] == 2 and sd["collected_params"] is None
    assert len(sd["shadow_params"]) == len(ps) and all(a.shape == p.shape for a, p in zip(sd["shadow_params"], ps))
    assert all(a.data_ptr() != s.data_ptr() for a, s in zip(sd["shadow_params"], ema.shadow_params))  # copies, not views
    other = ParamEma(_params(seed=5), 0.5)
    other.load_state_dict(sd)
    assert other.decay == 0.95 and other.num_updates == 2
    assert all(torch.equal(a, b) for a, b in zip(other.shadow_params, ema.shadow_params))
    other.update()
    assert other.num_updates == 3
    try:
        ParamEma(_params()[:2], 0.95).load_state_dict(sd)
        raise AssertionError("a state dict with another number of tensors was accepted")
    except ValueError:
        pass


def test_store_copy_to_restore():
    from radnerf.ema import ParamEma
    ps = _params()
    ema = ParamEma(ps, 0.95)
    with torch.no_grad():
        for p in ps:
            p.add_(1.0)
    ema.update()
    weights = [p.detach().clone() for p in ps]
    shadows = [s.clone() for s in ema.shadow_params]
    ema.store()
    ema.copy_to()
    assert all(torch.equal(p.detach(), s) for p, s in zip(ps, shadows)) and not torch.equal(ps[0].detach(), weights[0])
    assert ema.state_dict()["collected_params"] is not None
    ema.restore()
    assert all(torch.equal(p.detach(), w) for p, w in zip(ps, weights))
    assert all(torch.equal(s, t) for s, t in zip(ema.shadow_params, shadows)) and ema.collected_params is None


def test_a_parameter_no_optimizer_holds_keeps_shadow_equal_weight():
    """restrict(): a frozen parameter stores no shadow; its state-dict entry is a clone of the weight, and update / copy_to /
    restore leave it alone."""
    from radnerf.ema import ParamEma
    ps = _params()
    ema = ParamEma(ps, 0.95)
    ema.restrict(ps[:2])
    with torch.no_grad():
        for p in ps:
            p.add_(1.0)
    ema.update()
    sd = ema.state_dict()
    assert torch.equal(sd["shadow_params"][2], ps[2].detach()) and sd["shadow_params"][2].data_ptr() != ps[2].data_ptr()
    assert not torch.equal(sd["shadow_params"][0], ps[0].detach())
    before = ps[3].detach().clone()
    ema.store(); ema.copy_to(); ema.restore()
    assert torch.equal(ps[3].detach(), before) and len(ema.pairs()) == 2


def test_checkpoint_round_trip_with_and_without_ema(hiplib, tmp_path):
    from radnerf.checkpoint import load_checkpoint, save_checkpoint
    from radnerf.ema import ParamEma
    from radnerf.scene import SyntheticScene, default_opt
    opt = default_opt(torso=False)
    a = SyntheticScene(H=8, W=8, n_frames=8, device="cpu", opt=opt, seed=0).model
    ea = ParamEma(a.parameters(), 0.95, 1000)
    with torch.no_grad():
        a.sigma_net.net[0].weight.add_(0.25)
    ea.update()
    with_ema = save_checkpoint(a, os.path.join(tmp_path, "with.pth"), ema=ea, epoch=1, global_step=1000, stats={})
    without = save_checkpoint(a, os.path.join(tmp_path, "without.pth"))
    raw = torch.load(with_ema, weights_only=False)
    assert list(raw["ema"]) == ["decay", "num_updates", "shadow_params", "collected_params"]
    assert len(raw["ema"]["shadow_params"]) == len(list(a.parameters()))                 # model.parameters() order
    assert "ema" not in torch.load(without, weights_only=False)

    b = SyntheticScene(H=8, W=8, n_frames=8, device="cpu", opt=opt, seed=7).model
    eb = ParamEma(b.parameters(), 0.95, 1000)
    load_checkpoint(b, with_ema, ema=eb)
    assert eb.num_updates == 1
    assert all(torch.equal(s, t) for s, t in zip(eb.shadow_params, ea.shadow_params))
    i = [k for k, p in enumerate(b.parameters()) if p is b.sigma_net.net[0].weight][0]
    assert not torch.equal(eb.shadow_params[i], b.sigma_net.net[0].weight.detach())       # the average lags the weight

    c = SyntheticScene(H=8, W=8, n_frames=8, device="cpu", opt=opt, seed=9).model
    ec = ParamEma(c.parameters(), 0.95, 1000)
    ec.update()
    load_checkpoint(c, without, ema=ec)                                                    # no entry: shadows = the loaded weights
    assert ec.num_updates == 0
    assert all(torch.equal(s, p.detach()) for s, p in zip(ec.shadow_params, c.parameters()))
    load_checkpoint(c, with_ema)                                                           # a caller without an EMA is not disturbed


class _Stub(torch.nn.Module):
    """A model of one weight whose render scales fixed outputs (tests/test_train_host.py's stand-in)."""
    mean_count = 0

    def __init__(self, out):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(1))
        self.out = out

    def render(self, *a, **kw):
        return {k: v * self.w for k, v in self.out.items()}

    def get_params(self, lr, lr_net, wd=0):
        return [{"params": [self.w], "lr": lr_net}]


def test_trainer_updates_on_its_cadence_and_decays_the_rate_on_a_cpu_model():
    """Trainer(ema_decay=0.95, ema_update_interval=2) on a CPU model: the average moves on steps 2 and 4 only; with lr_gamma the
    optimizer's rate after step s is lr0 * gamma ** (s / iters), LambdaLR's."""
    from radnerf.train import Trainer
    N = 16
    g = torch.Generator().manual_seed(0)
    out = dict(image=torch.rand(1, N, 3, generator=g), weights_sum=torch.rand(N, generator=g), ambient=torch.rand(N, generator=g))
    data = dict(rays_o=None, rays_d=None, auds=None, bg_coords=None, poses=None, eye=None, index=[0], bg_color=None,
                images=torch.rand(1, N, 3, generator=g), face_mask=torch.rand(1, N, generator=g) > 0.5)
    opt = types.SimpleNamespace(torso=False, dt_gamma=1 / 256, max_steps=16)
    m = _Stub(out)
    tr = Trainer(m, opt, lr_net=1e-2, update_extra_interval=0, iters=10, ema_decay=0.95, ema_update_interval=2, lr_gamma=0.1)
    assert isinstance(tr.optimizer, torch.optim.Adam) and tr.ema.num_updates == 0
    moved, shadow = [], tr.ema.shadow_params[0].clone()
    for s in range(1, 6):
        tr.step(data)
        moved.append(not torch.equal(tr.ema.shadow_params[0], shadow))
        shadow = tr.ema.shadow_params[0].clone()
        assert np.isclose(tr.optimizer.param_groups[0]["lr"], 1e-2 * 0.1 ** (s / 10), rtol=1e-12)
    assert moved == [False, True, False, True, False] and tr.ema.num_updates == 2
    w = m.w.detach().clone()
    with tr.ema_scope():
        assert torch.equal(m.w.detach(), tr.ema.shadow_params[0]) and not torch.equal(m.w.detach(), w)
    assert torch.equal(m.w.detach(), w)
    try:
        with tr.ema_scope():
            raise KeyError("inside")
    except KeyError:
        pass
    assert torch.equal(m.w.detach(), w)                                                   # restored on an exception too
    plain = Trainer(_Stub(out), opt, update_extra_interval=0)
    assert plain.ema is None and plain.lr_gamma is None
    with plain.ema_scope():
        pass
