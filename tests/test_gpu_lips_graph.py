"""GraphedTrainer(lips_graphs=G): lip fine-tuning steps (DeviceTrainSet.batch_rect / batch_patch with PerceptualAlex as the patch
criterion) captured at their first occurrence and replayed from one graph per shape, against the eager Trainer.

Every run builds everything afresh from the same seeds, as tests/test_gpu_train_deterministic.py::_run does (the rocBLAS selection
before the scene included): the 64 x 64 scene, an 8-frame set with +-40 / 255 seeded noise on every frame (so that the perceptual
term is a visible part of each rect step, tests/test_gpu_percep_step.py), the seeded weights of tests/percepref64.py.  A run takes
three first-window steps on plain batches, sets model.mean_count and runs its schedule.

With RN_TRAIN_DETERMINISTIC=1 no float atomic runs in a step, the perceptual kernels have none, and the head step's bits do not
depend on the row capacity (test_a_graph_captured_before_the_workspace_grew_still_replays): a captured run equals the eager one
in every per-step loss, every parameter and every Adam moment, bit for bit.  `.grad` is left out, for the reason given there.

Rects on the 64 x 64 image -- the smallest shapes at which the key, the marcher's last workgroup and the perceptual plan can go
wrong:
    A   (16,48,12,52)  32 x 40   1 280 rays = 5 full 256-ray workgroups
    A2  ( 8,40,20,60)  32 x 40   A's shape elsewhere, on another frame
    T   (12,52,16,48)  40 x 32   the same 1 280 rays, other views
    S   (20,51,10,41)  31 x 31   MIN_SIDE; 961 rays: a partial wave and a partial workgroup"""
import os
import random

import numpy as np
import pytest
import torch

import percepref64 as R

pytestmark = pytest.mark.gpu

A, A2, T, S = (16, 48, 12, 52), (8, 40, 20, 60), (12, 52, 16, 48), (20, 51, 10, 41)
LOSS_RTOL = 2e-4                                          # tests/test_gpu_percep_step.py's


def _set_environment(monkeypatch, deterministic=True):
    for name in [n for n in os.environ if n.startswith("RN_")]:
        monkeypatch.delenv(name)
    monkeypatch.setenv("RN_TRAIN_NOISE", "torch")            # the seeded jitter, as conftest pins it for every test
    if deterministic:
        monkeypatch.setenv("RN_TRAIN_DETERMINISTIC", "1")


def _mean_abs(pred, target):
    """A criterion that is a plain Python function of torch operators."""
    return (pred - target).abs().mean(dim=(1, 2, 3), keepdim=True)


def _alternation(rects):
    """Test 1's schedule: a rect on even steps over `rects`, random pixels on odd ones, the frame changing every step."""
    return [("rect", s % 8, rects[s // 2]) if s % 2 == 0 else ("plain", s % 8, None) for s in range(2 * len(rects))]


def _run(graphed, phases, criterion="alex", num_rays=1024, perturb_color=False, probe=False, **trainer_kw):
    """phases: [(mean_count, [(kind, frame, rect | patch_size | pixel indices of a plain batch | None), ...]), ...] after three
    first-window steps on plain batches.
    -> (bits: {name: uint32 array} of the per-step losses, the parameters and the Adam moments; losses; trainer; probe MSEs)."""
    from radnerf.dataset import DeviceTrainSet
    from radnerf.percep import PerceptualAlex
    from radnerf.scene import SyntheticScene, default_opt
    from radnerf.train import GraphedTrainer, Trainer, train_step
    torch.backends.cuda.preferred_blas_library("cublas")        # before the scene: see tests/test_gpu_train_deterministic.py::_run
    torch.manual_seed(0)
    random.seed(0)
    np.random.seed(0)
    scene = SyntheticScene(H=64, W=64, n_frames=8, device="cuda", opt=default_opt(engine="ops", torso=False, smooth_lips=False))
    ds = DeviceTrainSet.from_scene(scene, 8, num_rays=num_rays, seed=3)
    g = torch.Generator(device="cuda").manual_seed(21)
    noise = torch.randint(-40, 41, ds.images.shape, generator=g, device="cuda")
    ds.images.copy_((ds.images.int() + noise).clamp(0, 255).to(torch.uint8))
    m = ds.install(scene.model)
    if criterion == "alex":
        criterion = PerceptualAlex(*R.seeded_weights()[:3]).cuda()
    if perturb_color:
        with torch.no_grad():
            m.color_net.net[-1].weight.add_(0.5 * torch.randn_like(m.color_net.net[-1].weight))
    trainer = (GraphedTrainer if graphed else Trainer)(m, scene.opt, update_extra_interval=0, patch_criterion=criterion, **trainer_kw)
    held = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in ds.batch([5], inds=torch.arange(0, 4096, 3)).items()
            if not k.startswith("_")} if probe else None

    def mse():
        m.train()
        with torch.no_grad():
            pred, rgb, _ = train_step(m, held, scene.opt)
        return float(((pred - rgb) ** 2).mean())

    def batch(kind, frame, arg):
        if kind == "rect":
            return ds.batch_rect([frame], rect=arg)
        if kind == "patch":
            return ds.batch_patch([frame], arg)
        return ds.batch([frame]) if arg is None else ds.batch([frame], inds=arg)       # a plain batch: its own draw, or the pixels `arg`

    probes = [mse()] if probe else []
    losses = [trainer.step(ds.batch([i])).clone() for i in range(3)]
    for mean_count, schedule in phases:
        m.mean_count = mean_count
        for kind, frame, arg in schedule:
            losses.append(trainer.step(batch(kind, frame, arg)).clone())
    torch.cuda.synchronize()
    ds.check()
    if probe:
        probes.append(mse())
    out = {"loss": torch.stack([v.reshape(()) for v in losses])}
    for pname, p in m.named_parameters():
        out["param." + pname] = p.detach()
        st = trainer.optimizer.state.get(p, {})
        for key in ("exp_avg", "exp_avg_sq"):
            if key in st:
                out[key + "." + pname] = st[key]
    bits = {k: v.detach().float().cpu().numpy().reshape(-1).view(np.uint32).copy() for k, v in out.items()}
    return bits, [float(v) for v in losses], trainer, probes


def _first_difference(a, b):
    assert list(a) == list(b)
    for k in a:
        if not np.array_equal(a[k], b[k]):
            return k, int((a[k] != b[k]).sum()), a[k].size
    return None


def _same_bits(what, eager, graphed):
    diff = _first_difference(eager, graphed)
    print(f"{what}: eager against captured, first difference: {diff}")
    assert len(eager) > 100 and any(eager[k].any() for k in eager if k.startswith("exp_avg.")) and diff is None


def test_rect_schedule_equals_the_eager_trainer_bit_for_bit(hiplib, monkeypatch):
    """Twelve steps, shapes A, T, A2, S, A, T: with 4 slots the graphs of plain, A, T, S; with 2 slots the least-recently-used
    order evicts T for S, then S for T.  A2 -- A's shape elsewhere, on another frame -- replays A's graph in both."""
    _set_environment(monkeypatch)
    phases = [(12000, _alternation([A, T, A2, S, A, T]))]
    eager, eager_losses, _, _ = _run(False, phases)
    assert np.isfinite(eager_losses).all()
    for slots, lips_captures in ((4, 3), (2, 4)):
        bits, _, tr, _ = _run(True, phases, lips_graphs=slots)
        print(f"lips_graphs = {slots}: capture_log {tr.capture_log}, lips_capture_log {tr.lips_capture_log}")
        _same_bits(f"lips_graphs = {slots}", eager, bits)
        assert tr.replays == 12 and tr.captures == 1 + lips_captures and tr.lips_captures == lips_captures
        assert len(tr.capture_log) == 1 and len(tr.capture_log[0]) == 3 and tr.capture_log[0][1:] == (12032, 16384)
        assert [(e[3], e[4]) for e in tr.lips_capture_log] == [("rect", (32, 40)), ("rect", (40, 32)), ("rect", (31, 31))] + (
            [("rect", (40, 32))] if slots == 2 else [])
        assert all(e[1:3] == (12032, 16384) for e in tr.lips_capture_log)
        assert len(tr._lips.graphs) == min(slots, 3) and len(tr._lips.inputs) == len(tr._lips.graphs)


def test_a_budget_that_leaves_and_comes_back(hiplib, monkeypatch):
    """Capacities 16 384, 20 480 and 16 384 again by step()'s own rule: two plain and two lips captures, none in the third
    phase -- both caches still hold the first capacity's graphs, and the two A graphs share one set of static inputs."""
    _set_environment(monkeypatch)
    schedule = [("rect", 0, A), ("plain", 1, None), ("rect", 2, A), ("plain", 3, None)]
    phases = [(count, schedule) for count in (12000, 17000, 12000)]
    eager, _, _, _ = _run(False, phases)
    bits, _, tr, _ = _run(True, phases, lips_graphs=4)
    print(f"capture_log {tr.capture_log}, lips_capture_log {tr.lips_capture_log}")
    _same_bits("three budgets", eager, bits)
    assert [c for _, _, c in tr.capture_log] == [16384, 20480] and [e[2] for e in tr.lips_capture_log] == [16384, 20480]
    assert tr.captures == 4 and tr.lips_captures == 2 and tr.replays == 12
    assert max(e[0] for e in tr.capture_log + tr.lips_capture_log) <= 3 + 8          # the third phase (steps 12 ...) captured nothing
    assert len(tr._lips.graphs) == 2 and len(tr._lips.inputs) == 1


def test_plain_batches_of_two_ray_counts_equal_the_eager_trainer_bit_for_bit(hiplib, monkeypatch):
    """Plain batches of 1 024 rays (the set's own draw) and of 512 rays (every 8th pixel) alternate for eight steps: two keys and
    two ray layouts, each with static inputs of its own -- one capture each, then replays.  Before the plain graphs kept their
    static inputs per layout, the second ray count was captured over the first one's and its feed raised."""
    _set_environment(monkeypatch)
    every_8th = torch.arange(0, 4096, 8)
    phases = [(12000, [("plain", s, None if s % 2 == 0 else every_8th) for s in range(8)])]
    eager, eager_losses, _, _ = _run(False, phases)
    assert np.isfinite(eager_losses).all()
    bits, _, tr, _ = _run(True, phases)
    print(f"capture_log {tr.capture_log}")
    _same_bits("two ray counts", eager, bits)
    assert tr.captures == 2 and tr.replays == 8
    assert [e[1:] for e in tr.capture_log] == [(12032, 16384)] * 2 and tr.lips_captures == 0
    assert list(tr._plain.inputs) == [("plain", (1, 1024, 3)), ("plain", (1, 512, 3))]


def test_patch_steps_equal_the_eager_trainer_bit_for_bit(hiplib, monkeypatch):
    """Two 32 x 32 patches of 2 048 rays beside plain batches of 2 048 rays -- the same rays shape [1,2048,3], two keys.  The
    captured patch step marches under a device budget of n * max_steps rows where the eager one reads its sample count back."""
    _set_environment(monkeypatch)
    kinds = ["patch", "plain", "patch", "patch", "plain", "patch"]
    phases = [(24000, [(k, i, 32 if k == "patch" else None) for i, k in enumerate(kinds)])]
    eager, _, _, _ = _run(False, phases, num_rays=2048)
    bits, _, tr, _ = _run(True, phases, num_rays=2048, lips_graphs=2)
    print(f"capture_log {tr.capture_log}, lips_capture_log {tr.lips_capture_log}")
    _same_bits("patch steps", eager, bits)
    assert tr.captures == 2 and tr.lips_captures == 1 and len(tr.capture_log) == 1 and tr.replays == 6
    rows = 2048 * 16 + 128                                    # n * max_steps, aligned as the running budget is
    assert [e[1:] for e in tr.lips_capture_log] == [(rows, rows, "patch", (2, 32, 32))]


@pytest.mark.parametrize("perturb", [False, True])
def test_a_budget_of_every_row_marches_what_force_all_rays_marches(hiplib, perturb):
    """What the captured patch step rests on: the budgeted marchers under a budget of N * max_steps rows against
    march_rays_train(force_all_rays=True) -- identical counters, rays and sample rows up to the count."""
    import raymarching
    from raymarching import ops
    from radnerf.scene import SyntheticScene, default_opt
    torch.manual_seed(0)
    scene = SyntheticScene(H=64, W=64, n_frames=8, device="cuda", opt=default_opt(engine="ops", torso=False, smooth_lips=False))
    m, f = scene.model, scene.frame(0)
    o, d = f["rays_o"].reshape(-1, 3).contiguous(), f["rays_d"].reshape(-1, 3).contiguous()
    N, max_steps = o.shape[0], scene.opt.max_steps
    nears, fars = raymarching.near_far_from_aabb(o, d, m.aabb_train, m.min_near)
    args = (o, d, m.bound, m.density_bitfield, m.cascade, m.grid_size, nears, fars)
    zeros = lambda: torch.zeros(2, dtype=torch.int32, device="cuda")
    c0 = zeros()
    torch.manual_seed(9)
    x0, d0, dl0, r0 = raymarching.march_rays_train(*args, c0, -1, perturb, 128, True, scene.opt.dt_gamma, max_steps)
    total = int(c0[0].item())
    assert 0 < total <= x0.shape[0] < N * max_steps and int(c0[1].item()) == N
    rows = N * max_steps + 128 - (N * max_steps) % 128
    bt = torch.tensor([rows], dtype=torch.int32, device="cuda")
    got = {}
    c1 = zeros()
    torch.manual_seed(9)                                        # the same jitter draw
    got["budget"] = (c1,) + tuple(ops.march_rays_train_budget(*args, c1, bt, rows, perturb, scene.opt.dt_gamma, max_steps))
    if ops.step_marcher_supported(N, o.device):
        c2 = torch.full((2,), 12345, dtype=torch.int32, device="cuda")      # SET by the launch
        torch.manual_seed(9)
        got["step"] = (c2,) + tuple(ops.march_rays_train_step(o, d, m.aabb_train, m.min_near, m.bound, m.density_bitfield, m.cascade,
                                                               m.grid_size, c2, bt, rows, perturb, scene.opt.dt_gamma, max_steps, True))[2:]
    assert (N + 255) // 256 > 4 and "step" in got               # several workgroups, and the one-launch marcher is exercised
    for name, (c, x, dd, dl, r) in got.items():
        assert x.shape[0] == rows, name
        assert torch.equal(c, c0) and torch.equal(r, r0), name
        assert torch.equal(x[:total], x0[:total]) and torch.equal(dd[:total], d0[:total]) and torch.equal(dl[:total], dl0[:total]), name


def test_default_switches_train_through_the_lips_graphs(hiplib, monkeypatch):
    """Without RN_TRAIN_DETERMINISTIC: the atomic scatter on its side stream, joined in HipAdam.  The colour net's last layer is
    perturbed (test_graphed_trainer_replays_the_step_and_learns) and 24 steps of the rect / pixel alternation bring the probe's
    MSE down.  Two eager runs differ in their last bits here, so the eager curve is printed beside the captured one, not required."""
    _set_environment(monkeypatch, deterministic=False)
    phases = [(12000, _alternation([A, T, A2, S, A, T] * 2))]
    _, losses, tr, (before, after) = _run(True, phases, perturb_color=True, probe=True, lr_net=5e-3, lips_graphs=4)
    _, eager_losses, _, eager_probes = _run(False, phases, perturb_color=True, probe=True, lr_net=5e-3)
    print("captured", " ".join(f"{v:.5f}" for v in losses), f"probe MSE {before:.5f} -> {after:.5f}")
    print("eager   ", " ".join(f"{v:.5f}" for v in eager_losses), "probe MSE %.5f -> %.5f" % tuple(eager_probes))
    assert np.isfinite(losses).all() and after < before, (before, after)
    assert tr.replays == 24 and tr.captures == 4 and tr.lips_captures == 3


def test_a_rect_batch_without_a_criterion_is_captured_as_a_plain_step(hiplib, monkeypatch):
    _set_environment(monkeypatch)
    phases = [(12000, [("rect", 0, A), ("plain", 1, None), ("rect", 2, A2), ("rect", 3, T)])]
    eager, _, _, _ = _run(False, phases, criterion=None)
    bits, _, tr, _ = _run(True, phases, criterion=None, lips_graphs=4)
    _same_bits("no criterion", eager, bits)
    assert tr.replays == 4 and tr.captures == 3 and tr.lips_captures == 2 and len(tr.capture_log) == 1


def test_a_criterion_of_torch_operators_is_captured(hiplib, monkeypatch):
    """A plain Python function of torch operators as the criterion: captured with the step, every loss at the loss bar of
    tests/test_gpu_percep_step.py against the eager trainer's."""
    _set_environment(monkeypatch)
    phases = [(12000, _alternation([A, T, S, A2]))]
    _, eager_losses, _, _ = _run(False, phases, criterion=_mean_abs)
    _, losses, tr, _ = _run(True, phases, criterion=_mean_abs, lips_graphs=4)
    _, bare_losses, _, _ = _run(False, phases, criterion=None)
    print("eager   ", " ".join(f"{v:.6f}" for v in eager_losses))
    print("captured", " ".join(f"{v:.6f}" for v in losses))
    assert tr.replays == 8 and tr.captures == 4
    assert np.allclose(losses, eager_losses, rtol=LOSS_RTOL, atol=0)
    assert eager_losses[3] > bare_losses[3] * (1 + 10 * LOSS_RTOL)          # the term is a visible part of a rect step's loss
