"""The reference's training schedule on the device (main.py:204-224): rn_adam_step_sched (LambdaLR rates and the EMA of the weights
inside the Adam launches), rn_param_swap, rn_image_error, and what radnerf/train.py builds on them -- HipAdam(schedule=, ema=),
Trainer.ema_scope / evaluate, GraphedTrainer with a captured step that carries all of it.  Shapes are chosen for the kernels' edges
(one element, the float4 boundary, the 1024-element workgroup, misaligned views, more than 48 tensors), not for the workload."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BETAS, EPS = (0.9, 0.99), 1e-15


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _tensors(seed, scale=1.0):
    """1, 3, 1023, 1025, 4101 elements, [64, 96], the 4-byte-aligned view buf[1:] of a 4100-element buffer, and 43 small tensors of
    2 .. 44 elements: 50 in all, two launches of 48 and 2."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g) * scale
    out = [r(1), r(3), r(1023), r(1025), r(4101), r(64, 96), r(4100)[1:]]
    out += [r(k) for k in range(2, 45)]
    assert len(out) == 50 and out[6].data_ptr() % 16 == 4
    return out


def _like(ts):
    """Copies with the same values AND the same alignment as `ts` (a view at +4 bytes stays one)."""
    out = []
    for t in ts:
        off = (t.data_ptr() % 16) // 4
        buf = torch.empty(t.numel() + off, device="cuda")
        v = buf[off:].view(t.shape)
        v.copy_(t)
        out.append(v)
    return out


def _sched_call(hip, P, G, M, V, S, lr0, state, gamma, iters, decay, interval):
    arr = (hip.abi.SchedTensorT * len(P))()
    for i in range(len(P)):
        arr[i].param, arr[i].grad = P[i].data_ptr(), (None if G[i] is None else G[i].data_ptr())
        arr[i].exp_avg, arr[i].exp_avg_sq = M[i].data_ptr(), V[i].data_ptr()
        arr[i].shadow = None if S[i] is None else S[i].data_ptr()
        arr[i].numel, arr[i].lr0 = P[i].numel(), lr0[i]
    hip.call("rn_adam_step_sched", arr, len(P), BETAS[0], BETAS[1], EPS, gamma, iters, decay, interval, hip.ptr(state["step"]),
             hip.ptr(state["corr"]), hip.ptr(state["lr_dev"]), hip.ptr(state["num_updates"]), hip.stream())


def _lr_call(hip, P, G, M, V, state):
    arr = (hip.abi.AdamTensorT * len(P))()
    for i in range(len(P)):
        arr[i].param, arr[i].grad, arr[i].exp_avg, arr[i].exp_avg_sq = (t.data_ptr() for t in (P[i], G[i], M[i], V[i]))
        arr[i].numel, arr[i].lr = P[i].numel(), 0.0
    hip.call("rn_adam_step_lr", arr, len(P), BETAS[0], BETAS[1], EPS, hip.ptr(state["step"]), hip.ptr(state["corr"]),
             hip.ptr(state["lr_dev"]), hip.stream())


def _state(n, num_updates=0):
    return dict(step=torch.zeros(1, dtype=torch.int32, device="cuda"), corr=torch.zeros(4, device="cuda"),
                lr_dev=torch.zeros(n, device="cuda"), num_updates=torch.full((1,), num_updates, dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("start", [0, 200])
def test_sched_step_is_the_lr_step_plus_torch_emas_update_bit_for_bit(hiplib, start):
    """Seven steps, interval 2, decay 0.95, from num_updates = 0 (the warm-up branch of the decay) and from 200 (the constant one).
    Parameters and both moments: bit-equal to rn_adam_step_lr on clones given the rates the schedule wrote.  Shadows: bit-equal to
    torch_ema's three expressions run by torch on the device; untouched after odd steps.  The shadow of the 1025-element tensor is
    itself a 4-byte-aligned view (only the shadow forces the scalar path there)."""
    hip = hiplib
    P = _tensors(1)
    n = len(P)
    M, V = [torch.zeros_like(p) for p in P], [torch.zeros_like(p) for p in P]
    S = [p.clone() + 0.1 for p in P]
    S[3] = (torch.zeros(1026, device="cuda")[1:]).copy_(P[3] + 0.1)
    assert S[3].data_ptr() % 16 == 4
    P2, M2, V2, S2 = _like(P), _like(M), _like(V), [s.clone() for s in S]
    lr0 = [5e-3 if i % 2 else 5e-4 for i in range(n)]
    st, st2 = _state(n, start), _state(n)
    g = torch.Generator(device="cuda").manual_seed(2)
    updates = start
    for s in range(1, 8):
        G = [torch.randn(p.shape, device="cuda", generator=g) * 10.0 ** (s - 4) for p in P]
        before = [x.clone() for x in S]
        _sched_call(hip, P, G, M, V, S, lr0, st, 0.1, 7, 0.95, 2)
        st2["lr_dev"].copy_(st["lr_dev"])
        _lr_call(hip, P2, G, M2, V2, st2)
        if s % 2 == 0:
            updates += 1
            one_minus_decay = 1.0 - min(0.95, (1 + updates) / (10 + updates))
            for sh, p in zip(S2, P2):
                tmp = sh - p
                tmp.mul_(one_minus_decay)
                sh.sub_(tmp)
        torch.cuda.synchronize()
        for i in range(n):
            assert _same(P[i], P2[i]) and _same(M[i], M2[i]) and _same(V[i], V2[i]), (s, i)
            assert _same(S[i], S2[i]), (s, i, float((S[i] - S2[i]).abs().max()))
            assert (s % 2 == 0) != _same(S[i], before[i]), (s, i)
        assert int(st["num_updates"].item()) == updates and int(st["step"].item()) == s
    assert updates == start + 3
    assert (min(0.95, (1 + start + 1) / (10 + start + 1)) == 0.95) == (start == 200)      # which branch of the decay this case took


def test_an_entry_without_a_gradient_keeps_its_weights_and_averages_its_shadow(hiplib):
    hip = hiplib
    P = _tensors(3)[:8]
    n = len(P)
    M, V = [torch.full_like(p, 0.25) for p in P], [torch.full_like(p, 0.5) for p in P]
    S = [p.clone() - 0.2 for p in P]
    S[7] = None                                                  # no gradient and no shadow: nothing at all happens to it
    keep = [(p.clone(), m.clone(), v.clone()) for p, m, v in zip(P, M, V)]
    frozen = (1, 4, 6, 7)
    st = _state(n)
    g = torch.Generator(device="cuda").manual_seed(4)
    updates = 0
    S2 = [None if s is None else s.clone() for s in S]
    for s in range(1, 5):
        G = [None if i in frozen else torch.randn(p.shape, device="cuda", generator=g) for i, p in enumerate(P)]
        _sched_call(hip, P, G, M, V, S, [1e-3] * n, st, 1.0, 0, 0.95, 2)
        if s % 2 == 0:
            updates += 1
            omd = 1.0 - min(0.95, (1 + updates) / (10 + updates))
            for sh, p in zip(S2, P):
                if sh is not None:
                    tmp = sh - p
                    tmp.mul_(omd)
                    sh.sub_(tmp)
        for i in range(n):
            moved = not _same(P[i], keep[i][0])
            assert moved == (i not in frozen), (s, i)
            if i in frozen:
                assert _same(M[i], keep[i][1]) and _same(V[i], keep[i][2]), (s, i)
            if S[i] is not None:
                assert _same(S[i], S2[i]), (s, i)
    assert int(st["num_updates"].item()) == 2
    assert not _same(S[1], P[1] - 0.2) and float((S[1] - P[1]).abs().max()) < 0.2          # the frozen tensor's shadow closed in on it


def _groups(ps):
    return [{"params": ps[:3], "lr": 5e-3}, {"params": ps[3:], "lr": 5e-4}]


def test_schedule_follows_lambda_lr(hiplib):
    """HipAdam(schedule=(0.1, 5)): after each of 6 steps lr_dev is within 1 ulp of numpy.float32(lr0 * 0.1 ** ((s - 1) / 5)) (lr0 the
    fp32 rate the kernel is given); the parameters follow torch.optim.Adam + LambdaLR stepping eagerly within the project's Adam
    bar, 2e-6 relative (test_hip_adam_matches_torch_adam)."""
    from radnerf.train import HipAdam
    pa = [torch.nn.Parameter(t.clone()) for t in _tensors(5)[:7]]
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    oa = HipAdam(_groups(pa), betas=BETAS, eps=EPS, schedule=(0.1, 5))
    ob = torch.optim.Adam(_groups(pb), betas=BETAS, eps=EPS)
    sched = torch.optim.lr_scheduler.LambdaLR(ob, lambda it: 0.1 ** (it / 5))
    g = torch.Generator(device="cuda").manual_seed(6)
    for s in range(1, 7):
        for a, b in zip(pa, pb):
            gr = torch.randn(a.shape, device="cuda", generator=g)
            a.grad, b.grad = gr.clone(), gr.clone()
        oa.step()
        ob.step()
        sched.step()
        got = oa._lr_dev[:7].cpu().numpy()
        want = np.array([np.float32(float(np.float32(5e-3 if i < 3 else 5e-4)) * 0.1 ** ((s - 1) / 5)) for i in range(7)], dtype=np.float32)
        ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        assert ulps.max() <= 1, (s, got, want)
        # the host mirror: the rate of the NEXT step, what the reference's param_groups show after scheduler.step()
        np.testing.assert_allclose(oa.current_lr(), [gp["lr"] for gp in ob.param_groups], rtol=1e-12)
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert float((a.detach() - b.detach()).abs().max()) <= 2e-6 * float(b.detach().abs().max()) + 1e-30, i
    assert oa.uploads == 0
    sd = oa.state_dict()
    np.testing.assert_allclose([gp["lr"] for gp in sd["param_groups"]], [gp["lr"] for gp in ob.param_groups], rtol=1e-12)
    assert all(float(v["step"]) == 6 for v in sd["state"].values())
    with pytest.raises(ValueError):
        HipAdam(_groups(pa), schedule=(0.1, 0))


def test_a_captured_step_carries_schedule_and_ema(hiplib):
    """One graph holds HipAdam.step with the schedule and the EMA at interval 2; six replays with fresh gradients are bit-equal to
    six eager steps of a twin -- parameters, moments, shadows, counters -- and refresh_lr() copies nothing on this route."""
    from radnerf.ema import ParamEma
    from radnerf.train import HipAdam
    src = _tensors(7)[:9]

    def build():
        ps = [torch.nn.Parameter(t.clone()) for t in src]
        ema = ParamEma(ps, 0.95, update_interval=2)
        return ps, ema, HipAdam(_groups(ps), betas=BETAS, eps=EPS, schedule=(0.1, 6), ema=ema)
    pa, ea, oa = build()
    pb, eb, ob = build()
    static = [torch.zeros_like(p) for p in pa]
    for p, s in zip(pa, static):
        p.grad = s
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        oa.step()
    assert int(oa._step.item()) == 0 and all(_same(a, t) for a, t in zip(pa, src))       # capturing ran nothing
    g = torch.Generator(device="cuda").manual_seed(8)
    for s in range(1, 7):
        for st, b in zip(static, pb):
            gr = torch.randn(b.shape, device="cuda", generator=g)
            st.copy_(gr)
            b.grad = gr.clone()
        oa.refresh_lr()
        graph.replay()
        oa.note_replayed()
        ob.step()
        for a, b in zip(pa, pb):
            assert _same(a, b) and _same(oa.state[a]["exp_avg"], ob.state[b]["exp_avg"]), s
            assert _same(oa.state[a]["exp_avg_sq"], ob.state[b]["exp_avg_sq"]) and _same(ea.shadow_of(a), eb.shadow_of(b)), s
    assert int(oa._step.item()) == int(ob._step.item()) == 6 and ea.num_updates == eb.num_updates == 3
    assert oa.uploads == ob.uploads == 0 and oa._lr_sent is None
    assert oa.current_lr() == ob.current_lr()
    assert _same(oa._lr_dev, ob._lr_dev) and float(oa._lr_dev[0]) < 5e-3 * 0.17             # 0.1 ** (5 / 6) = 0.147
    assert not _same(ea.shadow_of(pa[0]), pa[0]) and not _same(ea.shadow_of(pa[0]), src[0])


def test_param_swap_exchanges_and_restores(hiplib):
    hip = hiplib
    A = _tensors(9)
    B = [torch.randn_like(a) for a in A]
    B[3] = (torch.zeros(1026, device="cuda")[1:]).copy_(torch.randn(1025, device="cuda"))  # only b misaligned
    a0, b0 = [t.clone() for t in A], [t.clone() for t in B]
    n = len(A)
    pa, pb = (C.c_void_p * n)(*[t.data_ptr() for t in A]), (C.c_void_p * n)(*[t.data_ptr() for t in B])
    numel = (C.c_uint32 * n)(*[t.numel() for t in A])
    guard = A[6]._base if A[6]._base is not None else None                                 # buf[0] of the misaligned view
    g0 = guard[0].clone() if guard is not None else None
    hip.call("rn_param_swap", pa, pb, numel, n, hip.stream())
    for i in range(n):
        assert _same(A[i], b0[i]) and _same(B[i], a0[i]), i
    if guard is not None:
        assert _same(guard[0], g0)
    hip.call("rn_param_swap", pa, pb, numel, n, hip.stream())
    for i in range(n):
        assert _same(A[i], a0[i]) and _same(B[i], b0[i]), i


def test_ema_scope_swaps_the_weights_under_the_fused_engine(hiplib):
    """Under ema_scope() a 64 x 64 frame of the fused engine is the frame of a second model loaded with the shadow weights, bit for
    bit; afterwards the original frame comes back bit for bit -- the version bump reached FusedState both times."""
    from radnerf.scene import SyntheticScene, default_opt
    from radnerf.train import HipAdam, Trainer
    opt = lambda: default_opt(engine="fused", torso=False, smooth_lips=False)
    scene = SyntheticScene(H=64, W=64, n_frames=8, device="cuda", opt=opt(), seed=0)
    m = scene.model
    tr = Trainer(m, scene.opt, update_extra_interval=0, ema_decay=0.95, ema_update_interval=4)
    assert isinstance(tr.optimizer, HipAdam) and tr.ema.device_num_updates is not None
    g = torch.Generator(device="cuda").manual_seed(10)
    with torch.no_grad():
        for p, s in tr.ema.pairs():
            s.add_(0.02 * torch.randn(s.shape, device="cuda", generator=g) * s.abs().mean())
    m.eval()
    with torch.no_grad():
        frame = scene.render(0)["image"].clone()
    other = SyntheticScene(H=64, W=64, n_frames=8, device="cuda", opt=opt(), seed=0)
    other.model.load_state_dict(m.state_dict())
    shadows = tr.ema.state_dict()["shadow_params"]
    with torch.no_grad():
        for p, s in zip(other.model.parameters(), shadows):
            p.copy_(s)
        want = other.render(0)["image"].clone()
    assert not _same(want, frame)
    weights = [p.detach().clone() for p in m.parameters()]
    with torch.no_grad(), tr.ema_scope():
        got = scene.render(0)["image"].clone()
        assert all(_same(p, s) for p, s in zip(m.parameters(), shadows))
    assert _same(got, want)
    assert all(_same(p, w) for p, w in zip(m.parameters(), weights))
    with torch.no_grad():
        assert _same(scene.render(0)["image"], frame)
    with pytest.raises(KeyError):
        with tr.ema_scope():
            raise KeyError("inside")
    assert all(_same(p, w) for p, w in zip(m.parameters(), weights))                       # swapped back on an exception too


@pytest.mark.parametrize("H,W", [(5, 7), (33, 65), (64, 64)])
def test_image_error_sums(hiplib, H, W):
    """rect null, empty, full-frame, and touching two edges (the last row and the first column).  Sums within 1e-9 relative of a
    float64 restatement (reordering a double sum of <= 10^6 terms: N 2^-53 ~ 1e-10), counts exact, two calls the same bits."""
    hip = hiplib
    g = torch.Generator(device="cuda").manual_seed(H * 100 + W)
    pred = torch.rand(H * W, 3, device="cuda", generator=g)
    target = torch.rand(H * W, 3, device="cuda", generator=g)
    ws = torch.empty(int(hip._lib.rn_image_error_workspace(H, W)), dtype=torch.uint8, device="cuda")
    d = (pred - target).double().cpu().numpy().reshape(H, W, 3)                            # the difference in fp32, as the kernel takes it
    rects = {"null": None, "empty": (2, 2, 0, W), "full": (0, H, 0, W), "edges": (H - 2, H, 0, 3), "beyond": (-3, H + 5, 1, W + 9)}
    for name, rect in rects.items():
        r = None if rect is None else torch.tensor(rect, dtype=torch.int32, device="cuda")
        outs = []
        for _ in range(2):
            out = torch.full((4,), -1.0, dtype=torch.float64, device="cuda")
            hip.call("rn_image_error", hip.ptr(pred), hip.ptr(target), H, W, hip.ptr(r), hip.ptr(ws), hip.ptr(out), hip.stream())
            outs.append(out)
        assert torch.equal(outs[0].view(torch.int64), outs[1].view(torch.int64)), name
        got = outs[0].cpu().numpy()
        inside = d[0:0] if rect is None else d[max(rect[0], 0):max(rect[1], 0), max(rect[2], 0):max(rect[3], 0)]
        want = [float((d ** 2).sum()), float((inside ** 2).sum()), d.size, inside.size]
        assert got[2] == want[2] and got[3] == want[3], (name, got, want)
        assert abs(got[0] - want[0]) <= 1e-9 * want[0], (name, got, want)
        assert abs(got[1] - want[1]) <= 1e-9 * want[1], (name, got, want)
    assert rects["edges"][1] == H and rects["edges"][2] == 0


@pytest.mark.parametrize("engine", ["ops", "fused"])
def test_evaluate_reports_psnr_meters_numbers(hiplib, engine):
    """Trainer.evaluate over three frames of a 64 x 64 DeviceTrainSet (from_scene builds at least 8 frames) under the averaged
    weights: psnr within 1e-4 dB of PSNRMeter's formula in numpy on frames rendered one by one under the same weights, loss within
    1e-6 relative; weights and training mode afterwards are what they were, bit for bit."""
    from radnerf.dataset import DeviceTrainSet
    from radnerf.scene import SyntheticScene, default_opt
    from radnerf.train import Trainer
    scene = SyntheticScene(H=64, W=64, n_frames=8, device="cuda", opt=default_opt(engine=engine, torso=False, smooth_lips=False))
    ds = DeviceTrainSet.from_scene(scene, 8, num_rays=1024)
    m = ds.install(scene.model)
    tr = Trainer(m, scene.opt, update_extra_interval=0, ema_decay=0.95, ema_update_interval=2)
    g = torch.Generator(device="cuda").manual_seed(12)
    with torch.no_grad():
        for p, s in tr.ema.pairs():
            s.add_(0.05 * torch.randn(s.shape, device="cuda", generator=g) * s.abs().mean())
    m.train()
    weights = [p.detach().clone() for p in m.parameters()]
    indices = [0, 3, 6]
    res = tr.evaluate(ds, indices, rect="face")
    assert m.training and all(_same(p, w) for p, w in zip(m.parameters(), weights))
    # the restatement: the shadows copied in by torch, every frame rendered, read back and measured on the host
    m.eval()
    psnrs, mses, rect_psnrs = [], [], []
    with torch.no_grad():
        for p, s in tr.ema.pairs():
            p.copy_(s)
        for i in indices:
            f = ds.frame(i)
            out = m.render(f["rays_o"], f["rays_d"], f["auds"], f["bg_coords"], f["poses"], eye=f["eye"], index=f["index"], staged=True,
                           bg_color=f["bg_color"], perturb=False, dt_gamma=scene.opt.dt_gamma, max_steps=scene.opt.max_steps)
            preds = out["image"].reshape(1, 64, 64, 3).cpu().numpy()
            truths = f["images"].cpu().numpy()
            psnrs.append(-10 * np.log10(np.mean((preds - truths) ** 2)))
            mses.append(np.mean((preds.astype(np.float64) - truths) ** 2))
            x0, x1, y0, y1 = ds._rect_host[f["index"][0]]
            rect_psnrs.append(-10 * np.log10(np.mean((preds[:, x0:x1, y0:y1].astype(np.float64) - truths[:, x0:x1, y0:y1]) ** 2)))
    print("evaluate", res["psnr"], float(np.mean(psnrs)), res["loss"], float(np.mean(mses)), res["rect_psnr"], float(np.mean(rect_psnrs)))
    assert abs(res["psnr"] - float(np.mean(psnrs))) <= 1e-4
    assert abs(res["loss"] - float(np.mean(mses))) <= 1e-6 * float(np.mean(mses))
    assert abs(res["rect_psnr"] - float(np.mean(rect_psnrs))) <= 1e-4
    assert len(res["per_frame"]) == 3 and 5.0 < res["psnr"] < 80.0
    plain = Trainer(m, scene.opt, update_extra_interval=0)                                  # no EMA: the weights as they are
    assert plain.evaluate(ds, [0])["rect_psnr"] is None


def test_graphed_trainer_with_schedule_and_ema_follows_the_eager_trainer(hiplib, monkeypatch):
    """Twelve steps of GraphedTrainer(ema_decay=0.95, ema_update_interval=4, lr_gamma=0.1, iters=12) against the eager Trainer with
    the same arguments on the 64 x 64 scene: loss curves within 1e-2 relative (the bar of
    test_graphed_trainer_follows_a_learning_rate_schedule), three EMA updates on both, one capture.

    The table gradients are summed in a fixed order here (RN_TRAIN_DETERMINISTIC=1).  With the atomic scatter this run measures
    the scatter, not the schedule: iters = 12 ramps the ambient term to full weight within the run, and two EAGER runs of it with
    the same seeds already differ by 1.1e-1 in their loss curves (lr_net 5e-3; graph against eager 1.2e-2 and 1.1e-1 against the
    two), above the bar whatever the trainer.  With ordered sums eager and graph agree bit for bit, so any gap is the schedule's."""
    monkeypatch.setenv("RN_TRAIN_DETERMINISTIC", "1")
    from radnerf.train import GraphedTrainer, HipAdam, SyntheticTrainStream, Trainer
    from radnerf.scene import SyntheticScene, default_opt
    curves, shadows = {}, {}
    for kind in ("eager", "graph"):
        torch.manual_seed(21)
        scene = SyntheticScene(H=64, W=64, n_frames=8, device="cuda", opt=default_opt(engine="ops", torso=False, smooth_lips=False))
        stream = SyntheticTrainStream(scene, n_rays=2048, seed=4)
        m = scene.model
        with torch.no_grad():
            m.color_net.net[-1].weight.add_(0.5 * torch.randn_like(m.color_net.net[-1].weight))
        trainer = (Trainer if kind == "eager" else GraphedTrainer)(m, scene.opt, lr_net=5e-3, update_extra_interval=0, iters=12,
                                                                    ema_decay=0.95, ema_update_interval=4, lr_gamma=0.1)
        assert isinstance(trainer.optimizer, HipAdam)
        losses = []
        for i in range(12):
            if i == 3:
                m.mean_count = 40000
                torch.manual_seed(22)
            losses.append(float(trainer.step(stream.batch())))
        curves[kind] = np.array(losses)
        assert trainer.ema.num_updates == 3 and int(trainer.optimizer._step.item()) == 12
        assert trainer.optimizer.uploads == 0
        np.testing.assert_allclose(trainer.optimizer.current_lr()[0], trainer.optimizer.param_groups[0]["initial_lr"] * 0.1, rtol=1e-12)
        w = m.color_net.net[-1].weight
        shadows[kind] = trainer.ema.shadow_of(w).clone()
        assert not _same(shadows[kind], w)
        if kind == "graph":
            assert trainer.captures == 1 and trainer.replays == 9
    print("schedule + ema curves", {k: v.tolist() for k, v in curves.items()})
    np.testing.assert_allclose(curves["graph"], curves["eager"], rtol=1e-2, atol=1e-7)
