"""GPU parity of every marcher on every branch of the walk (csrc/rn_dda_dev.h: Dda::walk) -- the ray families of tests/walk_cases.py:
rays on both sides of the 0.58 seam of `one_step_skips`, rays the shortcut would get wrong, a clamp with interior dt values, two and
three cascades, H != 128, NaN / FLT_MAX ends.  tests/test_walk_cases.py shows on the CPU that each family reaches its branch.

Bar: bit equality with the CPU oracle (np.array_equal; NaNs compared by position) for samples, rays, counters, nears and fars.  The
whole-frame and training-step tests at the end reuse the bars of the tests they are modelled on; no tolerance is new.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import walk_cases as wc

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -12345.0


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def n(x):
    return x.detach().cpu().numpy()


def same(got, want):
    """Bit equality as the suite states it: np.array_equal with NaNs compared by position."""
    got = n(got) if torch.is_tensor(got) else got
    return got.shape == want.shape and np.array_equal(got, want, equal_nan=True)


def _pad128(m):
    return m + 128 - m % 128


class _Dev:
    """A family's inputs on the device, kept referenced for the test's duration."""

    def __init__(self, case, w):
        self.o, self.d, self.bits, self.aabb = t(case.o), t(case.d), t(case.bits), t(case.aabb)
        self.nears, self.fars = t(w["nears"]), t(w["fars"])


def _zero_samples(M):
    return torch.zeros(M, 3, device=DEV), torch.zeros(M, 3, device=DEV), torch.zeros(M, 2, device=DEV)


def _uniform(case, seed):
    """The jitter of a launch.  The needles are needles on the lattice of t that starts AT near (that is how they were found): a
    jittered start moves the lattice and they become ordinary short rays, so that family always walks without jitter."""
    if case.name == "needles":
        return np.zeros(case.N, np.float32)
    return np.random.default_rng(seed).uniform(0, 1, case.N).astype(np.float32)


def _train_march(hip, case, g, M, noises, budget=None):
    """rn_march_rays_train (budget None) / rn_march_rays_train_budget on zeroed buffers and counters."""
    x, d, dl = _zero_samples(M)
    rays = torch.full((case.N, 3), -7, dtype=torch.int32, device=DEV)
    counter = torch.zeros(2, dtype=torch.int32, device=DEV)
    ws = torch.zeros(hip.workspace_bytes("rn_march_rays_train_workspace", case.N), dtype=torch.uint8, device=DEV)
    nz = t(noises)
    bound, dt_gamma, max_steps, Cc, H = case.march_args
    head = (hip.ptr(g.o), hip.ptr(g.d), hip.ptr(g.bits), bound, dt_gamma, max_steps, case.N, Cc, H, M)
    tail = (hip.ptr(g.nears), hip.ptr(g.fars), hip.ptr(x), hip.ptr(d), hip.ptr(dl), hip.ptr(rays), hip.ptr(counter), hip.ptr(nz),
            hip.ptr(ws), hip.stream())
    if budget is None:
        hip.call("rn_march_rays_train", *head, *tail)
    else:
        hip.call("rn_march_rays_train_budget", *head, hip.ptr(budget), *tail)
    torch.cuda.synchronize()
    return x, d, dl, rays, counter


# ------------------------------------------------------------------------------------------------ the per-operator marchers


@pytest.mark.parametrize("name", wc.FAMILIES)
def test_near_far(po, hiplib, name):
    import radnerf_hip as hip
    case = wc.family(name, po)
    w = wc.oracle_walk(po, case)
    o, d, aabb = t(case.o), t(case.d), t(case.aabb)
    nears, fars = torch.full((case.N,), SENTINEL, device=DEV), torch.full((case.N,), SENTINEL, device=DEV)
    hip.call("rn_near_far_from_aabb", hip.ptr(o), hip.ptr(d), hip.ptr(aabb), case.N, wc.MIN_NEAR, hip.ptr(nears), hip.ptr(fars), hip.stream())
    assert same(nears, w["nears"]) and same(fars, w["fars"])
    if name == "degenerate":
        assert same(nears, wc.DEGENERATE_NEARS) and same(fars, wc.DEGENERATE_FARS)


@pytest.mark.parametrize("n_step", [1, 4, 8])
@pytest.mark.parametrize("name", wc.FAMILIES)
def test_march_rays(po, hiplib, name, n_step):
    """rn_march_rays on a sorted random three quarters of the rays, a third of them already advanced, noises on (the needles: all
    twelve-odd rays from near without jitter, see _uniform)."""
    import radnerf_hip as hip
    case = wc.family(name, po)
    w = wc.oracle_walk(po, case)
    g = _Dev(case, w)
    rng = np.random.default_rng(100 + n_step)
    alive = np.sort(rng.permutation(case.N)[: max(1, (case.N * 3) // 4)]).astype(np.int32)
    rays_t = w["nears"].copy()
    rays_t[alive[::3]] += np.float32(0.3)
    noises = rng.uniform(0, 1, alive.shape[0]).astype(np.float32)
    if name == "needles":
        alive, rays_t, noises = np.arange(case.N, dtype=np.int32), w["nears"].copy(), np.zeros(case.N, np.float32)
    n_alive = alive.shape[0]
    M = _pad128(n_alive * n_step)
    bound, dt_gamma, max_steps, Cc, H = case.march_args
    ex, ed, edl = po.march_rays(n_alive, n_step, alive, rays_t, case.o, case.d, bound, dt_gamma, max_steps, Cc, H, case.bits, w["nears"],
                                w["fars"], noises, M=M)
    x, d, dl = _zero_samples(M)
    al, rt, nz = t(alive), t(rays_t), t(noises)
    hip.call("rn_march_rays", n_alive, n_step, hip.ptr(al), hip.ptr(rt), hip.ptr(g.o), hip.ptr(g.d), bound, dt_gamma, max_steps, Cc, H,
             hip.ptr(g.bits), hip.ptr(g.nears), hip.ptr(g.fars), hip.ptr(x), hip.ptr(d), hip.ptr(dl), hip.ptr(nz), None, hip.stream())
    assert same(x, ex) and same(d, ed) and same(dl, edl)
    assert (edl[:, 0] > 0).any()


@pytest.mark.parametrize("mode", ["no_jitter", "jitter", "short_budget"])
@pytest.mark.parametrize("name", wc.FAMILIES)
def test_march_rays_train(po, hiplib, name, mode):
    """rn_march_rays_train with explicit noises: room for every sample, and (short_budget) M = 0.6 x total so that the drop rule
    (raymarching.cu:446-457) is met by rays of the family's branch."""
    import radnerf_hip as hip
    case = wc.family(name, po)
    w = wc.oracle_walk(po, case)
    g = _Dev(case, w)
    noises = np.zeros(case.N, np.float32) if mode == "no_jitter" else _uniform(case, 7)
    bound, dt_gamma, max_steps, Cc, H = case.march_args
    total = wc.oracle_walk(po, case, noises)["total"] if mode != "no_jitter" else w["total"]
    M = _pad128(total) if mode != "short_budget" else int(0.6 * total)
    ex, ed, edl, erays, ecnt = po.march_rays_train(case.o, case.d, case.bits, bound, dt_gamma, max_steps, Cc, H, M, w["nears"], w["fars"], noises)
    x, d, dl, rays, counter = _train_march(hip, case, g, M, noises)
    assert same(counter, ecnt) and same(rays, erays)
    assert same(x, ex) and same(d, ed) and same(dl, edl)
    if mode == "short_budget":
        assert ((erays[:, 1] + erays[:, 2] > M) & (erays[:, 2] > 0)).any()
    elif mode == "no_jitter":
        assert same(x[:total], w["xyzs"]) and same(dl[:total], w["deltas"])


@pytest.mark.parametrize("name", wc.FAMILIES)
def test_march_rays_train_budget(po, hiplib, name):
    """rn_march_rays_train_budget at *M_dev = 0.6 x total in buffers of budget + 3000 rows, compared as
    test_gpu_train.py::test_device_budget_marcher_equals_the_host_budget_marcher compares: dropped rays get count 0, everything else
    equals the host-budget call (and the oracle at M = budget)."""
    import radnerf_hip as hip
    case = wc.family(name, po)
    w = wc.oracle_walk(po, case)
    g = _Dev(case, w)
    noises = _uniform(case, 8)
    budget = int(0.6 * wc.oracle_walk(po, case, noises)["total"])
    cap = budget + 3000
    bound, dt_gamma, max_steps, Cc, H = case.march_args
    ex, ed, edl, erays, ecnt = po.march_rays_train(case.o, case.d, case.bits, bound, dt_gamma, max_steps, Cc, H, budget, w["nears"], w["fars"], noises)
    x1, d1, dl1, r1, c1 = _train_march(hip, case, g, budget, noises)
    bt = torch.tensor([budget], dtype=torch.int32, device=DEV)
    x2, d2, dl2, r2, c2 = _train_march(hip, case, g, cap, noises, budget=bt)
    assert same(c1, ecnt) and same(r1, erays) and same(x1, ex) and same(d1, ed) and same(dl1, edl)
    assert torch.equal(c1, c2)
    assert torch.equal(x1, x2[:budget]) and torch.equal(d1, d2[:budget]) and torch.equal(dl1, dl2[:budget])
    assert not x2[budget:].any() and not d2[budget:].any() and not dl2[budget:].any()
    dropped = (r1[:, 1] + r1[:, 2]) > budget
    assert bool((dropped & (r1[:, 2] > 0)).any())
    assert torch.equal(r1[~dropped], r2[~dropped]) and torch.equal(r1[dropped][:, :2], r2[dropped][:, :2]) and not r2[dropped][:, 2].any()


@pytest.mark.parametrize("frac", [1.3, 0.6])
@pytest.mark.parametrize("name", wc.FAMILIES)
def test_march_rays_train_step(po, hiplib, name, frac):
    """rn_march_rays_train_step (RECORD form for max_steps <= 32, the twice-walking form for 512 / 1024) on sentinel-filled
    buffers against the chain rn_near_far_from_aabb + zeroed counters + rn_march_rays_train_budget: rows [0, min(counter[0], M))
    equal the chain's, rows beyond still hold the sentinel, state[1] stays 0, and a second launch on the same state gives the same
    bits."""
    import radnerf_hip as hip
    case = wc.family(name, po)
    w = wc.oracle_walk(po, case)
    g = _Dev(case, w)
    noises = _uniform(case, 9)
    total = wc.oracle_walk(po, case, noises)["total"]
    budget = int(frac * total)
    cap = budget + 3000
    bt = torch.tensor([budget], dtype=torch.int32, device=DEV)
    bound, dt_gamma, max_steps, Cc, H = case.march_args
    # the chain (near / far from the device as well: test_near_far pins them to the oracle)
    g.nears, g.fars = torch.empty(case.N, device=DEV), torch.empty(case.N, device=DEV)
    hip.call("rn_near_far_from_aabb", hip.ptr(g.o), hip.ptr(g.d), hip.ptr(g.aabb), case.N, wc.MIN_NEAR, hip.ptr(g.nears), hip.ptr(g.fars),
             hip.stream())
    x1, d1, dl1, r1, c1 = _train_march(hip, case, g, cap, noises, budget=bt)
    assert int(c1[0]) == total and int(c1[1]) == case.N
    live = min(total, cap)

    state = torch.zeros(int(hip._lib.rn_march_rays_train_step_state(case.N)) // 4 + 2, dtype=torch.int32, device=DEV)
    assert state.data_ptr() % 8 == 0
    nz = t(noises)
    runs = []
    for rep in range(2):
        x = torch.full((cap, 3), SENTINEL, device=DEV)
        d = torch.full((cap, 3), SENTINEL, device=DEV)
        dl = torch.full((cap, 2), SENTINEL, device=DEV)
        nears, fars = torch.full((case.N,), SENTINEL, device=DEV), torch.full((case.N,), SENTINEL, device=DEV)
        rays = torch.full((case.N, 3), -7, dtype=torch.int32, device=DEV)
        counter = torch.full((2,), 12345, dtype=torch.int32, device=DEV)        # SET by the launch, whatever it held
        hip.call("rn_march_rays_train_step", hip.ptr(g.o), hip.ptr(g.d), hip.ptr(g.bits), hip.ptr(g.aabb), wc.MIN_NEAR, bound, dt_gamma,
                 max_steps, case.N, Cc, H, cap, hip.ptr(bt), hip.ptr(nz), hip.ptr(nears), hip.ptr(fars), hip.ptr(x), hip.ptr(d), hip.ptr(dl),
                 hip.ptr(rays), hip.ptr(counter), hip.ptr(state), 0, hip.stream())
        torch.cuda.synchronize()
        assert state[:2].tolist() == [rep + 1, 0]
        assert same(nears, w["nears"]) and same(fars, w["fars"])
        assert torch.equal(counter, c1) and torch.equal(rays, r1)
        assert torch.equal(x[:live], x1[:live]) and torch.equal(d[:live], d1[:live]) and torch.equal(dl[:live], dl1[:live])
        assert bool((x[live:] == SENTINEL).all()) and bool((d[live:] == SENTINEL).all()) and bool((dl[live:] == SENTINEL).all())
        runs.append((x, d, dl, rays, counter))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    # and the oracle itself, for the rays the budget keeps
    ex, ed, edl, erays, ecnt = po.march_rays_train(case.o, case.d, case.bits, bound, dt_gamma, max_steps, Cc, H, budget, w["nears"], w["fars"], noises)
    assert same(runs[0][4], ecnt)
    kept = ~((erays[:, 1] + erays[:, 2] > budget) & (erays[:, 2] > 0))
    assert np.array_equal(n(runs[0][3])[kept], erays[kept])
    rows = min(live, budget)
    assert same(runs[0][0][:rows], ex[:rows]) and same(runs[0][1][:rows], ed[:rows]) and same(runs[0][2][:rows], edl[:rows])
    assert bool(((erays[:, 1] + erays[:, 2] > budget) & (erays[:, 2] > 0)).any()) == (frac < 1)


# ------------------------------------------------------------------------------------------------ the device loop's prologue


def _short_and_needles(po):
    a, b = wc.family("short", po), wc.family("needles", po)
    return wc.Case("short+needles", np.concatenate([a.o[:1000], b.o]), np.concatenate([a.d[:1000], b.d]), bits=a.bits_kind)


@pytest.mark.parametrize("name", ["diagonal", "short+needles", "casc2", "casc3", "degenerate"])
def test_frame_begin_first_sample(po, hiplib, name):
    """rn_frame_begin with pose = NULL marches iteration 0 (n_step = 1) of the family's own rays: the one place a device-loop marcher
    can be held sample by sample without the network."""
    import radnerf_hip as hip
    from radnerf_hip import abi
    case = _short_and_needles(po) if name == "short+needles" else wc.family(name, po)
    N = case.N
    nears, fars = po.near_far_from_aabb(case.o, case.d, case.aabb, wc.MIN_NEAR)
    bound, dt_gamma, max_steps, Cc, H = case.march_args
    ex, ed, edl = po.march_rays(N, 1, np.arange(N, dtype=np.int32), nears, case.o, case.d, bound, dt_gamma, max_steps, Cc, H, case.bits, nears,
                                fars, np.zeros(N, np.float32))
    o, d, bits, aabb = t(case.o), t(case.d), t(case.bits), t(case.aabb)
    f32 = lambda *shape: torch.full(shape, SENTINEL, device=DEV)
    bufs = dict(nears=f32(N), fars=f32(N), weights_sum=f32(N), depth=f32(N), image=f32(N, 3), rays_t=f32(N), deltas=f32(N, 2), sigmas=f32(N),
                rgbs=f32(N, 3), xyzs=torch.zeros(N, 3, device=DEV), dirs=torch.zeros(N, 3, device=DEV),
                rays_alive_a=torch.full((N,), -7, dtype=torch.int32, device=DEV), rays_alive_b=torch.full((N,), -7, dtype=torch.int32, device=DEV),
                state=torch.zeros(abi.RN_HEAD_STATE_INTS, dtype=torch.int32, device=DEV),
                block_counts=torch.zeros(3 * ((N + 255) // 256 + 1), dtype=torch.int32, device=DEV))
    h = abi.HeadT(rays_o=hip.ptr(o), rays_d=hip.ptr(d), N=N, aabb=hip.ptr(aabb), min_near=wc.MIN_NEAR, bitfield=hip.ptr(bits), bound=bound,
                  dt_gamma=dt_gamma, max_steps=max_steps, cascade=Cc, grid_size=H, T_thresh=1e-4, live_slots=None, order_w=0,
                  **{k: hip.ptr(v) for k, v in bufs.items()})
    hip.call("rn_frame_begin", C.byref(h), None, 0.0, 0.0, 0.0, 0.0, 0, hip.stream())
    torch.cuda.synchronize()
    assert same(bufs["nears"], nears) and same(bufs["fars"], fars) and same(bufs["rays_t"], nears)
    assert same(bufs["xyzs"], ex) and same(bufs["dirs"], ed) and same(bufs["deltas"], edl)
    emitted = edl[:, 0] > 0
    assert emitted.any() and not n(bufs["deltas"])[~emitted].any()
    assert not bufs["weights_sum"].any() and not bufs["depth"].any() and not bufs["image"].any()
    assert same(bufs["rays_alive_a"], np.arange(N, dtype=np.int32))
    st = n(bufs["state"])
    assert st[:5].tolist() == [N, 0, 1, N, 1]                         # n_alive, step, n_step, slots, active
    nb = (N + 255) // 256 + 1
    assert int(n(bufs["block_counts"])[nb:2 * nb].sum()) == int(emitted.sum())


# ------------------------------------------------------------------------------------------------ whole frames, a training step

DIAG_SIZE, DIAG_FOVY = 96, 4.0


def _diagonal_scene(engine, size=DIAG_SIZE, **kw):
    """SyntheticScene whose pose stream starts with three poses with the optical axis on (yaw 45 deg, pitch asin(1 / sqrt 3)) and one degree
    either side of the cube's diagonal.  At the synthetic scene's 21.24 deg field of view a 64^2 / 96^2 image has 2 to 5 pixels with
    max|d_i| <= 0.58 (the seam is 0.19 deg from the diagonal, a pixel 0.22 to 0.33 deg wide), so the view is narrowed to 4 deg: about
    a hundred pixels of a 96^2 image then lie on the generic side and every other pixel within 0.05 of the seam."""
    from radnerf.rays import convert_poses, orbit_pose
    from radnerf.scene import SyntheticScene, default_opt
    scene = SyntheticScene(H=size, W=size, n_frames=8, device=DEV, opt=default_opt(engine=engine, fovy=DIAG_FOVY, **kw))
    pitch = math.degrees(math.asin(1 / math.sqrt(3)))
    poses = scene.poses.cpu().numpy().copy()
    poses[:3] = np.stack([orbit_pose(scene.opt.radius, 45.0 + dy, pitch) for dy in (0.0, 1.0, -1.0)])
    scene.poses = torch.from_numpy(poses).to(scene.device)
    on_device = engine == "fused" and getattr(scene.opt, "ray_engine", "fused") == "fused"
    if on_device:
        from radnerf import fused
        scene.poses6 = fused.convert_poses(scene.poses)
    else:
        scene.poses6 = convert_poses(scene.poses)
    scene._rays = {}
    return scene


def _seam_counts(scene, i):
    from radnerf.rays import get_rays
    d = get_rays(scene.poses[i:i + 1].cpu(), scene.intrinsics, scene.H, scene.W, -1)["rays_d"][0].numpy()
    m = np.abs(d).max(1)
    return int((m <= wc.SEAM).sum()), int((m > wc.SEAM).sum())


@pytest.mark.parametrize("engine,kw", [("fused", {}), ("fused", dict(loop_launch="coop")), ("ops", {})],
                         ids=["fused", "fused-coop", "ops"])
def test_frames_from_a_diagonal_camera_match_the_oracle(po, hiplib, engine, kw):
    """Three frames whose rays straddle the 0.58 seam, at the bars of test_gpu_fused.py::test_fused_frame_matches_oracle."""
    from test_gpu_fused import _oracle_frame
    scene = _diagonal_scene(engine, **kw)
    scene.model.count_samples = True                 # the per-operator loop counts its live samples only when asked to
    for i in range(3):
        generic, fast = _seam_counts(scene, i)
        assert generic >= 30 and fast >= 30, (generic, fast)
        f = scene.frame(i)
        with torch.no_grad():
            out = scene.render(i)
        img, dep, stats = _oracle_frame(po, scene, f, scene.model.enc_a)
        st = scene.model.last_stats
        assert st["iterations"] == stats["iterations"]
        assert st["live_samples"] == stats["live_samples"]
        got = out["image"].reshape(-1, 3).cpu().numpy()
        assert np.abs(got - img).max() <= 2e-3, np.abs(got - img).max()
        gd = out["depth"].reshape(-1).cpu().numpy()
        assert np.array_equal(np.isnan(gd), np.isnan(dep))
        ok = ~np.isnan(dep)
        assert np.abs(gd[ok] - dep[ok]).max() <= 1e-3
    if engine == "fused":
        from radnerf import fused
        assert fused.unfinished_frames(scene.model) == 0 and fused.stalled_workgroups(scene.model) == 0


def test_fused_equals_ops_engine_from_a_diagonal_camera(hiplib):
    """test_gpu_fused.py::test_fused_equals_ops_engine (same rays for both engines, 1e-4) with the diagonal pose stream."""
    a, b = _diagonal_scene("fused", ray_engine="torch"), _diagonal_scene("ops")
    for i in range(3):
        with torch.no_grad():
            ia = a.render(i)["image"]
            ib = b.render(i)["image"]
        assert (ia - ib).abs().max().item() <= 1e-4


def _train_losses(monkeypatch, head, steps):
    """test_gpu_train_head.py::_train_losses on 1024 rays of the diagonal pose."""
    import random
    from radnerf.train import SyntheticTrainStream, Trainer
    monkeypatch.setenv("RN_TRAIN_HEAD", head)
    monkeypatch.setenv("RN_TRAIN_LOSS", "fused" if head == "fused" else "torch")
    torch.manual_seed(0)
    scene = _diagonal_scene("ops", size=64, torso=False, smooth_lips=False)
    stream = SyntheticTrainStream(scene, n_rays=1024, seed=4)
    d = stream.f["rays_d"].reshape(-1, 3).abs().max(1).values
    assert int((d <= wc.SEAM).sum()) >= 30 and int((d > wc.SEAM).sum()) >= 30
    trainer = Trainer(scene.model, scene.opt, update_extra_interval=0)
    scene.model.mean_count = 0
    random.seed(0)
    losses = [float(trainer.step(stream.batch())) for _ in range(steps)]
    return losses, {k: p.detach().clone() for k, p in scene.model.named_parameters()}


def test_training_steps_from_a_diagonal_camera_equal_the_operator_path(hiplib, monkeypatch):
    """The routes above the marcher do not assume the +y geometry: RN_TRAIN_HEAD=fused follows =ops on rays of the diagonal pose, at
    the bar of test_gpu_train_head.py::test_training_steps_equal_the_operator_path."""
    steps = 2
    l_ops, p_ops = _train_losses(monkeypatch, "ops", steps)
    l_fused, p_fused = _train_losses(monkeypatch, "fused", steps)
    assert np.allclose(l_fused, l_ops, rtol=2e-4, atol=1e-7), (l_fused, l_ops)
    for name in p_ops:
        assert torch.isfinite(p_fused[name]).all(), name
        assert float((p_fused[name] - p_ops[name]).abs().max()) <= 2 * steps * 5e-3 + 1e-6, name
