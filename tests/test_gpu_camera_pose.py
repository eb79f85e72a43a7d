"""The opt-in camera-pose kernels of --train_camera (RN_TRAIN_CAMERA=fused; radnerf/train_camera.py, csrc/rn_train_camera.hip):
rn_camera_rays_forward / rn_camera_rays_backward against the torch pose code they replace (nerf/renderer.py:170-174) and its
float64 restatement -- operator by operator, through the renderer, through eight optimizer steps and through a captured step.
Bars that compare the new route with today's are set by what two legitimate evaluations of today's route differ by: the same
call with every ray direction moved to the next float (A')."""
import collections
import os

import numpy as np
import pytest
import torch

from test_gpu_options import _maxerr
from test_gpu_train_camera import _camera_scene, _camera_training, _count_calls

import cases  # noqa: E402  (tests/golden, put on the path by test_gpu_options)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FWD, BWD = "rn_camera_rays_forward", "rn_camera_rays_backward"
SIZES = [1, 255, 256, 257, 1024]
ROWS = [0, 3, 7]


def _inputs(N, seed):
    """8-row tables seeded in +-5 degrees / +-0.05, N rays with unit directions around (0, 0, 1), upstream gradients U(-1,1) + 0.5."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    u = lambda *s: torch.rand(*s, device="cuda", generator=g) * 2 - 1  # noqa: E731
    dR, dT = u(8, 3) * 5, u(8, 3) * 0.05
    o = u(N, 3)
    d = torch.nn.functional.normalize(torch.tensor([0.0, 0.0, 1.0], device="cuda") + 0.3 * u(N, 3), dim=-1)
    return o, d, dT, dR, u(N, 3) + 0.5, u(N, 3) + 0.5


def _torch_pose(o, d, dT, dR, index):
    """Today's code, in the dtype of its arguments."""
    from radnerf.rays import euler_angles_to_matrix
    return o + dT[index], d @ euler_angles_to_matrix(dR[index] / 180 * np.pi + 1e-8).squeeze(0)


def _kernel_pose(o, d, dT, dR, row):
    from radnerf.train_camera import _CameraRays
    return _CameraRays.apply(o, d, dT, dR, torch.tensor([row], dtype=torch.int64, device="cuda"))


def _torch_grads(o, d, dT, dR, row, up_o, up_d, dtype):
    dT, dR = dT.to(dtype).clone().requires_grad_(True), dR.to(dtype).clone().requires_grad_(True)
    oo, od = _torch_pose(o.to(dtype), d.to(dtype), dT, dR, [row])
    return torch.autograd.grad([oo, od], [dT, dR], [up_o.to(dtype), up_d.to(dtype)])


def _kernel_grads(o, d, dT, dR, row, up_o, up_d):
    dT, dR = dT.clone().requires_grad_(True), dR.clone().requires_grad_(True)
    oo, od = _kernel_pose(o, d, dT, dR, row)
    return torch.autograd.grad([oo, od], [dT, dR], [up_o, up_d])


# ------------------------------------------------------------------------------------------------- 1. forward, per operator
@pytest.mark.parametrize("row", ROWS)
@pytest.mark.parametrize("N", SIZES)
def test_forward_against_float64(hiplib, N, row):
    """rays_o + dT[row] and rays_d @ R(dR[row]) against the same formula in float64 on the same fp32 inputs: max-normalised
    e_kernel <= 4 e_torch32 + 1.2e-7, e_torch32 the error of today's fp32 torch code on the GPU."""
    o, d, dT, dR, _, _ = _inputs(N, 100 + N)
    ref = _torch_pose(o.double(), d.double(), dT.double(), dR.double(), [row])
    t32 = _torch_pose(o, d, dT, dR, [row])
    got = _kernel_pose(o, d, dT, dR, row)
    for name, k, t, r in zip(("rays_o", "rays_d"), got, t32, ref):
        assert k.shape == (N, 3) and torch.isfinite(k).all()
        e_k, e_t = _maxerr(k, r), _maxerr(t, r)
        print(f"forward N={N} row={row} {name}: e_kernel {e_k:.3e}  e_torch32 {e_t:.3e}")
        assert e_k <= 4 * e_t + 1.2e-7, (name, e_k, e_t)


# ------------------------------------------------------------------------------------------------ 2. backward, per operator
@pytest.mark.parametrize("row", ROWS)
@pytest.mark.parametrize("N", SIZES)
def test_backward_against_float64_autograd(hiplib, N, row):
    """The two gradient tables against float64 autograd of the torch pose code on the same fp32 inputs: the row at
    e_kernel <= 4 e_torch32 + 1e-6, every other row exactly 0, two calls bit-equal."""
    o, d, dT, dR, up_o, up_d = _inputs(N, 200 + N)
    ref = _torch_grads(o, d, dT, dR, row, up_o, up_d, torch.float64)
    t32 = _torch_grads(o, d, dT, dR, row, up_o, up_d, torch.float32)
    got = _kernel_grads(o, d, dT, dR, row, up_o, up_d)
    again = _kernel_grads(o, d, dT, dR, row, up_o, up_d)
    for name, k, k2, t, r in zip(("camera_dT", "camera_dR"), got, again, t32, ref):
        assert k.shape == (8, 3) and torch.isfinite(k).all() and torch.equal(k, k2), name
        e_k, e_t = _maxerr(k[row], r[row]), _maxerr(t[row], r[row])
        print(f"backward N={N} row={row} {name}: e_kernel {e_k:.3e}  e_torch32 {e_t:.3e} | {k[row].tolist()}")
        assert e_k <= 4 * e_t + 1e-6, (name, e_k, e_t)
        rest = k.clone()
        rest[row] = 0
        assert float(rest.abs().max()) == 0.0 and float(k[row].abs().max()) > 0.0, name


def test_backward_of_one_ray_and_of_zero_gradients_is_finite(hiplib):
    for N in (1, 300):
        o, d, dT, dR, up_o, up_d = _inputs(N, 300 + N)
        for k in _kernel_grads(o, d, dT, dR, 3, torch.zeros_like(up_o), torch.zeros_like(up_d)):
            assert torch.isfinite(k).all() and float(k.abs().max()) == 0.0
    for k in _kernel_grads(*_inputs(1, 301)[:4], 3, *_inputs(1, 301)[4:]):
        assert torch.isfinite(k).all() and float(k[3].abs().max()) > 0.0


def test_row_index_wraps_and_never_leaves_the_tables(hiplib):
    """A negative device index wraps as torch's does (bit-equal to the wrapped row); an index outside [-rows, rows) applies no
    offset and gives all-zero gradients."""
    o, d, dT, dR, up_o, up_d = _inputs(257, 400)
    for a, b in zip(_kernel_pose(o, d, dT, dR, -5), _kernel_pose(o, d, dT, dR, 3)):
        assert torch.equal(a, b)
    for a, b in zip(_kernel_grads(o, d, dT, dR, -5, up_o, up_d), _kernel_grads(o, d, dT, dR, 3, up_o, up_d)):
        assert torch.equal(a, b)
    for bad in (8, -9, 2 ** 40, -2 ** 40):
        oo, od = _kernel_pose(o, d, dT, dR, bad)
        assert torch.equal(oo, o) and torch.equal(od, d), bad
        for k in _kernel_grads(o, d, dT, dR, bad, up_o, up_d):
            assert k.shape == (8, 3) and float(k.abs().max()) == 0.0, bad


# ---------------------------------------------------------------------------------------------- 3. through the renderer
def _graph_nodes(t):
    """Names of the autograd nodes below tensor `t`."""
    seen, todo, names = set(), [t.grad_fn], []
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.append(type(fn).__name__)
        todo += [f for f, _ in fn.next_functions]
    return names


def _render_call(scene, f, px, monkeypatch, pose, index=(3,)):
    """One train-branch call of the renderer with the fused head at `index` and its backward (the call and the loss of
    test_gpu_train_camera.py::test_camera_gradients_through_the_renderer, unmasked, mean_count 49152)."""
    m, opt = scene.model, scene.opt
    m.train()
    monkeypatch.setenv("RN_TRAIN_HEAD", "fused")
    monkeypatch.setenv("RN_TRAIN_CAMERA", pose)
    seen = {}
    import raymarching.ops as ops
    inner = ops._rays

    def rays(rays_o, rays_d):                  # what the marcher is handed: the rays after the pose code
        seen["rays_o"], seen["rays_d"] = rays_o.detach().clone(), rays_d.detach().clone()
        return inner(rays_o, rays_d)
    monkeypatch.setattr(ops, "_rays", rays)
    calls = _count_calls(monkeypatch)
    m.zero_grad(set_to_none=True)
    m.mean_count, m.local_step = 49152, 0
    m.step_counter.zero_()
    res = m.render(f["rays_o"][:, px], f["rays_d"][:, px], f["auds"], f["bg_coords"][:, px], f["poses"], eye=f["eye"], index=list(index),
                   bg_color=f["bg_color"][:, px], staged=False, perturb=False, force_all_rays=False, dt_gamma=opt.dt_gamma,
                   max_steps=opt.max_steps)
    g = cases.rm_inputs(17)
    loss = (res["image"].reshape(-1, 3) * g(4096, 3, lo=-1, hi=1).cuda()).sum() + (res["weights_sum"] * g(4096, lo=-1, hi=1).cuda()).sum() \
        + (res["ambient"] * g(4096, lo=-1, hi=1).cuda()).sum()
    nodes = _graph_nodes(loss)
    loss.backward()
    monkeypatch.setattr(ops, "_rays", inner)
    return dict(calls=dict(calls), nodes=nodes, dT=m.camera_dT.grad.detach().clone(), dR=m.camera_dR.grad.detach().clone(), **seen)


def _ulps(a, b):
    """Distance of two fp32 tensors in representable floats."""
    def key(t):
        i = t.contiguous().view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7fffffff), i)
    return (key(a) - key(b)).abs()


def test_camera_gradients_through_the_renderer(hiplib, monkeypatch):
    """A: today's route; B: RN_TRAIN_CAMERA=fused; A': today's route with rays_d moved to the next float, which measures how far
    two legitimate evaluations drift when the rays differ in the last bit -- all B may differ from A by.  Rows dT[3], dR[3]:
    max-normalised |B - A| <= 4 |A' - A| + 1e-6; every other row exactly zero.  B calls each new entry point once, no
    rn_grid_encode_backward, and its autograd graph has lost exactly the two index nodes of camera_dT[index] / camera_dR[index],
    whose backward is torch's index_put.  A list index one past the tables' last row raises IndexError before anything is launched."""
    scene = _camera_scene()
    f = scene.frame(0)
    px = torch.from_numpy(np.load(os.path.join(HERE, "golden", "reference_frames.npz"), allow_pickle=False)["train_px"]).cuda()
    rows = scene.model.camera_dT.shape[0]       # one row per frame the model can hold (individual_num), not per frame of the scene
    assert px.numel() == 4096 and rows > 3
    f_next = dict(f)
    f_next["rays_d"] = torch.nextafter(f["rays_d"], torch.full_like(f["rays_d"], float("inf")))
    A = _render_call(scene, f, px, monkeypatch, "torch")
    B = _render_call(scene, f, px, monkeypatch, "fused")
    A2 = _render_call(scene, f_next, px, monkeypatch, "torch")
    ulps = torch.maximum(_ulps(B["rays_o"], A["rays_o"]).max(), _ulps(B["rays_d"], A["rays_d"]).max())
    print(f"rays handed to the marcher, B against A: at most {int(ulps)} ulps apart")
    index_nodes = lambda r: sum(n.startswith("IndexBackward") for n in r["nodes"])  # noqa: E731
    assert A["calls"].get(FWD, 0) == 0 and A["calls"].get(BWD, 0) == 0 and index_nodes(A) >= 2, (A["calls"], sorted(set(A["nodes"])))
    assert B["calls"].get(FWD) == 1 and B["calls"].get(BWD) == 1 and B["calls"].get("rn_grid_encode_backward", 0) == 0, B["calls"]
    assert B["calls"].get("rn_train_head_input_grads") == 1 and B["calls"].get("rn_march_rays_train_backward") == 1, B["calls"]
    assert index_nodes(B) == index_nodes(A) - 2 and not any("IndexPut" in n for n in B["nodes"]), sorted(set(B["nodes"]))
    for name in ("dT", "dR"):
        a, b, a2 = A[name], B[name], A2[name]
        scale = float(a[3].abs().max())
        d_b, d_ref = float((b[3] - a[3]).abs().max()) / scale, float((a2[3] - a[3]).abs().max()) / scale
        print(f"camera_{name}[3]: |B - A| {d_b:.3e}  |A' - A| {d_ref:.3e} | A {a[3].tolist()} B {b[3].tolist()}")
        for t in (a, b):
            rest = t.clone()
            rest[3] = 0
            assert torch.isfinite(t).all() and float(rest.abs().max()) == 0.0 and float(t[3].abs().max()) > 0.0, name
        assert d_b <= 4 * d_ref + 1e-6, (name, d_b, d_ref)
    calls = _count_calls(monkeypatch)
    with pytest.raises(IndexError):
        _render_call(scene, f, px, monkeypatch, "fused", index=(rows,))
    assert calls.get(FWD, 0) == 0 and calls.get(BWD, 0) == 0, dict(calls)


# ----------------------------------------------------------------------------------------------------------- 4. trainer
def test_camera_training_steps_follow_the_torch_pose_code(hiplib, monkeypatch):
    """The eight eager steps of test_gpu_train_camera._camera_training for A (today's pose code), B (RN_TRAIN_CAMERA=fused) and A'
    (A with rays_d moved to the next float): B follows A at rtol = max(2e-4, 4 d_ref), atol 1e-7, d_ref the largest relative loss
    difference between A' and A.  B calls each new entry point once per step, A never (the route is opt-in); the frame's camera
    rows moved and are finite, every other row is exactly zero."""
    import radnerf.train as train

    class NextFloatStream(train.SyntheticTrainStream):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.f = dict(self.f)
            self.f["rays_d"] = torch.nextafter(self.f["rays_d"], torch.full_like(self.f["rays_d"], float("inf")))

    monkeypatch.delenv("RN_TRAIN_CAMERA", raising=False)
    l_a, s_a, cam_a, frame = _camera_training(monkeypatch, "fused", True)
    monkeypatch.setenv("RN_TRAIN_CAMERA", "fused")
    l_b, s_b, cam_b, _ = _camera_training(monkeypatch, "fused", True)
    monkeypatch.delenv("RN_TRAIN_CAMERA")
    monkeypatch.setattr(train, "SyntheticTrainStream", NextFloatStream)
    l_a2, _, _, _ = _camera_training(monkeypatch, "fused", True)
    print("losses A ", l_a, "\nlosses B ", l_b, "\nlosses A'", l_a2)
    for i, c in enumerate(s_a):                 # without RN_TRAIN_CAMERA a camera step calls none of the new entry points
        assert c[FWD] == 0 and c[BWD] == 0 and c["rn_train_head_input_grads"] == 1, (i, dict(c))
    for i, c in enumerate(s_b):
        assert c[FWD] == 1 and c[BWD] == 1 and c["rn_train_head_input_grads"] == 1 and c["rn_march_rays_train_backward"] == 1, (i, dict(c))
        assert c["rn_grid_encode_backward"] == 0 and c["rn_train_head_forward"] == 1, (i, dict(c))
    d_ref = float(np.max(np.abs(np.array(l_a2) - np.array(l_a)) / np.abs(np.array(l_a))))
    d_b = float(np.max(np.abs(np.array(l_b) - np.array(l_a)) / np.abs(np.array(l_a))))
    print(f"largest relative loss difference: B against A {d_b:.3e}, A' against A {d_ref:.3e}")
    assert np.allclose(l_b, l_a, rtol=max(2e-4, 4 * d_ref), atol=1e-7), (l_b, l_a, d_ref)
    for dT, dR in (cam_a, cam_b):
        for t in (dT, dR):
            rest = t.clone()
            rest[frame] = 0
            assert torch.isfinite(t).all() and float(t[frame].abs().max()) > 0.0 and float(rest.abs().max()) == 0.0
    print("camera_dT[frame] A", cam_a[0][frame].tolist(), "B", cam_b[0][frame].tolist())


# ----------------------------------------------------------------------------------------------------- 5. captured step
FRAMES = (1, 4, 6)


def _set_training(monkeypatch, graphed, eager=2, steps=8):
    """Camera training on batches of a DeviceTrainSet whose frame changes every step (frames 1, 4, 6 in turn), RN_TRAIN_CAMERA=fused:
    `eager` steps of the first window, then `steps` with the sample budget on the device."""
    from radnerf.dataset import DeviceTrainSet
    from radnerf.scene import SyntheticScene, default_opt
    from radnerf.train import GraphedTrainer, Trainer
    monkeypatch.setenv("RN_TRAIN_HEAD", "fused")
    monkeypatch.setenv("RN_TRAIN_LOSS", "fused")
    monkeypatch.setenv("RN_TRAIN_CAMERA", "fused")
    torch.manual_seed(0)
    scene = SyntheticScene(H=64, W=64, n_frames=8, device="cuda",
                           opt=default_opt(engine="ops", torso=False, smooth_lips=False, train_camera=True))
    ds = DeviceTrainSet.from_scene(scene, 8, num_rays=1024, seed=2)
    m = ds.install(scene.model)
    trainer = (GraphedTrainer if graphed else Trainer)(m, scene.opt, update_extra_interval=0)
    m.mean_count = 0
    calls = _count_calls(monkeypatch)
    losses, per_step, captured = [], [], []
    for i in range(eager + steps):
        if i == eager:
            m.mean_count = int(m.step_counter[:eager, 0].float().mean().item() * 1.2)
            assert m.mean_count > 0
            torch.manual_seed(12)
        data = ds.batch([FRAMES[i % len(FRAMES)]])
        before, caps = collections.Counter(calls), getattr(trainer, "captures", 0)
        losses.append(float(trainer.step(data)))
        per_step.append(collections.Counter(calls) - before)
        if getattr(trainer, "captures", 0) > caps:
            captured.append(per_step[-1])
    ds.check()
    return losses, per_step, captured, trainer, (m.camera_dT.detach().clone(), m.camera_dR.detach().clone())


def test_captured_camera_step_follows_the_eager_one(hiplib, monkeypatch):
    """GraphedTrainer against Trainer, both on the new route, on a feed whose frame index changes between replays: the loss
    curves agree at rtol 2e-3, atol 1e-7 (the bar of test_gpu_train.py::test_packed_batches_train_like_separate_tensors); at
    most two captures serve eight replays; the capture pass ran the fused head with its input gradients and each camera entry
    point exactly once, and no operator backward of the grid; the rows of all three drawn frames moved, the rows of frames
    never drawn are exactly zero.

    Two first-window steps and eight replays, the fewest this comparison can have: a camera step is not reproducible bit for
    bit (the table scatter adds with float atomics), the pose update turns last-bit differences into other rays and the marcher
    into other samples, and the curves of two runs drift apart step by step.  Measured at this length, three eager and three
    graphed runs, largest relative loss difference of every pair: eager against eager 8.6e-4 -- 2.8e-3, graphed against eager
    4.9e-4 -- 3.0e-3, graphed against graphed 5.0e-4 -- 2.8e-3: the same drift on both sides.  At this loss (3e-5) the bar's atol
    of 1e-7 makes it 5.3e-3 relative.  At 4 + 12 steps two eager runs were 1.8e-3 -- 5.9e-3 apart and a graphed one 3.4e-3 -- 5.7e-3
    from them.
    """
    l_eager, _, _, _, cam_eager = _set_training(monkeypatch, False)
    l_graph, _, captured, trainer, cam_graph = _set_training(monkeypatch, True)
    print("losses eager", l_eager, "\nlosses graph", l_graph)
    assert 1 <= trainer.captures <= 2 and trainer.replays >= 8, (trainer.captures, trainer.replays)
    for c in captured:
        for name in ("rn_train_head_forward", "rn_train_head_input_grads", FWD, BWD):
            assert c[name] == 1, (name, dict(c))
        assert c["rn_grid_encode_backward"] == 0, dict(c)
    np.testing.assert_allclose(l_graph, l_eager, rtol=2e-3, atol=1e-7)
    for dT, dR in (cam_eager, cam_graph):
        for t in (dT, dR):
            assert torch.isfinite(t).all()
            assert sum(float(t[fr].abs().max()) > 0.0 for fr in FRAMES) >= 2
            rest = t.clone()
            rest[list(FRAMES)] = 0
            assert float(rest.abs().max()) == 0.0
