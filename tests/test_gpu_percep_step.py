"""PerceptualAlex (radnerf/percep.py, csrc/rn_percep.hip) as the patch criterion of a lip fine-tuning step and as the metric of
Trainer.evaluate: the 64 x 64 scene and 8-frame set of tests/test_gpu_lips_step.py, the seeded weights of tests/percepref64.py.

The fused loss route with the perceptual kernels (RN_PERCEP=hip: the term's gradient comes from rn_percep_backward and reaches the
ready-made gradients through rn_train_head_loss_chain) is held against RN_TRAIN_LOSS=torch with RN_PERCEP=torch -- autograd over
the PyTorch expressions end to end -- at the bars of tests/test_gpu_lips_step.py: the loss at rtol 2e-4, every parameter gradient
at max |d| / max |ref| < 2e-3 with cos > 0.99999.  The term is a small part of such a step, so the step's own term -- its [n,3] rows
viewed as [P,3,h,w] -- is held to the same bars on its own, kernels against the torch path."""
import numpy as np
import pytest
import torch

import percepref64 as R

pytestmark = pytest.mark.gpu

LOSS_RTOL, GRAD_REL, GRAD_COS = 2e-4, 2e-3, 0.99999
RECT = (16, 48, 12, 52)                                 # 32 x 40 = 1 280 rays


@pytest.fixture(scope="module")
def world(hiplib):
    """One scene, one 8-frame set, the model on it and the criterion, shared by the tests (none takes an optimizer step)."""
    from radnerf.dataset import DeviceTrainSet
    from radnerf.percep import PerceptualAlex
    from radnerf.scene import SyntheticScene, default_opt
    torch.manual_seed(0)
    scene = SyntheticScene(H=64, W=64, n_frames=8, device="cuda", opt=default_opt(engine="ops", torso=False, smooth_lips=False))
    ds = DeviceTrainSet.from_scene(scene, 8, num_rays=2048, seed=3)
    # the set's targets are the scene's own render, which the model fits: the perceptual term would vanish.  Frame 2 gets per-pixel
    # noise of +-40 / 255, so that the term and its gradient are a visible part of the step (asserted below)
    g = torch.Generator(device="cuda").manual_seed(21)
    noise = torch.randint(-40, 41, ds.images[2].shape, generator=g, device="cuda")
    ds.images[2] = (ds.images[2].int() + noise).clamp(0, 255).to(torch.uint8)
    m = ds.install(scene.model)
    m.mean_count = 0                                     # the first window's marcher: every sample of every ray
    m.train()
    ws, bs, lins, _ = R.seeded_weights()
    return scene, ds, m, PerceptualAlex(ws, bs, lins).cuda()


def _step(monkeypatch, m, data, opt, crit, loss_route, percep, seed=5):
    """One train_step + backward; -> (loss, {name: gradient}, the step's prediction [n,3])."""
    from radnerf.train import _backward, train_step
    monkeypatch.setenv("RN_TRAIN_LOSS", loss_route)
    monkeypatch.setenv("RN_PERCEP", percep)
    params = [(n, p) for n, p in m.named_parameters()]
    for _, p in params:
        p.grad = None
    torch.manual_seed(seed)                              # RN_TRAIN_NOISE=torch (conftest): both routes march the same samples
    pred, _, loss = train_step(m, data, opt, global_step=1000, patch_criterion=crit)
    assert (getattr(loss, "_rn_direct", None) is not None) == (loss_route == "fused")
    _backward(loss)
    torch.cuda.synchronize()
    return float(loss.detach()), {n: p.grad.detach().clone() for n, p in params if p.grad is not None}, pred.detach().reshape(-1, 3).clone()


def _compare(what, a, b):
    rel = abs(a[0] - b[0]) / abs(b[0])
    assert set(a[1]) == set(b[1]), set(a[1]) ^ set(b[1])
    worst, worst_name = 0.0, ""
    for name, ref in b[1].items():
        got = a[1][name]
        scale = float(ref.abs().max())
        if scale == 0.0:
            assert float(got.abs().max()) == 0.0, name
            continue
        err = float((got - ref).abs().max()) / scale
        x, y = got.flatten().double(), ref.flatten().double()
        cos = float(x @ y / (x.norm() * y.norm()))
        if err > worst:
            worst, worst_name = err, name
        assert err < GRAD_REL and cos > GRAD_COS, (what, name, err, cos)
    print(f"{what}: loss {a[0]:.6f} / {b[0]:.6f} (rel {rel:.2e}); worst gradient {worst:.2e} of its max ({worst_name}); {len(b[1])} tensors")
    assert rel < LOSS_RTOL, (what, a[0], b[0])


def _batch(ds, kind):
    if kind == "rect":
        data = ds.batch_rect([2], rect=RECT)
        assert data["rays_o"].shape[1] == 1280
    else:
        data = ds.batch_patch([2], 32)
        assert data["rays_o"].shape[1] == 2048              # two 32 x 32 patches
    return data


@pytest.mark.parametrize("kind", ["rect", "patch"])
def test_lips_step_with_the_perceptual_kernels_equals_autograd(world, monkeypatch, kind):
    scene, ds, m, crit = world
    data = _batch(ds, kind)
    fused = _step(monkeypatch, m, data, scene.opt, crit, "fused", "hip")
    torch_ = _step(monkeypatch, m, data, scene.opt, crit, "torch", "torch")
    _compare(f"{kind} step", fused, torch_)
    bare = _step(monkeypatch, m, data, scene.opt, None, "fused", "hip")
    assert fused[0] > bare[0] and any(not torch.equal(fused[1][k], bare[1][k]) for k in bare[1])
    # The term is a small part of this step (0.01 or 0.001 times a distance of a few 1e-3 beside an MSE of 8e-3; it moves the
    # gradients by 1e-3 of their max or less), so the comparison above alone would hardly see a wrong term.  The term itself,
    # then, as train_step forms it -- the [n,3] rows of the step's own prediction and target viewed as [P,3,h,w] -- and its
    # gradient: kernels against the torch path, at the same bars.
    from radnerf.train import _patch_term, _patch_views
    pred, rgb = fused[2], data["images"]
    weight, views, _ = _patch_views(data, pred.shape[0])
    out = {}
    for path in ("hip", "torch"):
        monkeypatch.setenv("RN_PERCEP", path)
        leaf = pred.clone().requires_grad_()
        term = _patch_term(crit, weight, views, leaf, rgb)
        out[path] = (float(term.detach()), torch.autograd.grad(term, leaf)[0])
    (v, g), (v_ref, g_ref) = out["hip"], out["torch"]
    rel, err = abs(v - v_ref) / v_ref, float((g - g_ref).abs().max() / g_ref.abs().max())
    cos = float(g.flatten().double() @ g_ref.flatten().double() / (g.double().norm() * g_ref.double().norm()))
    print(f"{kind} step: the term is {v_ref:.3e} ({v_ref / bare[0]:.1e} of the loss); kernels against the torch path: value rel {rel:.1e}, "
          f"gradient {err:.1e} of its max, 1 - cos {1 - cos:.1e}")
    assert v_ref > 0 and rel < LOSS_RTOL and err < GRAD_REL and cos > GRAD_COS


def test_deterministic_rect_steps_give_the_same_bits(world, monkeypatch):
    scene, ds, m, crit = world
    monkeypatch.setenv("RN_TRAIN_DETERMINISTIC", "1")
    data = _batch(ds, "rect")
    a = _step(monkeypatch, m, data, scene.opt, crit, "fused", "hip")
    b = _step(monkeypatch, m, data, scene.opt, crit, "fused", "hip")
    assert a[0] == b[0] and set(a[1]) == set(b[1]) and len(a[1]) > 8
    for name in a[1]:
        assert torch.equal(a[1][name], b[1][name]), name


def test_evaluate_carries_lpips_with_one_read_back(world, monkeypatch):
    from radnerf.train import Trainer
    scene, ds, m, crit = world
    tr = Trainer(m, scene.opt, update_extra_interval=0)
    monkeypatch.setenv("RN_PERCEP", "hip")
    plain = tr.evaluate(ds, [1, 4])
    fetched = []
    cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: (fetched.append(t.dtype), cpu(t, *a, **k))[1])
    res = tr.evaluate(ds, [1, 4], perceptual=crit)
    monkeypatch.setattr(torch.Tensor, "cpu", cpu)
    assert fetched.count(torch.float64) == 1               # the per-frame sums, lpips among them, in one read-back
    assert set(res) == set(plain) | {"lpips", "lpips_per_frame"} and res["per_frame"] == plain["per_frame"]
    want = []
    monkeypatch.setenv("RN_PERCEP", "torch")
    m.eval()
    with torch.no_grad():
        for i in (1, 4):
            f = ds.frame(i)
            out = m.render(f["rays_o"], f["rays_d"], f["auds"], f["bg_coords"], f["poses"], eye=f["eye"], index=f["index"], staged=True,
                           bg_color=f["bg_color"], perturb=False, dt_gamma=scene.opt.dt_gamma, max_steps=scene.opt.max_steps)
            nchw = lambda t: t.reshape(1, 64, 64, 3).permute(0, 3, 1, 2).float()
            want.append(float(crit(nchw(f["images"]), nchw(out["image"]), normalize=True)))      # LPIPSMeter: (truth, pred), 2x - 1
    m.train()
    print("lpips per frame", res["lpips_per_frame"], "torch path", want)
    assert all(v > 0 for v in want)
    assert np.allclose(res["lpips_per_frame"], want, rtol=2e-4, atol=0) and abs(res["lpips"] - np.mean(want)) <= 2e-4 * np.mean(want)
