"""The patch term of lip fine-tuning through the fused head loss (rn_train_head_loss_chain, csrc/rn_train_head.hip;
train_head.head_loss_chain; train_step's patch_criterion): the chain kernel alone against torch, a rect step and a patch step on
the fused loss route against RN_TRAIN_LOSS=torch (autograd over the PyTorch expression: the oracle), and eight steps of the
lips schedule.

The bound of the two-route comparison is the one tests/test_gpu_train_head.py holds the fused kernels to against the autograd
routes: the loss at rtol 2e-4 (test_training_steps_equal_the_operator_path), every parameter gradient at max |d| / max |ref| <
2e-3 with cos > 0.99999 (test_fused_head_matches_the_operator_path).  The plain step on the same scene is held to it in the same
test, which prints both differences.  Measured on this scene (worst gradient, relative to its max; the
losses agreed in every fp32 digit): plain step 3.3e-6 and 1.7e-6, rect step 8.1e-6, patch step 4.1e-6 -- all of it the float
atomics of the audio nets' gradients, which differ between two runs of ONE route as much; the chain adds one rounding per element."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
LOSS_RTOL, GRAD_REL, GRAD_COS = 2e-4, 2e-3, 0.99999


# --------------------------------------------------------------------------------------------------------- the kernel alone
@pytest.mark.parametrize("N", [35, 300])           # a 5 x 7 rect; more than one 256-thread workgroup
def test_chain_kernel_against_torch(hiplib, N):
    hip = hiplib
    g = torch.Generator(device="cuda").manual_seed(100 + N)
    rand = lambda *s: torch.rand(*s, device="cuda", generator=g)
    table = rand(N, 15)                                  # bg is a strided column block of a packed batch table (columns 8:11)
    bg, ws = table[:, 8:11], rand(N)
    # raw = image + (1 - ws) * bg: a quarter outside [0, 1] (an eighth on either side), none within 1e-3 of 0 or 1
    u = (torch.argsort(torch.argsort(rand(N * 3))).float() / (N * 3)).view(N, 3)       # ranks: exactly an eighth below 0.125 ...
    want_raw = torch.where(u < 0.125, -0.05 - rand(N, 3), torch.where(u > 0.875, 1.05 + rand(N, 3), 0.01 + 0.98 * rand(N, 3)))
    image = (want_raw - (1 - ws).unsqueeze(-1) * bg).contiguous()
    raw = image + (1 - ws).unsqueeze(-1) * bg            # fp32, product and sum rounded on their own: the kernels' expression
    passes = (raw >= 0) & (raw <= 1)
    assert float(torch.minimum(raw.abs(), (raw - 1).abs()).min()) > 1e-3
    assert 0.15 < 1 - float(passes.float().mean()) < 0.35
    g_pred = rand(N, 3) * 2 - 1
    g_image0, g_ws0 = rand(N, 3) * 2 - 1, rand(N) * 2 - 1
    loss0, term = torch.tensor([0.7312645], device="cuda"), torch.tensor([0.0123456789], device="cuda")
    g_image, g_ws, loss = g_image0.clone(), g_ws0.clone(), loss0.clone()
    hip.call("rn_train_head_loss_chain", hip.ptr(image), hip.ptr(ws), bg.data_ptr(), bg.stride(0), hip.ptr(g_pred), N, hip.ptr(term),
             hip.ptr(loss), hip.ptr(g_image), hip.ptr(g_ws), hip.stream())
    torch.cuda.synchronize()
    passed = torch.where(passes, g_pred, torch.zeros_like(g_pred))
    assert torch.equal(g_image, g_image0 + passed)       # one fp32 add per element: bit for bit
    want = g_ws0.double() - (passed.double() * bg.double()).sum(-1)
    bound = 4 * EPS32 * (g_ws0.abs().double() + (g_pred.double() * bg.double()).abs().sum(-1))      # three fp32 products, three adds
    err = (g_ws.double() - want).abs()
    print(f"N = {N}: g_ws max err / bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    assert not torch.equal(g_ws, g_ws0) and torch.equal(loss, loss0 + term)


# ------------------------------------------------------------------------------------------------------------------ the step
def _scene():
    from radnerf.scene import SyntheticScene, default_opt
    return SyntheticScene(H=64, W=64, n_frames=8, device="cuda", opt=default_opt(engine="ops", torso=False, smooth_lips=False))


@pytest.fixture(scope="module")
def world(hiplib):
    """One scene, one 8-frame set and the model on it, shared by the step tests (none of them takes an optimizer step)."""
    from radnerf.dataset import DeviceTrainSet
    torch.manual_seed(0)
    scene = _scene()
    ds = DeviceTrainSet.from_scene(scene, 8, num_rays=64, seed=3)
    m = ds.install(scene.model)
    m.mean_count = 0                                     # the first window's marcher: every sample of every ray
    m.train()
    return scene, ds, m


class _Criterion(torch.nn.Module):
    """A fixed, seeded stand-in for the perceptual network: two 3 x 3 convolutions (zero padding, as unfold + matmul: plain
    kernels) with a ReLU between them, then the mean absolute difference of the features per patch -> [P,1,1,1]."""

    def __init__(self, seed=1, scale=1.0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.w1 = torch.nn.Parameter(torch.randn(8, 27, generator=g) * 0.3)
        self.w2 = torch.nn.Parameter(torch.randn(8, 72, generator=g) * 0.2)
        self.scale = scale

    @staticmethod
    def _conv(x, w):
        P, _, h, wd = x.shape
        return (w @ torch.nn.functional.unfold(x, 3, padding=1)).view(P, w.shape[0], h, wd)

    def features(self, x):
        return self._conv(torch.relu(self._conv(x, self.w1)), self.w2)

    def forward(self, pred, target):
        return self.scale * (self.features(pred) - self.features(target)).abs().mean(dim=(1, 2, 3), keepdim=True)


def _zero_criterion(pred, target):
    return (pred * 0).sum(dim=(1, 2, 3), keepdim=True)


def _step(monkeypatch, m, data, opt, crit, loss_route, seed=5):
    """One train_step + backward on `loss_route`; -> (loss, {name: gradient}, d loss / d image of the fused route or None)."""
    from radnerf.train import _backward, train_step
    monkeypatch.setenv("RN_TRAIN_LOSS", loss_route)
    own = list(crit.named_parameters()) if isinstance(crit, torch.nn.Module) else []
    params = [(f"model.{n}", p) for n, p in m.named_parameters()] + [(f"criterion.{n}", p) for n, p in own]
    for _, p in params:
        p.grad = None
    torch.manual_seed(seed)                              # RN_TRAIN_NOISE=torch (conftest): both routes march the same samples
    _, _, loss = train_step(m, data, opt, global_step=1000, patch_criterion=crit)
    direct = getattr(loss, "_rn_direct", None)
    assert (direct is not None) == (loss_route == "fused")
    g_image = direct[1][0].clone() if direct is not None else None
    inputs = tuple(t.detach().clone() for t in direct[0][:2]) if direct is not None else None
    _backward(loss)
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in params if p.grad is not None}
    return float(loss.detach()), grads, g_image, inputs


def _compare(what, a, b):
    """(loss, gradients) of the fused route `a` against the autograd route `b` at the module's bars; prints what it measures."""
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
        cos = float(x @ y / (x.norm() * y.norm()))       # (cosine_similarity clamps the norms at 1e-8: these gradients are smaller)
        if err > worst:
            worst, worst_name = err, name
        assert err < GRAD_REL and cos > GRAD_COS, (what, name, err, cos)
    print(f"{what}: loss {a[0]:.6f} / {b[0]:.6f} (rel {rel:.2e}); worst gradient {worst:.2e} of its max ({worst_name}); {len(b[1])} tensors")
    assert rel < LOSS_RTOL, (what, a[0], b[0])
    return rel, worst


@pytest.mark.parametrize("kind", ["rect", "patch"])
def test_lips_step_on_the_fused_loss_equals_autograd(world, monkeypatch, kind):
    scene, ds, m = world
    crit = _Criterion().cuda()
    plain = ds.batch([2])
    fused, torch_ = (_step(monkeypatch, m, plain, scene.opt, None, r) for r in ("fused", "torch"))
    _compare("plain step", fused, torch_)
    data = ds.batch_rect([2]) if kind == "rect" else ds.batch_patch([2], 4)
    n = data["rays_o"].shape[1]
    assert (kind == "rect" and n == (lambda r: (r[1] - r[0]) * (r[3] - r[2]))(ds.lips_rect[2]) and n > 64) or (kind == "patch" and n == 64)
    fused, torch_ = (_step(monkeypatch, m, data, scene.opt, crit, r) for r in ("fused", "torch"))
    _compare(f"{kind} step", fused, torch_)
    assert {"criterion.w1", "criterion.w2"} <= set(fused[1]) and float(fused[1]["criterion.w1"].abs().max()) > 0
    bare = _step(monkeypatch, m, data, scene.opt, None, "torch")         # the term is really in the loss and in the gradients
    assert fused[0] > bare[0] * (1 + 1e-4) and any(not torch.equal(fused[1][k], bare[1][k]) for k in bare[1])


@pytest.mark.parametrize("kind", ["rect", "patch"])
def test_zero_criterion_is_the_plain_step_bit_for_bit(world, monkeypatch, kind):
    """A criterion that returns zero: loss and gradients of the plain step on the same pixels.  RN_TRAIN_DETERMINISTIC=1 takes
    the float atomics out of the table gradients, so that two steps can be compared bit for bit at all."""
    scene, ds, m = world
    monkeypatch.setenv("RN_TRAIN_DETERMINISTIC", "1")
    data = ds.batch_rect([5]) if kind == "rect" else ds.batch_patch([5], 4)
    chained = _step(monkeypatch, m, data, scene.opt, _zero_criterion, "fused")
    other = ds.clone()
    same_pixels = other.batch([5], inds=ds.inds.clone())
    assert torch.equal(same_pixels["_packed"], data["_packed"])
    plain = _step(monkeypatch, m, same_pixels, scene.opt, None, "fused")
    assert chained[0] == plain[0] and set(chained[1]) == set(plain[1])
    for name in plain[1]:
        assert torch.equal(chained[1][name], plain[1][name]), name
    assert torch.equal(chained[2], plain[2])


def test_the_terms_gradient_is_really_delivered(world, monkeypatch):
    """d loss / d image of the fused route = the loss kernel's own + where(pass, g_pred, 0), g_pred = d (0.01 * term) / d pred from
    autograd -- exactly, and with a doubled criterion exactly twice that contribution.  The fused loss hands autograd ready-made
    gradients: before the chain existed, a caller's extra term on pred changed nothing in them."""
    scene, ds, m = world
    data = ds.batch_rect([3])
    xmin, xmax, ymin, ymax = data["rect"]
    g0 = _step(monkeypatch, m, data, scene.opt, None, "fused")
    g1 = _step(monkeypatch, m, data, scene.opt, _Criterion().cuda(), "fused")
    g2 = _step(monkeypatch, m, data, scene.opt, _Criterion(scale=2.0).cuda(), "fused")
    image, ws = g1[3]
    assert torch.equal(image, g0[3][0]) and torch.equal(ws, g0[3][1])   # the three steps rendered the same rays
    bg = data["bg_color"].reshape(-1, 3)
    raw = image + (1 - ws).unsqueeze(-1) * bg
    passes = (raw >= 0) & (raw <= 1)
    leaf = raw.clamp(0, 1).detach().requires_grad_()
    nchw = lambda t: t.reshape(1, xmax - xmin, ymax - ymin, 3).permute(0, 3, 1, 2).contiguous()
    term = 0.01 * _Criterion().cuda()(nchw(leaf), nchw(data["images"])).mean()
    (g_pred,) = torch.autograd.grad(term, leaf)
    passed = torch.where(passes, g_pred, torch.zeros_like(g_pred))
    assert float(passed.abs().max()) > 0 and not torch.equal(g1[2], g0[2])
    assert torch.equal(g1[2], g0[2] + passed)
    assert torch.equal(g2[2], g0[2] + 2 * passed)
    assert abs((g1[0] - g0[0]) - float(term.detach())) < 4 * EPS32 * g1[0] and abs((g2[0] - g0[0]) - 2 * float(term.detach())) < 4 * EPS32 * g2[0]


# ---------------------------------------------------------------------------------------------------------- training progress
class _Logged:
    def __init__(self, crit):
        self.crit, self.values = crit, []

    def __call__(self, pred, target):
        v = self.crit(pred, target)
        self.values.append(float(v.detach().mean()))
        return v


def test_lips_schedule_trains_the_patch_term_down(hiplib):
    """Eight eager steps (HipAdam) of the lips schedule on frame 2 of an 8-frame set: rect, pixels, rect, ...  The target is the
    scene's own render, which the model already fits; inside the lips rect it is moved by a fixed offset, and the patch term of
    the last rect step is below the first one's."""
    from radnerf.dataset import DeviceTrainSet
    from radnerf.train import HipAdam, Trainer, lips_schedule
    torch.manual_seed(0)
    scene = _scene()
    ds = DeviceTrainSet.from_scene(scene, 8, num_rays=256, seed=1)
    xmin, xmax, ymin, ymax = ds.lips_rect[2]
    ds.images[2, xmin:xmax, ymin:ymax] = (ds.images[2, xmin:xmax, ymin:ymax].int() + 40).clamp(0, 255).to(torch.uint8)
    m = ds.install(scene.model)
    crit = _Logged(_Criterion().cuda().requires_grad_(False))
    trainer = Trainer(m, scene.opt, patch_criterion=crit)
    assert isinstance(trainer.optimizer, HipAdam)
    losses, sizes = [], []
    for step in range(8):
        data = lips_schedule(ds, [2], step)
        sizes.append(data["rays_o"].shape[1])
        losses.append(float(trainer.step(data)))
    print("losses", [f"{v:.5f}" for v in losses], "patch term on the rect steps", [f"{v:.5f}" for v in crit.values])
    assert sizes == [(xmax - xmin) * (ymax - ymin), 256] * 4
    assert all(np.isfinite(losses)) and len(crit.values) == 4 and all(np.isfinite(crit.values))
    assert crit.values[-1] < crit.values[0]
    ds.check()
