"""The per-sample network kernels off the default model options and at tile edges: the fused inference kernels (f32, f32x2,
f16), their weight packers and the frame-bias kernel, the torso kernel, and the fused training head (rn_train_head.hip) at
the option sets of tests/golden/cases.py OPTION_SETS -- A: no eye input, no individual codes; B: odd code widths (row strides
65 / 87 / 99 / 131, not multiples of 4) -- and at the default options.  References: the oracle (as in test_gpu_fused.py), the
float64 restatement tests/netref64.py, and the reference-generated tests/golden/reference_options.npz."""
import os
import sys

import numpy as np
import pytest
import torch

import netref64
from test_gpu_fused import _close_up_to_rounding_flips
from test_gpu_train_head import _stable_samples

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import cases  # noqa: E402

pytestmark = pytest.mark.gpu

SETS = {"default": {}, **cases.OPTION_SETS}
_SCENES = {}


def _scene(tag, size=16, **kw):
    from radnerf.scene import SyntheticScene, default_opt
    key = (tag, size, tuple(sorted(kw.items())))
    if key not in _SCENES:
        torch.manual_seed(0)
        _SCENES[key] = SyntheticScene(H=size, W=size, n_frames=8, device="cuda", opt=default_opt(**SETS[tag], **kw))
    return _SCENES[key]


def _code(m, row=0):
    return m.individual_codes[row].detach() if m.individual_dim else None


def _code_torso(m, row=0):
    return m.individual_codes_torso[row].detach() if m.individual_dim_torso else None


def _np(t):
    return t.detach().cpu().numpy() if t is not None else np.zeros(0, np.float32)


def _maxerr(a, ref):
    return float((a.double() - ref.double()).abs().max()) / (float(ref.double().abs().max()) + 1e-30)


# ------------------------------------------------------------------------------------------------------ inference
@pytest.mark.parametrize("M", [1, 31, 32, 33, 64, 65, 4097])
@pytest.mark.parametrize("mlp", ["f32", "f32x2", "f16"])
@pytest.mark.parametrize("tag", sorted(SETS))
def test_network_forward_off_default_options(po, hiplib, tag, mlp, M):
    from radnerf import fused
    m = _scene(tag, engine="fused", mlp_dtype=mlp).model
    rng = np.random.default_rng(M + 101)
    x = rng.uniform(-0.7, 0.7, (M, 3)).astype(np.float32)
    if M > 10:
        x[3] = (1.5, 0.0, 0.0)
    d = rng.standard_normal((M, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    enc_a = rng.standard_normal((1, 64)).astype(np.float32)
    eye = np.array([[0.25]], np.float32)
    c = _code(m)
    e = torch.from_numpy(eye).cuda() if m.exp_eye else None
    with torch.no_grad():
        sigma, color, amb = fused.network_forward(m, torch.from_numpy(x).cuda(), torch.from_numpy(d).cuda(),
                                                  torch.from_numpy(enc_a).cuda(), c, e)
    sigma, color, amb = sigma.cpu().numpy(), color.cpu().numpy(), amb.cpu().numpy()
    om = po.model_from_module(m)
    es, ec, ea = po.nerf_forward(om, x, d, enc_a, _np(c), eye, mlp_dtype="f16" if mlp == "f16" else "f32")
    if mlp == "f16":
        _close_up_to_rounding_flips(amb, ea, 1e-4)
        _close_up_to_rounding_flips(sigma, es, 1e-3, rel=True)
        _close_up_to_rounding_flips(color, ec, 1e-4)
        return
    np.testing.assert_allclose(amb, ea, rtol=0, atol=2e-5)
    np.testing.assert_allclose(sigma, es, rtol=2e-4, atol=1e-6)
    np.testing.assert_allclose(color, ec, rtol=0, atol=2e-5)
    ref = netref64.Net64(m)
    with torch.no_grad():
        rs, rc, ra = ref.forward(torch.from_numpy(x).cuda(), torch.from_numpy(d).cuda(), torch.from_numpy(enc_a).cuda().double(),
                                 c, e)
    np.testing.assert_allclose(amb, ra.cpu().numpy(), rtol=0, atol=2e-5)
    np.testing.assert_allclose(sigma, rs.cpu().numpy(), rtol=2e-4, atol=1e-6)
    np.testing.assert_allclose(color, rc.cpu().numpy(), rtol=0, atol=2e-5)


def _bias64(m, enc_a, eye, c):
    """The three broadcast-column blocks of the first layers in float64: [W0_amb[:, 32:] @ enc_a | W0_sig[:, 64:] @ eye |
    W0_col[:, 80:] @ c] (zero where the model has no such column)."""
    wa, ws, wc = (net.net[0].weight.detach().double() for net in (m.ambient_net, m.sigma_net, m.color_net))
    amb = enc_a.double() @ wa[:, 32:].t()
    sig = (eye.double().reshape(1, 1) @ ws[:, 64:].t()).expand(enc_a.shape[0], -1) if m.exp_eye else torch.zeros_like(amb)
    col = (c.double().reshape(1, -1) @ wc[:, 80:].t()).expand(enc_a.shape[0], -1) if m.individual_dim else torch.zeros_like(amb)
    return torch.cat([amb, sig, col], -1)


@pytest.mark.parametrize("tag", sorted(SETS))
def test_frame_bias_off_default_options(hiplib, tag):
    import ctypes as C
    import radnerf_hip as hip
    from radnerf import fused
    m = _scene(tag, engine="fused").model
    st = fused._state(m)
    st.refresh()
    g = torch.Generator(device="cuda").manual_seed(7)
    codes = torch.randn(5, 64, device="cuda", generator=g)
    eye = torch.full((1, 1), 0.25, device="cuda")
    c = _code(m)
    want = _bias64(m, codes, eye, c)
    if m.exp_eye:
        assert float(want[:, 64:128].abs().max()) > 0
    st.bias.fill_(float("nan"))
    hip.call("rn_nerf_frame_bias", C.byref(st.nw), hip.ptr(codes[0].contiguous()), hip.ptr(eye), hip.ptr(c), hip.ptr(st.bias), hip.stream())
    got1 = st.bias[:192].clone()
    got = fused.frame_bias_batch(m, codes, eye, c)
    scale = max(1.0, float(want.abs().max()))
    assert torch.isfinite(got1).all() and float((got1.double() - want[0]).abs().max()) <= 2e-6 * scale
    assert torch.isfinite(got).all() and float((got[:, :192].double() - want).abs().max()) <= 2e-6 * scale
    if not m.exp_eye:
        assert float(got[:, 64:128].abs().max()) == 0.0
    if not m.individual_dim:
        assert float(got[:, 128:192].abs().max()) == 0.0


@pytest.mark.parametrize("engine", ["fused", "fused-f32x2"])
@pytest.mark.parametrize("tag", sorted(SETS))
def test_fused_frame_off_default_options(po, hiplib, tag, engine):
    mlp = "f32x2" if engine == "fused-f32x2" else "f32"
    scene = _scene(tag, 32, engine="fused", mlp_dtype=mlp)
    m = scene.model
    assert m.torso
    f = scene.frame(0)
    with torch.no_grad():
        out = scene.render(0)
    om = po.model_from_module(m)
    rc = po.render_cfg_from_module(m, scene.opt.dt_gamma, scene.opt.max_steps)
    img, dep, stats = po.render_frame(om, rc, _np(f["rays_o"]), _np(f["rays_d"]), _np(m.enc_a), _np(_code(m)), _np(f["eye"]),
                                      _np(f["bg_coords"]), _np(f["poses"]), _np(_code_torso(m)), _np(f["bg_color"]).reshape(-1, 3))
    st = m.last_stats
    assert st["iterations"] == stats["iterations"] and st["live_samples"] == stats["live_samples"]
    assert stats["live_samples"] > 0 and stats["torso_pixels"] > 0
    got = out["image"].reshape(-1, 3).cpu().numpy()
    assert np.abs(got - img).max() <= 2e-3, np.abs(got - img).max()


@pytest.mark.parametrize("ind_dim_torso", [0, 3, 8])
def test_torso_kernel_code_widths(po, hiplib, ind_dim_torso):
    import torch.nn.functional as F
    from radnerf import fused
    scene = _scene("default", 32, engine="fused", ind_dim_torso=ind_dim_torso)
    m = scene.model
    assert m.individual_dim_torso == ind_dim_torso
    f = scene.frame(0)
    N = 32 * 32
    bg_coords = f["bg_coords"].reshape(-1, 2).contiguous()
    poses = f["poses"].reshape(-1).contiguous()
    ct = _code_torso(m)
    bg_in = torch.rand(N, 3, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    deform = torch.empty(N, 2, device="cuda")
    thresh = min(m.density_thresh_torso, m.mean_density_torso)
    bg_out, alpha = fused.torso_forward(m, bg_coords, poses, ct, thresh, bg_in=bg_in, deform_out=deform)
    occ = F.grid_sample(m.density_grid_torso.view(1, 1, 128, 128), bg_coords.view(1, -1, 1, 2), align_corners=True).view(-1)
    mask = (occ > thresh).cpu().numpy()
    assert mask.sum() > 100
    ea, ec, edx = po.torso_forward(po.model_from_module(m), bg_coords.cpu().numpy()[mask], poses.cpu().numpy(), _np(ct))
    ga, gd = alpha.reshape(-1).cpu().numpy(), deform.cpu().numpy()
    np.testing.assert_allclose(gd[mask], edx, rtol=0, atol=3e-5)
    np.testing.assert_allclose(ga[mask], ea[:, 0], rtol=0, atol=3e-5)
    exp_bg = bg_in.cpu().numpy().copy()
    exp_bg[mask] = ec * ea + exp_bg[mask] * (1 - ea)
    np.testing.assert_allclose(bg_out.cpu().numpy(), exp_bg, rtol=0, atol=5e-5)
    with torch.no_grad():
        ra, rc, rdx = netref64.Net64(m).forward_torso(bg_coords[torch.from_numpy(mask).cuda()], poses, ct)
    np.testing.assert_allclose(gd[mask], rdx.cpu().numpy(), rtol=0, atol=3e-5)
    np.testing.assert_allclose(ga[mask], ra[:, 0].cpu().numpy(), rtol=0, atol=3e-5)


# ----------------------------------------------------------------------------------------------- training head
def _train_scene(tag):
    return _scene(tag, 32, engine="ops", torso=False, smooth_lips=False)


def _stable_batch(m, M, seed, monkeypatch):
    """M samples at which the network is smooth in its parameters (_stable_samples), the first 7 outside [-bound, bound]."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    pool = 3 * M + 512
    xyzs = (torch.rand(pool, 3, device="cuda", generator=g) * 2 - 1) * 0.98
    xyzs[:7] = 1.25
    dirs = torch.nn.functional.normalize(torch.randn(pool, 3, device="cuda", generator=g), dim=-1)
    enc_a = torch.randn(1, 64, device="cuda", generator=g) * 0.5
    eye = torch.full((1, 1), 0.25, device="cuda")
    stable = _stable_samples(m, xyzs, dirs, enc_a, eye if m.exp_eye else None, _code(m), monkeypatch)
    idx = torch.nonzero(stable).reshape(-1)[:M]
    assert idx.numel() == M
    up = [torch.randn(M, device="cuda", generator=g), torch.randn(M, 3, device="cuda", generator=g),
          torch.randn(M, device="cuda", generator=g) * 0.3, torch.randn(M, 2, device="cuda", generator=g) * 0.3]
    return xyzs[idx].contiguous(), dirs[idx].contiguous(), enc_a, eye, up


def _loss(sigma, rgb, amb, up):
    return (sigma * up[0]).sum() + (rgb * up[1]).sum() + (amb.abs().sum(-1) * up[2]).sum() + (amb * up[3]).sum()


def _run_head(m, xyzs, dirs, enc_a, eye, up, mode, monkeypatch, row=False):
    monkeypatch.setenv("RN_TRAIN_HEAD", mode)
    for p in m.parameters():
        p.grad = None
    enc_a = enc_a.clone().requires_grad_(True)
    eye = eye.clone().requires_grad_(True) if m.exp_eye else None
    if row:
        from radnerf import train_head
        idx = torch.tensor([0], dtype=torch.int64, device="cuda")
        sigma, rgb, amb, _ = train_head.head_forward(m, xyzs, dirs, enc_a, None, eye, ind_index=idx)
    else:
        sigma, rgb, amb = m(xyzs, dirs, enc_a, m.individual_codes[0] if m.individual_dim else None, eye)
    _loss(sigma, rgb, amb, [u.to(sigma.dtype) for u in up]).backward()
    grads = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    grads["enc_a"] = enc_a.grad.clone()
    if eye is not None:
        grads["eye"] = eye.grad.clone()
    return (sigma.detach(), rgb.detach(), amb.detach()), grads


def _run_ref64(m, xyzs, dirs, enc_a, eye, up):
    ref = netref64.Net64(m)
    enc_a = enc_a.double().clone().requires_grad_(True)
    eye = eye.double().clone().requires_grad_(True) if m.exp_eye else None
    c = ref.P["individual_codes"][0] if m.individual_dim else None
    sigma, rgb, amb = ref.forward(xyzs, dirs, enc_a, c, eye)
    leaves = dict(ref.P)
    leaves["enc_a"] = enc_a
    if eye is not None:
        leaves["eye"] = eye
    names = [n for n in leaves if n.split(".")[0] in ("encoder", "encoder_ambient", "ambient_net", "sigma_net", "color_net", "enc_a", "eye")
             or n == "individual_codes" and c is not None]
    gs = torch.autograd.grad(_loss(sigma, rgb, amb, [u.double() for u in up]), [leaves[n] for n in names])
    return (sigma.detach(), rgb.detach(), amb.detach()), dict(zip(names, gs))


RATIOS = {}


@pytest.mark.parametrize("M", [1, 31, 32, 33, 255, 256, 257, 4099, 100003])
@pytest.mark.parametrize("tag", sorted(SETS))
def test_fused_head_against_float64(hiplib, monkeypatch, tag, M):
    """Outputs and every gradient of the fused head against netref64 on smooth samples; each gradient tensor's max-normalised
    error e_fused <= 4 e_ops + 1e-6 (e_ops: the per-operator path in the reference's own torch formulation) and < 2e-3.  For
    the sets with an individual code also the row-indexed form (the code picked on the device)."""
    monkeypatch.setenv("RN_MLP_TRAIN", "torch")
    monkeypatch.setenv("RN_TRAIN_GLUE", "torch")
    m = _train_scene(tag).model
    m.train()
    xyzs, dirs, enc_a, eye, up = _stable_batch(m, M, 1000 + M, monkeypatch)
    out64, g64 = _run_ref64(m, xyzs, dirs, enc_a, eye, up)
    _, g_ops = _run_head(m, xyzs, dirs, enc_a, eye, up, "ops", monkeypatch)
    forms = [False] + ([True] if m.individual_dim else [])
    for row in forms:
        out, g = _run_head(m, xyzs, dirs, enc_a, eye, up, "fused", monkeypatch, row=row)
        np.testing.assert_allclose(out[0].cpu().numpy(), out64[0].cpu().numpy(), rtol=2e-4, atol=1e-6)
        np.testing.assert_allclose(out[1].cpu().numpy(), out64[1].cpu().numpy(), rtol=0, atol=2e-5)
        np.testing.assert_allclose(out[2].cpu().numpy(), out64[2].cpu().numpy(), rtol=0, atol=2e-5)
        assert set(g) == set(g_ops) == set(g64), (set(g) ^ set(g64))
        for name in sorted(g64):
            assert g[name].shape == g64[name].shape, name
            assert torch.isfinite(g[name]).all(), name
            e_f, e_o = _maxerr(g[name], g64[name]), _maxerr(g_ops[name], g64[name])
            RATIOS[(tag, M, row, name)] = (e_f, e_o)
            assert e_f <= 4 * e_o + 1e-6, (name, e_f, e_o)
            # the absolute bar holds wherever the reference's own fp32 formulation meets it; upstream of the 2-D grid (ambient_net,
            # enc_a) at M >= 257 it does not (measured e_ops up to 2.4e-2 at M = 100003: each contribution carries the ~2047 x
            # table-difference derivative, the contributions cancel in the sum, so fp32 rounding grows with M)
            assert e_f < 2e-3 or e_o >= 2e-3, (name, e_f, e_o)
    worst = max(((v[0] / (v[1] + 1e-12), k[3], v) for k, v in RATIOS.items() if k[0] == tag and k[1] == M), key=lambda t: t[0])
    print(f"{tag} M={M}: worst e_fused/e_ops = {worst[0]:.2f} ({worst[1]}: e_fused {worst[2][0]:.2e}, e_ops {worst[2][1]:.2e})")


@pytest.mark.parametrize("live", [0, 1, 31, 32, 33, 4096])
@pytest.mark.parametrize("tag", sorted(SETS))
def test_fused_head_live_counts(hiplib, monkeypatch, tag, live):
    """Rows past the device-side live count are untouched and contribute nothing: outputs and gradients equal a run on the
    first `live` rows; with live = 0 every gradient is exactly zero (tables included) and equals the host M == 0 path."""
    monkeypatch.setenv("RN_TRAIN_HEAD_ZERO", "1")
    from radnerf import train_head
    m = _train_scene(tag).model
    m.train()
    M = 4096
    g = torch.Generator(device="cuda").manual_seed(17)
    xyzs = (torch.rand(M, 3, device="cuda", generator=g) * 2 - 1) * 0.98
    dirs = torch.nn.functional.normalize(torch.randn(M, 3, device="cuda", generator=g), dim=-1)
    enc_a = torch.randn(1, 64, device="cuda", generator=g) * 0.5
    eye = torch.full((1, 1), 0.25, device="cuda") if m.exp_eye else None
    ind = m.individual_codes[0] if m.individual_dim else None

    def run(x, d, m_dev):
        for p in m.parameters():
            p.grad = None
        s, c, a, aa = train_head.head_forward(m, x, d, enc_a, ind, eye, m_dev=m_dev)
        ((s[:live] ** 2).sum() + (c[:live] ** 2).sum() + aa[:live].sum() + a[:live].sum()).backward()
        grads = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
        return (s.detach().clone(), c.detach().clone(), a.detach().clone()), grads

    cnt = torch.tensor([live, 0], dtype=torch.int32, device="cuda")
    out_a, g_a = run(xyzs, dirs, cnt)
    out_b, g_b = run(xyzs[:live].contiguous(), dirs[:live].contiguous(), None)
    for a, b in zip(out_a, out_b):
        assert torch.equal(a[:live], b)
        assert float(a[live:].abs().max()) == 0.0 if live < M else True
    assert g_a.keys() == g_b.keys() and "encoder.embeddings" in g_a and "encoder_ambient.embeddings" in g_a
    for name in g_b:
        assert torch.isfinite(g_a[name]).all(), name
        if live == 0:
            assert float(g_a[name].abs().max()) == 0.0 and float(g_b[name].abs().max()) == 0.0, name
        else:
            scale = float(g_b[name].abs().max()) + 1e-12
            assert float((g_a[name] - g_b[name]).abs().max()) / scale < 1e-4, name


@pytest.mark.parametrize("tag", sorted(SETS))
def test_fused_head_with_no_samples(hiplib, tag):
    """The host M == 0 path: empty outputs, every gradient exactly zero and of its parameter's shape."""
    from radnerf import train_head
    m = _train_scene(tag).model
    m.train()
    for p in m.parameters():
        p.grad = None
    x = torch.empty(0, 3, device="cuda")
    enc_a = (torch.randn(1, 64, device="cuda") * 0.5).requires_grad_(True)
    eye = torch.full((1, 1), 0.25, device="cuda").requires_grad_(True) if m.exp_eye else None
    s, c, a, aa = train_head.head_forward(m, x, x, enc_a, _code(m) if m.individual_dim else None, eye)
    assert s.shape == (0,) and c.shape == (0, 3) and a.shape == (0, 2)
    (s.sum() + c.sum() + a.sum() + aa.sum()).backward()
    got = {n: p.grad for n, p in m.named_parameters() if p.grad is not None}
    assert {"encoder.embeddings", "encoder_ambient.embeddings", "sigma_net.net.0.weight", "color_net.net.0.weight"} <= set(got)
    for name, gr in list(got.items()) + [("enc_a", enc_a.grad)] + ([("eye", eye.grad)] if eye is not None else []):
        assert gr is not None and torch.isfinite(gr).all() and float(gr.abs().max()) == 0.0, name


# ------------------------------------------------------------------------------------------------- training steps
def _train_losses(monkeypatch, tag, head, steps=6):
    from radnerf.scene import SyntheticScene, default_opt
    from radnerf.train import SyntheticTrainStream, Trainer
    monkeypatch.setenv("RN_TRAIN_HEAD", head)
    monkeypatch.setenv("RN_TRAIN_LOSS", "fused" if head == "fused" else "torch")
    torch.manual_seed(0)
    scene = SyntheticScene(H=64, W=64, n_frames=8, device="cuda", opt=default_opt(engine="ops", torso=False, smooth_lips=False, **SETS[tag]))
    stream = SyntheticTrainStream(scene, n_rays=1024, seed=4)
    trainer = Trainer(scene.model, scene.opt, update_extra_interval=0)
    scene.model.mean_count = 0
    import random
    random.seed(0)
    losses = [float(trainer.step(stream.batch())) for _ in range(steps)]
    return losses, {n: p.detach().clone() for n, p in scene.model.named_parameters()}


@pytest.mark.parametrize("tag", sorted(cases.OPTION_SETS))
def test_training_steps_equal_the_operator_path_off_default_options(hiplib, monkeypatch, tag):
    """test_gpu_train_head.py::test_training_steps_equal_the_operator_path at the option sets A and B, same bars."""
    l_ops, p_ops = _train_losses(monkeypatch, tag, "ops")
    l_fused, p_fused = _train_losses(monkeypatch, tag, "fused")
    assert np.allclose(l_fused, l_ops, rtol=2e-4, atol=1e-7), (l_fused, l_ops)
    for name in p_ops:
        assert torch.isfinite(p_fused[name]).all(), name
        assert float((p_fused[name] - p_ops[name]).abs().max()) <= 2 * 6 * 5e-3 + 1e-6, name


def test_graphed_trainer_without_eye_or_codes(hiplib):
    """GraphedTrainer (the step captured in a hipGraph and replayed) at option set A: the replays run and the model learns."""
    from radnerf.scene import SyntheticScene, default_opt
    from radnerf.train import GraphedTrainer, SyntheticTrainStream, train_step
    torch.manual_seed(0)
    scene = SyntheticScene(H=64, W=64, n_frames=8, device="cuda", opt=default_opt(engine="ops", torso=False, smooth_lips=False, **SETS["A"]))
    stream = SyntheticTrainStream(scene, n_rays=2048)
    m = scene.model
    assert not m.exp_eye and m.individual_dim == 0
    with torch.no_grad():
        m.color_net.net[-1].weight.add_(0.5 * torch.randn_like(m.color_net.net[-1].weight))
    trainer = GraphedTrainer(m, scene.opt, lr_net=5e-3, update_extra_interval=0)
    probe = stream.batch()

    def mse():
        m.train()
        with torch.no_grad():
            pred, rgb, _ = train_step(m, probe, scene.opt)
        return float(((pred - rgb) ** 2).mean())
    before = mse()
    losses = [float(trainer.step(stream.batch())) for _ in range(4)]
    m.mean_count = int(m.step_counter[:4, 0].float().mean().item() * 1.2)
    losses += [float(trainer.step(stream.batch())) for _ in range(20)]
    after = mse()
    assert trainer.replays == 20 and trainer.captures == 1
    assert all(np.isfinite(losses)) and after < 0.7 * before, (before, after)
    for name, p in m.named_parameters():
        assert torch.isfinite(p).all(), name


# --------------------------------------------------------------------------------------------------------- golden
@pytest.mark.parametrize("head", ["fused", "ops"])
@pytest.mark.parametrize("tag", sorted(cases.OPTION_SETS))
def test_head_reproduces_reference_options(hiplib, monkeypatch, tag, head):
    """tests/golden/reference_options.npz (the unmodified reference at the option set): outputs and smooth-sample gradients at
    the bars of test_golden_frames.py::test_hip_train_branch_gradients_on_smooth_samples."""
    import hashlib
    gold = np.load(os.path.join(HERE, "golden", "reference_options.npz"), allow_pickle=False)
    scene = _scene(tag, 32, engine="ops")
    m = scene.model
    params = dict(m.named_parameters())
    flat = np.concatenate([params[n].detach().cpu().numpy().reshape(-1) for n in sorted(params)])
    assert hashlib.sha256(np.ascontiguousarray(flat).tobytes()).hexdigest() == str(gold[f"{tag}_params_sha256"])
    m.train()
    t = {k: torch.from_numpy(gold[k]).cuda() for k in ("x", "d", "enc_a", "eye", "up_sigma", "up_rgb", "up_ambient")}
    mask = torch.from_numpy(gold[f"{tag}_mask"]).cuda().float()
    monkeypatch.setenv("RN_TRAIN_HEAD", head)
    for p in m.parameters():
        p.grad = None
    enc_a = t["enc_a"].clone().requires_grad_(True)
    eye = t["eye"].clone().requires_grad_(True) if m.exp_eye else None
    sigma, rgb, amb = m(t["x"], t["d"], enc_a, m.individual_codes[0] if m.individual_dim else None, eye)
    loss = (sigma * t["up_sigma"] * mask).sum() + (rgb * t["up_rgb"] * mask[:, None]).sum() + (amb * t["up_ambient"] * mask[:, None]).sum()
    loss.backward()
    n = lambda v: v.detach().float().cpu().numpy()  # noqa: E731
    for name, got in (("sigma", sigma), ("rgb", rgb), ("ambient", amb)):
        want = gold[f"{tag}_{name}"]
        assert np.abs(n(got) - want).max() <= {"sigma": 2e-5, "rgb": 2e-6, "ambient": 2e-7}[name] * max(1.0, float(np.abs(want).max())), name
    worst = {}
    for key in gold.files:
        if key.startswith(f"{tag}_grad::"):
            name = key.split("::")[1]
            got = {"enc_a": enc_a.grad, "eye": eye.grad if eye is not None else None}.get(name)
            got = n(got) if got is not None else n(params[name].grad if name != "individual_codes" else params[name].grad[:1])
            want = gold[key]
            worst[name] = float(np.abs(got - want).max() / (np.abs(want).max() + 1e-30))
    for name in ("encoder", "encoder_ambient"):
        gt = getattr(m, name).embeddings.grad
        rows = torch.from_numpy(gold[f"{tag}_gradrows::{name}"]).long().cuda()
        want = gold[f"{tag}_gradvals::{name}"]
        worst[name] = float(np.abs(n(gt[rows]) - want).max() / np.abs(want).max())
        s, sa, nz = gold[f"{tag}_gradsum::{name}"]
        assert abs(float(gt.double().abs().sum()) - sa) <= 2e-3 * sa
        assert abs(float((gt.abs().sum(1) > 0).sum()) - nz) <= 0.002 * nz + 2
    print(f"{tag}/{head}: smooth-sample gradients, max |d| / max |ref|:", {k: f"{v:.1e}" for k, v in worst.items()})
    # upstream of the 2-D grid the fused kernel's own ambient rounding is magnified like the reference's (measured: 1.4e-4 for
    # ambient_net at set B, where float64 itself is 1.6e-3 from the reference -- test_oracle_options.py); everything else 1e-4
    upstream = {k: v for k, v in worst.items() if k.startswith("ambient_net") or k == "enc_a"}
    assert max(upstream.values()) <= 2e-4, upstream
    assert max(v for k, v in worst.items() if k not in upstream) <= 1e-4, worst
