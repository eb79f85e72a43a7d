"""Gradients of the sample positions and directions through the fused training head (rn_train_head_input_grads, csrc/rn_train_head.hip)
-- what --train_camera needs: the rays carry the gradient of camera_dR / camera_dT (nerf/renderer.py:104-107, 170-174) -- against
the float64 restatement tests/netref64.py and the per-operator path (RN_TRAIN_HEAD=ops: grid / SH operators with their dy_dx
backward under torch.autograd), per sample, with a device-side live count, through the renderer's three marchers and through
eight optimizer steps.  Every test asserts that the fused kernels ran (names counted at radnerf_hip.call)."""
import collections
import os

import numpy as np
import pytest
import torch

import netref64
from test_gpu_options import SETS, _loss, _maxerr, _scene, _stable_batch, _train_scene
from test_gpu_train_head import _stable_samples

import cases  # noqa: E402  (tests/golden, put on the path by test_gpu_options)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = "rn_train_head_input_grads"
# Cell margin of the smooth-sample mask in the renderer test, in normalised ambient coordinates.  _stable_samples' default 2e-5
# keeps 54.3 % of this scene's 19 447 live samples by the cell rule and 91.0 % by the ReLU rule: 49.5 % together, short of the half
# the test must keep.  The margin only has to exceed the disagreement of the two paths in that coordinate: the ambient outputs
# agree to 2e-7 (the bar of test_golden_frames.py::test_hip_train_branch_gradients_on_smooth_samples), the coordinate
# (ambient + 1) / 2 to 1e-7; 1e-5 is a hundred times that, and keeps more samples near cell boundaries IN the comparison.
CELL_MARGIN = 1e-5
HASH19 = dict(xyz_grid="hashgrid", xyz_log2_hashmap_size=19)


def _count_calls(monkeypatch):
    """Counter of the C entry points called from here on (radnerf_hip.call is the one door to the library)."""
    import radnerf_hip as hip
    calls = collections.Counter()
    inner = hip.call

    def call(name, *a):
        calls[name] += 1
        return inner(name, *a)
    monkeypatch.setattr(hip, "call", call)
    return calls


def _record_scatter(monkeypatch):
    """Copies of what train_head.grid_scatter is handed from here on: per call [(feature gradients [16, M, 2], coordinates [M, D],
    encoder), ...] for the two grids."""
    from radnerf import train_head
    seen = []
    inner = train_head.grid_scatter

    def grid_scatter(jobs, M, m_dev):
        seen.append([(j[0].clone(), j[1].clone(), j[2]) for j in jobs])
        return inner(jobs, M, m_dev)
    monkeypatch.setattr(train_head, "grid_scatter", grid_scatter)
    return seen, inner


def _run(m, xyzs, dirs, enc_a, eye, up, mode, monkeypatch, input_grads):
    """NeRFNetwork.forward + backward of _loss; -> (outputs, parameter / enc_a / eye gradients, d loss / d xyzs, d loss / d dirs)."""
    monkeypatch.setenv("RN_TRAIN_HEAD", mode)
    for p in m.parameters():
        p.grad = None
    x = xyzs.clone().requires_grad_(input_grads)
    d = dirs.clone().requires_grad_(input_grads)
    enc_a = enc_a.clone().requires_grad_(True)
    eye = eye.clone().requires_grad_(True) if m.exp_eye else None
    sigma, rgb, amb = m(x, d, enc_a, m.individual_codes[0] if m.individual_dim else None, eye)
    _loss(sigma, rgb, amb, up).backward()
    grads = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    grads["enc_a"] = enc_a.grad.clone()
    if eye is not None:
        grads["eye"] = eye.grad.clone()
    return (sigma.detach(), rgb.detach(), amb.detach()), grads, x.grad, d.grad


def _ref64_input_grads(m, xyzs, dirs, enc_a, eye, ups, row=0):
    """float64 d/d xyzs, d/d dirs of sum(sigma u0) + sum(rgb u1) + sum(|ambient|.sum(-1) u2) + sum(ambient u3) (None = absent)."""
    ref = netref64.Net64(m)
    x = xyzs.detach().double().requires_grad_(True)
    d = dirs.detach().double().requires_grad_(True)
    c = ref.P["individual_codes"][row] if m.individual_dim else None
    e = eye.detach().double() if (m.exp_eye and eye is not None) else None
    sigma, rgb, amb = ref.forward(x, d, enc_a.detach().double(), c, e)
    terms = [sigma, rgb, amb.abs().sum(-1), amb]
    loss = sum((t * u.double()).sum() for t, u in zip(terms, ups) if u is not None)
    return torch.autograd.grad(loss, [x, d])


# ------------------------------------------------------------------------------------------------- 1. per sample
@pytest.mark.parametrize("grid", ["tiledgrid16", "hashgrid19"])
@pytest.mark.parametrize("M", [1, 31, 32, 33, 257, 4099])
@pytest.mark.parametrize("tag", sorted(SETS))
def test_input_gradients_against_float64(hiplib, monkeypatch, tag, M, grid):
    """d loss / d xyzs and d loss / d dirs of the fused head on smooth samples (the first 7 outside the box) against float64 autograd
    with the fp32 cell choice: max-normalised error e_fused <= 4 e_ops + 1e-6, e_ops the per-operator path's.  Rows outside the
    box: d/d xyzs exactly 0, d/d dirs at the same bar.  Every other gradient is bit-equal to a fused run whose inputs do not
    require grad -- with one mended step for the two TABLE gradients: their scatter adds with float atomics, so two identical
    runs of the parent commit already differ in them (measured, default scene, three repeats each: 11 -- 27 entries of the
    ambient table at M = 31, 8 -- 19 / 270 -- 358 entries of the xyz / ambient table at M = 257, 2063 -- 2734 / 1399 -- 2657 at
    M = 4099, with the scatter on the side stream or not).  What is compared bit for bit instead is everything the scatter is
    handed (feature gradients and coordinates of both grids), which fixes the table gradients up to the order of the sums; the
    tables themselves must agree within that order's rounding, row by row: (addends - 1) <= 8 M - 1 times 2^-24 times the
    sum of |addend|, for both orders (the sum of |addend| comes from the same scatter run on |feature gradients|)."""
    monkeypatch.setenv("RN_MLP_TRAIN", "torch")
    monkeypatch.setenv("RN_TRAIN_GLUE", "torch")
    m = (_train_scene(tag) if grid == "tiledgrid16" else _scene(tag, 32, engine="ops", torso=False, smooth_lips=False, **HASH19)).model
    m.train()
    assert (m.encoder.gridtype == "hash") == (grid == "hashgrid19")
    xyzs, dirs, enc_a, eye, up = _stable_batch(m, M, 2000 + M, monkeypatch)
    gx64, gd64 = _ref64_input_grads(m, xyzs, dirs, enc_a, eye, [up[0], up[1], up[2], up[3]])
    _, _, gx_o, gd_o = _run(m, xyzs, dirs, enc_a, eye, up, "ops", monkeypatch, True)
    calls = _count_calls(monkeypatch)
    scattered, grid_scatter = _record_scatter(monkeypatch)
    out, g, gx_f, gd_f = _run(m, xyzs, dirs, enc_a, eye, up, "fused", monkeypatch, True)
    assert calls["rn_train_head_forward"] == 1 and calls["rn_train_head_backward"] == 1 and calls[NEW] == 1, dict(calls)
    assert calls["rn_grid_encode_backward"] == 0 and calls["rn_sh_encode_backward"] == 0, dict(calls)
    out0, g0, gx_none, gd_none = _run(m, xyzs, dirs, enc_a, eye, up, "fused", monkeypatch, False)
    assert calls[NEW] == 1 and gx_none is None and gd_none is None          # no call when neither input needs a gradient
    assert gx_f is not None and gd_f is not None and gx_f.shape == (M, 3) and gd_f.shape == (M, 3)
    assert torch.isfinite(gx_f).all() and torch.isfinite(gd_f).all()
    oob = (xyzs.abs() > m.bound).any(-1)
    for name, f, o, r in (("xyzs", gx_f, gx_o, gx64), ("dirs", gd_f, gd_o, gd64)):
        e_f, e_o = _maxerr(f, r), _maxerr(o, r)
        print(f"{tag} {grid} M={M} d/d {name}: e_fused {e_f:.3e}  e_ops {e_o:.3e}")
        assert e_f <= 4 * e_o + 1e-6, (name, e_f, e_o)
    if oob.any():
        assert float(gx_f[oob].abs().max()) == 0.0 and float(gx64[oob].abs().max()) == 0.0
        e_f, e_o = _maxerr(gd_f[oob], gd64[oob]), _maxerr(gd_o[oob], gd64[oob])
        print(f"{tag} {grid} M={M} d/d dirs on the {int(oob.sum())} rows outside the box: e_fused {e_f:.3e}  e_ops {e_o:.3e}")
        assert e_f <= 4 * e_o + 1e-6, (e_f, e_o)
    # the feature perturbs nothing that existed
    for a, b in zip(out, out0):
        assert torch.equal(a, b)
    assert set(g) == set(g0) and "encoder.embeddings" in g and "encoder_ambient.embeddings" in g and "enc_a" in g
    tables = {"encoder.embeddings": 0, "encoder_ambient.embeddings": 1}
    for name in sorted(g0):
        if name not in tables:
            assert torch.equal(g[name], g0[name]), name
    assert len(scattered) == 2 and len(scattered[0]) == 2 and len(scattered[1]) == 2
    from radnerf.fused import _grid_desc
    for name, i in tables.items():
        (gf, xn, enc), (gf0, xn0, _) = scattered[0][i], scattered[1][i]
        assert torch.equal(gf, gf0) and torch.equal(xn, xn0), name
        sum_abs = torch.zeros_like(g0[name])
        grid_scatter([(gf.abs(), xn, enc, _grid_desc(enc, enc.embeddings.detach()), sum_abs)], M, None)
        bound = 2 * (8 * M - 1) * 2.0 ** -24 * sum_abs.double()
        assert bool(((g[name].double() - g0[name].double()).abs() <= bound).all()), name


# ------------------------------------------------------------------------------------------------- 2. live count
@pytest.mark.parametrize("live", [0, 1, 31, 32, 33, 4096])
def test_input_gradients_live_count(hiplib, monkeypatch, live):
    """Rows >= the device-side live count of both input gradients are exactly zero (written by the kernel); rows below it match
    a run on the truncated batch to 1e-4 of the largest entry; live = 0: all zero, as on the host M == 0 path."""
    monkeypatch.setenv("RN_TRAIN_HEAD_ZERO", "1")
    monkeypatch.setenv("RN_TRAIN_HEAD", "fused")
    from radnerf import train_head
    m = _train_scene("default").model
    m.train()
    M = 4096
    g = torch.Generator(device="cuda").manual_seed(23)
    xyzs = (torch.rand(M, 3, device="cuda", generator=g) * 2 - 1) * 0.98
    dirs = torch.nn.functional.normalize(torch.randn(M, 3, device="cuda", generator=g), dim=-1)
    enc_a = torch.randn(1, 64, device="cuda", generator=g) * 0.5
    eye = torch.full((1, 1), 0.25, device="cuda")
    ind = m.individual_codes[0]
    calls = _count_calls(monkeypatch)

    def run(x, d, m_dev):
        for p in m.parameters():
            p.grad = None
        x, d = x.clone().requires_grad_(True), d.clone().requires_grad_(True)
        s, c, a, aa = train_head.head_forward(m, x, d, enc_a, ind, eye, m_dev=m_dev)
        ((s[:live] ** 2).sum() + (c[:live] ** 2).sum() + aa[:live].sum() + a[:live].sum()).backward()
        return x.grad, d.grad

    cnt = torch.tensor([live, 0], dtype=torch.int32, device="cuda")
    gx_a, gd_a = run(xyzs, dirs, cnt)
    assert calls[NEW] == 1
    gx_b, gd_b = run(xyzs[:live].contiguous(), dirs[:live].contiguous(), None)
    assert calls[NEW] == (2 if live else 1)                      # M == 0 is answered on the host
    for a, b in ((gx_a, gx_b), (gd_a, gd_b)):
        assert a.shape == (M, 3) and b.shape == (live, 3) and torch.isfinite(a).all() and torch.isfinite(b).all()
        if live < M:
            assert float(a[live:].abs().max()) == 0.0
        if live == 0:
            assert float(a.abs().max()) == 0.0
        else:
            scale = float(b.abs().max())
            assert scale > 0 and float((a[:live] - b).abs().max()) / scale < 1e-4


# ---------------------------------------------------------------------------------------- 3. through the renderer
def _camera_scene():
    from radnerf.scene import SyntheticScene, default_opt
    torch.manual_seed(0)
    return SyntheticScene(H=256, W=256, n_frames=8, device="cuda", opt=default_opt(train_camera=True, torso=False, smooth_lips=False))


def _camera_call(scene, f, px, head, monkeypatch, force_all_rays, masked):
    """One train-branch call of the renderer at index [3] and its backward.  masked: the upstream gradients of the network's
    outputs are restricted to this call's own smooth samples (_stable_samples), and a float64 value of the two camera rows is
    built from the same sample buffers and the same masked upstream gradients: Net64 per-sample gradients, rounded to fp32,
    through the marcher's backward operator and the torch pose code (the call's own autograd graph from the samples up)."""
    m, opt = scene.model, scene.opt
    m.train()
    monkeypatch.setenv("RN_TRAIN_HEAD", head)
    seen = []

    def restrict(xyzs, dirs, enc_a, outs):
        live = int(m.step_counter[0, 0])
        mask = torch.zeros(xyzs.shape[0], dtype=torch.bool, device=xyzs.device)
        if masked:
            n = min(live, xyzs.shape[0])
            mask[:n] = _stable_samples(m, xyzs[:n].detach(), dirs[:n].detach(), enc_a.detach(), f["eye"], m.individual_codes[3].detach(),
                                       monkeypatch, cell_margin=CELL_MARGIN)
            monkeypatch.setenv("RN_TRAIN_HEAD", head)            # _stable_samples switches to the operator path
        rec = dict(xyzs=xyzs, dirs=dirs, enc_a=enc_a, live=live, mask=mask, up={})
        seen.append(rec)
        for i, t in enumerate(outs):
            if masked and t is not None and t.requires_grad:
                def hook(g, i=i):
                    if g is None:                        # an output nobody differentiates (set_materialize_grads(False))
                        return None
                    g = g * mask.to(g.dtype).reshape(-1, *([1] * (g.dim() - 1)))
                    rec["up"][i] = g.detach().clone()
                    return g
                t.register_hook(hook)

    from radnerf.network import _train_head
    th = _train_head()
    inner = th.head_forward

    def head_forward(model, xyzs, dirs, enc_a, *a, **k):
        outs = inner(model, xyzs, dirs, enc_a, *a, **k)
        restrict(xyzs, dirs, enc_a, [outs[0], outs[1], outs[3], outs[2]])        # sigma, rgb, |ambient| sum, ambient
        return outs
    monkeypatch.setattr(th, "head_forward", head_forward)
    # the operator path: (sigma, rgb, ambient); |ambient|.sum(-1) is taken outside, its gradient arrives through ambient's.  The
    # module's own `ambient` also feeds the 2-D grid, so its gradient holds that inner path too: the caller gets views, whose
    # gradients are the upstream ones alone
    def module_hook(mod, args, outs):
        outs = tuple(t.view_as(t) for t in outs)
        restrict(args[0], args[1], args[2], [outs[0], outs[1], None, outs[2]])
        return outs
    hook = m.register_forward_hook(module_hook)
    calls = _count_calls(monkeypatch)
    m.zero_grad(set_to_none=True)
    m.mean_count, m.local_step = (0 if force_all_rays else 49152), 0
    m.step_counter.zero_()
    res = m.render(f["rays_o"][:, px], f["rays_d"][:, px], f["auds"], f["bg_coords"][:, px], f["poses"], eye=f["eye"], index=[3],
                   bg_color=f["bg_color"][:, px], staged=False, perturb=False, force_all_rays=force_all_rays, dt_gamma=opt.dt_gamma,
                   max_steps=opt.max_steps)
    g = cases.rm_inputs(17)
    loss = (res["image"].reshape(-1, 3) * g(4096, 3, lo=-1, hi=1).cuda()).sum() + (res["weights_sum"] * g(4096, lo=-1, hi=1).cuda()).sum() \
        + (res["ambient"] * g(4096, lo=-1, hi=1).cuda()).sum()
    loss.backward(retain_graph=masked)
    hook.remove()
    monkeypatch.setattr(th, "head_forward", inner)
    assert len(seen) == 1, "the network's outputs were not seen exactly once"
    rec = seen[0]
    out = dict(res={k: res[k].detach().clone() for k in ("image", "weights_sum", "ambient", "depth")}, calls=dict(calls), live=rec["live"],
               kept=int(rec["mask"].sum()), dT=m.camera_dT.grad.detach().clone(), dR=m.camera_dR.grad.detach().clone())
    if masked:
        n = rec["live"]
        ups = [rec["up"].get(i) for i in range(4)]
        ups = [None if (u is None or u.numel() == 0) else u[:n] for u in ups]
        gx64, gd64 = _ref64_input_grads(m, rec["xyzs"][:n], rec["dirs"][:n], rec["enc_a"], f["eye"], ups, row=3)
        gx = torch.zeros_like(rec["xyzs"])
        gd = torch.zeros_like(rec["dirs"])
        gx[:n], gd[:n] = gx64.float(), gd64.float()
        out["dT64"], out["dR64"] = (t.detach().clone() for t in torch.autograd.grad([rec["xyzs"], rec["dirs"]], [m.camera_dT, m.camera_dR],
                                                                                   grad_outputs=[gx, gd]))
    return out


@pytest.mark.parametrize("force_all_rays", [False, True])
def test_camera_gradients_through_the_renderer(hiplib, monkeypatch, force_all_rays):
    """run_cuda's train branch with --train_camera on 4096 pixels of a 256 x 256 scene, index [3], the loss of
    test_golden_frames.py::test_hip_train_branch_matches_reference.  The rays carry a gradient, so the marcher's samples do, and
    the fused head now takes the call: camera_dT.grad / camera_dR.grad are non-zero in row 3 and exactly zero elsewhere, the
    outputs equal the operator path's at that test's bars, and on smooth samples the two camera rows meet
    e_fused <= 4 e_ops + 1e-6 against the float64 value of _camera_call.  Printed, not asserted: the unmasked fused-vs-ops
    difference and cosine."""
    scene = _camera_scene()
    m = scene.model
    assert m.train_camera and m.camera_dT.shape[1] == 3
    f = scene.frame(0)                      # the rays of test_hip_train_branch_matches_reference; the call is made as frame index 3
    px = torch.from_numpy(np.load(os.path.join(HERE, "golden", "reference_frames.npz"), allow_pickle=False)["train_px"]).cuda()
    assert px.numel() == 4096
    tag = "force_all_rays" if force_all_rays else "mean_count 49152"
    runs = {(head, masked): _camera_call(scene, f, px, head, monkeypatch, force_all_rays, masked)
            for masked in (True, False) for head in ("ops", "fused")}
    for (head, masked), r in runs.items():
        c = r["calls"]
        if head == "fused":
            assert c.get("rn_train_head_forward") == 1 and c.get("rn_train_head_backward") == 1 and c.get(NEW) == 1, c
            assert c.get("rn_grid_encode_backward", 0) == 0 and c.get("rn_sh_encode_backward", 0) == 0, c
        else:
            assert c.get(NEW, 0) == 0 and c.get("rn_train_head_forward", 0) == 0 and c.get("rn_grid_encode_backward", 0) >= 1, c
        assert c.get("rn_march_rays_train_backward") == 1, c
        for name in ("dT", "dR"):
            gr = r[name]
            assert torch.isfinite(gr).all() and float(gr[3].abs().max()) > 0.0, (head, masked, name)
            rest = gr.clone()
            rest[3] = 0
            assert float(rest.abs().max()) == 0.0, (head, masked, name)
    for masked in (True, False):
        a, b = runs[("fused", masked)], runs[("ops", masked)]
        assert a["live"] == b["live"] and a["live"] > 0
        n = lambda t: t.float().cpu().numpy()  # noqa: E731
        np.testing.assert_allclose(n(a["res"]["weights_sum"]), n(b["res"]["weights_sum"]), rtol=0, atol=2e-6)
        np.testing.assert_allclose(n(a["res"]["ambient"]), n(b["res"]["ambient"]), rtol=0, atol=2e-6)
        np.testing.assert_allclose(n(a["res"]["image"]), n(b["res"]["image"]), rtol=0, atol=2e-6)
        np.testing.assert_allclose(n(a["res"]["depth"]), n(b["res"]["depth"]), rtol=0, atol=2e-4)
    fm, om = runs[("fused", True)], runs[("ops", True)]
    for r in (fm, om):
        print(f"{tag}: smooth mask keeps {r['kept']} of {r['live']} live samples ({r['kept'] / r['live']:.1%})")
        assert 2 * r["kept"] >= r["live"]
    fu, ou = runs[("fused", False)], runs[("ops", False)]
    for name in ("dT", "dR"):
        e_f, e_o = _maxerr(fm[name][3], fm[name + "64"][3]), _maxerr(om[name][3], om[name + "64"][3])
        d = _maxerr(fu[name][3], ou[name][3])
        cos = float(torch.nn.functional.cosine_similarity(fu[name][3].double(), ou[name][3].double(), dim=0))
        print(f"{tag} camera_{name}[3]: smooth samples e_fused {e_f:.3e}  e_ops {e_o:.3e} | unmasked fused vs ops: max-normalised "
              f"difference {d:.3e}, cosine {cos:.8f} | fused {fu[name][3].tolist()}")
        print(f"{tag} camera_{name}[3]: smooth samples, fused vs ops {_maxerr(fm[name][3], om[name][3]):.3e}, their float64 values "
              f"{_maxerr(fm[name + '64'][3], om[name + '64'][3]):.3e} | fused {fm[name][3].tolist()} ops {om[name][3].tolist()} "
              f"float64 {fm[name + '64'][3].tolist()} / {om[name + '64'][3].tolist()}")
        assert e_f <= 4 * e_o + 1e-6, (name, e_f, e_o)


# ----------------------------------------------------------------------------------------------------- 4. trainer
def _camera_training(monkeypatch, head, train_camera, steps=8):
    from radnerf.scene import SyntheticScene, default_opt
    from radnerf.train import SyntheticTrainStream, Trainer
    monkeypatch.setenv("RN_TRAIN_HEAD", head)
    monkeypatch.setenv("RN_TRAIN_LOSS", "fused" if head == "fused" else "torch")
    torch.manual_seed(0)
    scene = SyntheticScene(H=64, W=64, n_frames=8, device="cuda",
                           opt=default_opt(engine="ops", torso=False, smooth_lips=False, train_camera=train_camera))
    stream = SyntheticTrainStream(scene, n_rays=1024, seed=4)
    m = scene.model
    trainer = Trainer(m, scene.opt, update_extra_interval=0)
    m.mean_count = 0
    import random
    random.seed(0)
    calls = _count_calls(monkeypatch)
    losses, per_step = [], []
    for i in range(steps):
        if i == steps // 2:      # second half: the running-average budget, i.e. the one-launch marcher with buffers that are not zeroed
            m.mean_count = int(m.step_counter[:steps // 2, 0].float().mean().item() * 1.2)
            assert m.mean_count > 0
        before = collections.Counter(calls)
        losses.append(float(trainer.step(stream.batch())))
        per_step.append(collections.Counter(calls) - before)
    cam = (m.camera_dT.detach().clone(), m.camera_dR.detach().clone()) if train_camera else None
    return losses, per_step, cam, stream.frame


def test_camera_training_steps_equal_the_operator_path(hiplib, monkeypatch):
    """Eight eager optimizer steps with --train_camera (four of the first window, four with the sample budget on the device):
    the fused steps follow the per-operator steps in their losses (rtol 2e-4, atol 1e-7), the frame's camera row has moved and is
    finite in both, and every fused step called rn_train_head_input_grads exactly once and no operator backward of the encoders."""
    l_ops, s_ops, cam_ops, frame = _camera_training(monkeypatch, "ops", True)
    l_fused, s_fused, cam_fused, _ = _camera_training(monkeypatch, "fused", True)
    print("losses fused", l_fused, "\nlosses ops  ", l_ops)
    for i, c in enumerate(s_fused):
        assert c[NEW] == 1 and c["rn_train_head_forward"] == 1 and c["rn_train_head_backward"] == 1, (i, dict(c))
        assert c["rn_grid_encode_backward"] == 0 and c["rn_sh_encode_backward"] == 0, (i, dict(c))
        assert c["rn_march_rays_train_backward"] == 1, (i, dict(c))
    assert any(c["rn_march_rays_train_step"] == 1 for c in s_fused[4:]), [dict(c) for c in s_fused[4:]]
    for c in s_ops:
        assert c[NEW] == 0 and c["rn_grid_encode_backward"] >= 1
    assert np.allclose(l_fused, l_ops, rtol=2e-4, atol=1e-7), (l_fused, l_ops)
    for dT, dR in (cam_ops, cam_fused):
        assert torch.isfinite(dT).all() and torch.isfinite(dR).all()
        assert float(dT[frame].abs().max()) > 0.0 and float(dR[frame].abs().max()) > 0.0
        rest = dT.clone()
        rest[frame] = 0
        assert float(rest.abs().max()) == 0.0
    print("camera_dT[frame] fused", cam_fused[0][frame].tolist(), "ops", cam_ops[0][frame].tolist())


def test_training_without_train_camera_never_calls_the_new_entry_point(hiplib, monkeypatch):
    losses, per_step, _, _ = _camera_training(monkeypatch, "fused", False)
    assert all(np.isfinite(losses))
    for c in per_step:
        assert c[NEW] == 0 and c["rn_train_head_forward"] == 1 and c["rn_march_rays_train_backward"] == 0, dict(c)
