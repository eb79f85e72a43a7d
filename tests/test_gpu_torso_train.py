"""The fused training kernels of the torso layer (csrc/rn_train_torso.hip, radnerf/train_torso.py; RN_TORSO_TRAIN=fused) held to
what pins the per-operator path in test_gpu_torso.py: the float64 restatement netref64.Net64.forward_torso is the truth, the
per-operator path with RN_MLP_TRAIN=torch the yardstick, and the bar the project's own (test_gpu_torso._compare):
e_fused <= 4 e_torch + 1e-6, and e_fused < 2e-3 wherever e_torch is.

Sizes are the smallest at which a kernel on 32-pixel tiles can go wrong: around one and two tiles, 1057 = 33 tiles + 1 (more than
one workgroup, a ragged last tile), and the same with the launch capped at one and at two workgroups (RN_TORSO_TRAIN_BLOCKS), so
that every wave walks the grid-stride loop.  A case's pixels, float64 truth and yardstick run are computed once and shared."""
import numpy as np
import pytest
import torch

import netref64
from test_gpu_torso import (CLAMP_K, _code, _collect, _compare, _gen, _grad_names, _occupancy, _pixels, _poses, _quadrants,
                            _scaled_deform, _smooth_batch, _spy, _torso_loss, _train_scene)

pytestmark = pytest.mark.gpu

ROW = 3
PAD = 64
ENTRIES = ["rn_train_torso_pack", "rn_train_torso_forward", "rn_train_torso_backward", "rn_train_torso_weight_grads",
           "rn_grid_scatter_jobs"]
_CASES = {}


def _env(monkeypatch, fused, blocks=None, mlp=None):
    for name, value in (("RN_TORSO_TRAIN", "fused" if fused else None), ("RN_TORSO_TRAIN_BLOCKS", blocks), ("RN_MLP_TRAIN", mlp)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(value))


def _step(m, names, ind, xy, poses, up):
    """One forward + backward of forward_torso -> ({gradients, out:*}, the C entry points it called)."""
    for p in m.parameters():
        p.grad = None
    with _spy() as called:
        out = m.forward_torso(xy, poses, None, m.individual_codes_torso[ROW] if ind else None)
        _torso_loss(*out, up).backward()
    return dict(_collect(m, names, ROW), **{f"out:{k}": v.detach() for k, v in zip(("alpha", "color", "dx"), out)}), called


def _case(monkeypatch, ind, P, clamp):
    """P smooth pixels, upstream gradients, the float64 outputs and gradients and the yardstick run (per-operator path,
    RN_MLP_TRAIN=torch) of one case -- computed once."""
    key = (ind, P, clamp)
    if key not in _CASES:
        scene = _train_scene(ind)
        m, poses = scene.model, _poses(scene)
        names = _grad_names(m)
        with _scaled_deform(m, CLAMP_K[ind] if clamp else 1.0):
            xy, gen = _smooth_batch(m, P, 7000 + P + ind, poses, _code(m, ROW))
            up = [torch.randn(P, 1, device="cuda", generator=gen), torch.randn(P, 3, device="cuda", generator=gen),
                  torch.randn(P, 2, device="cuda", generator=gen)]
            ref = netref64.Net64(m)
            out64 = ref.forward_torso(xy, poses, ref.P["individual_codes_torso"][ROW] if ind else None)
            g64 = dict(zip(names, torch.autograd.grad(_torso_loss(*out64, [u.double() for u in up]), [ref.P[n] for n in names])))
            if ind:
                g64["individual_codes_torso"] = g64["individual_codes_torso"][ROW]
            if clamp:
                un = xy.double() * float(np.float32(m.opt.torso_shrink)) + out64[2].detach()
                share = float((un.abs() > 1).any(1).double().mean())
                print(f"torso train clamp ind={ind}: float64 clamps {100 * share:.1f} % of {P} pixels")
                assert 0.10 <= share <= 0.90, share
            g64.update({f"out:{k}": v.detach() for k, v in zip(("alpha", "color", "dx"), out64)})
            _env(monkeypatch, fused=False, mlp="torch")
            g_torch, called = _step(m, names, ind, xy, poses, up)
            assert not [c for c in called if c.startswith(("rn_mlp64_", "rn_train_torso_"))], called
        _CASES[key] = dict(xy=xy, up=up, g64=g64, g_torch=g_torch)
    return _CASES[key]


GRAD_CASES = [(8, n, False, None) for n in (1, 31, 32, 33, 64, 65, 1057)] + [(3, 33, False, None), (0, 33, False, None)] + \
             [(i, 65, True, None) for i in (8, 3, 0)] + [(8, 1057, False, 1), (8, 1057, False, 2)]


@pytest.mark.parametrize("ind,P,clamp,blocks", GRAD_CASES)
def test_fused_torso_gradients_against_float64(hiplib, monkeypatch, ind, P, clamp, blocks):
    """Outputs, all seven parameter gradients and the picked code row.  blocks: the launch capped at that many workgroups of four
    waves (33 tiles: up to nine rounds of the grid-stride loop per wave)."""
    case = _case(monkeypatch, ind, P, clamp)
    scene = _train_scene(ind)
    m, poses = scene.model, _poses(scene)
    names = _grad_names(m)
    with _scaled_deform(m, CLAMP_K[ind] if clamp else 1.0):
        _env(monkeypatch, fused=True, blocks=blocks)
        g_fused, called = _step(m, names, ind, case["xy"], poses, case["up"])
    assert sorted(called) == sorted(ENTRIES), called
    worst = _compare(g_fused, case["g_torch"], case["g64"], f"fused ind={ind} P={P} clamp={clamp} blocks={blocks}")
    print(f"torso train ind={ind} P={P} clamp={clamp} blocks={blocks}: worst e_fused / e_torch = {worst:.2f}")


def test_dispatch(hiplib, monkeypatch):
    """RN_TORSO_TRAIN=fused: each of the five entries once and nothing of the per-operator path; unset, under autocast, under
    no_grad and with a half table: the per-operator path."""
    scene = _train_scene(8)
    m, poses = scene.model, _poses(scene)
    names = _grad_names(m)
    case = _case(monkeypatch, 8, 65, False)
    xy, up = case["xy"], case["up"]
    per_op = ("rn_mlp64_", "rn_grid_encode", "rn_freq_encode")
    _env(monkeypatch, fused=True)
    _, called = _step(m, names, 8, xy, poses, up)
    for name in ENTRIES:
        assert called.count(name) == 1, (name, called)
    assert not [c for c in called if c.startswith(per_op)], called
    _env(monkeypatch, fused=False)
    _, called = _step(m, names, 8, xy, poses, up)
    assert not [c for c in called if c.startswith("rn_train_torso_")] and [c for c in called if c.startswith("rn_freq_encode")], called

    _env(monkeypatch, fused=True)
    code = m.individual_codes_torso[ROW]

    def forward_only():
        with _spy() as called:
            m.forward_torso(xy, poses, None, code)
        assert not [c for c in called if c.startswith("rn_train_torso_")], called
        assert [c for c in called if c.startswith("rn_freq_encode")] and [c for c in called if c.startswith("rn_grid_encode")], called
    with torch.autocast("cuda", dtype=torch.float16):
        forward_only()
    with torch.no_grad():
        forward_only()
    emb = m.torso_encoder.embeddings
    keep = emb.data
    try:
        emb.data = keep.half()
        forward_only()
    finally:
        emb.data = keep
    with _spy() as called:                                       # and back on the kernels
        m.forward_torso(xy, poses, None, code)
    assert called == ENTRIES[:2], called


class _Guard:
    """alloc() of radnerf.train_torso: every buffer the kernels write is cut out of a larger one, PAD rows of a marker on either
    side and NaN inside; check() wants the margins back untouched."""

    def __init__(self):
        self.full = []

    def new(self, n, *tail):
        full = torch.full((n + 2 * PAD, *tail), -77.0, dtype=torch.float32, device="cuda")
        view = full[PAD:PAD + n]
        view.fill_(float("nan"))
        self.full.append((full, view))
        return view

    def check(self):
        for full, view in self.full:
            n = view.shape[0]
            assert bool((full[:PAD] == -77.0).all()) and bool((full[PAD + n:] == -77.0).all()), "write outside the buffer"


def test_live_count(hiplib, monkeypatch):
    """Buffers of 97 pixels with a device live count of 65: rows >= 65 of xy are NaN and must never be read; output rows >= 65
    and the margins of every buffer come back untouched; the gradients are those of the first 65 pixels."""
    from radnerf import train_torso
    P, live = 97, 65
    case = _case(monkeypatch, 8, live, False)
    scene = _train_scene(8)
    m, poses = scene.model, _poses(scene)
    names = _grad_names(m)
    xy = torch.full((P, 2), float("nan"), device="cuda")
    xy[:live] = case["xy"]
    p_dev = torch.tensor([live], dtype=torch.int32, device="cuda")
    gd = _Guard()
    _env(monkeypatch, fused=True)
    for p in m.parameters():
        p.grad = None
    with _spy() as called:
        out = train_torso.torso_forward(m, xy, poses, m.individual_codes_torso[ROW], p_dev=p_dev, alloc=gd.new)
        _torso_loss(*[o[:live] for o in out], case["up"]).backward()
    assert sorted(called) == sorted(ENTRIES), called
    gd.check()
    shapes = [tuple(v.shape) for _, v in gd.full]
    assert shapes[:4] == [(P, 1), (P, 3), (P, 2), (P, 2)] and (16 * P, 2) in shapes, shapes
    for _, view in gd.full:
        if view.shape[0] == P:                        # alpha, color, dx, wn
            assert bool(torch.isnan(view[live:]).all()) and bool(torch.isfinite(view[:live]).all())
        elif view.shape[0] == 16 * P:                 # level-major feature gradients
            lv = view.view(16, P, 2)
            assert bool(torch.isnan(lv[:, live:]).all()) and bool(torch.isfinite(lv[:, :live]).all())
        else:                                         # weight and code gradients: every element written
            assert bool(torch.isfinite(view).all()), tuple(view.shape)
    got = dict(_collect(m, names, ROW), **{f"out:{k}": v[:live].detach() for k, v in zip(("alpha", "color", "dx"), out)})
    _compare(got, case["g_torch"], case["g64"], f"live count {live} of {P}")


def test_forward_agrees_with_the_inference_kernel(hiplib, monkeypatch):
    """alpha and dx of the training forward against rn_torso_fused with every pixel covered (thresh = -1): the standing bars of
    test_gpu_torso.py."""
    from radnerf import fused, train_torso
    scene = _train_scene(8)
    m, poses = scene.model, _poses(scene)
    P = 1057
    xy = (torch.rand(P, 2, device="cuda", generator=_gen(31)) * 2 - 1).contiguous()
    code = m.individual_codes_torso[ROW].detach()
    alpha_i, dx_i = torch.empty(P, 1, device="cuda"), torch.empty(P, 2, device="cuda")
    fused.torso_forward(m, xy, poses, code, -1.0, alpha_out=alpha_i, deform_out=dx_i)
    assert bool((alpha_i > 0).all())
    alpha, _, dx = train_torso.torso_forward(m, xy, poses, code)
    e_a, e_d = float((alpha - alpha_i).abs().max()), float((dx - dx_i).abs().max())
    print(f"torso train forward vs inference kernel: alpha {e_a:.2e}  dx {e_d:.2e}")
    assert e_a <= 3e-5 and e_d <= 3e-5, (e_a, e_d)


def test_through_the_renderer(hiplib, monkeypatch):
    """NeRFRenderer._torso_layer at N = 4097 on the quadrant occupancy with the fused kernels on the covered pixels: the blended
    background, torso_alpha / torso_color and every gradient against the float64 restatement in which uncovered pixels contribute
    nothing; the yardstick is the default path."""
    scene = _train_scene(8)
    m, poses = scene.model, _poses(scene)
    names = _grad_names(m)
    N = 4097
    gen = _gen(4900)
    mask = torch.rand(N, device="cuda", generator=gen) < 0.5
    idx = torch.nonzero(mask).reshape(-1)
    xy = _pixels(mask, gen)
    xy[idx], _ = _smooth_batch(m, idx.numel(), 4901, poses, _code(m, ROW), inside=True)
    bg = torch.rand(N, 3, device="cuda", generator=gen)
    up = torch.randn(N, 3, device="cuda", generator=gen)
    with _occupancy(m, _quadrants()):
        ref = netref64.Net64(m)
        bg64 = bg.double().requires_grad_(True)
        a, c, _ = ref.forward_torso(xy[idx], poses, ref.P["individual_codes_torso"][ROW])
        out64 = bg64.index_put((idx,), c * a + bg64[idx] * (1 - a))
        g64 = dict(zip(names + ["background"], torch.autograd.grad((out64 * up.double()).sum(), [ref.P[n] for n in names] + [bg64])))
        g64["individual_codes_torso"] = g64["individual_codes_torso"][ROW]
        g64["out:bg"] = out64.detach()
        g64["out:torso_alpha"] = torch.zeros(N, 1, dtype=torch.float64, device="cuda").index_copy(0, idx, a.detach())
        runs = {}
        for mode in ("default", "fused"):
            _env(monkeypatch, fused=mode == "fused")
            for p in m.parameters():
                p.grad = None
            bg_leaf = bg.clone().requires_grad_(True)
            res = {}
            with _spy() as called:
                out = m._torso_layer(xy, poses, None, ROW, bg_leaf, res)
                (out * up).sum().backward()
            if mode == "fused":
                assert sorted(called) == sorted(ENTRIES + ["rn_torso_mask"]), called
            else:
                assert not [c for c in called if c.startswith("rn_train_torso_")], called
            un = ~mask
            assert torch.equal(out[un], bg[un]) and torch.equal(bg_leaf.grad[un], up[un])     # exactly nothing from uncovered pixels
            assert int(torch.count_nonzero(res["torso_alpha"][un])) == 0 and torch.equal(res["torso_alpha"].reshape(-1) > 0, mask)
            assert res["torso_color"] is out and res["deform"].shape == (idx.numel(), 2)
            runs[mode] = dict(_collect(m, names, ROW), background=bg_leaf.grad.clone(),
                              **{"out:bg": out.detach(), "out:torso_alpha": res["torso_alpha"].detach()})
    _compare(runs["fused"], runs["default"], g64, f"_torso_layer N={N} fused")


def test_no_pixels(hiplib, monkeypatch):
    """P == 0: empty outputs, zero gradients of the right shapes, no entry point called."""
    scene = _train_scene(8)
    m, poses = scene.model, _poses(scene)
    names = _grad_names(m)
    _env(monkeypatch, fused=True)
    for p in m.parameters():
        p.grad = None
    with _spy() as called:
        alpha, color, dx = m.forward_torso(torch.empty(0, 2, device="cuda"), poses, None, m.individual_codes_torso[ROW])
        assert alpha.shape == (0, 1) and color.shape == (0, 3) and dx.shape == (0, 2)
        (alpha.sum() + color.sum() + dx.sum()).backward()
    assert called == [], called
    params = dict(m.named_parameters())
    for n in names:
        g = params[n].grad
        assert g is not None and g.shape == params[n].shape and int(torch.count_nonzero(g)) == 0, n
