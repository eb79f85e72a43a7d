"""compref64.py held on the CPU: its closed-form backward against float64 autograd of its own forward, the share of rays it
leaves out as knife edges, the fp32 oracle through the same check_* functions that test_gpu_composite.py hands the kernels'
outputs to (the worst error / (2^-24 * magnitude) per output is printed: K is four times it), and the sensitivity of those
checks: an fp32 restatement of the operators' loops, with one wrong line at a time, must be rejected."""
import numpy as np
import pytest
import torch

import composite_cases as cc
import compref64 as ref

F = np.float32


# ------------------------------------------------------------------------------------------------ the oracle, called on a case

def oracle_train_forward(po, case, M=None):
    M = case["M"] if M is None else M
    N = case["N"]
    ws, am, dp, im = np.full(N, np.nan, F), np.full(N, np.nan, F), np.full(N, np.nan, F), np.full((N, 3), np.nan, F)
    po.lib().orc_composite_rays_train_forward(po._p(case["sigmas"]), po._p(case["rgbs"]), po._p(case["ambient"]), po._p(case["deltas"]),
                                              po._p(case["rays"]), po.u32(M), po.u32(N), po.f32(case["T_thresh"]), po._p(ws), po._p(am),
                                              po._p(dp), po._p(im))
    return dict(ws=ws, ambient_sum=am, depth=dp, image=im)


def grad_buffers(case):
    R = case["rows"]
    return dict(grad_sigmas=np.full(R, cc.SENTINEL, F), grad_rgbs=np.full((R, 3), cc.SENTINEL, F), grad_ambient=np.full(R, cc.SENTINEL, F))


def oracle_train_backward(po, case):
    f = ref.forward32(case)
    g = grad_buffers(case)
    po.lib().orc_composite_rays_train_backward(po._p(case["g_ws"]), po._p(case["g_am"]), po._p(case["g_im"]), po._p(case["sigmas"]),
                                               po._p(case["rgbs"]), po._p(case["ambient"]), po._p(case["deltas"]), po._p(case["rays"]),
                                               po._p(f["ws"]), po._p(f["ambient_sum"]), po._p(f["image"]), po.u32(case["M"]),
                                               po.u32(case["N"]), po.f32(case["T_thresh"]), po._p(g["grad_sigmas"]),
                                               po._p(g["grad_rgbs"]), po._p(g["grad_ambient"]))
    return g


def oracle_composite(po):
    def composite(n_alive, n_step, T_thresh, alive, rays_t, sig, rgb, dl, ws, depth, image, limit):
        po.composite_rays(n_alive if limit is None else limit, n_step, T_thresh, alive, rays_t, sig, rgb, dl, ws, depth, image)
    return composite


def oracle_march_backward(po, case):
    go, gd = case["go0"].copy(), case["gd0"].copy()
    po.lib().orc_march_rays_train_backward(po._p(case["gx"]), po._p(case["gd"]), po._p(case["rays"]), po._p(case["deltas"]),
                                           po.u32(case["N"]), po.u32(case["M"]), po._p(go), po._p(gd))
    return dict(grad_rays_o=go, grad_rays_d=gd)


# ------------------------------------------------------------------------------------------------ the reference itself

@pytest.mark.parametrize("name", cc.TRAIN_CASES)
def test_closed_form_backward_is_the_autograd_of_the_forward(name):
    """Float64 autograd through the truncated forward (the truncation length frozen: it is an integer) against the closed form,
    to 1e-12 of the ray's incoming gradient; rows outside the mask receive exactly nothing."""
    case = cc.train_case(name)
    r = ref.train_reference(case)
    sig = torch.tensor(case["sigmas"], dtype=torch.float64, requires_grad=True)
    rgb = torch.tensor(case["rgbs"], dtype=torch.float64, requires_grad=True)
    amb = torch.tensor(case["ambient"], dtype=torch.float64, requires_grad=True)
    dl = torch.tensor(case["deltas"], dtype=torch.float64)
    loss = torch.zeros((), dtype=torch.float64)
    scale = np.zeros(case["rows"])
    for n, (idx, off, cnt) in enumerate(case["rays"].astype(np.int64)):
        L = int(r["L"][n])
        if L == 0:
            continue
        s = slice(off, off + L)
        a = 1 - torch.exp(-sig[s] * dl[s, 0])
        T = torch.cumprod(torch.cat([torch.ones(1, dtype=torch.float64), 1 - a[:-1]]), 0)
        w = a * T
        fwd = r["fwd"]
        np.testing.assert_allclose(w.sum().item(), fwd["ws"][idx], rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose((w[:, None] * rgb[s]).sum(0).detach().numpy(), fwd["image"][idx], rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose((w * dl[s, 1]).sum().item(), fwd["depth"][idx], rtol=1e-12, atol=1e-15)
        loss = loss + w.sum() * float(case["g_ws"][idx]) + (w[:, None] * rgb[s] * torch.tensor(case["g_im"][idx], dtype=torch.float64)).sum() \
            + amb[s].sum() * float(case["g_am"][idx]) + (w * dl[s, 1]).sum() * 0.0
        scale[s] = 1.0
    if not loss.requires_grad:
        assert not r["mask"].any()
        return
    loss.backward()
    for got, want in ((sig.grad, "grad_sigmas"), (rgb.grad, "grad_rgbs"), (amb.grad, "grad_ambient")):
        got, want = got.numpy(), r["grad"][want]
        assert not got[~r["mask"]].any() and not want[~r["mask"]].any()
        assert np.array_equal(scale > 0, r["mask"])
        # relative to the ray's incoming gradient: every term of a sample's gradient is that times a factor of at most 1
        # (weights, colours, transmittances, delta), and the terms of d/d sigma cancel
        for idx, off, cnt in case["rays"].astype(np.int64):
            s = slice(off, off + cnt)
            g_in = np.abs(case["g_im"][idx]).sum() + abs(case["g_ws"][idx]) + abs(case["g_am"][idx])
            assert np.abs(got[s] - want[s]).max(initial=0.0) <= 1e-12 * g_in, (name, idx)


def test_every_branch_is_in_the_cases():
    """What the cases are chosen for is there: truncated rays, rays that go on after a nearly opaque sample, skipped rays."""
    for name in cc.TRAIN_CASES:
        case, r = cc.train_case(name), ref.train_reference(cc.train_case(name))
        cnt, off = case["rays"][:, 2].astype(np.int64), case["rays"][:, 1].astype(np.int64)
        assert (off + cnt <= case["rows"] - cc.SPARE).all()                           # every slice inside what is allocated
        if case["N"] >= 255:
            assert (cnt == 0).sum() >= 3 and (off + cnt > case["M"]).sum() >= 2
            assert sorted(set(case["rays"][:, 0])) == list(range(case["N"])) and (case["rays"][:, 0] != np.arange(case["N"])).any()
            if case["T_thresh"] > 0:
                assert r["truncated"] >= 20 and (r["L"] == 1).sum() >= 3 and r["truncated"] < r["live"]
            if 0 < case["T_thresh"] < 0.01:     # a sample with alpha > 0.99 that does not end its ray
                x = case["sigmas"].astype(np.float64) * case["deltas"][:, 0]
                assert sum(bool((x[o:o + L - 1] > 4.6).any()) for o, L in zip(off, r["L"]) if L > 1) >= 20
    for name in cc.INFER_CASES:
        case, r = cc.infer_case(name), ref.infer_reference(cc.infer_case(name))
        assert (np.sort(case["alive"]) != case["alive"]).any() or case["N"] == 1
        if case["N"] > 1 and case["limit"] is None:
            ends = [int((c["alive_in"] & ~c["alive_out"]).sum()) for c in r["calls"]]
            assert min(ends) > 0 and r["calls"][-1]["alive_out"].any(), ends          # rays end in every call, some never


@pytest.mark.parametrize("name", cc.TRAIN_CASES + cc.INFER_CASES)
def test_flagged_share(name):
    r = ref.infer_reference(cc.infer_case(name)) if name in cc.INFER_CASES else ref.train_reference(cc.train_case(name))
    assert r["share"] <= 0.02, f"{name}: {r['share']:.3%} of the live rays are knife edges"


# ------------------------------------------------------------------------------------------------ the oracle against it

_RATIOS = {}


def _note(ratios):
    for k, v in ratios.items():
        _RATIOS[k] = max(_RATIOS.get(k, 0.0), v)


@pytest.mark.parametrize("name", cc.TRAIN_CASES)
def test_oracle_training_compositor(po, name):
    case = cc.train_case(name)
    _note(ref.check_train_forward(case, oracle_train_forward(po, case)))
    _note(ref.check_train_backward(case, oracle_train_backward(po, case)))


@pytest.mark.parametrize("name", cc.INFER_CASES)
def test_oracle_inference_compositor(po, name):
    case = cc.infer_case(name)
    _note(ref.check_inference(case, cc.run_inference(case, oracle_composite(po))))


@pytest.mark.parametrize("name", cc.MARCH_BWD_CASES)
def test_oracle_march_backward(po, name):
    case = cc.train_case(name)
    _note(ref.check_march_backward(case, oracle_march_backward(po, case)))


def test_k_is_four_times_what_the_oracle_needs(po):
    """Runs every case once more (the tests above may have been deselected) and prints the table of DESIGN.md."""
    for name in cc.TRAIN_CASES:
        case = cc.train_case(name)
        _note(ref.check_train_forward(case, oracle_train_forward(po, case)))
        _note(ref.check_train_backward(case, oracle_train_backward(po, case)))
    for name in cc.INFER_CASES:
        _note(ref.check_inference(cc.infer_case(name), cc.run_inference(cc.infer_case(name), oracle_composite(po))))
    for name in cc.MARCH_BWD_CASES:
        _note(ref.check_march_backward(cc.train_case(name), oracle_march_backward(po, cc.train_case(name))))
    live = sum(ref.train_reference(cc.train_case(n))["live"] for n in cc.TRAIN_CASES)
    trunc = sum(ref.train_reference(cc.train_case(n))["truncated"] for n in cc.TRAIN_CASES)
    print(f"\ncompositor bars: {live} live training rays, {trunc} truncated")
    for k in ref.K:
        print(f"  {k:12s} oracle needs {_RATIOS[k]:7.3f}   k = {ref.K[k]:g}")
        assert 4 * _RATIOS[k] <= ref.K[k], f"{k}: the oracle needs {_RATIOS[k]:.3f}, k = {ref.K[k]} is not four times that"
        assert ref.K[k] <= 4 * _RATIOS[k] * 1.25, f"{k}: k = {ref.K[k]} is wider than four times the oracle's {_RATIOS[k]:.3f}"


# ------------------------------------------------------------------------------------------------ sensitivity

def train32(case, ws_in=None, image_in=None, mut=None):
    """The training compositor's loop in numpy fp32, forward and backward in one (the backward reads `ws_in` / `image_in`);
    `mut` names one wrong line."""
    N, M, Tth = case["N"], case["M"], F(case["T_thresh"])
    sg, rg, am, dl = case["sigmas"], case["rgbs"], case["ambient"], case["deltas"]
    out = dict(ws=np.zeros(N, F), ambient_sum=np.zeros(N, F), depth=np.zeros(N, F), image=np.zeros((N, 3), F))
    g = grad_buffers(case)
    one = F(1)
    for n, (index, off, cnt) in enumerate(case["rays"]):
        if cnt == 0 or off + cnt > M:
            continue
        at = n if mut == "row_n" else index
        gws, gas, gi = case["g_ws"][at], case["g_am"][at], case["g_im"][at]
        fin_ws = None if ws_in is None else ws_in[at]
        fin_c = None if image_in is None else image_in[at]
        T, ws, d, a_sum, c = one, F(0), F(0), F(0), np.zeros(3, F)
        for j in range(off, off + cnt):
            T_pre = T
            alpha = one - np.exp(-sg[j] * dl[j, 0])
            w = alpha * T
            c = c + w * rg[j]
            d, ws, a_sum = d + w * dl[j, 1], ws + w, a_sum + am[j]
            T = T * (one - alpha)
            if fin_ws is not None:
                g["grad_rgbs"][j] = gi * (alpha * T if mut == "T_after" else w)
                g["grad_ambient"][j] = gas
                last = F(0) if mut == "no_gws" else gws * (one - fin_ws)
                g["grad_sigmas"][j] = dl[j, 0] * (gi[0] * (T * rg[j, 0] - (fin_c[0] - c[0])) + gi[1] * (T * rg[j, 1] - (fin_c[1] - c[1]))
                                                   + gi[2] * (T * rg[j, 2] - (fin_c[2] - c[2])) + last)
            if (T_pre if mut == "test_before" else T) < Tth:
                if mut == "zero_tail":
                    for name in g:
                        g[name][j + 1:off + cnt] = 0
                break
        out["ws"][at], out["ambient_sum"][at], out["depth"][at], out["image"][at] = ws, a_sum, d, c
    return out, g


def infer32(mut=None):
    def composite(n_alive, n_step, Tth, alive, rays_t, sig, rgb, dl, ws, depth, image, limit):
        one, Tth = F(1), F(Tth)
        for n in range(n_alive if limit is None else limit):
            index = n if mut == "row_n" else alive[n]
            t, s, d, c = rays_t[index], ws[index], depth[index], image[index].copy()
            step = 0
            while step < n_step:
                j = n * n_step + step
                if dl[j, 0] == 0:
                    break
                alpha = one - np.exp(-sig[j] * dl[j, 0])
                T = one - s
                w = alpha * T
                s, t = s + w, dl[j, 1]
                d, c = d + w * t, c + w * rgb[j]
                if (one - s if mut == "test_after" else T) < Tth:
                    break
                step += 1
            if step < n_step:
                alive[n] = -1
            if step == n_step or mut == "t_on_end":
                rays_t[index] = t
            ws[index], depth[index], image[index] = s, d, c
    return composite


def march32(case, mut=None):
    go, gd = case["go0"].copy(), case["gd0"].copy()
    for n, (index, off, cnt) in enumerate(case["rays"]):
        if cnt == 0 or off + cnt > case["M"]:
            continue
        at = index if mut == "row_index" else n
        o, d = (np.zeros(3, F), np.zeros(3, F)) if mut == "overwrite" else (go[at].copy(), gd[at].copy())
        for j in range(off, off + cnt):
            o = o + case["gx"][j]
            d = d + (case["gx"][j] * case["deltas"][j, 1] + case["gd"][j])
        go[at], gd[at] = o, d
    return dict(grad_rays_o=go, grad_rays_d=gd)


TRAIN_SENS = ("N257-T0.0001", "N257-T0.3")


def _train32(case, mut=None):
    f = ref.forward32(case)
    return train32(case, f["ws"], f["image"], mut)


def test_restatement_passes_unmutated():
    """Without a wrong line the fp32 restatement is accepted by every check: the rejections below are the mutations' doing."""
    for name in TRAIN_SENS:
        case = cc.train_case(name)
        out, g = _train32(case)
        ref.check_train_forward(case, out)
        ref.check_train_backward(case, g)
        ref.check_march_backward(case, march32(case))
    for name in ("N257-s4-T0.0001", "N257-s4-T0"):
        ref.check_inference(cc.infer_case(name), cc.run_inference(cc.infer_case(name), infer32()))


@pytest.mark.parametrize("mut,where", [("row_n", "forward"), ("row_n", "backward"), ("test_before", "forward"), ("test_before", "backward"),
                                       ("no_gws", "backward"), ("T_after", "backward"), ("zero_tail", "backward")])
@pytest.mark.parametrize("name", TRAIN_SENS)
def test_training_mutations_are_rejected(name, mut, where):
    case = cc.train_case(name)
    out, g = _train32(case, mut)
    with pytest.raises(AssertionError):
        if where == "forward":
            ref.check_train_forward(case, out)
        else:
            ref.check_train_backward(case, g)


@pytest.mark.parametrize("mut", ["row_n", "test_after", "t_on_end"])
def test_inference_mutations_are_rejected(mut):
    case = cc.infer_case("N257-s4-T0.0001")
    with pytest.raises(AssertionError):
        ref.check_inference(case, cc.run_inference(case, infer32(mut)))


@pytest.mark.parametrize("mut", ["overwrite", "row_index"])
def test_march_backward_mutations_are_rejected(mut):
    case = cc.train_case("N257-T0")
    with pytest.raises(AssertionError):
        ref.check_march_backward(case, march32(case, mut))
