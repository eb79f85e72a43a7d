"""The compositing kernels against the float64 restatement of tests/compref64.py, on the seeded cases of
tests/composite_cases.py: k_composite_train_fwd / k_composite_train_bwd / k_march_train_backward and composite_ray behind
rn_composite_rays, called through the C ABI, and the autograd wrapper's two short cuts.

Every float output element is held to K[output] * 2^-24 * its own magnitude (compref64's error model; K is four times what the
fp32 CPU oracle needs, test_compref64.py); alive flags and rays_t are bit-exact outside the rays that compref64 flags as knife
edges, and rows that belong to no gradient keep the sentinel bit for bit.  The device-resident loop's composite_chunk is held
bit-equal to rn_composite_rays by test_gpu_fused.py and needs no case here.
"""
import contextlib

import numpy as np
import pytest
import torch

import composite_cases as cc
import compref64 as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
_WORST = {}


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def n(x):
    return x.detach().cpu().numpy()


@contextlib.contextmanager
def _spy():
    """Names of the C entry points called inside the block (radnerf_hip.call is the one door to the library)."""
    import radnerf_hip as hip
    names, real = [], hip.call

    def call(name, *a):
        names.append(name)
        return real(name, *a)
    hip.call = call
    try:
        yield names
    finally:
        hip.call = real


def _note(ratios):
    for k, v in ratios.items():
        _WORST[k] = max(_WORST.get(k, 0.0), v)
    print("  ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


def _inputs(case):
    return {k: t(case[k]) for k in ("sigmas", "rgbs", "ambient", "deltas", "rays")}


def train_forward(hip, case, M=None):
    N, d = case["N"], _inputs(case)
    out = dict(ws=torch.full((N,), np.nan, device=DEV), ambient_sum=torch.full((N,), np.nan, device=DEV),
               depth=torch.full((N,), np.nan, device=DEV), image=torch.full((N, 3), np.nan, device=DEV))
    hip.call("rn_composite_rays_train_forward", hip.ptr(d["sigmas"]), hip.ptr(d["rgbs"]), hip.ptr(d["ambient"]), hip.ptr(d["deltas"]),
             hip.ptr(d["rays"]), case["M"] if M is None else M, N, case["T_thresh"], hip.ptr(out["ws"]), hip.ptr(out["ambient_sum"]),
             hip.ptr(out["depth"]), hip.ptr(out["image"]), hip.stream())
    return {k: n(v) for k, v in out.items()}


def train_backward(hip, case):
    N, R, d = case["N"], case["rows"], _inputs(case)
    f = {k: t(v) for k, v in ref.forward32(case).items()}
    g_ws, g_am, g_im = t(case["g_ws"]), t(case["g_am"]), t(case["g_im"])
    s = float(cc.SENTINEL)
    out = dict(grad_sigmas=torch.full((R,), s, device=DEV), grad_rgbs=torch.full((R, 3), s, device=DEV),
               grad_ambient=torch.full((R,), s, device=DEV))
    hip.call("rn_composite_rays_train_backward", hip.ptr(g_ws), hip.ptr(g_am), hip.ptr(g_im), hip.ptr(d["sigmas"]), hip.ptr(d["rgbs"]),
             hip.ptr(d["ambient"]), hip.ptr(d["deltas"]), hip.ptr(d["rays"]), hip.ptr(f["ws"]), hip.ptr(f["ambient_sum"]),
             hip.ptr(f["image"]), case["M"], N, case["T_thresh"], hip.ptr(out["grad_sigmas"]), hip.ptr(out["grad_rgbs"]),
             hip.ptr(out["grad_ambient"]), hip.stream())
    return {k: n(v) for k, v in out.items()}


def composite(hip):
    """One rn_composite_rays call in place on numpy arrays, for composite_cases.run_inference."""
    def call(n_alive, n_step, T_thresh, alive, rays_t, sig, rgb, dl, ws, depth, image, limit):
        host = dict(alive=alive, rays_t=rays_t, ws=ws, depth=depth, image=image)
        dev = {k: t(v) for k, v in host.items()}
        dsig, drgb, ddl = t(sig), t(rgb), t(dl)
        count = None if limit is None else torch.tensor([limit], dtype=torch.int32, device=DEV)
        hip.call("rn_composite_rays", int(n_alive), int(n_step), float(T_thresh), hip.ptr(dev["alive"], torch.int32), hip.ptr(dev["rays_t"]),
                 hip.ptr(dsig), hip.ptr(drgb), hip.ptr(ddl), hip.ptr(dev["ws"]), hip.ptr(dev["depth"]), hip.ptr(dev["image"]),
                 hip.ptr(count), hip.stream())
        for k, v in host.items():
            v[...] = n(dev[k])
    return call


@pytest.mark.parametrize("name", cc.TRAIN_CASES)
def test_train_forward(hiplib, name):
    case = cc.train_case(name)
    _note(ref.check_train_forward(case, train_forward(hiplib, case)))


@pytest.mark.parametrize("name", cc.TRAIN_CASES)
def test_train_backward(hiplib, name):
    """The backward on the reference's own forward (rounded to fp32), into buffers that hold the sentinel."""
    case = cc.train_case(name)
    _note(ref.check_train_backward(case, train_backward(hiplib, case)))


@pytest.mark.parametrize("name", cc.INFER_CASES)
def test_inference_frame(hiplib, name):
    """Three calls over the same rays, the list compacted in between: the accumulators are the kernel's own from the second
    call on.  `device-count`: the count comes from n_alive_dev, half the launch bound."""
    case = cc.infer_case(name)
    _note(ref.check_inference(case, cc.run_inference(case, composite(hiplib))))


@pytest.mark.parametrize("name", cc.MARCH_BWD_CASES)
def test_march_backward(hiplib, name):
    hip, case = hiplib, cc.train_case(name)
    d = {k: t(case[k]) for k in ("gx", "gd", "rays", "deltas")}
    go, gd = t(case["go0"]), t(case["gd0"])
    hip.call("rn_march_rays_train_backward", hip.ptr(d["gx"]), hip.ptr(d["gd"]), hip.ptr(d["rays"]), hip.ptr(d["deltas"]), case["N"],
             case["M"], hip.ptr(go), hip.ptr(gd), hip.stream())
    _note(ref.check_march_backward(case, dict(grad_rays_o=n(go), grad_rays_d=n(gd))))


def _through_autograd(case):
    import raymarching
    leaves = [t(case[k]).requires_grad_() for k in ("sigmas", "rgbs", "ambient")]
    out = raymarching.composite_rays_train(*leaves, t(case["deltas"]), t(case["rays"]), case["T_thresh"])
    return leaves, dict(zip(("ws", "ambient_sum", "depth", "image"), out))


def test_autograd_with_only_the_image_downstream(hiplib):
    """weights_sum's and ambient_sum's gradients are None (set_materialize_grads(False)): the wrapper stands zeros in for them.
    The wrapper's M is the buffers' length, so no ray is cut off; the backward reads the kernel's own forward."""
    case = cc.train_case("N257-T0.0001/image")
    M = case["rows"]
    leaves, out = _through_autograd(case)
    _note(ref.check_train_forward(case, {k: n(v) for k, v in out.items()}, M=M))
    with _spy() as called:
        (out["image"] * t(case["g_im"])).sum().backward()
    assert called == ["rn_composite_rays_train_backward"]
    grads = dict(zip(("grad_sigmas", "grad_rgbs", "grad_ambient"), (n(x.grad) for x in leaves)))
    assert not grads["grad_ambient"].any()
    _note(ref.check_train_backward(case, grads, M=M, sentinel=None))


def test_autograd_with_only_the_depth_downstream(hiplib):
    """depth receives no gradient: all three gradients are zero and the backward kernel is not launched."""
    case = cc.train_case("N257-T0.0001")
    leaves, out = _through_autograd(case)
    with _spy() as called:
        out["depth"].sum().backward()
    assert called == []
    for x in leaves:
        assert x.grad is not None and x.grad.shape == x.shape and not n(x.grad).any()


def test_inference_and_training_compositors_agree(hiplib):
    """The same samples through rn_composite_rays (first call of a frame) and rn_composite_rays_train_forward at
    T_thresh = 0: the two float64 restatements give the same numbers, each kernel is within its bound of them, and so the two
    kernels are within the sum of the bounds of each other."""
    icase = cc.infer_case("N257-s8-T0")
    tcase = cc.train_case("as-training:N257-s8-T0")
    alive = icase["alive"]
    outs = cc.run_inference(icase, composite(hiplib))
    ref.check_inference(icase, outs)
    tout = train_forward(hiplib, tcase)
    ref.check_train_forward(tcase, tout)
    i64, t64 = ref.infer_reference(icase)["calls"][0], ref.train_reference(tcase)
    keep = ~i64["flagged"][alive] & ~t64["flagged"]
    assert keep.mean() >= 0.98
    for name in ("ws", "depth", "image"):
        a, b = i64[name][alive], t64["fwd"][name]
        assert np.abs(a - b).max() <= 1e-13 * max(np.abs(a).max(), 1.0), name
        bound = ref.U * (ref.K["inf_" + name] * i64["mag"][name][alive] + ref.K[name] * t64["fwd_mag"][name])
        err = np.abs(outs[0][name][alive].astype(np.float64) - tout[name].astype(np.float64))
        assert (err[keep] <= bound[keep]).all(), name


def test_worst_ratios_reported():
    """Last in the file: the kernels' worst error / (2^-24 * magnitude) per output over the cases above (DESIGN.md's table)."""
    print("\n" + "\n".join(f"  {k:12s} kernel needs {v:7.3f}   k = {ref.K[k]:g}" for k, v in sorted(_WORST.items())))
    for k, v in _WORST.items():
        assert v <= ref.K[k]
