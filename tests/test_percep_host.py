"""radnerf/percep.py without a GPU: the torch path of PerceptualAlex against the float64 helper's float32 run (tests/percepref64.py),
the two loaders, the size limit, the exact properties of the arithmetic, Trainer.evaluate(..., perceptual=...) on a CPU model, and
the argument checks of the rn_percep_* entry points (which run before anything touches a device)."""
import ctypes as C
import types

import pytest
import torch

import percepref64 as R


def _module():
    from radnerf.percep import PerceptualAlex
    ws, bs, lins, _ = R.seeded_weights()
    return PerceptualAlex(ws, bs, lins)


@pytest.mark.parametrize("shape", [(1, 31, 31), (1, 37, 50), (3, 32, 32)])
def test_torch_path_equals_the_helpers_float32_run(shape):
    """Same expressions in the same order; the helper runs pred and target as one batch of 2P images, the module one after the
    other -- on the CPU that leaves the value within 4 ulp (measured: equal bits) and the gradient within 1e-6 of its maximum."""
    seed = R.USABLE_SEEDS[shape]
    ref = R.reference(*shape, seed, torch.float32)
    pred, target = R.inputs(*shape, seed)
    pred.requires_grad_()
    m = _module()
    value = m(pred, target)
    assert value.shape == (shape[0], 1, 1, 1) and value.dtype == torch.float32
    (g,) = torch.autograd.grad(value.sum(), pred)
    ulp = float(((value.detach().view(-1) - ref["value"]).abs() / (ref["value"].abs() * 2.0 ** -23)).max())
    gerr = float((g - ref["g_pred"]).abs().max() / ref["g_pred"].abs().max())
    print(f"{shape}: value differs by {ulp:.2f} ulp, gradient by {gerr:.2e} of its maximum")
    assert ulp <= 4 and gerr <= 1e-6
    for p in m.buffers():
        assert not p.requires_grad
    assert not list(m.parameters())


def test_helper_float32_run_is_close_to_float64():
    """The yardstick's own error (the figures the GPU tests print their ratios against)."""
    for shape, seed in R.USABLE_SEEDS.items():
        assert R.usable(*shape, seed), (shape, seed)
        r64, r32 = R.reference(*shape, seed), R.reference(*shape, seed, torch.float32)
        rel = float(((r32["value"].double() - r64["value"]) / r64["value"]).abs().max())
        gerr = float((r32["g_pred"].double() - r64["g_pred"]).abs().max() / r64["g_pred"].abs().max())
        print(f"{shape} seed {seed}: margins {r64['pre_margin']:.1e} / {r64['pool_gap']:.1e}; float32 value rel {rel:.1e}, gradient {gerr:.1e}")
        assert rel < 1e-6 and gerr < 1e-5
    assert not R.usable(1, 96, 80, 0)


def test_closed_form_distance_gradient_is_autograds():
    """distance_closed_form (what the GPU tests hold the distance kernel to) against autograd over `distance`, in float64."""
    g = torch.Generator().manual_seed(3)
    x = torch.relu(torch.randn(2, 64, 3, 5, generator=g, dtype=torch.float64)).requires_grad_()
    y = torch.relu(torch.randn(2, 64, 3, 5, generator=g, dtype=torch.float64))
    with torch.no_grad():
        x[0, :, 1, 2] = 0                                  # a position whose channels are all zero: gradient u / eps there, finite
    lin = torch.rand(1, 64, 1, 1, generator=g, dtype=torch.float64) / 64
    value = R.distance(x, y, lin)
    (auto,) = torch.autograd.grad(value.sum(), x)
    v, av, D, aD = R.distance_closed_form(x.detach(), y, lin)
    assert torch.allclose(v, value.detach(), rtol=1e-13, atol=0) and bool((av >= v).all())
    assert bool(torch.isfinite(auto).all()) and bool((aD >= D.abs()).all())
    assert float((D - auto).abs().max()) <= 1e-12 * float(auto.abs().max())


def test_loaders_round_trip_and_name_what_is_wrong():
    from radnerf.percep import PerceptualAlex
    m = _module()
    sd = m.lpips_state_dict()
    sd["lins.0.model.1.weight"] = sd["lin0.model.1.weight"].clone()             # the package's duplicate entries: ignored
    again = PerceptualAlex.from_lpips_state_dict(sd)
    for (na, a), (nb, b) in zip(m.named_buffers(), again.named_buffers()):
        assert na == nb and torch.equal(a, b), na
    alex = {k.replace("net.slice1.0", "features.0").replace("net.slice2.3", "features.3").replace("net.slice3.6", "features.6")
            .replace("net.slice4.8", "features.8").replace("net.slice5.10", "features.10"): v for k, v in sd.items() if k.startswith("net.")}
    alex["classifier.1.weight"] = torch.zeros(4, 4)                             # ignored
    lin_sd = {k: v for k, v in sd.items() if k.startswith("lin")}
    parts = PerceptualAlex.from_parts(alex, lin_sd)
    for (na, a), (nb, b) in zip(m.named_buffers(), parts.named_buffers()):
        assert torch.equal(a, b), na
    pred, target = R.inputs(1, 31, 31, 0)
    assert torch.equal(m(pred, target), again(pred, target)) and torch.equal(m(pred, target), parts(pred, target))
    # a missing key, a wrong shape and an unexpected key are named
    clean = m.lpips_state_dict()
    broken = dict(clean)
    del broken["net.slice3.6.bias"]
    with pytest.raises(KeyError, match=r"net\.slice3\.6\.bias"):
        PerceptualAlex.from_lpips_state_dict(broken)
    broken = dict(clean)
    broken["lin2.model.1.weight"] = torch.zeros(1, 256, 1, 1)
    with pytest.raises(ValueError, match=r"lin2\.model\.1\.weight.*\(1, 256, 1, 1\).*\(1, 384, 1, 1\)"):
        PerceptualAlex.from_lpips_state_dict(broken)
    broken = dict(clean)
    broken["net.slice9.0.weight"] = torch.zeros(1)
    with pytest.raises(KeyError, match=r"net\.slice9\.0\.weight"):
        PerceptualAlex.from_lpips_state_dict(broken)
    with pytest.raises(KeyError, match=r"features\.8\.weight"):
        PerceptualAlex.from_parts({k: v for k, v in alex.items() if k != "features.8.weight"}, lin_sd)
    with pytest.raises(KeyError, match=r"lin4\.model\.1\.weight"):
        PerceptualAlex.from_parts(alex, {k: v for k, v in lin_sd.items() if not k.startswith("lin4")})


def test_the_smallest_image_is_31_by_31():
    m = _module()
    for h, w in ((30, 31), (31, 30)):
        with pytest.raises(ValueError, match="smallest image"):
            m(torch.rand(1, 3, h, w), torch.rand(1, 3, h, w))
    assert m(torch.rand(1, 3, 31, 31), torch.rand(1, 3, 31, 31)).shape == (1, 1, 1, 1)
    with pytest.raises(ValueError, match=r"\[P,3,h,w\]"):
        m(torch.rand(1, 4, 31, 31), torch.rand(1, 4, 31, 31))


def test_identical_images_give_exactly_zero():
    m = _module()
    pred, _ = R.inputs(2, 33, 35, 4)
    pred.requires_grad_()
    value = m(pred, pred.detach().clone())
    (g,) = torch.autograd.grad(value.sum(), pred)
    assert float(value.abs().max()) == 0.0 and float(g.abs().max()) == 0.0


def test_normalize_is_the_plain_call_on_2x_minus_1():
    m = _module()
    pred, target = R.inputs(1, 37, 50, 0)
    assert torch.equal(m(pred, target, normalize=True), m(2 * pred - 1, 2 * target - 1))
    assert not torch.equal(m(pred, target, normalize=True), m(pred, target))


class _StubModel(torch.nn.Module):
    """What Trainer.evaluate needs of a model, on the CPU: parameters, get_params, render -> a fixed image per frame."""

    def __init__(self, images):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.images = images

    def get_params(self, lr, lr_net):
        return [dict(params=[self.p], lr=lr)]

    def render(self, rays_o, rays_d, auds, bg_coords, poses, index=None, **kw):
        return dict(image=self.images[int(index[0])])


def test_evaluate_carries_lpips_on_a_cpu_model():
    from radnerf.train import Trainer
    H, W = 33, 40
    g = torch.Generator().manual_seed(11)
    truths, preds = torch.rand(3, H, W, 3, generator=g), torch.rand(3, H, W, 3, generator=g)
    frame = lambda i: dict(rays_o=None, rays_d=None, auds=None, bg_coords=None, poses=None, eye=None, index=[i], bg_color=None, images=truths[i])
    ds = types.SimpleNamespace(H=H, W=W, frame=frame, face_rect=None, lips_rect=None)
    tr = Trainer(_StubModel(preds), types.SimpleNamespace(dt_gamma=0.0, max_steps=16), update_extra_interval=0)
    m = _module()
    plain = tr.evaluate(ds, [0, 2])
    assert set(plain) == {"loss", "psnr", "per_frame", "rect_psnr"}
    res = tr.evaluate(ds, [0, 2], perceptual=m)
    assert set(res) == set(plain) | {"lpips", "lpips_per_frame"}
    assert res["loss"] == plain["loss"] and res["psnr"] == plain["psnr"] and res["per_frame"] == plain["per_frame"]
    nchw = lambda t: t.permute(2, 0, 1).unsqueeze(0)
    want = [float(m(nchw(truths[i]), nchw(preds[i]), normalize=True)) for i in (0, 2)]      # LPIPSMeter: (truth, pred), [0,1] images
    assert res["lpips_per_frame"] == pytest.approx(want, rel=1e-6) and res["lpips"] == pytest.approx(sum(want) / 2, rel=1e-6)
    assert all(v > 0 for v in want)


def test_entry_points_refuse_bad_arguments(hiplib):
    """As tests/test_abi.py does for the other training entry points: RN_ERR_INVALID_ARG with a message, no launch.  Host memory
    stands in for the device buffers: every call below is one the library refuses."""
    lib, err = hiplib._lib, hiplib.last_error
    buf = (C.c_float * 64)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)
    five = (C.c_void_p * 5)(*([p.value] * 5))
    assert lib.rn_percep_image_floats() == 364 * 64 + 1600 * 192 + 1728 * 384 + 3456 * 256 + 2304 * 256 \
        + 4800 * 64 + 3456 * 192 + 2304 * 384 + 2304 * 256 + 2 * 1152 + 8
    assert lib.rn_percep_workspace(1, 31, 31) > 0 and lib.rn_percep_workspace(3, 32, 32) > lib.rn_percep_workspace(1, 32, 32)
    assert lib.rn_percep_workspace(0, 31, 31) == 0 and lib.rn_percep_workspace(1, 30, 31) == 0 and lib.rn_percep_workspace(1, 31, 30) == 0
    assert lib.rn_percep_pack(None, five, five, p, p, None) == -1 and "null pointer" in err()
    four = (C.c_void_p * 5)(p.value, p.value, None, p.value, p.value)
    assert lib.rn_percep_pack(five, four, five, p, p, None) == -1 and "layer 3" in err()
    off, c, oh, ow = C.c_size_t(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    assert lib.rn_percep_tap(1, 37, 50, 1, C.byref(off), C.byref(c), C.byref(oh), C.byref(ow)) == 0
    assert (c.value, oh.value, ow.value) == (192, 3, 5) and off.value == 64 * 2 * 8 * 11
    assert lib.rn_percep_tap(1, 37, 50, 5, C.byref(off), C.byref(c), C.byref(oh), C.byref(ow)) == -1 and "layer" in err()
    assert lib.rn_percep_tap(1, 30, 50, 0, C.byref(off), C.byref(c), C.byref(oh), C.byref(ow)) == -1 and "31" in err()
    assert lib.rn_percep_tap_values(1, 37, 50, C.byref(off)) == 0 and 0 < off.value * 4 < lib.rn_percep_workspace(1, 37, 50)
    assert lib.rn_percep_tap_values(0, 37, 50, C.byref(off)) == -1 and lib.rn_percep_tap_values(1, 37, 50, None) == -1
    big = lib.rn_percep_workspace(1, 31, 31)

    def fwd(P=1, h=31, w=31, image=p, ws=p, nbytes=big, pred=p, target=p, out=p):
        return lib.rn_percep_forward(image, ws, nbytes, pred, 3 * h * w, 1, h * w, target, 3 * h * w, 1, h * w, P, h, w, 0, out, None)

    def bwd(P=1, h=31, w=31, image=p, ws=p, nbytes=big, up=p, ustride=0, g=p):
        return lib.rn_percep_backward(image, ws, nbytes, up, ustride, g, 3 * h * w, 1, h * w, P, h, w, 0, None, None)

    for call in (fwd, bwd):
        assert call(P=0) == -1 and "P must be positive" in err()
        assert call(h=30) == -1 and "31 x 31" in err()
        assert call(w=30) == -1 and "31 x 31" in err()
        assert call(image=None) == -1 and "null pointer" in err()
        assert call(ws=None) == -1 and "null pointer" in err()
        assert call(nbytes=big - 4) == -1 and "rn_percep_workspace" in err()
        assert call(ws=C.c_void_p(p.value + 4)) == -1 and "16-byte" in err()
    assert fwd(pred=None) == -1 and fwd(target=None) == -1 and fwd(out=None) == -1 and "null pointer" in err()
    assert bwd(up=None) == -1 and bwd(g=None) == -1 and "null pointer" in err()
    assert bwd(ustride=2) == -1 and "upstream_stride" in err()
