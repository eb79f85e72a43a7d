"""The perceptual kernels (csrc/rn_percep.hip; rn_percep_forward / rn_percep_backward; radnerf/percep.py) against the float64 helper
tests/percepref64.py on the seeded weights.

Layer by layer, every map of the workspace is held to a bound derived from the arithmetic, not from what the kernels give: a layer
is recomputed in float64 FROM THE KERNELS' OWN input map, so that only that layer's rounding is in the difference.
  forward layer   |out - out64| <= (K + 2) eps32 (sum |w x| + |b|) per element, K = Cin k^2: the worst case of an fp32 sum of K
                  products in any order (first-order bound K eps32 / 2) with the roundings of the products, the bias and, for
                  conv1, of (x - shift) / scale.  One dropped tap position is about 1 / k^2 of the sum: the test shows that it fails.
  tap values      |v - v64| <= (2 C + hw + 16) eps32 * (the same expression on absolute values): the norm is a C-term sum under a
                  square root (C / 2 + 1 roundings of each normalised value), the difference is squared (x 2), C terms are summed,
                  then hw positions.
  tap gradients   the gradient of tap l-1 is recomputed from the kernels' gradient of tap l (`keep`), their taps and the weights:
                  d = D + route(W^T (g * mask)), with |d - d64| <= (K + 3) eps32 route(sum |w| |g|) + (2 C + 16) eps32 |D|_abs,
                  K = Cout * (kernel taps that reach the element) (+ 4 where the pool routing adds up to four windows),
                  |D|_abs the closed-form distance gradient on absolute values (helper: distance_closed_form; same counting
                  as for the values).
End to end the module is held to the bars the project holds its fused kernels to against autograd (tests/test_gpu_train_head.py):
value at rtol 2e-4, gradient max |d| / max |ref| < 2e-3 with cos > 0.99999, on inputs whose float64 run keeps every ReLU and every
pool arg-max 2e-5 away from a flip; the ratio to the helper's own float32 run is printed, not asserted."""
import ctypes as C

import numpy as np
import pytest
import torch

import percepref64 as R

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
SHAPES = [(1, 31, 31), (1, 37, 50), (3, 32, 32), (1, 96, 80)]
VALUE_RTOL, GRAD_REL, GRAD_COS = 2e-4, 2e-3, 0.99999


@pytest.fixture(scope="module")
def module(hiplib):
    from radnerf.percep import PerceptualAlex
    ws, bs, lins, _ = R.seeded_weights()
    return PerceptualAlex(ws, bs, lins).cuda()


class Run:
    """One forward (+ backward) through the C ABI on a workspace the test can read."""

    def __init__(self, hip, module, pred, target, normalize=False):
        self.hip, self.normalize = hip, int(normalize)
        self.pred, self.target = pred, target
        self.P, _, self.h, self.w = pred.shape
        self.image = module.packed_image()
        self.nbytes = int(hip._lib.rn_percep_workspace(self.P, self.h, self.w))
        assert self.nbytes > 0
        self.ws = torch.full((self.nbytes // 4 + 64,), float("nan"), device="cuda")        # 64 guard floats behind the workspace
        self.value = torch.empty(self.P, device="cuda")

    @staticmethod
    def strides(t):
        s = t.stride()
        assert s[2] == t.shape[3] * s[3]
        return s[0], s[3], s[1]

    def forward(self):
        hip = self.hip
        hip.call("rn_percep_forward", hip.ptr(self.image), self.ws.data_ptr(), self.nbytes, self.pred.data_ptr(), *self.strides(self.pred),
                 self.target.data_ptr(), *self.strides(self.target), self.P, self.h, self.w, self.normalize, hip.ptr(self.value), hip.stream())
        return self

    def backward(self, upstream=None, keep=True, like=None):
        hip = self.hip
        up = torch.ones(1, device="cuda") if upstream is None else upstream
        g = torch.full_like(self.pred if like is None else like, float("nan"))
        self.keep = [torch.full((c, self.P, oh, ow), float("nan"), device="cuda") for c, oh, ow in self.dims()] if keep else None
        arr = (C.c_void_p * 5)(*[t.data_ptr() for t in self.keep]) if keep else None
        hip.call("rn_percep_backward", hip.ptr(self.image), self.ws.data_ptr(), self.nbytes, hip.ptr(up), 0 if up.numel() == 1 else 1,
                 g.data_ptr(), *self.strides(g), self.P, self.h, self.w, self.normalize, arr, hip.stream())
        torch.cuda.synchronize()
        assert bool(torch.isnan(self.ws[-64:]).all()), "a kernel wrote behind the workspace"
        return g

    def dims(self):
        out = []
        for l in range(5):
            off, c, oh, ow = C.c_size_t(), C.c_uint32(), C.c_uint32(), C.c_uint32()
            assert self.hip._lib.rn_percep_tap(self.P, self.h, self.w, l, C.byref(off), C.byref(c), C.byref(oh), C.byref(ow)) == 0
            out.append((c.value, oh.value, ow.value))
        return out

    def tap(self, l):
        """Tap l as [2P,C,oh,ow] float64 on the CPU."""
        off, c, oh, ow = C.c_size_t(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        assert self.hip._lib.rn_percep_tap(self.P, self.h, self.w, l, C.byref(off), C.byref(c), C.byref(oh), C.byref(ow)) == 0
        n = c.value * 2 * self.P * oh.value * ow.value
        return self.ws[off.value:off.value + n].view(c.value, 2 * self.P, oh.value, ow.value).permute(1, 0, 2, 3).double().cpu()

    def tap_values(self):
        off = C.c_size_t()
        assert self.hip._lib.rn_percep_tap_values(self.P, self.h, self.w, C.byref(off)) == 0
        return self.ws[off.value:off.value + 5 * self.P].view(5, self.P).double().cpu()

    def kept(self, l):
        return self.keep[l].permute(1, 0, 2, 3).double().cpu()


def _run(hiplib, module, shape, normalize=False):
    pred, target = R.inputs(*shape, R.USABLE_SEEDS[shape])
    return Run(hiplib, module, pred.cuda(), target.cuda(), normalize).forward()


CASES = [(s, False) for s in SHAPES] + [((1, 37, 50), True)]


@pytest.mark.parametrize("shape,normalize", CASES)
def test_forward_layer_by_layer(hiplib, module, shape, normalize):
    ws, bs, lins, ss = R.seeded_weights()
    run = _run(hiplib, module, shape, normalize)
    torch.cuda.synchronize()
    P = shape[0]
    src = R.scale_input(torch.cat([run.pred, run.target]).double().cpu(), normalize, ss)
    for l, (cin, cout, k, _, _) in enumerate(R.LAYERS):
        got = run.tap(l)
        z, base = R.forward_layer(l, src, ws[l], bs[l], with_abs=True)
        bound = (cin * k * k + 2) * EPS32 * base
        err = (got - torch.relu(z)).abs()
        print(f"{shape} normalize={normalize} conv{l + 1}: [{cout}] x [{got.shape[0] * got.shape[2] * got.shape[3]}], max err / bound = {float((err / bound).max()):.4f}")
        assert got.shape == z.shape and bool((err <= bound).all()), (l, float((err / bound).max()))
        if l in (0, 2) and shape == (1, 37, 50):           # the bound is sharp: drop one tap position (the centre one, which no
            w = ws[l].clone()                              # padding ever hides) and it fails
            w[:, :, k // 2, k // 2] = 0
            z_drop = R.forward_layer(l, src, w, bs[l])
            assert not bool(((got - torch.relu(z_drop)).abs() <= bound).all())
        src = got                                          # the next layer is recomputed from the kernels' own tap
    values = run.tap_values()
    for l in range(5):
        t = run.tap(l)
        v, av, _, _ = R.distance_closed_form(t[:P], t[P:], lins[l])
        C_, hw = t.shape[1], t.shape[2] * t.shape[3]
        bound = (2 * C_ + hw + 16) * EPS32 * av
        err = (values[l] - v).abs()
        print(f"{shape} tap {l + 1} value: max err / bound = {float((err / bound).max()):.4f}")
        assert bool((err <= bound).all()), (l, values[l], v)
    want = values[0].float()                               # value_out: the five values added in tap order, fp32
    for l in range(1, 5):
        want = want + values[l].float()
    assert torch.equal(run.value.cpu(), want)


@pytest.mark.parametrize("shape,normalize", CASES)
def test_backward_layer_by_layer(hiplib, module, shape, normalize):
    ws, bs, lins, ss = R.seeded_weights()
    run = _run(hiplib, module, shape, normalize)
    g_pred = run.backward().double().cpu()
    P = shape[0]
    taps = [run.tap(l) for l in range(5)]
    dist = [R.distance_closed_form(t[:P], t[P:], lins[l]) for l, t in enumerate(taps)]

    def check(what, got, want, bound):
        ratio = float((((got - want).abs()) / bound.clamp_min(1e-300)).max())
        print(f"{shape} normalize={normalize} {what}: max err / bound = {ratio:.4f}")
        assert got.shape == want.shape and bool(torch.isfinite(got).all()) and bool(((got - want).abs() <= bound).all()), (what, ratio)

    C5 = taps[4].shape[1]
    check("gradient of tap 5 (distance alone)", run.kept(4), dist[4][2], (2 * C5 + 16) * EPS32 * dist[4][3])
    for l in range(4, 0, -1):
        g = run.kept(l) * (taps[l][:P] > 0)
        below = taps[l - 1][:P]
        in_hw = taps[l].shape[2:]                          # stride 1, "same" padding: the layer's input has its output's size
        grad, agrad, terms = R.input_grad(l, g, ws[l], tuple(in_hw))
        if R.POOL_BEFORE[l]:
            # an element collects up to four windows: each within (terms + 3) eps32 of its own sum, then up to four more additions
            grad, agrad, terms = R.pool_route(below, grad), R.pool_route(below, agrad), terms.max() + 4
        Cb = below.shape[1]
        want = dist[l - 1][2] + grad
        bound = (terms + 3) * EPS32 * agrad + (2 * Cb + 16) * EPS32 * dist[l - 1][3]
        check(f"gradient of tap {l}", run.kept(l - 1), want, bound)
    g = run.kept(0) * (taps[0][:P] > 0)
    grad, agrad, terms = R.input_grad(0, g, ws[0], (shape[1], shape[2]))
    factor = (2.0 if normalize else 1.0) / ss[3:].double().view(1, 3, 1, 1)
    check("gradient of pred", g_pred, grad * factor, (terms + 4) * EPS32 * agrad * factor)
    assert float(g_pred.abs().max()) > 0


def test_exact_properties(hiplib, module):
    shape = (1, 37, 50)
    run = _run(hiplib, module, shape)
    g1 = run.backward(keep=False)
    assert float(g1[..., 49].abs().max()) == 0.0 and float(g1[..., 48].abs().max()) > 0     # no conv1 window holds column 49
    v1 = run.value.clone()
    again = _run(hiplib, module, shape)
    g2 = again.backward(keep=False)
    assert torch.equal(again.value, v1) and torch.equal(g1, g2)                              # no atomics: the same bits
    up = torch.tensor([0.37], device="cuda")
    assert torch.equal(run.backward(upstream=up, keep=False), g1 * up)                       # one fp32 multiply
    # per-image upstream factors
    run3 = _run(hiplib, module, (3, 32, 32))
    ones = run3.backward(keep=False)
    ups = torch.tensor([0.5, -1.25, 3.0], device="cuda")
    assert torch.equal(run3.backward(upstream=ups, keep=False), ones * ups.view(3, 1, 1, 1))


def test_all_zero_positions_give_a_finite_zero_gradient(hiplib):
    """conv1 biases at -1e3: tap 1 is all zeros, pred and target then share every later tap.  d|x| / dx is taken as 0 there, so the
    value and the gradient are exactly 0 (autograd through torch's sqrt gives NaN)."""
    from radnerf.percep import PerceptualAlex
    ws, bs, lins, _ = R.seeded_weights()
    m = PerceptualAlex(ws, [torch.full_like(bs[0], -1e3)] + list(bs[1:]), lins).cuda()
    run = _run(hiplib, m, (1, 37, 50))
    g = run.backward()
    assert float(run.tap(0).abs().max()) == 0.0 and float(run.tap(4).abs().max()) > 0
    assert float(run.value.abs().max()) == 0.0
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) == 0.0
    for l in range(5):
        assert bool(torch.isfinite(run.keep[l]).all())


@pytest.mark.parametrize("shape", SHAPES)
def test_module_end_to_end_against_float64(hiplib, module, shape, monkeypatch):
    seed = R.USABLE_SEEDS[shape]
    r64 = R.reference(*shape, seed)
    assert r64["pre_margin"] >= R.MARGIN and r64["pool_gap"] >= R.MARGIN         # a condition on the input, not on the kernels
    r32 = R.reference(*shape, seed, torch.float32)
    pred, target = (t.cuda() for t in R.inputs(*shape, seed))
    out = {}
    for path in ("hip", "torch"):
        monkeypatch.setenv("RN_PERCEP", path)
        p = pred.clone().requires_grad_()
        value = module(p, target)
        assert value.shape == (shape[0], 1, 1, 1)
        (g,) = torch.autograd.grad(value.sum(), p)
        out[path] = (value.detach().view(-1).double().cpu(), g.double().cpu())
    for path, (v, g) in out.items():
        rel = float(((v - r64["value"]) / r64["value"]).abs().max())
        gerr = float((g - r64["g_pred"]).abs().max() / r64["g_pred"].abs().max())
        cos = float((g.flatten() @ r64["g_pred"].flatten()) / (g.norm() * r64["g_pred"].norm()))
        rel32 = float(((r32["value"].double() - r64["value"]) / r64["value"]).abs().max())
        gerr32 = float((r32["g_pred"].double() - r64["g_pred"]).abs().max() / r64["g_pred"].abs().max())
        print(f"{shape} RN_PERCEP={path}: value rel {rel:.2e} ({rel / rel32:.2f} x the float32 helper), gradient {gerr:.2e} of its max "
              f"({gerr / gerr32:.2f} x), 1 - cos {1 - cos:.1e}")
        assert rel < VALUE_RTOL and gerr < GRAD_REL and cos > GRAD_COS, (path, rel, gerr, cos)


def test_row_view_and_nchw_view_give_the_same_bits(hiplib, module):
    """The [n,3] rows of train_step (pixel stride 3, channel stride 1) and a contiguous NCHW copy of the same image."""
    shape = (2, 33, 40)
    pred, target = (t.cuda() for t in R.inputs(*shape, 3))
    rows_p, rows_t = (t.permute(0, 2, 3, 1).contiguous() for t in (pred, target))             # [P,h,w,3]: the rows of a batch
    view_p, view_t = rows_p.permute(0, 3, 1, 2), rows_t.permute(0, 3, 1, 2)
    assert not view_p.is_contiguous() and torch.equal(view_p, pred)
    a = Run(hiplib, module, pred, target).forward()
    ga = a.backward(keep=False)
    b = Run(hiplib, module, view_p, view_t).forward()
    gb = b.backward(keep=False, like=view_p)
    assert gb.stride() == view_p.stride()
    assert torch.equal(a.value, b.value) and torch.equal(ga, gb)
    # and through the module: the strided view goes in without a copy and gives the same bits
    p1, p2 = pred.clone().requires_grad_(), view_p.clone(memory_format=torch.preserve_format).requires_grad_()
    assert p2.stride() == view_p.stride()
    v1, v2 = module(p1, target), module(p2, view_t)
    (g1,), (g2,) = torch.autograd.grad(v1.mean(), p1), torch.autograd.grad(v2.mean(), p2)
    assert torch.equal(v1, v2) and torch.equal(g1, g2) and torch.equal(v1.view(-1), a.value)


def test_captured_forward_and_backward_replay_the_eager_bits(hiplib, module):
    shape = (3, 32, 32)
    pred, target = (t.cuda() for t in R.inputs(*shape, 0))
    run = Run(hiplib, module, pred.clone(), target.clone())
    hip = hiplib
    up = torch.tensor([0.01 / 3], device="cuda")
    g = torch.empty_like(run.pred)

    def both():
        run.forward()
        hip.call("rn_percep_backward", hip.ptr(run.image), run.ws.data_ptr(), run.nbytes, hip.ptr(up), 0, g.data_ptr(), *run.strides(g),
                 run.P, run.h, run.w, 0, None, hip.stream())

    both()                                                 # eager once: everything exists before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                          # one stream: a linear chain of launches
        both()
    new_p, new_t = (t.cuda() for t in R.inputs(*shape, 9))
    run.pred.copy_(new_p)
    run.target.copy_(new_t)
    graph.replay()
    torch.cuda.synchronize()
    v_graph, g_graph = run.value.clone(), g.clone()
    eager = Run(hiplib, module, new_p, new_t).forward()
    g_eager = eager.backward(upstream=up, keep=False)
    assert torch.equal(v_graph, eager.value) and torch.equal(g_graph, g_eager)
    old = Run(hiplib, module, pred, target).forward()
    torch.cuda.synchronize()
    assert not torch.equal(v_graph, old.value)
