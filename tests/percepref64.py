"""The perceptual (LPIPS-alex) arithmetic of include/radnerf_train.h in plain torch on the CPU, float64 by default: the yardstick of
tests/test_percep_host.py, tests/test_gpu_percep.py and tests/test_gpu_percep_step.py.  Independent of radnerf/percep.py.

Weights are seeded (nothing trained, nothing from a package): torch.Generator().manual_seed(7); for conv 1..5 the weight
randn * sqrt(2 / (Cin k^2)) then the bias randn * 0.1; then five lin vectors rand(1,C,1,1) / C (non-negative, as the package's).
Inputs come from manual_seed(seed): pred = rand(P,3,h,w) then target = rand(P,3,h,w), drawn in fp32 and widened, so that every
precision sees the same numbers.

Besides the whole computation (`reference`) the module has the single steps the GPU tests recompute from the kernels' own
intermediate maps, each with the sum of absolute values that scales its rounding bound:
  forward_layer    conv l (+ the pool before it) from tap l-1         -> pre-activation, sum |w x| + |b|
  distance         per-tap value [P] and d value / d tap (closed form) -> with their absolute-value evaluations
  input_grad       the data gradient of conv l from dZ                 -> value, sum |w| |dz|, terms per element
  pool_route       a pooled map's gradient back to the first maximum of each window
At a position whose channels are all zero d|x|/dx is taken as 0 (the kernels' decision; torch's sqrt backward gives NaN).
"""
import functools

import torch
import torch.nn.functional as F

LAYERS = ((3, 64, 11, 4, 2), (64, 192, 5, 1, 2), (192, 384, 3, 1, 1), (384, 256, 3, 1, 1), (256, 256, 3, 1, 1))   # cin, cout, k, stride, pad
POOL_BEFORE = (False, True, True, False, False)
SHIFT, SCALE = (-.030, -.088, -.188), (.458, .448, .450)
MARGIN = 2e-5
# (P, h, w) -> seed whose float64 run keeps every pre-activation and every pool arg-max MARGIN away from a flip
# (found by a search on the CPU: at 96 x 80 seeds 0..4 fail the condition, e.g. seed 0 with 4.2e-6 / 7.1e-6, seed 5 has 2.2e-5 / 4.7e-5)
USABLE_SEEDS = {(1, 31, 31): 0, (1, 37, 50): 0, (3, 32, 32): 0, (1, 96, 80): 5}


@functools.lru_cache(maxsize=None)
def seeded_weights():
    """-> (weights [5], biases [5], lins [5] as [1,C,1,1], shift_scale [6]) in fp32."""
    g = torch.Generator().manual_seed(7)
    ws, bs = [], []
    for cin, cout, k, _, _ in LAYERS:
        ws.append(torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5)
        bs.append(torch.randn(cout, generator=g) * 0.1)
    lins = [torch.rand(1, cout, 1, 1, generator=g) / cout for _, cout, _, _, _ in LAYERS]
    return ws, bs, lins, torch.tensor(SHIFT + SCALE, dtype=torch.float32)


def inputs(P, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    pred = torch.rand(P, 3, h, w, generator=g)
    target = torch.rand(P, 3, h, w, generator=g)
    return pred, target


def scale_input(x, normalize, shift_scale):
    ss = shift_scale.to(x.dtype)
    if normalize:
        x = 2 * x - 1
    return (x - ss[:3].view(1, 3, 1, 1)) / ss[3:].view(1, 3, 1, 1)


def out_size(l, h, w):
    _, _, k, stride, pad = LAYERS[l]
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


def forward_layer(l, x, weight, bias, with_abs=False):
    """x: the layer's source map [P,Cin,h,w] -- the scaled image for l = 0, else tap l-1 (pooled here where the layer pools).
    -> pre-activation [P,Cout,oh,ow] (and sum_k |w x| + |b| when asked)."""
    cin, cout, k, stride, pad = LAYERS[l]
    if POOL_BEFORE[l]:
        x = F.max_pool2d(x, 3, 2)
    P, _, h, w = x.shape
    oh, ow = out_size(l, h, w)
    cols = F.unfold(x, k, padding=pad, stride=stride)
    W, b = weight.to(x.dtype).view(cout, -1), bias.to(x.dtype).view(1, cout, 1)
    z = (W @ cols + b).view(P, cout, oh, ow)
    if not with_abs:
        return z
    return z, (W.abs() @ cols.abs() + b.abs()).view(P, cout, oh, ow)


def _norm(x):
    s = (x * x).sum(1, keepdim=True)
    live = s > 0
    return torch.sqrt(torch.where(live, s, torch.ones_like(s))) * live      # sqrt with a zero gradient at 0


def distance(x, y, lin):
    """Tap distance of [P,C,h,w] maps: -> value [P]."""
    lin = lin.to(x.dtype).view(1, -1, 1, 1)
    nx, ny = x / (_norm(x) + 1e-10), y / (_norm(y) + 1e-10)
    return (lin * (nx - ny) ** 2).sum(1, keepdim=True).mean((2, 3)).view(-1)


def distance_closed_form(x, y, lin):
    """-> (value [P], its absolute-value evaluation [P], D = d value[p] / d x [P,C,h,w], the absolute-value evaluation of D)."""
    lin = lin.to(x.dtype).view(1, -1, 1, 1)
    hw = x.shape[2] * x.shape[3]
    nx, ny = _norm(x), _norm(y)
    dx, dy = nx + 1e-10, ny + 1e-10
    diff, adiff = x / dx - y / dy, x.abs() / dx + y.abs() / dy
    value, avalue = (lin * diff ** 2).sum(1).mean((1, 2)), (lin * adiff ** 2).sum(1).mean((1, 2))
    u, au = 2 * lin * diff / hw, 2 * lin * adiff / hw
    safe = torch.where(nx > 0, nx, torch.ones_like(nx))
    back = torch.where(nx > 0, (u * x).sum(1, keepdim=True) / (dx * dx * safe), torch.zeros_like(nx))
    aback = torch.where(nx > 0, (au * x.abs()).sum(1, keepdim=True) / (dx * dx * safe), torch.zeros_like(nx))
    return value, avalue, u / dx - x * back, au / dx + x.abs() * aback


def input_grad(l, dz, weight, in_hw):
    """The data gradient of conv l: dz [P,Cout,oh,ow] (already ReLU-masked) -> (d input [P,Cin,h,w], sum |w| |dz|, number of
    products per element) for an input of spatial size in_hw (after the pool, where the layer pools)."""
    cin, cout, k, stride, pad = LAYERS[l]
    P = dz.shape[0]
    W = weight.to(dz.dtype).view(cout, -1)
    flat = dz.reshape(P, cout, -1)
    fold = lambda cols: F.fold(cols, in_hw, k, padding=pad, stride=stride)
    terms = cout * fold(torch.ones(1, k * k, flat.shape[2], dtype=dz.dtype))         # [1,1,h,w]
    return fold(W.t() @ flat), fold(W.abs().t() @ flat.abs()), terms


def pool_route(tap, g):
    """Gradient g of max_pool2d(tap, 3, 2) back onto tap (first maximum of each window in row-major order, torch's choice)."""
    t = tap.detach().clone().requires_grad_()
    (out,) = torch.autograd.grad(F.max_pool2d(t, 3, 2), t, grad_outputs=g)
    return out


def margins(zs, taps):
    """(smallest |pre-activation| / rms of its layer, smallest gap between the two largest values of a pool window whose maximum is
    positive) over both images' maps."""
    pre = min(float(z.abs().min() / z.pow(2).mean().sqrt()) for z in zs)
    gap = float("inf")
    for l in (0, 1):                                     # the taps that are pooled
        t = taps[l]
        P, C, h, w = t.shape
        win = F.unfold(t, 3, stride=2).view(P, C, 9, -1)
        top = win.topk(2, dim=2).values
        live = top[:, :, 0] > 0
        if bool(live.any()):
            gap = min(gap, float((top[:, :, 0] - top[:, :, 1])[live].min()))
    return pre, gap


@functools.lru_cache(maxsize=None)
def reference(P, h, w, seed, dtype=torch.float64, normalize=False):
    """The whole computation on the seeded weights and inputs(P, h, w, seed), pred and target as one batch of 2P images.
    -> dict(value [P], g_pred [P,3,h,w] = d sum(value) / d pred, taps [5] of [2P,C,oh,ow], tap_grads [5] of [P,C,oh,ow],
    pre_margin, pool_gap).  Cached: callers must not write into the tensors."""
    ws, bs, lins, ss = seeded_weights()
    pred, target = inputs(P, h, w, seed)
    pred = pred.to(dtype).requires_grad_()
    x = scale_input(torch.cat([pred, target.to(dtype)]), normalize, ss)
    zs, taps, halves = [], [], []
    for l in range(5):
        z = forward_layer(l, x, ws[l], bs[l])
        t = torch.relu(z)
        half = t[:P]                                    # the node the gradient of tap l is taken at
        x = torch.cat([half, t[P:]])
        zs.append(z.detach())
        taps.append(x)
        halves.append(half)
    value = sum(distance(halves[l], t[P:], lins[l]) for l, t in enumerate(taps))
    grads = torch.autograd.grad(value.sum(), [pred] + halves)
    pre, gap = margins(zs, [t.detach() for t in taps])
    return dict(value=value.detach(), g_pred=grads[0], taps=[t.detach() for t in taps], tap_grads=list(grads[1:]), pre_margin=pre,
                pool_gap=gap)


def usable(P, h, w, seed):
    r = reference(P, h, w, seed)
    return r["pre_margin"] >= MARGIN and r["pool_gap"] >= MARGIN
