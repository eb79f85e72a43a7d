"""The two loss kernels of a training step -- k_train_head_loss (csrc/rn_train_head.hip, radnerf.train_head.head_loss: blend over
the background, clamp, loss and its input gradients in one workgroup) and k_train_loss (csrc/rn_train.hip,
radnerf.train_glue.train_loss: the same on a ready prediction) -- against ONE float64 restatement of nerf/utils.py:772-803 with
the blend and clamp of nerf/renderer.py:306, at N = 1, 1023, 1024, 1025, 4097 (one workgroup of 1024 threads with a stride
loop), contiguous and strided inputs, and rows on either side of every clamp.

Tolerances.  eps = 2^-24 bounds the relative error of one fp32 rounding.  Every output is a fixed expression of a few fp32
operations on values of magnitude <= 1.2; its absolute error is bounded by k * eps * (the sum of the magnitudes of the
expression's terms) -- never by the size of the result, since pred - target and log2(1 - a) - log2(a) cancel:

* pred = clamp(image + tr * b), tr = 1 - ws: the rounding of tr (eps |tr| b), of the product (eps |tr b|; none with a fused
  multiply-add) and of the sum (eps |raw| <= eps (|image| + |tr b|))          -> 2 eps (|image| + |tr b|)
* g_image = 2 d (1 / N) / 3 on [0, 1], d = pred - target: the error of pred, the rounding of d (eps |d| <= eps (|pred| +
  |target|)), of 1 / N, of the division by 3 and of the product (3 eps |d|)   -> 4 eps (|image| + |tr b| + |pred| + |target|) * 2 / (3 N)
* the blend term of g_ws = - sum_c g_c b_c: the error of each g_c times b_c, a product and two sums (3 eps |g_c b_c|)
                                                                               -> sum_c (bound(g_c) + 3 eps |g_c|) |b_c|
* the entropy term of g_ws = 1e-4 (1 / N) (lb - la), la = log2 a, lb = log2(1 - a): log2f within 2 ulp each (2 eps (|la| + |lb|)),
  the rounding of 1 - a in lb's argument (eps / ln 2 = 1.44 eps), of the difference, of 1e-4 as a float, of 1 / N and of two
  products (5 eps |lb - la| <= 5 eps (|la| + |lb|))                            -> 8 eps (|la| + |lb| + 1) * 1e-4 / N
* g_amb = w_amb (1 / N) (1 - face): three roundings                            -> 4 eps w_amb / N
* the loss is accumulated in double from fp32 rows: with T = |image| + |tr b| + |target| (train_loss: |pred| + |target|), the
  squared difference errs by 2 |d| err(d) + 5 eps d^2 <= 11 eps T^2, the entropy by 8 eps (a |la| + (1 - a) |lb| + 1), the
  ambient term by 3 eps |ambient| w_amb
                                  -> 16 eps mean_n [mean_c T^2 + 1e-4 (a |la| + (1 - a) |lb| + 1) + w_amb |ambient|] (`scale` below)

The bars of the fp32 comparisons (test_head_loss_kernel_matches_the_pytorch_expression, test_glue_kernels_match_the_torch_
expressions) stay the upper cap: the loss and pred with their absolute bars as they are; the gradients with their relative bars
applied to the same sum of magnitudes (against float64 a relative bar on a cancelling difference cannot hold: one rounding of
pred, 6e-8, is 6e-5 of a difference of 1e-3)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
LO, HI = np.float32(1e-5), np.float32(1.0) - np.float32(1e-5)          # the entropy clamp as fp32 arithmetic has it
SIZES = [1, 1023, 1024, 1025, 4097]
W_AMB = 0.037


def loss64(target, ws, amb, face, w_amb, image=None, bg=None, pred=None):
    """Float64: pred = clamp(image + (1 - ws) bg, 0, 1) (or the given one), loss = mean_n mean_c (pred - target)^2
    + 1e-4 mean_n H(clamp(ws, 1e-5, 1 - 1e-5)) + w_amb mean_n ambient_n (1 - face_n), H(a) = -a log2 a - (1 - a) log2(1 - a);
    the clamps pass the gradient on their closed intervals.  -> (loss, pred, gradients of (image or pred, ws, amb))."""
    ws, amb = ws.double().requires_grad_(True), amb.double().requires_grad_(True)
    first = (image if pred is None else pred).double().requires_grad_(True)
    p = first if pred is not None else (first + (1.0 - ws).unsqueeze(-1) * bg.double()).clamp(0.0, 1.0)
    a = ws.clamp(float(LO), float(HI))
    entropy = -a * torch.log2(a) - (1.0 - a) * torch.log2(1.0 - a)
    loss = ((p - target.double()) ** 2).mean(-1).mean() + 1e-4 * entropy.mean() + w_amb * (amb * (1.0 - face.double())).mean()
    return loss.detach(), p.detach(), torch.autograd.grad(loss, [first, ws, amb])


def _inputs(N, strided):
    """Rows 0 .. : the special rows (as many as fit in N), then uniform rows; every value a fp32 number."""
    g = torch.Generator().manual_seed(100 + N)
    table = torch.rand(N, 15, generator=g)
    table[:, 14] = (table[:, 14] > 0.5).float()
    image = torch.rand(N, 3, generator=g) * 1.2 - 0.1                    # some blends leave [0, 1]
    ws, amb = torch.rand(N, generator=g), torch.rand(N, generator=g)
    lo, hi = torch.tensor(LO), torch.tensor(HI)
    below = lambda t: torch.nextafter(t, torch.tensor(-1.0))
    above = lambda t: torch.nextafter(t, torch.tensor(2.0))
    # (weights_sum, image row, background row): raw = image + (1 - ws) bg exactly 0.0 / 1.0 (the gradient passes), 1e-3 outside on
    # either side (it does not); the entropy clamp at its ends (passes), one fp32 neighbour outside (does not), 0, 1, 1e-6
    special = [(1.0, [0.0, 1.0, 0.5], None), (0.5, [0.75, -0.25, 0.25], [0.5, 0.5, 0.5]), (1.0, [-1e-3, 1.001, 0.5], None),
               (0.5, [0.751, -0.251, 0.25], [0.5, 0.5, 0.5]), (0.0, None, None), (1.0, None, None), (float(lo), None, None),
               (float(hi), None, None), (float(below(lo)), None, None), (float(above(hi)), None, None), (1e-6, None, None)]
    if N == 1:
        special = special[1:2]
    for i, (w, im, b) in enumerate(special[:N]):
        ws[i] = w
        if im is not None:
            image[i] = torch.tensor(im)
        if b is not None:
            table[i, 8:11] = torch.tensor(b)
    # a uniform row whose blend lies within 1e-5 of a clamp end would let fp32 and float64 decide differently: moved inside
    raw = image.double() + (1.0 - ws.double()).unsqueeze(-1) * table[:, 8:11].double()
    near = ((raw.abs() < 1e-5) | ((raw - 1.0).abs() < 1e-5)) & (raw != 0.0) & (raw != 1.0)
    image[near] = 0.4
    raw = image.double() + (1.0 - ws.double()).unsqueeze(-1) * table[:, 8:11].double()
    assert not bool((((raw.abs() < 1e-5) | ((raw - 1.0).abs() < 1e-5)) & (raw != 0.0) & (raw != 1.0)).any())
    table, image, ws, amb = table.cuda(), image.cuda(), ws.cuda(), amb.cuda()
    bg, target, face = table[:, 8:11], table[:, 11:14], table[:, 14]
    if not strided:
        bg, target, face = bg.contiguous(), target.contiguous(), face.contiguous()
    return image, ws, amb, bg, target, face, len(special[:N])


def _check(name, got, want, bound, cap):
    err = (got.double() - want).abs()
    worst = float((err / bound.clamp_min(1e-300)).max()) if bound.numel() else 0.0
    print(f"  {name:8s} max err {float(err.max()):.3e}  largest err / bound {worst:.3f}  largest bound {float(bound.max()):.3e}")
    assert bool((err <= torch.minimum(bound, cap)).all()), (name, float(err.max()), worst)


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("N", SIZES)
def test_head_loss_kernel_against_float64(hiplib, N, strided):
    from radnerf import train_head
    image, ws, amb, bg, target, face, n_special = _inputs(N, strided)
    assert bg.is_contiguous() != strided or N == 1
    w_amb = torch.tensor(W_AMB, device="cuda")
    image.requires_grad_(True), ws.requires_grad_(True), amb.requires_grad_(True)
    loss, pred = train_head.head_loss(image, ws, amb, bg, target, face, w_amb)
    loss.backward()
    l64, p64, (gi64, gw64, ga64) = loss64(target, ws.detach(), amb.detach(), face, float(w_amb), image=image.detach(), bg=bg)
    print(f"\nhead_loss N={N} strided={strided}")
    im, b, t = image.detach().double().abs(), bg.double().abs(), target.double().abs()
    trb = (1.0 - ws.detach().double()).abs().unsqueeze(-1) * b
    a = ws.detach().double().clamp(float(LO), float(HI))
    la, lb = torch.log2(a).abs(), torch.log2(1.0 - a).abs()
    b_pred = 2 * EPS * (im + trb)
    b_gi = 4 * EPS * (im + trb + p64.abs() + t) * 2.0 / (3.0 * N)
    b_gw = ((b_gi + 3 * EPS * gi64.abs()) * b).sum(-1) + 8 * EPS * (la + lb + 1.0) * 1e-4 / N
    b_ga = torch.full_like(ga64, 4 * EPS * W_AMB / N)
    scale = float((((im + trb + t) ** 2).mean(-1) + 1e-4 * (a * la + (1.0 - a) * lb + 1.0) + W_AMB * amb.detach().double().abs()).mean())
    err_loss = abs(float(loss.detach()) - float(l64))
    print(f"  loss     {float(loss.detach()):.9g}  float64 {float(l64):.9g}  err {err_loss:.3e}  bound {16 * EPS * scale:.3e}")
    assert err_loss <= min(16 * EPS * scale, 1e-6 * max(1.0, abs(float(l64))))
    _check("pred", pred, p64, b_pred, torch.full_like(p64, 1e-7))
    _check("g_image", image.grad, gi64, b_gi, 1e-10 + 1e-5 * (im + trb + p64.abs() + t) * 2.0 / (3.0 * N))
    _check("g_ws", ws.grad, gw64, b_gw, 1e-9 + 2e-5 * (((im + trb + p64.abs() + t) * 2.0 / (3.0 * N) * b).sum(-1) + (la + lb + 1.0) * 1e-4 / N))
    _check("g_amb", amb.grad, ga64, b_ga, torch.full_like(ga64, 1e-10 + 1e-5 * W_AMB / N))
    # the clamp rows decide as float64 does: the gradient passes at raw == 0.0 and 1.0 and at both ends of the entropy clamp, and
    # is exactly zero 1e-3 outside / one fp32 neighbour outside
    gi, gw = image.grad, ws.grad
    if N >= 11:
        assert n_special == 11
        assert bool((gi[0:2, 0:2] != 0).all()) and bool((gi64[0:2, 0:2] != 0).all())
        assert float(gi[2, 0]) == 0.0 and float(gi[2, 1]) == 0.0 and float(gi[3, 0]) == 0.0 and float(gi[3, 1]) == 0.0
        blend = -(gi.double() * bg.double()).sum(-1)
        for r in (6, 7):                                              # at the clamp's ends: the entropy term is there
            assert abs(float(gw[r]) - float(blend[r])) > 1e-4 / N, r
        for r in (4, 5, 8, 9, 10):                                    # outside: only the blend term
            assert abs(float(gw[r]) - float(blend[r])) <= 4 * EPS * float((gi[r].abs().double() * bg[r].double()).sum()), r
            assert abs(float(gw64[r]) - float(-(gi64[r] * bg[r].double()).sum())) <= 1e-18, r
        # rows 2 and 3: no gradient reaches image columns 0 and 1, so the blend term of g_ws has only column 2's share
        for r in (2, 3):
            assert abs(float(gw64[r]) + float(gi64[r, 2] * bg[r, 2].double())) <= 1e-18


@pytest.mark.parametrize("N", SIZES)
def test_train_loss_kernel_against_float64(hiplib, N):
    """radnerf.train_glue.train_loss on the float64 prediction rounded to fp32: the same restatement without the blend."""
    from radnerf import train_glue
    image, ws, amb, bg, target, face, _ = _inputs(N, False)
    _, p64, _ = loss64(target, ws, amb, face, W_AMB, image=image, bg=bg)
    pred = p64.float().requires_grad_(True)
    ws.requires_grad_(True), amb.requires_grad_(True)
    w_amb = torch.tensor([W_AMB], device="cuda")
    loss = train_glue.train_loss(pred, target, ws, amb, face, w_amb)
    gp, gw, ga = torch.autograd.grad(loss, [pred, ws, amb])
    l64, _, (gp64, gw64, ga64) = loss64(target, ws.detach(), amb.detach(), face, float(w_amb), pred=pred.detach())
    print(f"\ntrain_loss N={N}")
    p, t = pred.detach().double().abs(), target.double().abs()
    a = ws.detach().double().clamp(float(LO), float(HI))
    la, lb = torch.log2(a).abs(), torch.log2(1.0 - a).abs()
    scale = float((((p + t) ** 2).mean(-1) + 1e-4 * (a * la + (1.0 - a) * lb + 1.0) + W_AMB * amb.detach().double().abs()).mean())
    err_loss = abs(float(loss.detach()) - float(l64))
    print(f"  loss     {float(loss.detach()):.9g}  float64 {float(l64):.9g}  err {err_loss:.3e}  bound {16 * EPS * scale:.3e}")
    assert err_loss <= min(16 * EPS * scale, 2e-6 * abs(float(l64)))
    _check("g_pred", gp, gp64, 4 * EPS * (p + t) * 2.0 / (3.0 * N), 1e-12 + 2e-5 * (p + t) * 2.0 / (3.0 * N))
    _check("g_ws", gw, gw64, 8 * EPS * (la + lb + 1.0) * 1e-4 / N, 1e-12 + 2e-5 * (la + lb + 1.0) * 1e-4 / N)
    _check("g_amb", ga, ga64, torch.full_like(ga64, 4 * EPS * W_AMB / N), torch.full_like(ga64, 1e-12 + 2e-5 * W_AMB / N))
    if N >= 11:
        assert bool((gw[6:8] != 0).all()) and bool((gw64[6:8] != 0).all())
        for r in (4, 5, 8, 9, 10):
            assert float(gw[r]) == 0.0 and float(gw64[r]) == 0.0, r
