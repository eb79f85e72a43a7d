"""Float64 restatement of the volume-rendering compositors and of the marcher's backward, written from the operations'
definitions, with an fp32 error bound for every output element.  Runs on the CPU, in numpy; the kernels under test are
k_composite_train_fwd / k_composite_train_bwd / k_march_train_backward (rn_raymarching.hip) and composite_ray (rn_ray_dev.h).

    ref = train_reference(case)                    # forward values, closed-form backward, write mask, bounds, knife-edge flags
    check_train_forward(case, dict(ws=, ambient_sum=, depth=, image=))           # plain numpy outputs of an implementation
    check_train_backward(case, dict(grad_sigmas=, grad_rgbs=, grad_ambient=))    # buffers that held SENTINEL on entry
    check_inference(case, composite_cases.run_inference(case, fn))
    check_march_backward(case, dict(grad_rays_o=, grad_rays_d=))

The CPU test hands the oracle's outputs to the check_* functions, the GPU test the kernels': the assertions are the same.

The operations
    x_j = sigma_j delta_j,  e_j = exp(-x_j),  alpha_j = 1 - e_j,  T_j = prod_{i<j} e_i  (the transmittance before sample j),
    w_j = alpha_j T_j.
  Training: a ray (index, offset, count) sums w_j, w_j c_j, w_j t_j and the ambient over its first L samples, L - 1 being the
  first j with T_{j+1} < T_thresh (L = count without one); count == 0 or offset + count > M gives zeros.  Its backward is the
  gradient of that sum with L frozen:
    d/d c_j = g_image w_j,   d/d ambient_j = g_ambient,
    d/d sigma_j = delta_j (g_image . (T_{j+1} c_j - sum_{j<i<L} w_i c_i) + g_ws T_L)
  (d w_i / d sigma_j is delta_j T_{j+1} for i = j and -delta_j w_i for i > j; sum_{j<i<L} w_i = T_{j+1} - T_L).  depth
  receives no gradient.  Rows j >= L, rows of skipped rays and rows of no ray are not written.
  Inference: an entry of the alive list adds its n_step slots to its ray's accumulators with T = 1 - weights_sum at every
  sample; a slot with delta == 0 ends the ray, and so does a pre-sample T < T_thresh, after that sample has been blended; a
  ray that ends leaves the list (-1) and keeps its rays_t, one that goes on takes the t of its last sample.
  Marcher backward: grad_rays_o[n] += sum gx, grad_rays_d[n] += sum (t gx + gd), by the row n of `rays`.

The error model (magnitudes in units of u = 2^-24; an fp32 implementation must stay within K[output] * u * magnitude)
  * alpha_j and 1 - alpha_j are each known to an ABSOLUTE unit, not a relative one: exp(-x) <= 1 is rounded at 2^-24 and
    1 - exp(-x) inherits that (x = 1e-12 gives alpha = 0).  So the error of e_j as a factor of T is 1 unit, and
        E_T(0) = 0,  E_T(j+1) = E_T(j) e_j + T_j + T_{j+1}          (the factor's unit, and the product's rounding)
    which is T_{j+1} sum_{i<=j} (1 / e_i + 1): the relative error of T grows by 1 / (1 - alpha_i) per sample, so that one
    nearly opaque sample that does not yet end the ray (e_i just above T_thresh) costs every later weight up to 1 / T_thresh
    units of relative error.  Written as a recursion it needs no division and stays finite where e_i underflows in fp32.
  * E_w(j) = alpha_j E_T(j) + T_j + w_j                             (T's error, alpha's unit, the product's rounding)
  * a running sum s_j = s_{j-1} + a_j costs |s_j| per addition, a product its own magnitude.
  * the backward's `c_final - c_running` carries the forward's bound of c_final (the kernel is given the forward's output) and
    the running sum's; `1 - ws_final` carries the forward's bound of ws and one unit.
  * inference: T = 1 - ws carries E_ws + 1, and since 1 - ws' = (1 - ws)(1 - alpha) what ws carries in is damped by
    1 - alpha: E_ws' = E_ws (1 - alpha) + T + alpha + w + ws'.  The accumulators' bounds run on across the calls of a frame.
Knife edges: a tested T within its own bound of T_thresh, K[ws] * u * E_T, is not decided in fp32; the ray is flagged and
left out of the value comparisons (for inference from that call on).  The training T is a product of non-negative factors, so
`T < 0` is decided whatever the error; the inference T = 1 - ws is not, and a ray whose T comes within its bound of 0 is
flagged as well.  The flagged share of every case is asserted in test_compref64.py.
"""
import functools

import numpy as np

import composite_cases as cc

U = 2.0 ** -24
# 4 x the worst ratio error / (u * magnitude) that the CPU oracle (libm expf, the operator's order of operations) needs over
# all cases of composite_cases.py, rounded up to the next tenth (0.05 below 1); the factor covers __expf's argument rounding (at most about
# x e^-x log2(e) u < 0.6 u of exp(-x)) and another association of the running sums.  test_compref64.py prints the ratios and
# asserts that 4 x ratio stays within these; DESIGN.md carries the table.
K = {
    "ws": 2.0, "ambient_sum": 3.2, "depth": 2.0, "image": 2.0,
    "grad_sigmas": 0.85, "grad_rgbs": 2.7,
    "inf_ws": 2.1, "inf_depth": 2.1, "inf_image": 2.1,
    "grad_rays_o": 3.8, "grad_rays_d": 3.1,
}


def _pad(case, M):
    """[N, Kmax] views of the rays' samples; `cnt` is 0 for a ray that the operator skips."""
    rays = case["rays"].astype(np.int64)
    off, cnt = rays[:, 1], rays[:, 2].copy()
    cnt[off + cnt > M] = 0
    Kmax = max(int(cnt.max(initial=0)), 1)
    j = np.arange(Kmax)[None]
    valid = j < cnt[:, None]
    rows = np.where(valid, off[:, None] + j, 0)
    return rays[:, 0], off, cnt, valid, rows


@functools.lru_cache(maxsize=None)
def _train_reference(name, M):
    case = cc.train_case(name)
    index, off, cnt, valid, rows = _pad(case, M)
    N, Kmax = valid.shape
    f8 = lambda a: a.astype(np.float64)  # noqa: E731
    x = f8(case["sigmas"])[rows] * f8(case["deltas"][:, 0])[rows] * valid
    dt = f8(case["deltas"][:, 0])[rows] * valid
    t = f8(case["deltas"][:, 1])[rows] * valid
    c = f8(case["rgbs"])[rows] * valid[..., None]
    amb = f8(case["ambient"])[rows] * valid
    Tth = case["T_thresh"]

    e, alpha = np.exp(-x), -np.expm1(-x)
    Ta = np.cumprod(e, 1)                                   # after the sample
    Tb = np.concatenate([np.ones((N, 1)), Ta[:, :-1]], 1)   # before it
    below = (Ta < Tth) & valid
    L = np.where(below.any(1), below.argmax(1) + 1, cnt)
    v = np.arange(Kmax)[None] < L[:, None]

    # bounds of T and w, in units
    ETb, ETa = np.zeros((N, Kmax)), np.zeros((N, Kmax))
    for j in range(Kmax):
        if j:
            ETb[:, j] = ETa[:, j - 1]
        ETa[:, j] = ETb[:, j] * e[:, j] + Tb[:, j] + Ta[:, j]
    flagged = np.zeros(N, bool)
    if Tth > 0:
        flagged = ((np.abs(Ta - Tth) <= K["ws"] * U * ETa) & v).any(1)

    w = alpha * Tb * v
    Ew = (alpha * ETb + Tb + w) * v
    wc, wt = w[..., None] * c, w * t
    cs_w, cs_c, cs_t, cs_a = np.cumsum(w, 1), np.cumsum(wc, 1), np.cumsum(wt, 1), np.cumsum(amb * v, 1)
    ws, image, depth, ambient_sum = w.sum(1), wc.sum(1), wt.sum(1), (amb * v).sum(1)
    mag_ws = ((Ew + cs_w) * v).sum(1)
    part_c = np.cumsum((Ew[..., None] * np.abs(c) + np.abs(wc) + np.abs(cs_c)) * v[..., None], 1)    # bound of the running colour
    mag_image = part_c[:, -1]
    mag_depth = ((Ew * np.abs(t) + np.abs(wt) + np.abs(cs_t)) * v).sum(1)
    mag_amb = (np.abs(cs_a) * v).sum(1)

    def by_index(a):
        out = np.zeros_like(a)
        out[index] = a
        return out

    fwd = {k: by_index(a) for k, a in dict(ws=ws, ambient_sum=ambient_sum, depth=depth, image=image).items()}
    fwd_mag = {k: by_index(a) for k, a in dict(ws=mag_ws, ambient_sum=mag_amb, depth=mag_depth, image=mag_image).items()}

    # the backward, in closed form; the incoming gradients are read at [index]
    g_ws, g_am, g_im = f8(case["g_ws"])[index], f8(case["g_am"])[index], f8(case["g_im"])[index]
    suffix = np.cumsum(wc[:, ::-1], 1)[:, ::-1] - wc                                  # sum_{j<i<L} w_i c_i
    T_L = np.where(L > 0, np.take_along_axis(Ta, np.maximum(L - 1, 0)[:, None], 1)[:, 0], 1.0)
    term = Ta[..., None] * c - suffix
    inner = (g_im[:, None] * term).sum(-1) + (g_ws * T_L)[:, None]
    gs = dt * inner * v
    gr = g_im[:, None] * w[..., None]
    ga = np.broadcast_to(g_am[:, None], (N, Kmax))
    E_term = (ETa[..., None] + Ta[..., None]) * np.abs(c) + mag_image[:, None] + part_c + np.abs(suffix) + np.abs(term)
    gterm = np.abs(g_im[:, None] * term)
    E_gws = np.abs(g_ws) * (mag_ws + 1.0 + T_L)
    E_inner = (np.abs(g_im)[:, None] * E_term).sum(-1) + gterm.sum(-1) + E_gws[:, None] \
        + 3.0 * (gterm.sum(-1) + np.abs(g_ws * T_L)[:, None])
    mag_gs = dt * (E_inner + np.abs(inner)) * v
    mag_gr = np.abs(g_im)[:, None] * (Ew + w)[..., None]

    R = case["rows"]
    mask = np.zeros(R, bool)
    grad = dict(grad_sigmas=np.zeros(R), grad_rgbs=np.zeros((R, 3)), grad_ambient=np.zeros(R))
    grad_mag = dict(grad_sigmas=np.zeros(R), grad_rgbs=np.zeros((R, 3)))
    flag_rows = np.zeros(R, bool)
    sel = rows[v]
    mask[sel] = True
    grad["grad_sigmas"][sel], grad["grad_rgbs"][sel], grad["grad_ambient"][sel] = gs[v], gr[v], ga[v]
    grad_mag["grad_sigmas"][sel], grad_mag["grad_rgbs"][sel] = mag_gs[v], mag_gr[v]
    # every row of a flagged ray's slice is left out: where it stops writing is what fp32 does not decide
    fl_rows = rows[valid & flagged[:, None]]
    flag_rows[fl_rows] = True
    live = cnt > 0
    return dict(fwd=fwd, fwd_mag=fwd_mag, grad=grad, grad_mag=grad_mag, mask=mask, flag_rows=flag_rows,
                flagged=by_index(flagged), L=L, live=int(live.sum()), truncated=int((L < cnt).sum()),
                share=float(flagged.sum()) / max(int(live.sum()), 1))


def train_reference(case, M=None):
    """`M`: the budget the operator is given (default: the case's, which cuts the last rays off)."""
    return _train_reference(case["name"], case["M"] if M is None else int(M))


def forward32(case, M=None):
    """The reference's forward rounded to fp32: the weights_sum / image that the C-ABI backward is handed."""
    f = train_reference(case, M)["fwd"]
    return {k: a.astype(np.float32) for k, a in f.items()}


def _within(what, got, ref, mag, k, keep=None):
    """max error / (u * magnitude) over the kept elements; asserts it within k, and exact equality where the magnitude is 0."""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    if keep is None:
        keep = np.ones(ref.shape[:1], bool)
    got, ref, mag = got[keep], ref[keep], mag[keep]
    if got.size == 0:
        return 0.0
    assert np.isfinite(got).all(), f"{what}: not finite"
    err = np.abs(got - ref)
    zero = mag == 0
    assert not (err[zero] > 0).any(), f"{what}: {int((err[zero] > 0).sum())} elements with no rounding in them are not exact"
    ratio = float((err[~zero] / (U * mag[~zero])).max(initial=0.0))
    assert ratio <= k, f"{what}: error / (2^-24 * magnitude) = {ratio:.3g} > k = {k:g}"
    return ratio


def check_train_forward(case, out, M=None):
    ref = train_reference(case, M)
    keep = ~ref["flagged"]
    return {name: _within(f"{case['name']} {name}", out[name], ref["fwd"][name], ref["fwd_mag"][name], K[name], keep)
            for name in ("ws", "ambient_sum", "depth", "image")}


def check_train_backward(case, out, M=None, sentinel=cc.SENTINEL):
    """`out`: buffers that held `sentinel` (a float, or None for buffers that were zero) in every row on entry."""
    ref = train_reference(case, M)
    keep, untouched = ref["mask"] & ~ref["flag_rows"], ~ref["mask"] & ~ref["flag_rows"]
    fill = np.float32(0 if sentinel is None else sentinel)
    for name in ("grad_sigmas", "grad_rgbs", "grad_ambient"):
        a = np.asarray(out[name])
        assert a.dtype == np.float32 and a.shape == ref["grad"][name].shape, f"{case['name']} {name}: {a.dtype} {a.shape}"
        bad = a[untouched].view(np.uint32) != fill.view(np.uint32)
        assert not bad.any(), f"{case['name']} {name}: {int(bad.sum())} values of rows that belong to no gradient were written"
    ga = np.asarray(out["grad_ambient"])[keep]
    assert np.array_equal(ga, ref["grad"]["grad_ambient"][keep].astype(np.float32)), f"{case['name']} grad_ambient: not the ray's gradient"
    return {name: _within(f"{case['name']} {name}", out[name], ref["grad"][name], ref["grad_mag"][name], K[name], keep)
            for name in ("grad_sigmas", "grad_rgbs")}


# ------------------------------------------------------------------------------------------------ inference

@functools.lru_cache(maxsize=None)
def _infer_reference(name):
    case = cc.infer_case(name)
    R, s, Tth = case["R"], case["n_step"], case["T_thresh"]
    f8 = lambda a: a.astype(np.float64)  # noqa: E731
    sig, dl, tt, col = f8(case["sigmas"]), f8(case["deltas"][..., 0]), f8(case["deltas"][..., 1]), f8(case["rgbs"])
    alive = np.zeros(R, bool)
    listed = case["alive"] if case["limit"] is None else case["alive"][: case["limit"]]
    alive[listed] = True
    ws, dp, im, rt = f8(case["ws0"]), f8(case["depth0"]), f8(case["image0"]), case["rays_t0"].copy()
    E_ws, E_dp, E_im = np.zeros(R), np.zeros(R), np.zeros((R, 3))
    flagged = np.zeros(R, bool)
    calls = []
    for c in range(case["calls"]):
        alive_in = alive.copy()
        ended = np.zeros(R, bool)
        tlast = rt.copy()
        for j in range(c * s, (c + 1) * s):
            proc = alive & ~ended
            ended |= proc & (dl[:, j] == 0)
            go = proc & ~ended
            T = 1.0 - ws
            E_T = E_ws + 1.0
            flagged |= go & (np.abs(T - Tth) <= K["inf_ws"] * U * E_T)
            a = np.where(go, -np.expm1(-sig[:, j] * dl[:, j]), 0.0)
            w = a * T
            E_w = np.where(go, a * E_T + T + w, 0.0)
            ws = ws + w
            dp = dp + w * tt[:, j]
            im = im + w[:, None] * col[:, j]
            # 1 - ws' = (1 - ws)(1 - alpha): what ws carries in is damped by 1 - alpha; the rest is this sample's own
            E_ws = E_ws * (1.0 - a) + go * (T + a + w + np.abs(ws))
            E_dp = E_dp + E_w * tt[:, j] + w * tt[:, j] + go * np.abs(dp)
            E_im = E_im + (E_w + w)[:, None] * col[:, j] + go[:, None] * np.abs(im)
            tlast = np.where(go, case["deltas"][:, j, 1], tlast)
            ended |= go & (T < Tth)
        alive = alive & ~ended
        rt = np.where(alive, tlast, rt).astype(np.float32)
        calls.append(dict(alive_in=alive_in, alive_out=alive.copy(), rays_t=rt.copy(), ws=ws.copy(), depth=dp.copy(), image=im.copy(),
                          mag=dict(ws=E_ws.copy(), depth=E_dp.copy(), image=E_im.copy()), flagged=flagged.copy()))
    return dict(calls=calls, share=float(flagged.sum()) / max(len(listed), 1))


def infer_reference(case):
    return _infer_reference(case["name"])


def check_inference(case, outs):
    """`outs`: what composite_cases.run_inference returns for an implementation."""
    ref = infer_reference(case)
    assert len(outs) == case["calls"]
    prev = dict(rays_t=case["rays_t0"], ws=case["ws0"], depth=case["depth0"], image=case["image0"])
    ratios = {"inf_ws": 0.0, "inf_depth": 0.0, "inf_image": 0.0}
    for c, (o, r) in enumerate(zip(outs, ref["calls"])):
        what = f"{case['name']} call {c}"
        fl_before = ref["calls"][c - 1]["flagged"] if c else np.zeros(case["R"], bool)
        a_in, a_out = np.asarray(o["alive_in"]), np.asarray(o["alive_out"])
        limit = a_in.size if case["limit"] is None else case["limit"]
        # the list that went in: the reference's survivors, in the order of the first list (flagged rays may differ)
        expect_in = np.array([i for i in case["alive"] if r["alive_in"][i] and not fl_before[i]], np.int64)
        assert np.array_equal(a_in[:limit][~fl_before[a_in[:limit]]], expect_in), f"{what}: the compacted alive list is not the reference's"
        assert np.array_equal(a_out[limit:], a_in[limit:]), f"{what}: an entry past the device-side count was touched"
        ray = a_in[:limit]
        ok = ~r["flagged"][ray]
        want = np.where(r["alive_out"][ray], ray, -1)
        assert np.array_equal(a_out[:limit][ok], want[ok]), f"{what}: {int((a_out[:limit][ok] != want[ok]).sum())} alive flags differ"
        touched = np.zeros(case["R"], bool)
        touched[ray] = True
        keep = touched & ~r["flagged"]
        assert np.array_equal(np.asarray(o["rays_t"])[keep].view(np.uint32), r["rays_t"][keep].view(np.uint32)), f"{what}: rays_t"
        for name in ("rays_t", "ws", "depth", "image"):
            same = np.asarray(o[name])[~touched].view(np.uint32) == np.asarray(prev[name])[~touched].view(np.uint32)
            assert same.all(), f"{what}: {name} of a ray that is not in the list was written"
        for name in ("ws", "depth", "image"):
            ratio = _within(f"{what} {name}", o[name], r[name], r["mag"][name], K["inf_" + name], keep)
            ratios["inf_" + name] = max(ratios["inf_" + name], ratio)
        prev = o
    return ratios


# ------------------------------------------------------------------------------------------------ marcher backward

@functools.lru_cache(maxsize=None)
def _march_reference(name, M):
    case = cc.train_case(name)
    _, off, cnt, valid, rows = _pad(case, M)
    f8 = lambda a: a.astype(np.float64)  # noqa: E731
    gx, gd = f8(case["gx"])[rows] * valid[..., None], f8(case["gd"])[rows] * valid[..., None]
    t = (f8(case["deltas"][:, 1])[rows] * valid)[..., None]
    vv = valid[..., None]
    po = f8(case["go0"])[:, None] + np.cumsum(gx, 1)
    term = t * gx + gd
    pd = f8(case["gd0"])[:, None] + np.cumsum(term, 1)
    out = dict(grad_rays_o=po[:, -1], grad_rays_d=pd[:, -1])
    mag = dict(grad_rays_o=(np.abs(po) * vv).sum(1), grad_rays_d=((np.abs(t * gx) + np.abs(term) + np.abs(pd)) * vv).sum(1))
    return dict(out=out, mag=mag)


def march_reference(case, M=None):
    return _march_reference(case["name"], case["M"] if M is None else int(M))


def check_march_backward(case, out, M=None):
    ref = march_reference(case, M)
    return {name: _within(f"{case['name']} {name}", out[name], ref["out"][name], ref["mag"][name], K[name])
            for name in ("grad_rays_o", "grad_rays_d")}
