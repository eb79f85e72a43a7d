"""float64 reference of the audio code (csrc/rn_audio.hip): NeRFNetwork.encode_audio = AudioNet on every frame of a window
[+ AudioAttNet over the 8 frames], its backward, the window cutting of get_audio_features(feats, 2, i) and the lip-smoothing
recurrence -- restated in plain numpy, with explicit loops over input channels and taps, calling no torch module.

The same restatement runs in three arithmetics: float64 (THE reference), and float32 with every dot product summed in ascending
or in descending index order.  Together with the project's own nn.Modules in fp32 on the CPU those are the three `evaluations`
that measure how far honest fp32 arithmetic lies from float64: for a compared tensor T,

    E_T = max over evaluations and elements of |eval - ref64|,   floored at u * max|ref64|,   u = 2^-24.

tests/test_gpu_audio_ref.py holds the kernels to 4 * E_T per element.

Tensor order everywhere: rn_audio_grads_t -- conv_w[4], conv_b[4], fc_w[2], fc_b[2] | att_conv_w[5], att_conv_b[5], att_fc_w,
att_fc_b (NAMES); without attention the first 12.
"""
import functools
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24
SLOPE32 = np.float32(0.02)                       # the constant the kernels hold (leaky / leaky_grad)
SEQ, WIN = 8, 16
NAMES = ([f"conv_w{l}" for l in range(4)] + [f"conv_b{l}" for l in range(4)] + ["fc_w0", "fc_w1", "fc_b0", "fc_b1"]
         + [f"att_conv_w{l}" for l in range(5)] + [f"att_conv_b{l}" for l in range(5)] + ["att_fc_w", "att_fc_b"])
ACT_NAMES = ("y1", "y2", "y3", "y4", "y5")       # kept activations, the kActs layout y1 [32][8] | y2 [32][4] | y3 [64][2] | y4 [64] | y5 [64]
K_ACTS = 32 * 8 + 32 * 4 + 64 * 2 + 64 + 64
DIM_PAIRS = ((44, 64), (29, 64), (64, 29), (1, 3), (32, 1))


def gamma(k):
    return k * U / (1.0 - k * U)


# ---- the arithmetic, generic in dtype and summation order ----------------------------------------------------------------------
def _order(n, descending):
    return range(n - 1, -1, -1) if descending else range(n)


def _leaky(z, dtype):
    return np.where(z > 0, z, z * dtype(SLOPE32))


def _slope(z, dtype):
    return np.where(z > 0, dtype(1.0), dtype(SLOPE32))


def _conv(x, w, b, stride, desc):
    """Conv1d(k = 3, pad 1): x [F][cin][L], w [cout][cin][3] -> pre-activation z [F][cout][Lout], one product added at a time in
    flattened (ci, k) order (a padded tap adds w * 0 = 0, which changes nothing)."""
    F, cin, L = x.shape
    lout = (L - 1) // stride + 1
    xp = np.zeros((F, cin, L + 2), x.dtype)
    xp[:, :, 1:L + 1] = x
    acc = np.zeros((F, w.shape[0], lout), x.dtype)
    for e in _order(cin * 3, desc):
        ci, k = divmod(e, 3)
        acc += w[None, :, ci, k, None] * xp[:, ci, None, k:k + stride * lout:stride]
    return acc + b[None, :, None]


def _linear(x, w, b, desc):
    """x [F][din], w [dout][din] -> [F][dout]"""
    acc = np.zeros((x.shape[0], w.shape[0]), x.dtype)
    for k in _order(w.shape[1], desc):
        acc += w[None, :, k] * x[:, k, None]
    return acc + b[None, :]


def _sum0(a, desc):
    """Sum over the leading axis, one term at a time."""
    acc = np.zeros(a.shape[1:], a.dtype)
    for i in _order(a.shape[0], desc):
        acc += a[i]
    return acc


def _conv_bwd(x, w, dz, stride, desc, need_dx):
    """-> (gw [cout][cin][3], gb [cout], dx [F][cin][L] or None): sums over positions first, then over frames."""
    F, cin, L = x.shape
    cout, lout = dz.shape[1], dz.shape[2]
    xp = np.zeros((F, cin, L + 2), x.dtype)
    xp[:, :, 1:L + 1] = x
    gw_f = np.zeros((F, cout, cin, 3), x.dtype)
    gb_f = np.zeros((F, cout), x.dtype)
    for pos in _order(lout, desc):
        for k in range(3):
            gw_f[:, :, :, k] += dz[:, :, None, pos] * xp[:, None, :, pos * stride + k]
        gb_f += dz[:, :, pos]
    dx = None
    if need_dx:
        dxp = np.zeros((F, cin, L + 2), x.dtype)
        for co in _order(cout, desc):
            for k in range(3):
                dxp[:, :, k:k + stride * lout:stride] += w[None, co, :, k, None] * dz[:, co, None, :]
        dx = dxp[:, :, 1:L + 1]
    return _sum0(gw_f, desc), _sum0(gb_f, desc), dx


def _linear_bwd(x, w, dz, desc):
    gw = _sum0(dz[:, :, None] * x[:, None, :], desc)
    gb = _sum0(dz, desc)
    dx = np.zeros_like(x)
    for r in _order(w.shape[0], desc):
        dx += w[None, r, :] * dz[:, r, None]
    return gw, gb, dx


def forward(weights, auds, att, dtype=np.float64, desc=False):
    """weights: the 24 (12) arrays of NAMES; auds [n][frames][dim_in][16], frames = 8 with attention, 1 without.
    -> namespace: z1..z5 / y1..y5 (AudioNet pre-activations / layer outputs per frame), codes [n * frames][A], and with attention
    az / ay (lists of the five conv layers' [n][c][8]), logits, att [n][8]; enc [n][A]."""
    W = [np.asarray(t, dtype) for t in weights]
    n, frames = auds.shape[0], auds.shape[1]
    assert frames == (SEQ if att else 1) and auds.shape[3] == WIN
    r = SimpleNamespace()
    x = np.asarray(auds, dtype).reshape(n * frames, auds.shape[2], WIN)
    r.x0 = x
    for l in range(4):
        z = _conv(x, W[l], W[4 + l], 2, desc)
        x = _leaky(z, dtype)
        setattr(r, f"z{l + 1}", z)
        setattr(r, f"y{l + 1}", x)
    r.z5 = _linear(r.y4[:, :, 0], W[8], W[10], desc)
    r.y5 = _leaky(r.z5, dtype)
    r.codes = _linear(r.y5, W[9], W[11], desc)
    if not att:
        r.enc = r.codes
        return r
    A = r.codes.shape[1]
    c = r.codes.reshape(n, SEQ, A)
    a = np.ascontiguousarray(c.transpose(0, 2, 1))                 # x.permute(0, 2, 1): [A channels][8 positions]
    r.a0, r.az, r.ay = a, [], []
    for l in range(5):
        z = _conv(a, W[12 + l], W[17 + l], 1, desc)
        a = _leaky(z, dtype)
        r.az.append(z)
        r.ay.append(a)
    r.logits = _linear(a[:, 0, :], W[22], W[23], desc)
    e = np.exp(r.logits - r.logits.max(axis=1, keepdims=True))
    r.att = e / _sum0(np.ascontiguousarray(e.T), desc)[:, None]
    r.enc = _sum0(np.ascontiguousarray((r.att[:, :, None] * c).transpose(1, 0, 2)), desc)
    return r


def backward(weights, fwd, grad_enc, att, dtype=np.float64, desc=False):
    """-> (grad_codes [n * frames][A], the 24 (12) parameter gradients).  The slope of every LeakyReLU is taken from the sign of
    the pre-activation of `fwd` (in float64: of the float64 pre-activation)."""
    W = [np.asarray(t, dtype) for t in weights]
    genc = np.asarray(grad_enc, dtype)
    n, A = genc.shape
    g = [None] * (24 if att else 12)
    if att:
        c = fwd.codes.reshape(n, SEQ, A)
        datt = np.zeros((n, SEQ), dtype)
        for i in _order(A, desc):
            datt += genc[:, None, i] * c[:, :, i]
        dot = _sum0(np.ascontiguousarray((fwd.att * datt).T), desc)
        dlogit = fwd.att * (datt - dot[:, None])
        score = fwd.ay[4][:, 0, :]
        g[22], g[23], dscore = _linear_bwd(score, W[22], dlogit, desc)
        dy = dscore[:, None, :]
        for l in range(4, -1, -1):
            x = fwd.ay[l - 1] if l else fwd.a0
            dz = dy * _slope(fwd.az[l], dtype)
            g[12 + l], g[17 + l], dy = _conv_bwd(x, W[12 + l], dz, 1, desc, True)
        grad_codes = (dy.transpose(0, 2, 1) + fwd.att[:, :, None] * genc[:, None, :]).reshape(n * SEQ, A)
    else:
        grad_codes = genc
    g[9], g[11], dy = _linear_bwd(fwd.y5, W[9], grad_codes, desc)
    g[8], g[10], dy = _linear_bwd(fwd.y4[:, :, 0], W[8], dy * _slope(fwd.z5, dtype), desc)
    dy = dy[:, :, None]
    for l in range(3, -1, -1):
        x = getattr(fwd, f"y{l}") if l else fwd.x0
        dz = dy * _slope(getattr(fwd, f"z{l + 1}"), dtype)
        g[l], g[4 + l], dy = _conv_bwd(x, W[l], dz, 2, desc, l > 0)
    return grad_codes, g


def cut_window(feats, i):
    """get_audio_features(feats, 2, i): frames i-4 .. i+3 of feats [T][...], zero outside [0, T)."""
    T = feats.shape[0]
    out = np.zeros((SEQ,) + feats.shape[1:], feats.dtype)
    for t in range(SEQ):
        f = i - 4 + t
        if 0 <= f < T:
            out[t] = feats[f]
    return out


def smooth(enc, lam, state, state_valid):
    """s <- keep * s + take * e in float64 over the rows of enc [n][dim], keep = float32(lam), take = float32(1 - float64(keep))
    (the kernel's two constants).  -> (states [n][dim], bounds [n][dim]).

    Bound of the fp32 recurrence against this one: with |s^_{f-1} - s_{f-1}| <= B_{f-1}, the step computes keep * s^ + take * e
    with two products and one sum, each rounded (or, contracted, one product and one fma): at most two nested roundings either
    way, |fl(..) - (keep s^ + take e)| <= gamma(2) (keep |s^| + take |e|), gamma(k) = k u / (1 - k u), and keep * s^ carries
    keep * B_{f-1} of the earlier error.  Hence B_f = keep B_{f-1} + gamma(3) (keep |s_{f-1}| + take |e|): gamma(3) instead of
    gamma(2) pays for writing |s| for |s^| <= |s| + B, which costs gamma(2) keep B_{f-1} <= (gamma(3) - gamma(2)) (keep |s| +
    take |e|) as long as 3 keep B_{f-1} <= keep |s| + take |e| -- asserted here, it is a precondition on the data.  A first state
    that is copied (state_valid = 0) or given is exact: B = 0."""
    keep = np.float64(np.float32(lam))
    take = np.float64(np.float32(1.0 - keep))
    enc = np.asarray(enc, np.float64)
    s = None if not state_valid else np.asarray(state, np.float64).reshape(-1)
    B = np.zeros(enc.shape[1])
    states, bounds = [], []
    for e in enc:
        if s is None:
            s = e.copy()
        else:
            mag = keep * np.abs(s) + take * np.abs(e)
            assert np.all(3 * keep * B <= mag), "smooth: data too close to zero for the derived bound"
            B = keep * B + gamma(3) * mag
            s = keep * s + take * e
        states.append(s.copy())
        bounds.append(B.copy())
    return np.array(states), np.array(bounds)


# ---- the three fp32 evaluations and E_T -----------------------------------------------------------------------------------------
def modules(weights, dim_in, A, att):
    import torch
    from radnerf.network import AudioAttNet, AudioNet
    net, attn = AudioNet(dim_in, A), (AudioAttNet(A) if att else None)
    params = params_in_names_order(net, attn)
    with torch.no_grad():
        for p, w in zip(params, weights):
            p.copy_(torch.from_numpy(np.asarray(w, np.float32)))
    return net, attn, params


def params_in_names_order(net, attn):
    import torch
    convs = [m for m in net.encoder_conv if isinstance(m, torch.nn.Conv1d)]
    fcs = [m for m in net.encoder_fc1 if isinstance(m, torch.nn.Linear)]
    ps = [c.weight for c in convs] + [c.bias for c in convs] + [f.weight for f in fcs] + [f.bias for f in fcs]
    if attn is not None:
        aconvs = [m for m in attn.attentionConvNet if isinstance(m, torch.nn.Conv1d)]
        ps += [c.weight for c in aconvs] + [c.bias for c in aconvs] + [attn.attentionNet[0].weight, attn.attentionNet[0].bias]
    return ps


def torch_eval(weights, auds, grad_enc, att, dtype="float32"):
    """The project's nn.Modules + torch autograd on the CPU -> (forward namespace, grad_codes, gradients) as numpy arrays.
    The Sequentials are walked module by module so that every pre-activation is seen (their LeakyReLUs work in place)."""
    import torch
    td = getattr(torch, dtype)
    n, frames, dim_in = auds.shape[0], auds.shape[1], auds.shape[2]
    A = weights[9].shape[0]
    net, attn, params = modules(weights, dim_in, A, att)
    net, attn = net.to(td), (attn.to(td) if att else None)
    params = params_in_names_order(net, attn)
    # nn.LeakyReLU(0.02) keeps the slope as a Python float: in fp32 it is rounded to float32(0.02), the kernels' constant; in
    # double it would stay 0.02, 4.5e-10 away.  Writing float32(0.02) into the modules changes nothing in fp32 and makes the
    # double evaluation the same function.
    for seq in [net.encoder_conv, net.encoder_fc1] + ([attn.attentionConvNet] if att else []):
        for m in seq:
            if isinstance(m, torch.nn.LeakyReLU):
                m.negative_slope = float(SLOPE32)
    r = SimpleNamespace()
    x = torch.from_numpy(np.asarray(auds)).to(td).reshape(n * frames, dim_in, WIN)

    def walk(seq, x, zs, ys):
        for m in seq:
            x = m(x)
            (zs if not isinstance(m, torch.nn.LeakyReLU) else ys).append(x.detach().clone().numpy())
        return x
    zs, ys = [], []
    x = walk(net.encoder_conv, x, zs, ys).squeeze(-1)
    codes = walk(net.encoder_fc1, x, zs, ys)
    for l in range(5):
        setattr(r, f"z{l + 1}", zs[l].reshape(zs[l].shape[0], zs[l].shape[1], -1) if l < 4 else zs[l])
        setattr(r, f"y{l + 1}", ys[l].reshape(ys[l].shape[0], ys[l].shape[1], -1) if l < 4 else ys[l])
    r.codes = codes.detach().numpy().copy()
    if att:
        codes.retain_grad()
        r.az, r.ay, encs, atts, logits = [[] for _ in range(5)], [[] for _ in range(5)], [], [], []
        for wdx in range(n):
            cw = codes[wdx * SEQ:(wdx + 1) * SEQ].unsqueeze(0)
            z, y = [], []
            s = walk(attn.attentionConvNet, cw.permute(0, 2, 1), z, y)
            lg = attn.attentionNet[0](s.view(1, SEQ))
            a = attn.attentionNet[1](lg)
            encs.append(torch.sum(a.view(1, SEQ, 1) * cw, dim=1))
            for l in range(5):
                r.az[l].append(z[l][0])
                r.ay[l].append(y[l][0])
            atts.append(a.detach().numpy()[0].copy())
            logits.append(lg.detach().numpy()[0].copy())
        r.az, r.ay = [np.array(z) for z in r.az], [np.array(y) for y in r.ay]
        r.att, r.logits = np.array(atts), np.array(logits)
        enc = torch.cat(encs)
    else:
        enc = codes
    r.enc = enc.detach().numpy().copy()
    if grad_enc is None:
        return r, None, None
    enc.backward(torch.from_numpy(np.asarray(grad_enc)).to(td))
    grad_codes = codes.grad.numpy().copy() if att else np.asarray(grad_enc).astype(r.enc.dtype)
    return r, grad_codes, [p.grad.numpy().copy() for p in params]


def compared(fwd, grad_codes, grads, att):
    """name -> array of everything a kernel output is compared with."""
    t = {"codes": fwd.codes, "enc": fwd.enc}
    for nm in ACT_NAMES:
        t[nm] = getattr(fwd, nm).reshape(fwd.codes.shape[0], -1)
    if grads is not None:
        if att:
            t["grad_codes"] = grad_codes
        for nm, g in zip(NAMES, grads):
            t[nm] = g
    return t


def evaluate(weights, auds, grad_enc, att):
    """-> (ref: name -> float64 array, E: name -> E_T, fwd64, evals: the three fp32 forward namespaces)."""
    f64 = forward(weights, auds, att)
    gc64, g64 = backward(weights, f64, grad_enc, att) if grad_enc is not None else (None, None)
    ref = compared(f64, gc64, g64, att)
    E = {nm: 0.0 for nm in ref}
    evals = []
    for kind in ("ascending", "descending", "modules"):
        if kind == "modules":
            f, gc, g = torch_eval(weights, auds, grad_enc, att)
        else:
            f = forward(weights, auds, att, np.float32, kind == "descending")
            gc, g = backward(weights, f, grad_enc, att, np.float32, kind == "descending") if grad_enc is not None else (None, None)
        evals.append(f)
        for nm, t in compared(f, gc, g, att).items():
            assert t.shape == ref[nm].shape and t.dtype == np.float32, (kind, nm, t.shape, ref[nm].shape, t.dtype)
            E[nm] = max(E[nm], float(np.abs(t.astype(np.float64) - ref[nm]).max()))
    for nm in E:
        E[nm] = max(E[nm], U * float(np.abs(ref[nm]).max()))
    return ref, E, f64, evals


# ---- the case picker ------------------------------------------------------------------------------------------------------------
POOL, ZERO_FRAMES, CLEAN_FACTOR = 64, 4, 64.0
MIN_CLEAN, MAX_DRAWS = 48, 16                     # caps: conditions, not measurements
ROBUST = 2.0                                      # no decision of a committed case may turn on a twofold change of the measured noise
NEG_LO, NEG_HI = 0.25, 0.75
ATT_MAX, ATT_MIN, ATT_RATIO = 0.9, 0.005, 2.0
MIN_GRAD = 1e-4
NET_GAIN, BIAS_STD = 3.0, 0.2
# the attention net's gain: the module initialisation leaves the softmax nearly flat (weights within a few percent of 1/8);
# at about 3 the chosen windows' weights spread as the picker demands
ATT_GAIN = {64: 3.0, 29: 2.5, 3: 3.0, 1: 3.0}     # per dim_aud (at 29 a gain of 3 saturates the softmax of most windows)
# seeds at which every condition and cap of the picker holds (tests/test_audioref64.py asserts them; found by trying 1, 2, ... and 101, 102, ...)
SEED = {(44, 64, False): 2, (44, 64, True): 215, (29, 64, False): 4, (29, 64, True): 384, (64, 29, False): 1, (64, 29, True): 286,
        (1, 3, False): 2, (1, 3, True): 186, (32, 1, False): 1, (32, 1, True): 234}


def make_weights(dim_in, A, att, seed, net_gain=NET_GAIN, att_gain=None):
    """The modules' own initialisation (torch's, from `seed`), matrices times a gain, biases N(0, BIAS_STD); float32 arrays."""
    import torch
    from radnerf.network import AudioAttNet, AudioNet
    torch.manual_seed(seed)
    net, attn = AudioNet(dim_in, A), (AudioAttNet(A) if att else None)
    rng = np.random.default_rng(seed)
    att_gain = ATT_GAIN.get(A, 3.0) if att_gain is None else att_gain
    out = []
    for i, p in enumerate(params_in_names_order(net, attn)):
        a = p.detach().numpy().astype(np.float32)
        if a.ndim > 1:
            a = a * np.float32(net_gain if i < 12 else att_gain)
        else:
            a = (rng.standard_normal(a.shape) * BIAS_STD).astype(np.float32)
        out.append(np.ascontiguousarray(a))
    return out


def _preacts(f, att):
    return [getattr(f, f"z{l + 1}") for l in range(5)] + (list(f.az) if att else [])


def _layer_noise(f64, evals, layers):
    """s_layer: the largest |z_fp32 - z64| of each layer over everything evaluated and the three evaluations."""
    return [max(float(np.abs(layers(e)[l].astype(np.float64) - z).max()) for e in evals) for l, z in enumerate(layers(f64))]


@functools.lru_cache(maxsize=None)
def case(dim_in, A, att):
    """The case of one width pair: weights, n = 3 windows (the first with two zero frames in front) with attention or n = 5
    frames (one of them zero) without, grad_enc, the float64 reference, E_T per tensor and the picker's figures (`picked`)."""
    return build_case(dim_in, A, att, SEED[(dim_in, A, att)])


def _margin(zs, noise, rows):
    """Per row (frame or window): the smallest |z64| / (64 s_layer) over the layers; clean means > 1."""
    m = np.full(rows, np.inf)
    for s, z in zip(noise, zs):
        m = np.minimum(m, (np.abs(z).reshape(rows, -1) / (CLEAN_FACTOR * s)).min(axis=1))
    return m


def _decide(margins, other_ok, marginal, what):
    """Accept a draw iff every margin is > 1 and the noise-free conditions hold.  The draws themselves never depend on the
    measured noise (fixed generator, whole pool), so a case is the same on every machine unless a decision that mattered was
    close: one is noted in `marginal` when the noise measured elsewhere, up to ROBUST times smaller or larger, could turn it."""
    m = float(np.min(margins))
    if other_ok and 1.0 / ROBUST <= m <= ROBUST:
        marginal.append(f"{what}: margin {m:.2f}")
    return other_ok and m > 1.0


def build_case(dim_in, A, att, seed, att_gain=None):
    weights = make_weights(dim_in, A, att, seed, att_gain=att_gain)
    rng = np.random.default_rng(seed + 1000)
    pool = (rng.standard_normal((POOL, dim_in, WIN)) * 2).astype(np.float32)
    zero_ids = [5, 21, 38, 60]
    pool[zero_ids] = 0.0
    live_ids = [i for i in range(POOL) if i not in zero_ids]
    picked = SimpleNamespace(seed=seed, marginal=[])
    # clean frames: no AudioNet pre-activation within 64 x the layer's fp32 noise of the kink
    w_net = weights[:12]
    f64 = forward(w_net, pool[:, None], False)
    evals = [forward(w_net, pool[:, None], False, np.float32, False), forward(w_net, pool[:, None], False, np.float32, True),
             torch_eval(w_net, pool[:, None], None, False)[0]]
    s_net = _layer_noise(f64, evals, lambda f: _preacts(f, False))
    m_frame = _margin(_preacts(f64, False), s_net, POOL)
    picked.n_clean = int((m_frame > 1.0).sum())
    picked.zero_clean = _decide(m_frame[zero_ids], True, picked.marginal, "zero frames")
    picked.neg_net = [float((z < 0).mean()) for z in _preacts(f64, False)]
    if not att:
        n = 5
        ids, order = [], [int(i) for i in rng.permutation(live_ids)]
        for tried, i in enumerate(order):              # the first four clean frames of a fixed order, and a zero frame
            if _decide(m_frame[i:i + 1], True, picked.marginal, f"frame {i}"):
                ids.append(i)
            if len(ids) == n - 1:
                break
        picked.draws = [tried + 1 - (n - 2)]
        auds = pool[ids + zero_ids[:1]][:, None]
    else:
        n = 3
        # candidates: MAX_DRAWS windows per slot; slot 0 starts with two zero frames like a window cut at the stream's head
        cand = np.zeros((n, MAX_DRAWS, SEQ, dim_in, WIN), np.float32)
        cand_ids = {}
        for slot in range(n):
            for d in range(MAX_DRAWS):
                k = SEQ - 2 if slot == 0 else SEQ
                cand_ids[slot, d] = rng.choice(live_ids, k, replace=False)
                cand[slot, d, SEQ - k:] = pool[cand_ids[slot, d]]
        flat = cand.reshape(n * MAX_DRAWS, SEQ, dim_in, WIN)
        c64 = forward(weights, flat, True)
        cev = [forward(weights, flat, True, np.float32, False), forward(weights, flat, True, np.float32, True),
               torch_eval(weights, flat, None, True)[0]]
        s_att = _layer_noise(c64, cev, lambda f: list(f.az))
        m_win = _margin(c64.az, s_att, n * MAX_DRAWS).reshape(n, MAX_DRAWS)
        a = c64.att
        spread = ((a.max(axis=1) <= ATT_MAX) & (a.min(axis=1) >= ATT_MIN) & (a.max(axis=1) >= ATT_RATIO * a.min(axis=1))).reshape(n, MAX_DRAWS)
        picked.draws, chosen = [], []
        for slot in range(n):
            for d in range(MAX_DRAWS):
                margins = np.append(m_frame[cand_ids[slot, d]], m_win[slot, d])
                if _decide(margins, bool(spread[slot, d]), picked.marginal, f"window {slot} draw {d + 1}"):
                    break
            else:
                d = MAX_DRAWS
            picked.draws.append(d + 1)
            chosen.append(cand[slot, min(d, MAX_DRAWS - 1)])
        auds = np.stack(chosen)
    grad_enc = rng.standard_normal((n, A)).astype(np.float32)
    ref, E, f64c, _ = evaluate(weights, auds, grad_enc, att)
    picked.neg_att = [float((z < 0).mean()) for z in f64c.az] if att else []
    picked.att = f64c.att if att else None
    picked.min_grad = min(float(np.abs(ref[nm]).max()) for nm in NAMES[:24 if att else 12])
    return SimpleNamespace(dim_in=dim_in, A=A, att=att, n=n, weights=weights, auds=np.ascontiguousarray(auds), grad_enc=grad_enc,
                           ref=ref, E=E, fwd=f64c, picked=picked, s_net=s_net)


def picker_failures(c):
    """Every condition and cap of the picker that case `c` misses (empty = all hold)."""
    p, bad = c.picked, []
    if p.n_clean < MIN_CLEAN:
        bad.append(f"only {p.n_clean} of {POOL} frames are clean")
    if not p.zero_clean:
        bad.append("a zero frame is not clean")
    if max(p.draws) > MAX_DRAWS:
        bad.append(f"not found within {MAX_DRAWS} draws: {p.draws}")
    bad += [f"a decision hinges on the measured noise within a factor {ROBUST:g}: {m}" for m in p.marginal]
    for nm, fr in (("AudioNet", p.neg_net), ("AudioAttNet", p.neg_att)):
        for l, v in enumerate(fr):
            if not NEG_LO <= v <= NEG_HI:
                bad.append(f"{nm} layer {l}: {v:.3f} of the pre-activations are negative")
    if c.att:
        a = p.att
        if a.max() > ATT_MAX or a.min() < ATT_MIN or (a.max(axis=1) < ATT_RATIO * a.min(axis=1)).any():
            bad.append(f"attention weights out of range: max {a.max():.4f} min {a.min():.4f}")
    if p.min_grad < MIN_GRAD:
        bad.append(f"a gradient tensor's maximum is {p.min_grad:.3e}")
    return bad


STRUCTURAL_SEED = {"p0": 11, "p15": 12, "zero": 13}


@functools.lru_cache(maxsize=None)
def structural_case(kind):
    """att = 0, n = 1, weights of case(44, 64, False): a frame that is nonzero only at position 0 ('p0') or 15 ('p15'), or all
    zero ('zero').  -> (case-like namespace, the frame's margin: clean means > 1, and > ROBUST that it is clean on any machine)."""
    return build_structural(kind, STRUCTURAL_SEED[kind])


def build_structural(kind, seed):
    base = case(44, 64, False)
    rng = np.random.default_rng(seed)
    frame = np.zeros((1, 1, 44, WIN), np.float32)
    if kind != "zero":
        frame[0, 0, :, 0 if kind == "p0" else 15] = (rng.standard_normal(44) * 2).astype(np.float32)
    grad_enc = rng.standard_normal((1, 64)).astype(np.float32)
    ref, E, f64, _ = evaluate(base.weights, frame, grad_enc, False)
    margin = float(_margin(_preacts(f64, False), base.s_net, 1)[0])
    return SimpleNamespace(dim_in=44, A=64, att=False, n=1, weights=base.weights, auds=frame, grad_enc=grad_enc, ref=ref, E=E,
                           fwd=f64, kind=kind), margin
