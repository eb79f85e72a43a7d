"""The nine kernels of csrc/rn_audio.hip, through the C ABI, against the float64 restatement of tests/audioref64.py -- element by
element, at every width the entries accept on paper (dim_in 1 .. 64, dim_aud 1 .. 64), with more than one window, through all
three backward entries, with guards around everything an entry writes.

THE comparator (`hold`): |gpu - ref64| <= 4 * E_T per element, E_T = the largest distance of three honest fp32 evaluations of the
same arithmetic from float64 (audioref64.evaluate); where the reference is exactly 0.0 the kernel's value is exactly 0.0.  The 4
is the margin for the kernels summing in yet another order (16-lane split + shuffle tree, atomics over 8 n workgroups).  The
smoothing recurrence is held to its derived running bound (audioref64.smooth).  There is no other tolerance in this file."""
import ctypes as C

import numpy as np
import pytest
import torch

import audioref64 as R

pytestmark = pytest.mark.gpu

FACTOR = 4.0
GUARD = 256
SENTINEL = -7777.0
FAMILY = {"codes": "codes", "enc": "enc", "grad_codes": "grad_codes", **{nm: "acts" for nm in R.ACT_NAMES},
          **{nm: "AudioNet gradients" for nm in R.NAMES[:12]}, **{nm: "attention gradients" for nm in R.NAMES[12:]}}
_seen = {}      # family -> [(largest gpu / E_T, where), (largest E_T / max|ref|, where)]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for fam, (ratio, rel) in sorted(_seen.items()):
        print(f"\naudio_ref family {fam:20s} max gpu/E_T {ratio[0]:.3f} ({ratio[1]})   max E_T/max|ref| {rel[0]:.3e} ({rel[1]})", end="")
    print()


def hold(c, name, gpu, offset=0.0, what=""):
    """The one comparator: gpu (fp32, from the device) against c.ref[name] (+ offset, for a prefilled buffer)."""
    ref, E = c.ref[name], c.E[name]
    got = np.asarray(gpu, np.float32).astype(np.float64).reshape(ref.shape)
    assert np.isfinite(got).all(), (what, name)
    want = ref + offset
    zero = ref == 0.0
    if zero.all():                                     # E_T = 0: the exact-zero rule below is the whole comparison
        ratio = 0.0 if np.all(got == offset) else float("inf")
    else:
        ratio = float(np.abs(got - want).max()) / E
        fam = _seen.setdefault(FAMILY[name], [(0.0, ""), (0.0, "")])
        tag = f"{name} {getattr(c, 'dim_in', '')}x{getattr(c, 'A', '')} att{int(getattr(c, 'att', 1))} {what}"
        fam[0], fam[1] = max(fam[0], (ratio, tag)), max(fam[1], (E / float(np.abs(ref).max()), tag))
    assert np.all(got[zero] == offset), f"{what} {name}: max|gpu - ref64| / E_T = {ratio:.3f}; a structural zero is not exact"
    assert ratio <= FACTOR, f"{what} {name} {ref.shape}: max|gpu - ref64| / E_T = {ratio:.3f} (E_T = {E:.3e})"


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


class Guarded:
    """`numel` floats filled with `fill` (NaN: must be written before it is read) between two guards of sentinels, in ONE
    allocation -- and, for a gradient buffer, `tail` more sentinels behind the real size (room for the tensor at width 64)."""

    def __init__(self, numel, fill=float("nan"), tail=0):
        self.full = torch.full((GUARD + numel + tail + GUARD,), SENTINEL, device="cuda")
        self.t = self.full[GUARD:GUARD + numel]
        self.t.fill_(fill)
        self.numel = numel

    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        f = self.full.cpu().numpy()
        return bool((f[:GUARD] == SENTINEL).all() and (f[GUARD + self.numel:] == SENTINEL).all())

    def untouched_nan(self):
        return bool(torch.isnan(self.t).all())


class Net:
    """What radnerf.audio._weights reads of a model: widths outside NeRFNetwork's three ASR choices."""

    def __init__(self, c):
        net, attn, _ = R.modules(c.weights, c.dim_in, c.A, c.att)
        self.audio_net = net.cuda()
        self.audio_att_net = attn.cuda() if c.att else None
        self.audio_in_dim, self.audio_dim, self.att = c.dim_in, c.A, (2 if c.att else 0)


def make_run(c):
    from radnerf import audio
    m = Net(c)
    w, keep = audio._weights(m)
    return SimpleRun(c, m, w, keep)


class SimpleRun:
    def __init__(self, c, m, w, keep):
        import radnerf_hip as hip
        self.c, self.m, self.w, self.keep, self.hip = c, m, w, keep, hip
        self.frames = R.SEQ if c.att else 1
        self.auds = torch.from_numpy(c.auds).cuda()
        self.grad_enc = torch.from_numpy(c.grad_enc).cuda()
        self.buffers = []

    def buf(self, numel, fill=float("nan"), tail=0):
        g = Guarded(numel, fill, tail)
        self.buffers.append(g)
        return g

    def guards_intact(self):
        torch.cuda.synchronize()
        return all(g.intact() for g in self.buffers)

    def forward(self, auds=None, train=False):
        """-> (enc, codes workspace, acts or None) as Guarded buffers."""
        hip, c = self.hip, self.c
        auds = self.auds if auds is None else auds
        n = auds.shape[0]
        enc, ws = self.buf(n * c.A), self.buf(n * R.SEQ * c.A)
        if train:
            acts = self.buf(int(hip._lib.rn_audio_train_acts_floats(n, int(c.att))))
            assert acts.numel == n * self.frames * R.K_ACTS
            hip.call("rn_audio_encode_windows_train", C.byref(self.w), hip.ptr(auds), n, enc.ptr(), ws.ptr(), acts.ptr(), hip.stream())
            return enc, ws, acts
        hip.call("rn_audio_encode_windows", C.byref(self.w), hip.ptr(auds), n, enc.ptr(), ws.ptr(), hip.stream())
        return enc, ws, None

    def grad_buffers(self, prefill=0.0):
        """Gradient buffers in rn_audio_grads_t order, each with room for the tensor at dim_in = dim_aud = 64 behind its real size."""
        from radnerf_hip.abi import AudioGradsT
        shapes = [tuple(t.shape) for t in self.c.weights]
        wide = {"conv_w0": 32 * 64 * 3, "fc_w1": 64 * 64, "fc_b1": 64, "att_conv_w0": 16 * 64 * 3}
        gs = [self.buf(int(np.prod(s)), prefill, tail=max(0, wide.get(nm, 0) - int(np.prod(s)))) for nm, s in zip(R.NAMES, shapes)]
        g = AudioGradsT()
        for i in range(4):
            g.conv_w[i], g.conv_b[i] = gs[i].ptr(), gs[4 + i].ptr()
        for i in range(2):
            g.fc_w[i], g.fc_b[i] = gs[8 + i].ptr(), gs[10 + i].ptr()
        if self.c.att:
            for i in range(5):
                g.att_conv_w[i], g.att_conv_b[i] = gs[12 + i].ptr(), gs[17 + i].ptr()
            g.att_fc_w, g.att_fc_b = gs[22].ptr(), gs[23].ptr()
        return gs, g

    def backward(self, entry, codes, acts, auds=None, grad_enc=None, prefill=0.0):
        """entry: 'recompute' | 'acts' | 'ordered' -> (grad_codes, gradient buffers, partials or None) as Guarded buffers."""
        hip, c = self.hip, self.c
        auds = self.auds if auds is None else auds
        grad_enc = self.grad_enc if grad_enc is None else grad_enc
        n = auds.shape[0]
        gs, g = self.grad_buffers(prefill)
        grad_codes, partials = self.buf(n * R.SEQ * c.A), None
        head = (C.byref(self.w), hip.ptr(auds), n, codes.ptr(), hip.ptr(grad_enc), C.byref(g), grad_codes.ptr())
        if entry == "recompute":
            hip.call("rn_audio_encode_windows_backward", *head, hip.stream())
        elif entry == "acts":
            hip.call("rn_audio_encode_windows_backward_acts", *head, acts.ptr(), hip.stream())
        else:
            partials = self.buf(int(hip._lib.rn_audio_backward_partials_floats(n, int(c.att))))
            hip.call("rn_audio_encode_windows_backward_ordered", *head, acts.ptr(), partials.ptr(), hip.stream())
        return grad_codes, gs, partials

    def hold_forward(self, enc, ws, acts, what):
        c = self.c
        hold(c, "enc", enc.t.cpu().numpy(), what=what)
        if c.att:
            hold(c, "codes", ws.t.cpu().numpy(), what=what)
        else:
            assert ws.untouched_nan(), what           # one frame per window: the frame code is the result, no workspace
        if acts is not None:
            a = acts.t.cpu().numpy().reshape(-1, R.K_ACTS)
            at = 0
            for nm in R.ACT_NAMES:                     # kActs: y1 [32][8] | y2 [32][4] | y3 [64][2] | y4 [64] | y5 [64]
                k = c.ref[nm].shape[1]
                hold(c, nm, a[:, at:at + k], what=what)
                at += k
            assert at == R.K_ACTS

    def hold_backward(self, grad_codes, gs, what, offset=0.0):
        c = self.c
        if c.att:
            hold(c, "grad_codes", grad_codes.t.cpu().numpy(), what=what)
        else:
            assert grad_codes.untouched_nan(), what
        assert len(gs) == (24 if c.att else 12)
        for nm, g in zip(R.NAMES, gs):
            hold(c, nm, g.t.cpu().numpy(), offset=offset, what=what)


CASES = [pytest.param(di, A, att, id=f"{di}x{A}-att{int(att)}") for di, A in R.DIM_PAIRS for att in (True, False)]


@pytest.mark.parametrize("dim_in,A,att", CASES)
def test_forward_entries(hiplib, dim_in, A, att):
    c = R.case(dim_in, A, att)
    r = make_run(c)
    enc, ws, _ = r.forward()
    r.hold_forward(enc, ws, None, "encode_windows")
    tenc, tws, acts = r.forward(train=True)
    r.hold_forward(tenc, tws, acts, "encode_windows_train")
    assert same_bits(tenc.t, enc.t) and same_bits(tws.t, ws.t)
    for k in range(c.n):                               # each window alone equals its row of the batch
        e1, w1, _ = r.forward(r.auds[k:k + 1].contiguous())
        assert same_bits(e1.t, enc.t[k * A:(k + 1) * A]), k
        if att:
            assert same_bits(w1.t, ws.t[k * R.SEQ * A:(k + 1) * R.SEQ * A]), k
    assert r.guards_intact()


@pytest.mark.parametrize("dim_in,A,att", CASES)
def test_backward_three_entries(hiplib, dim_in, A, att):
    c = R.case(dim_in, A, att)
    r = make_run(c)
    _, codes, acts = r.forward(train=True)
    out = {}
    for entry in ("recompute", "acts", "ordered"):
        grad_codes, gs, _ = r.backward(entry, codes, acts)
        r.hold_backward(grad_codes, gs, f"backward[{entry}]")
        out[entry] = grad_codes
    assert same_bits(out["recompute"].t, out["acts"].t) and same_bits(out["ordered"].t, out["acts"].t)
    if att:                                            # grad_codes of the batch equals each window's own call
        per = R.SEQ * A
        for k in range(c.n):
            rows = slice(k * per, (k + 1) * per)
            a1 = acts.t[k * R.SEQ * R.K_ACTS:(k + 1) * R.SEQ * R.K_ACTS]
            one, _, _ = r.backward("acts", SimpleView(codes.t[rows]), SimpleView(a1), r.auds[k:k + 1].contiguous(), r.grad_enc[k:k + 1].contiguous())
            assert same_bits(one.t, out["acts"].t[rows]), k
    for entry in ("recompute", "acts"):                # the atomic entries ADD to what the buffers hold
        grad_codes, gs, _ = r.backward(entry, codes, acts, prefill=0.5)
        r.hold_backward(grad_codes, gs, f"backward[{entry}] + 0.5", offset=0.5)
    assert r.guards_intact()


class SimpleView:
    """A slice of a Guarded buffer handed to an entry as an input."""

    def __init__(self, t):
        assert t.is_contiguous()
        self.t = t

    def ptr(self):
        return self.t.data_ptr()


@pytest.mark.parametrize("dim_in,A", R.DIM_PAIRS)
def test_one_workgroup_recompute_equals_kept_activations(hiplib, dim_in, A):
    """att = 0, n = 1: one workgroup, one add per element into zeroed buffers -- nothing to reorder, so the recompute entry's
    gradients carry the bits of the entry that starts from the kept activations: the kept ones ARE the recomputed ones."""
    c = R.case(dim_in, A, False)
    r = make_run(c)
    for k in range(c.n):
        auds, ge = r.auds[k:k + 1].contiguous(), r.grad_enc[k:k + 1].contiguous()
        _, codes, acts = r.forward(auds, train=True)
        _, ga, _ = r.backward("recompute", codes, acts, auds, ge)
        _, gb, _ = r.backward("acts", codes, acts, auds, ge)
        for nm, a, b in zip(R.NAMES, ga, gb):
            assert same_bits(a.t, b.t), (k, nm)
            assert float(b.t.abs().max()) > 0 or nm == "conv_w0", (k, nm)      # conv_w0 of the zero frame is all zero
    assert r.guards_intact()


@pytest.mark.parametrize("kind", ["p0", "p15", "zero"])
def test_structural_zeros_on_the_device(hiplib, kind):
    c, margin = R.structural_case(kind)
    assert margin > 1.0
    r = make_run(c)
    assert int((c.ref["conv_w0"] == 0.0).sum()) == {"p0": 2, "p15": 2, "zero": 3}[kind] * 32 * 44
    enc, codes, acts = r.forward(train=True)
    r.hold_forward(enc, codes, acts, f"structural[{kind}] forward")
    grad_codes, gs, _ = r.backward("acts", codes, acts)
    r.hold_backward(grad_codes, gs, f"structural[{kind}]")       # the comparator's exact-zero rule does the work
    assert r.guards_intact()


@pytest.mark.parametrize("dim_in,A", [(64, 29), (1, 3)])
@pytest.mark.parametrize("att", [True, False])
def test_entries_write_only_what_they_own(hiplib, dim_in, A, att):
    """Widths below 64, where a stride of 64 would leave a row: guards unchanged, everything owned written (no NaN left),
    gradient buffers untouched behind each tensor's real size (Guarded's tail is part of what `intact` reads)."""
    c = R.case(dim_in, A, att)
    r = make_run(c)
    frames = R.SEQ if att else 1
    enc, ws, acts = r.forward(train=True)
    torch.cuda.synchronize()
    assert not torch.isnan(enc.t).any() and not torch.isnan(acts.t).any()
    assert enc.numel == c.n * A and ws.numel == c.n * R.SEQ * A
    owned = c.n * frames * A if att else 0             # the first n * frames * A floats of the workspace are the per-frame codes
    assert not torch.isnan(ws.t[:owned]).any() and torch.isnan(ws.t[owned:]).all()
    assert r.guards_intact()
    for entry in ("recompute", "acts", "ordered"):
        grad_codes, gs, partials = r.backward(entry, ws, acts)
        torch.cuda.synchronize()
        if att:
            assert grad_codes.numel == c.n * R.SEQ * A and not torch.isnan(grad_codes.t).any(), entry
        else:
            assert grad_codes.untouched_nan(), entry
        for nm, g in zip(R.NAMES, gs):
            assert not torch.isnan(g.t).any() and g.numel == c.ref[nm].size, (entry, nm)
        if partials is not None:
            assert partials.numel == int(r.hip._lib.rn_audio_backward_partials_floats(c.n, int(att)))
        assert r.guards_intact(), entry


def _stream_case(T):
    """Weights of the (44, 64) attention case, a stream of T frames, the reference of ALL T windows (frame i's window at row i)."""
    base = R.case(44, 64, True)
    feats = (np.random.default_rng(200 + T).standard_normal((T, 44, R.WIN)) * 2).astype(np.float32)
    wins = np.stack([R.cut_window(feats, i) for i in range(T)])
    ref, E, _, _ = R.evaluate(base.weights, wins, None, True)
    return base, feats, wins, ref, E


@pytest.mark.parametrize("T,first,n", [(8, 3, 20), (24, 23, 5)])
def test_stream_windows(hiplib, T, first, n):
    from types import SimpleNamespace
    from radnerf import audio
    from radnerf.rays import get_audio_features
    base, feats, wins, ref, E = _stream_case(T)
    r = make_run(base)
    ids = [(first + i) % T for i in range(n)]
    c = SimpleNamespace(ref={"enc": ref["enc"][ids], "codes": ref["codes"].reshape(T, -1)[ids].reshape(n * R.SEQ, 64)}, E=E)
    f = torch.from_numpy(feats).cuda()
    enc, ws = r.buf(n * 64), r.buf(n * R.SEQ * 64)
    r.hip.call("rn_audio_encode_stream", C.byref(r.w), r.hip.ptr(f), T, first, n, enc.ptr(), ws.ptr(), r.hip.stream())
    hold(c, "enc", enc.t.cpu().numpy(), what="encode_stream")
    hold(c, "codes", ws.t.cpu().numpy(), what="encode_stream")
    cut = torch.stack([get_audio_features(f, 2, i) for i in ids]).contiguous()
    assert np.array_equal(cut.cpu().numpy(), wins[ids])
    want = audio.encode_windows(r.m, cut)
    assert same_bits(enc.t, want.reshape(-1))
    assert same_bits(audio.encode_stream(r.m, f, first, n).reshape(-1), enc.t)
    assert same_bits(audio.encode_stream(r.m, f, first + T, n).reshape(-1), enc.t)      # 47 -> 23 through the wrapper's modulo
    assert r.guards_intact()


def test_stream_refuses_short_streams_and_no_attention(hiplib):
    base = R.case(44, 64, True)
    r = make_run(base)
    f = torch.zeros(8, 44, R.WIN, device="cuda")
    enc, ws = r.buf(64), r.buf(R.SEQ * 64)
    rc = r.hip._lib.rn_audio_encode_stream(C.byref(r.w), r.hip.ptr(f), 7, 0, 1, enc.ptr(), ws.ptr(), r.hip.stream())
    assert rc != 0 and "8 frames" in r.hip.last_error()
    from radnerf_hip.abi import AudioWeightsT
    w0 = AudioWeightsT.from_buffer_copy(r.w)
    w0.has_att = 0
    rc = r.hip._lib.rn_audio_encode_stream(C.byref(w0), r.hip.ptr(f), 8, 0, 1, enc.ptr(), ws.ptr(), r.hip.stream())
    assert rc != 0 and "has_att" in r.hip.last_error()
    torch.cuda.synchronize()
    assert enc.untouched_nan() and ws.untouched_nan() and r.guards_intact()


@pytest.mark.parametrize("dim", [1, 63, 64, 65, 130])
def test_smoothing_recurrence(hiplib, dim):
    import radnerf_hip as hip
    rng = np.random.default_rng(dim)
    for n in (1, 5):
        for valid in (0, 1):
            for lam in (0.35, 0.0, 0.9):
                codes = rng.standard_normal((n, dim)).astype(np.float32)
                state0 = rng.standard_normal(dim).astype(np.float32)
                want, bound = R.smooth(codes, lam, state0, valid)
                enc = torch.from_numpy(codes).cuda()
                what = (dim, n, valid, lam)

                def fresh():
                    s = Guarded(dim)
                    if valid:
                        s.t.copy_(torch.from_numpy(state0))
                    return s
                state, out = fresh(), Guarded(n * dim)
                hip.call("rn_audio_smooth_seq", hip.ptr(enc), n, dim, lam, state.ptr(), valid, out.ptr(), hip.stream())
                got = out.t.cpu().numpy().reshape(n, dim)
                assert np.all(np.abs(got.astype(np.float64) - want) <= bound), (what, float((np.abs(got - want) - bound).max()))
                if not valid:
                    assert np.array_equal(got[0].view(np.uint32), codes[0].view(np.uint32)), what
                assert same_bits(state.t, out.t[(n - 1) * dim:]), what
                single, folded = fresh(), fresh()
                for i in range(n):                      # row i = the state after i + 1 single-code calls
                    row = enc[i:i + 1].contiguous()
                    hip.call("rn_audio_smooth", hip.ptr(row), 1, dim, lam, single.ptr(), 1 if (valid or i) else 0, hip.stream())
                    assert same_bits(single.t, out.t[i * dim:(i + 1) * dim]), (what, i)
                hip.call("rn_audio_smooth", hip.ptr(enc), n, dim, lam, folded.ptr(), valid, hip.stream())
                assert same_bits(folded.t, state.t), what
                # n = 0: RN_OK, nothing touched
                idle, idle_out = fresh(), Guarded(dim)
                before = bits(idle.t).copy()
                hip.call("rn_audio_smooth", hip.ptr(enc), 0, dim, lam, idle.ptr(), valid, hip.stream())
                hip.call("rn_audio_smooth_seq", hip.ptr(enc), 0, dim, lam, idle.ptr(), valid, idle_out.ptr(), hip.stream())
                torch.cuda.synchronize()
                assert np.array_equal(bits(idle.t), before) and idle_out.untouched_nan(), what
                assert all(g.intact() for g in (state, out, single, folded, idle, idle_out)), what


@pytest.mark.parametrize("att", [True, False])
def test_zero_windows_write_nothing(hiplib, att):
    c = R.case(64, 29, att)
    r = make_run(c)
    hip = r.hip
    enc, ws, acts, grad_codes, partials = r.buf(29), r.buf(R.SEQ * 29), r.buf(R.SEQ * R.K_ACTS), r.buf(R.SEQ * 29), r.buf(1024)
    gs, g = r.grad_buffers(prefill=float("nan"))
    a, ge, f = r.auds, r.grad_enc, torch.zeros(8, 64, R.WIN, device="cuda")
    hip.call("rn_audio_encode_windows", C.byref(r.w), hip.ptr(a), 0, enc.ptr(), ws.ptr(), hip.stream())
    hip.call("rn_audio_encode_windows_train", C.byref(r.w), hip.ptr(a), 0, enc.ptr(), ws.ptr(), acts.ptr(), hip.stream())
    hip.call("rn_audio_encode_stream", C.byref(r.w), hip.ptr(f), 8, 0, 0, enc.ptr(), ws.ptr(), hip.stream())
    head = (C.byref(r.w), hip.ptr(a), 0, ws.ptr(), hip.ptr(ge), C.byref(g), grad_codes.ptr())
    hip.call("rn_audio_encode_windows_backward", *head, hip.stream())
    hip.call("rn_audio_encode_windows_backward_acts", *head, acts.ptr(), hip.stream())
    hip.call("rn_audio_encode_windows_backward_ordered", *head, acts.ptr(), partials.ptr(), hip.stream())
    torch.cuda.synchronize()
    for b in [enc, ws, acts, grad_codes, partials] + gs:
        assert b.untouched_nan()
    assert r.guards_intact()
