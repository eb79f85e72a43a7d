"""tests/audioref64.py -- the float64 reference tests/test_gpu_audio_ref.py holds the audio kernels to -- checked on the CPU: it
is the arithmetic of the project's AudioNet / AudioAttNet modules and of get_audio_features, its case picker meets every
condition it states, and its exact zeros are where the convolution's geometry puts them."""
import numpy as np
import pytest
import torch

import audioref64 as R


@pytest.mark.parametrize("dims", [(44, 64), (7, 5)])
@pytest.mark.parametrize("att", [True, False])
def test_reference_is_the_modules_in_double(dims, att):
    dim_in, A = dims
    n = 3
    weights = R.make_weights(dim_in, A, att, seed=9)
    rng = np.random.default_rng(10)
    auds = (rng.standard_normal((n, R.SEQ if att else 1, dim_in, R.WIN)) * 2).astype(np.float32)
    grad_enc = rng.standard_normal((n, A)).astype(np.float32)
    fwd = R.forward(weights, auds, att)
    grad_codes, grads = R.backward(weights, fwd, grad_enc, att)
    tf, tgc, tg = R.torch_eval(weights, auds, grad_enc, att, dtype="float64")
    pairs = [(f"z{l}", getattr(fwd, f"z{l}"), getattr(tf, f"z{l}")) for l in range(1, 6)]
    pairs += [(f"y{l}", getattr(fwd, f"y{l}"), getattr(tf, f"y{l}")) for l in range(1, 6)]
    pairs += [("codes", fwd.codes, tf.codes), ("enc", fwd.enc, tf.enc), ("grad_codes", grad_codes, tgc)]
    if att:
        pairs += [(f"az{l}", fwd.az[l], tf.az[l]) for l in range(5)] + [(f"ay{l}", fwd.ay[l], tf.ay[l]) for l in range(5)]
        pairs += [("logits", fwd.logits, tf.logits), ("att", fwd.att, tf.att)]
    assert len(grads) == len(tg) == (24 if att else 12)
    pairs += [(nm, a, b) for nm, a, b in zip(R.NAMES, grads, tg)]
    for nm, mine, want in pairs:
        assert mine.dtype == want.dtype == np.float64 and mine.shape == want.shape, (nm, mine.shape, want.shape)
        scale = float(np.abs(want).max())
        assert scale > 0, nm
        assert float(np.abs(mine - want).max()) <= 1e-12 * scale, (nm, float(np.abs(mine - want).max()) / scale)


@pytest.mark.parametrize("T", [8, 24])
def test_stream_cutting_is_get_audio_features(T):
    from radnerf.rays import get_audio_features
    feats = np.random.default_rng(T).standard_normal((T, 5, R.WIN)).astype(np.float32)
    for centre in (0, 3, T - 4, T - 1):
        want = get_audio_features(torch.from_numpy(feats), 2, centre).numpy()
        got = R.cut_window(feats, centre)
        assert got.shape == want.shape == (8, 5, R.WIN) and np.array_equal(got, want), centre


@pytest.mark.parametrize("dims", R.DIM_PAIRS)
@pytest.mark.parametrize("att", [True, False])
def test_picker_conditions_hold_for_every_gpu_case(dims, att):
    c = R.case(dims[0], dims[1], att)
    assert R.picker_failures(c) == []
    assert c.auds.shape == ((3, 8) if att else (5, 1)) + (dims[0], R.WIN) and c.auds.dtype == np.float32
    if att:
        assert not c.auds[0, :2].any() and c.auds[0, 2:].any(axis=(1, 2)).all()      # two zero frames in front of window 0
    for nm, e in c.E.items():
        assert e >= R.U * float(np.abs(c.ref[nm]).max()) > 0, nm


@pytest.mark.parametrize("kind,live_taps", [("p0", (1,)), ("p15", (2,)), ("zero", ())])
def test_structural_zeros(kind, live_taps):
    """conv 0 reads x[2 pos - 1 + k], pos = 0 .. 7: position 0 is reached by tap 1 alone (pos 0), position 15 by tap 2 alone
    (pos 7); a tap that never meets the one nonzero position has a gradient of exactly 0.0."""
    c, margin = R.structural_case(kind)
    assert margin > R.ROBUST
    for p in (0, 15):
        taps = tuple(k for k in range(3) if any(2 * pos - 1 + k == p for pos in range(8)))
        assert taps == {0: (1,), 15: (2,)}[p]
    g = c.ref["conv_w0"]
    for k in range(3):
        if k in live_taps:
            assert np.all(g[:, :, k] != 0.0)
        else:
            assert np.all(g[:, :, k] == 0.0)
    assert np.all(c.ref["conv_b0"] != 0.0)
