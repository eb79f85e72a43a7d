"""The audio nets' parameter gradients without float atomics (rn_audio_encode_windows_backward_ordered, csrc/rn_audio.hip) against
the existing backward, BIT FOR BIT: the ordered entry stores every workgroup's contribution into its own slice and adds the slices
in ascending workgroup order, so it must equal the fp32 fold, in that order, of the existing backward run on one workgroup's work
at a time into zeroed buffers (0 + x is exact; a one-workgroup call has nothing to reorder)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K_ACTS = 32 * 8 + 32 * 4 + 64 * 2 + 64 + 64      # floats of one frame's kept activations (csrc/rn_audio.hip, kActs)


def _scene(**kw):
    from radnerf.scene import SyntheticScene, default_opt
    return SyntheticScene(H=32, W=32, n_frames=24, device="cuda", opt=default_opt(engine="fused", **kw))


def _grad_buffers(m, att):
    """Zeroed gradient buffers in the order of rn_audio_grads_t -> (views, struct)."""
    from radnerf import audio
    from radnerf_hip.abi import AudioGradsT
    params = audio._parameters(m)
    if not att:
        params = params[:12]
    views = [torch.zeros_like(p) for p in params]
    g, it = AudioGradsT(), iter(v.data_ptr() for v in views)
    for i in range(4):
        g.conv_w[i], g.conv_b[i] = next(it), next(it)
    for i in range(2):
        g.fc_w[i], g.fc_b[i] = next(it), next(it)
    if att:
        for i in range(5):
            g.att_conv_w[i], g.att_conv_b[i] = next(it), next(it)
        g.att_fc_w, g.att_fc_b = next(it), next(it)
    return views, g


def _forward(m, w, auds, n):
    import radnerf_hip as hip
    enc = torch.empty(n, m.audio_dim, device="cuda")
    codes = torch.empty(n * 8, m.audio_dim, device="cuda")
    acts = torch.empty(int(hip._lib.rn_audio_train_acts_floats(n, int(w.has_att))), device="cuda")
    hip.call("rn_audio_encode_windows_train", C.byref(w), hip.ptr(auds), n, hip.ptr(enc), hip.ptr(codes), hip.ptr(acts), hip.stream())
    return codes, acts


def _ordered(m, w, auds, n, codes, grad_enc, acts, att):
    import radnerf_hip as hip
    views, g = _grad_buffers(m, att)
    scratch = torch.full_like(codes, float("nan"))
    partials = torch.full((int(hip._lib.rn_audio_backward_partials_floats(n, int(att))),), float("nan"), device="cuda")
    hip.call("rn_audio_encode_windows_backward_ordered", C.byref(w), hip.ptr(auds), n, hip.ptr(codes), hip.ptr(grad_enc), C.byref(g),
             hip.ptr(scratch), hip.ptr(acts), hip.ptr(partials), hip.stream())
    torch.cuda.synchronize()
    return views, scratch


def _existing(m, w, auds, n, codes, grad_enc, acts, att):
    import radnerf_hip as hip
    views, g = _grad_buffers(m, att)
    scratch = torch.empty_like(codes)
    hip.call("rn_audio_encode_windows_backward_acts", C.byref(w), hip.ptr(auds), n, hip.ptr(codes), hip.ptr(grad_enc), C.byref(g),
             hip.ptr(scratch), hip.ptr(acts), hip.stream())
    torch.cuda.synchronize()
    return views, scratch


def _same_bits(a, b):
    return np.array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32))


def _fold(parts):
    """((p0 + p1) + p2) + ... per tensor, in fp32 on the device (an elementwise IEEE add)."""
    acc = [t.clone() for t in parts[0]]
    for views in parts[1:]:
        acc = [a + v for a, v in zip(acc, views)]
    return acc


def test_no_attention_five_windows_equal_the_fold_of_single_window_calls(hiplib):
    from radnerf import audio
    m = _scene(att=0).model
    w, keep = audio._weights(m)
    n = 5
    g = torch.Generator(device="cuda").manual_seed(3)
    auds = torch.randn(n, 1, m.audio_in_dim, 16, device="cuda", generator=g) * 2
    grad_enc = torch.randn(n, m.audio_dim, device="cuda", generator=g)
    codes, acts = _forward(m, w, auds, n)
    got, _ = _ordered(m, w, auds, n, codes, grad_enc, acts, False)
    again, _ = _ordered(m, w, auds, n, codes, grad_enc, acts, False)
    parts = [_existing(m, w, auds[k:k + 1].contiguous(), 1, codes, grad_enc[k:k + 1].contiguous(), acts[k * K_ACTS:(k + 1) * K_ACTS].contiguous(), False)[0]
             for k in range(n)]
    want = _fold(parts)
    assert len(got) == len(want) == 12
    for i, (a, b, c) in enumerate(zip(got, want, again)):
        assert float(b.abs().max()) > 0, i
        assert _same_bits(a, b), (i, tuple(a.shape), float((a - b).abs().max()))
        assert _same_bits(a, c), i
    # the entry ADDS to the buffers it is given, as the existing one does: grads = grads + acc
    import radnerf_hip as hip
    views, gs = _grad_buffers(m, False)
    for v in views:
        v.fill_(0.5)
    partials = torch.empty(int(hip._lib.rn_audio_backward_partials_floats(n, 0)), device="cuda")
    hip.call("rn_audio_encode_windows_backward_ordered", C.byref(w), hip.ptr(auds), n, hip.ptr(codes), hip.ptr(grad_enc), C.byref(gs),
             None, hip.ptr(acts), hip.ptr(partials), hip.stream())
    for v, b in zip(views, want):
        assert _same_bits(v, b + 0.5)


def test_attention_window_equals_the_fold_over_its_eight_frames(hiplib):
    """has_att = 1, n = 1 (the training shape).  AudioNet: the fold over f = 0 .. 7 of the has_att = 0 backward of frame f fed
    grad_codes[f] (the per-frame arithmetic is the same code in both modes); AudioAttNet: one workgroup in both entries."""
    from radnerf import audio
    from radnerf.rays import get_audio_features
    from radnerf_hip.abi import AudioWeightsT
    m = _scene(att=2).model
    w, keep = audio._weights(m)
    g = torch.Generator(device="cuda").manual_seed(5)
    feats = torch.randn(24, m.audio_in_dim, 16, device="cuda", generator=g) * 2
    auds = get_audio_features(feats, 2, 2).unsqueeze(0).contiguous()        # frames -2 .. 5: two zero-padded ones
    assert tuple(auds.shape) == (1, 8, m.audio_in_dim, 16)
    grad_enc = torch.randn(1, m.audio_dim, device="cuda", generator=g)
    codes, acts = _forward(m, w, auds, 1)
    got, grad_codes = _ordered(m, w, auds, 1, codes, grad_enc, acts, True)
    again, _ = _ordered(m, w, auds, 1, codes, grad_enc, acts, True)
    old, grad_codes_old = _existing(m, w, auds, 1, codes, grad_enc, acts, True)
    assert _same_bits(grad_codes, grad_codes_old) and not torch.isnan(grad_codes).any()
    w0 = AudioWeightsT.from_buffer_copy(w)
    w0.has_att = 0
    parts = [_existing(m, w0, auds[0, f:f + 1].unsqueeze(0).contiguous(), 1, codes, grad_codes[f:f + 1].contiguous(),
                       acts[f * K_ACTS:(f + 1) * K_ACTS].contiguous(), False)[0] for f in range(8)]
    want = _fold(parts)
    assert len(got) == 24
    for i in range(12):
        assert float(want[i].abs().max()) > 0, i
        assert _same_bits(got[i], want[i]), (i, tuple(got[i].shape), float((got[i] - want[i]).abs().max()))
    for i in range(12, 24):                       # the attention net's gradients: the existing entry's, from its one workgroup
        assert float(old[i].abs().max()) > 0, i
        assert _same_bits(got[i], old[i]), (i, tuple(got[i].shape))
    for a, c in zip(got, again):
        assert _same_bits(a, c)


def test_the_switch_routes_the_autograd_backward(hiplib, monkeypatch):
    """RN_TRAIN_DETERMINISTIC=1: NeRFNetwork.encode_audio's backward gives the same bits twice, within the tolerance
    tests/test_gpu_audio.py holds the atomic entry to (1e-4 of the largest magnitude) of the default route's."""
    from radnerf.rays import get_audio_features
    m = _scene(att=2).model
    m.train()
    g = torch.Generator(device="cuda").manual_seed(6)
    feats = torch.randn(24, m.audio_in_dim, 16, device="cuda", generator=g) * 2
    a = get_audio_features(feats, 2, 7)
    gy = torch.randn(1, 64, device="cuda", generator=g)
    params = [p for mod in (m.audio_net, m.audio_att_net) for p in mod.parameters()]
    runs = {}
    for key, value in (("off", "0"), ("on", "1"), ("again", "1")):
        monkeypatch.setenv("RN_TRAIN_DETERMINISTIC", value)
        runs[key] = torch.autograd.grad(m.encode_audio(a), params, gy)
    for p, off, on, again in zip(params, runs["off"], runs["on"], runs["again"]):
        assert _same_bits(on, again)
        assert (on - off).abs().max().item() <= 1e-4 * max(float(off.abs().max()), 1e-3), tuple(p.shape)
