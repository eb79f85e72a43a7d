"""The wav2vec2 CTC kernels (csrc/rn_asr.hip, radnerf/asr.py) against float64: tests/golden/asr_tiny.npz (transformers' own model)
and tests/asrref64.py.

The bound: errors are max-normalised against float64; the yardstick is torch's own fp32 run of the same model on the CPU
(`err_f32_cpu` of the fixture; for the other configs measured here, the largest over the config's cases), and the device gets
8 x that: both are fp32 and differ only in summation order and in erf / rsqrt, while a 16-bit product anywhere would sit about
three orders of magnitude higher.
"""
import json
import os

import numpy as np
import pytest
import torch

import asrref64 as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FACTOR = 8.0
LENGTHS = (400, 961, 3200, 22400)                  # T = 1, 2, 9, 69
WIDE = dict(R.TINY, hidden_size=192, num_attention_heads=3, num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=3, vocab_size=32)
REAL = dict(R.TINY, conv_dim=[512] * 7, hidden_size=1024, num_attention_heads=16, intermediate_size=4096, num_conv_pos_embeddings=128,
            num_conv_pos_embedding_groups=16, num_hidden_layers=1)


@pytest.fixture(autouse=True)
def _kernels(monkeypatch):
    """These tests are about the kernels: RN_ASR=hip (the switch's default is the torch path)."""
    monkeypatch.setenv("RN_ASR", "hip")


def _module(sd, cfg, device="cuda"):
    from radnerf.asr import Wav2Vec2CTC
    return Wav2Vec2CTC.from_state_dict(sd, cfg).to(device)


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(HERE, "golden", "asr_tiny.npz"))
    cfg = json.loads(bytes(z["config"]).decode())
    sd = {k[3:]: torch.from_numpy(z[k]).float() for k in z.files if k.startswith("sd/")}
    return dict(cfg=cfg, sd=sd, windows=[torch.from_numpy(z[f"window{i}"]) for i in range(2)],
                logits=[torch.from_numpy(z[f"logits{i}"]) for i in range(2)], yard=float(z["err_f32_cpu"]))


def _windows(B, S, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.1 * torch.randn(B, S, generator=g) * (1.0 + torch.sin(torch.arange(S) / 300.0))).float()


@pytest.fixture(scope="module")
def cases(hiplib):
    """Per config: the state dict, every (S, B) case's windows and float64 logits, and the config's yardstick, computed once."""
    out = {}
    for name, cfg, seed in (("tiny", R.TINY, 3), ("wide", WIDE, 4)):
        sd = R.random_state_dict(cfg, seed=seed, old_names=(name == "tiny"))
        cpu = _module(sd, cfg, "cpu")
        entry = dict(cfg=cfg, sd=sd, runs={}, yard=0.0)
        for S in LENGTHS:
            for B in (1, 3):
                w = _windows(B, S, 100 * B + S % 97)
                want = R.forward(sd, cfg, w)
                entry["runs"][(S, B)] = (w, want)
                entry["yard"] = max(entry["yard"], R.err(cpu(w), want))
        out[name] = entry
    return out


def test_golden_windows(golden, hiplib):
    m = _module(golden["sd"], golden["cfg"])
    for w, want in zip(golden["windows"], golden["logits"]):
        got = m(w[None].cuda())[0]
        assert got.shape == want.shape
        e = R.err(got, want)
        print(f"golden window of {w.numel()} samples: device error {e:.3e}, yardstick {golden['yard']:.3e}")
        assert e <= FACTOR * golden["yard"]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("S", LENGTHS)
@pytest.mark.parametrize("name", ["tiny", "wide"])
def test_shapes_and_edges(cases, name, S, B):
    c = cases[name]
    w, want = c["runs"][(S, B)]
    got = _module(c["sd"], c["cfg"])(w.cuda())
    assert got.shape == want.shape == (B, (S - 400) // 320 + 1, c["cfg"]["vocab_size"])
    e = R.err(got, want)
    print(f"{name} S = {S} B = {B}: device error {e:.3e}, yardstick {c['yard']:.3e}")
    assert e <= FACTOR * c["yard"]


def test_real_widths(hiplib):
    """conv_dim 512, hidden 1024, 16 heads, 4096, K = 128, G = 16, one encoder layer, two windows of 3200 samples."""
    sd = R.random_state_dict(REAL, seed=5, old_names=False)
    w = _windows(2, 3200, 7)
    want = R.forward(sd, REAL, w)
    yard = R.err(_module(sd, REAL, "cpu")(w), want)
    got = _module(sd, REAL)(w.cuda())
    e = R.err(got, want)
    print(f"real widths: device error {e:.3e}, yardstick {yard:.3e}")
    assert got.shape == (2, 9, 44) and e <= FACTOR * yard


@pytest.mark.parametrize("n,lmr,shape", [(48137, (10, 50, 10), (76, 16, 44)), (8001, (2, 6, 2), (12, 16, 44))])
def test_features_against_the_sequential_loop(golden, hiplib, n, lmr, shape):
    x = _windows(1, n, n)[0]
    want, _ = R.features(golden["sd"], golden["cfg"], x.numpy(), *lmr)
    m = _module(golden["sd"], golden["cfg"])
    got = m.features_from_samples(x, *lmr)
    assert tuple(got.shape) == tuple(want.shape) == shape and got.dtype == torch.float32
    e = R.err(got, want)
    print(f"features of {n} samples: device error {e:.3e}, yardstick {golden['yard']:.3e}")
    assert e <= FACTOR * golden["yard"]
    fc16 = m.features_from_samples(x, *lmr, layout="FC16")
    assert fc16.is_contiguous() and torch.equal(fc16.permute(0, 2, 1), got)
    # the rows the unfold pads with are exact zeros
    assert torch.count_nonzero(got[0, :8]) == 0


def test_two_calls_and_two_batch_sizes_give_the_same_bits(golden, hiplib):
    m = _module(golden["sd"], golden["cfg"])
    x = _windows(1, 8001, 11)[0]
    a = m.features_from_samples(x, 2, 6, 2, max_batch=2)
    b = m.features_from_samples(x, 2, 6, 2, max_batch=2)
    c = m.features_from_samples(x, 2, 6, 2, max_batch=8)
    d = m.features_from_samples(x, 2, 6, 2, max_batch=1)
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)
    w = golden["windows"][0][None].cuda()
    assert torch.equal(m(w), m(w))
    both = m(torch.cat([w, w.flip(1)]))
    assert torch.equal(both[0], m(w)[0])                       # a window's logits do not depend on its neighbours in the launch


def test_torch_path_on_the_gpu(golden, hiplib, monkeypatch):
    m = _module(golden["sd"], golden["cfg"])
    w = golden["windows"][0][None].cuda()
    hip_out = m(w)
    monkeypatch.setenv("RN_ASR", "torch")                       # also the switch's default
    torch_out = m(w)
    assert not torch.equal(hip_out, torch_out)                 # another path, not the same kernels
    for got in (hip_out, torch_out):
        assert R.err(got, golden["logits"][0]) <= FACTOR * golden["yard"]
    x = _windows(1, 4480, 13)[0]
    want, _ = R.features(golden["sd"], golden["cfg"], x.numpy(), 2, 6, 2)
    assert R.err(m.features_from_samples(x, 2, 6, 2), want) <= FACTOR * golden["yard"]


def test_refusals_on_the_device(golden, hiplib):
    m = _module(golden["sd"], golden["cfg"])
    with pytest.raises(ValueError, match="receptive field"):
        m(torch.zeros(1, 399, device="cuda"))
    with pytest.raises(ValueError, match="unsupported shape"):
        m(torch.zeros(1, 400 + 320 * 96, device="cuda"))       # 97 steps: past the attention kernel's cap
