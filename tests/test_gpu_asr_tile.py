"""The two tilings of the wav2vec2 matrix products (csrc/rn_asr.hip: k_gemm on 128-row tiles through LDS, k_gemm32 with one wave per
32 x 32 tile) give the same bits: RN_ASR_TILE = 32 | 128 | auto against each other, the 32-row tiling against float64.

Shapes: the `tiny` and `wide` configs of test_gpu_asr.py at S = 400, 961, 3200, 10640, 22400 (T = 1, 2, 9, 33, 69) and B = 1, 3 put
the M of the encoder's products at 1, 2, 3, 6, 9, 27, 33, 69, 99 and 207 -- both sides of the 32- and 64-row edges -- and the conv
layers' M up to 3 x 4479; N = 44 and 32 (the heads) and 8 (a group of `tiny`'s positional conv) are no multiples of 32; conv layers
1 - 6 walk K in one segment per row, the positional conv in one segment per tap, over blockIdx.z groups.  The `REAL` widths run one
window of 22400 samples (M = 69 at N = 1024, 3072, 4096 and K up to 4096).

The bound against float64 is test_gpu_asr.py's: 8 x the largest error of torch's own fp32 CPU run over the config's cases.
"""
import pytest
import torch

import asrref64 as R
from test_gpu_asr import REAL, WIDE, _module, _windows

pytestmark = pytest.mark.gpu

FACTOR = 8.0
LENGTHS = (400, 961, 3200, 10640, 22400)
GUARD = 1024
SENTINEL = -12345.5


@pytest.fixture(autouse=True)
def _kernels(monkeypatch):
    monkeypatch.setenv("RN_ASR", "hip")


@pytest.fixture(scope="module")
def cases(hiplib):
    """Per config: the device module, every (S, B) case's windows and float64 logits, and the config's yardstick, computed once."""
    out = {}
    for name, cfg, seed in (("tiny", R.TINY, 3), ("wide", WIDE, 4)):
        sd = R.random_state_dict(cfg, seed=seed, old_names=(name == "tiny"))
        cpu = _module(sd, cfg, "cpu")
        entry = dict(cfg=cfg, module=_module(sd, cfg), runs={}, yard=0.0)
        for S in LENGTHS:
            for B in (1, 3):
                w = _windows(B, S, 100 * B + S % 97)
                want = R.forward(sd, cfg, w)
                entry["runs"][(S, B)] = (w, want)
                entry["yard"] = max(entry["yard"], R.err(cpu(w), want))
        out[name] = entry
    return out


def _guarded(module, w, tile, monkeypatch):
    """forward_hip into the middle of a buffer of sentinels -> (logits, whether both guards are untouched)."""
    monkeypatch.setenv("RN_ASR_TILE", tile)
    B, S = w.shape
    T, C = (S - 400) // 320 + 1, module.vocab_size
    buf = torch.full((2 * GUARD + B * T * C,), SENTINEL, device="cuda")
    out = module.forward_hip(w, out=buf[GUARD:GUARD + B * T * C].view(B, T, C))
    torch.cuda.synchronize()
    return out.clone(), bool((buf[:GUARD] == SENTINEL).all() and (buf[GUARD + B * T * C:] == SENTINEL).all())


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("S", LENGTHS)
@pytest.mark.parametrize("name", ["tiny", "wide"])
def test_both_tilings_give_the_same_bits(cases, name, S, B, monkeypatch):
    c = cases[name]
    w, want = c["runs"][(S, B)]
    got = {tile: _guarded(c["module"], w.cuda(), tile, monkeypatch) for tile in ("32", "128", "auto")}
    assert all(ok for _, ok in got.values()), "a write outside the logits"
    assert got["32"][0].shape == want.shape and torch.isfinite(got["32"][0]).all()
    assert torch.equal(got["32"][0], got["128"][0])
    assert torch.equal(got["auto"][0], got["128"][0])
    e = R.err(got["32"][0], want)
    print(f"{name} S = {S} B = {B}: 32-row tiles against float64 {e:.3e}, yardstick {c['yard']:.3e}")
    assert e <= FACTOR * c["yard"]


def test_real_widths_one_window(hiplib, monkeypatch):
    """conv_dim 512, hidden 1024, 16 heads, 4096, K = 128, G = 16, one encoder layer: the live window, M = 69."""
    sd = R.random_state_dict(REAL, seed=5, old_names=False)
    m = _module(sd, REAL)
    w = _windows(1, 22400, 7).cuda()
    got = {tile: _guarded(m, w, tile, monkeypatch) for tile in ("32", "128", "auto")}
    assert all(ok for _, ok in got.values())
    assert got["32"][0].shape == (1, 69, 44) and torch.isfinite(got["32"][0]).all() and float(got["32"][0].abs().max()) > 0
    assert torch.equal(got["32"][0], got["128"][0])
    assert torch.equal(got["auto"][0], got["128"][0])


def test_the_entry_point_names_a_bad_tile(hiplib):
    import ctypes as C
    sd = R.random_state_dict(R.TINY, seed=3)
    m = _module(sd, R.TINY)
    w = _windows(1, 961, 1).cuda()
    n = m.workspace_bytes(1, 961)
    ws, out = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(1, 2, 44, device="cuda")
    rc = hiplib._lib.rn_asr_forward_tile(C.byref(m.c_config()), hiplib.ptr(m.packed_image()), ws.data_ptr(), n, hiplib.ptr(w), 1, 961,
                                         hiplib.ptr(out), 64, None)
    assert rc == -1 and "tile must be 0 (auto), 32 or 128" in hiplib.last_error()
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("RN_ASR_TILE", "64")
        with pytest.raises(ValueError, match="RN_ASR_TILE"):
            m.forward_hip(w)
