"""Live mode on the device: the two ring kernels against numpy, LiveASR through the kernels against the features of the whole file,
and `python -m radnerf.live` end to end on tests/dataset_dir.py's directory with the setup of test_gpu_asr_cli.py (its `runs`
fixture: 24 training iterations, the 19200-sample wav, the clip rendered by radnerf.cli from the wav).

Every comparison is exact: the ring kernels are copies, and with RN_ASR=hip a window's logits do not depend on the batch it ran in,
so the live loop's one-window passes and the file mode's batched pass give the same rows.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dataset_dir as dd
import jpegref64 as J
from test_gpu_asr_cli import runs  # noqa: F401  (the fixture: dataset, checkpoint, wav, and radnerf.cli's render of it)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "rad-nerf_amd")
GUARD = 512
SENTINEL = -777.25
OPEN = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------------------------ the kernels
def _np_push(ring, logits, left, right, first, zeros):
    out = ring.copy()
    for i in range(right - left + zeros):
        out[(first + i) % len(ring)] = logits[left + i] if i < right - left else 0.0
    return out


def _np_window(ring, k, n_slices):
    rows, Cc = ring.shape
    out = np.zeros((8, Cc, 16), np.float32)
    for e in range(8):
        s = k - 4 + e
        if 0 <= s < n_slices:
            for t in range(16):
                out[e, :, t] = ring[(rows - 8 + 2 * s + t) % rows]
    return out


@pytest.mark.parametrize("Cc", [44, 32])
@pytest.mark.parametrize("rows,T,left,right,firsts", [(24, 9, 2, 8, (0, 18, 20, 23)), (200, 69, 10, 60, (0, 150, 170, 199))])
def test_ring_push_against_numpy(hiplib, rng, rows, T, left, right, firsts, Cc):
    """first_row at 0, where only the zero tail wraps, where the copy wraps too, and on the last row."""
    logits = rng.standard_normal((T, Cc)).astype(np.float32)
    d_logits = torch.from_numpy(logits).cuda()
    for first in firsts:
        for zeros in (0, 16):
            ring = rng.standard_normal((rows, Cc)).astype(np.float32)
            buf = torch.full((2 * GUARD + rows * Cc,), SENTINEL, device="cuda")
            d_ring = buf[GUARD:GUARD + rows * Cc].view(rows, Cc)
            d_ring.copy_(torch.from_numpy(ring))
            hiplib.call("rn_asr_ring_push", hiplib.ptr(d_logits), T, Cc, left, right, hiplib.ptr(d_ring), rows, first, zeros, hiplib.stream())
            torch.cuda.synchronize()
            assert np.array_equal(d_ring.cpu().numpy(), _np_push(ring, logits, left, right, first, zeros)), (first, zeros)
            assert bool((buf[:GUARD] == SENTINEL).all() and (buf[GUARD + rows * Cc:] == SENTINEL).all())
    lib, err = hiplib._lib, hiplib.last_error
    assert lib.rn_asr_ring_push(hiplib.ptr(d_logits), T, Cc, left, T + 1, hiplib.ptr(d_ring), rows, 0, 0, None) == -1 and "rows" in err()
    assert lib.rn_asr_ring_push(hiplib.ptr(d_logits), T, Cc, 0, T, hiplib.ptr(d_ring), rows, rows, 0, None) == -1 and "first_row" in err()
    assert lib.rn_asr_ring_push(hiplib.ptr(d_logits), T, Cc, 0, min(T, rows), hiplib.ptr(d_ring), rows, 0, rows, None) == -1 and "zero rows" in err()
    assert lib.rn_asr_ring_push(hiplib.ptr(d_logits), T, Cc, 0, 1, hiplib.ptr(d_ring), 8, 0, 0, None) == -1 and "ring_rows" in err()


@pytest.mark.parametrize("Cc", [44, 32])
@pytest.mark.parametrize("rows", [24, 200])
def test_ring_window_against_numpy(hiplib, rng, rows, Cc):
    """k = 0 .. 3 (the zero slices in front), k around every wrap of the reader, n_slices cutting 1, 2 and 3 slices and all."""
    ring = rng.standard_normal((rows, Cc)).astype(np.float32)
    d_ring = torch.from_numpy(ring).cuda()
    n = 8 * Cc * 16
    wrap = rows // 2
    for k in (0, 1, 2, 3, 4, 7, wrap - 5, wrap - 4, wrap, wrap + 3, wrap + 4, 3 * wrap + 1, 100003):
        for n_slices in (OPEN, k + 3, k + 2, k + 1, max(k - 4, 0), 0):
            buf = torch.full((2 * GUARD + n,), SENTINEL, device="cuda")
            out = buf[GUARD:GUARD + n].view(8, Cc, 16)
            hiplib.call("rn_asr_ring_window", hiplib.ptr(d_ring), rows, Cc, k, n_slices, hiplib.ptr(out), hiplib.stream())
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy(), _np_window(ring, k, n_slices)), (k, n_slices)
            assert bool((buf[:GUARD] == SENTINEL).all() and (buf[GUARD + n:] == SENTINEL).all())
    assert np.count_nonzero(_np_window(ring, 0, OPEN)[:4]) == 0 and np.count_nonzero(_np_window(ring, 9, 10)[-3:]) == 0
    assert hiplib._lib.rn_asr_ring_window(hiplib.ptr(d_ring), 8, Cc, 0, OPEN, hiplib.ptr(out), None) == -1 and "ring_rows" in hiplib.last_error()


# ------------------------------------------------------------------------------------------------------------------ LiveASR
def _samples(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.1 * torch.randn(n, generator=g) * (1.0 + torch.sin(torch.arange(n) / 300.0))).float().numpy()


@pytest.mark.parametrize("n,lmr,ring_windows", [(83323, (10, 50, 10), 4), (29243, (3, 12, 3), 8)])
def test_live_windows_equal_the_file_features(hiplib, monkeypatch, n, lmr, ring_windows):
    """83323 samples at 10/50/10: five full windows (the write index wraps the ring of 200 rows) and a terminal one with a short
    last chunk; 29243 samples at 3/12/3 with 8 windows of ring."""
    import json
    from radnerf import live
    from radnerf.asr import Wav2Vec2CTC
    from radnerf.rays import get_audio_features
    monkeypatch.setenv("RN_ASR", "hip")
    z = np.load(os.path.join(HERE, "golden", "asr_tiny.npz"))
    sd = {k[3:]: torch.from_numpy(z[k]).float() for k in z.files if k.startswith("sd/")}
    model = Wav2Vec2CTC.from_state_dict(sd, json.loads(bytes(z["config"]).decode())).cuda()
    x = _samples(n, n % 1000)
    feats = model.features_from_samples(x, *lmr, layout="FC16")
    asr = live.LiveASR(model, *lmr, ring_windows=ring_windows, tail="flush")
    got = [asr.next_window(k).clone() for k in live.schedule(asr, live.chunks_of(x))]
    assert asr.n_frames == len(got) == feats.shape[0] and asr.rows_written // 2 + 1 == feats.shape[0]
    assert asr.windows_run >= 6 and (n < 80000 or asr.rows_written > asr.ring_rows)
    for k, w in enumerate(got):
        assert w.is_cuda and tuple(w.shape) == (8, model.vocab_size, 16)
        assert torch.equal(w, get_audio_features(feats, 2, k)), k


# ------------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def live_runs(runs, tmp_path_factory):  # noqa: F811
    from radnerf import live
    out = str(tmp_path_factory.mktemp("live"))
    args = runs["base"] + ["--pose", os.path.join(runs["root"], "clip.json"), "--asr_weights", runs["weights"], "--asr_config", runs["config"]]
    lines = []
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("RN_ASR", "hip")
        raw = os.path.join(out, "frames.rgb")
        by_wav = live.main(args + ["--wav", runs["wav"], "--video", "--raw_out", raw],
                           log=lambda *a: lines.append(" ".join(str(x) for x in a)), decode=dd.npy_decode)
        frames_by_wav = np.load(by_wav["video"])                       # the next run writes the same file name
        os.remove(by_wav["video"])                                      # what is loaded below is what the child wrote
        env = dict(os.environ, RN_ASR="hip", PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
        child = subprocess.run([sys.executable, "-m", "radnerf.live"] + args + ["--pcm", "-"], input=runs["pcm"], env=env,
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        frames_by_pcm = np.load(by_wav["video"]) if child.returncode == 0 else None
    return dict(by_wav=by_wav, frames_by_wav=frames_by_wav, raw=raw, lines=lines, child=child, frames_by_pcm=frames_by_pcm)


def test_a_live_render_of_the_wav_is_the_clip_of_aud_wav(runs, live_runs):  # noqa: F811
    want = np.load(runs["by_wav"]["video"])
    got = live_runs["frames_by_wav"]
    assert got.dtype == np.uint8 and got.shape == want.shape == (30, dd.H, dd.W, 3) and np.array_equal(got, want)
    assert live_runs["by_wav"]["n_frames"] == 30 and live_runs["by_wav"]["windows"] == 2
    assert any("expected latency = 1.480000s" in ln for ln in live_runs["lines"])          # (50 + 10 + 14) / 50


def test_raw_out_holds_the_same_bytes(live_runs):
    with open(live_runs["raw"], "rb") as fh:
        assert fh.read() == live_runs["frames_by_wav"].tobytes()


def test_the_same_frames_from_a_pipe(live_runs):
    child = live_runs["child"]
    assert child.returncode == 0, child.stdout.decode(errors="replace")[-2000:]
    assert np.array_equal(live_runs["frames_by_pcm"], live_runs["frames_by_wav"])
    assert b"expected latency = 1.480000s" in child.stdout


def test_the_live_video_carries_the_wav(runs, live_runs):  # noqa: F811
    done = live_runs["by_wav"]
    assert done["avi"] and os.path.isfile(done["avi"])
    avi = J.read_avi(open(done["avi"], "rb").read())
    assert avi["avih"]["total_frames"] == 30 and len(avi["streams"]) == 2
    assert b"".join(c[2] for c in avi["movi"] if c[0] == b"01wb") == runs["pcm"]
