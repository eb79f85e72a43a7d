"""The resampling stage on the device: rn_pcm_decode bit for bit against numpy, rn_resample against the float64 restatement
(resampleref64.py) under the float32 chain's own bound, streaming equal to the whole file in every bit, and the three routes that
use it -- radnerf.cli's --aud_wav --resample, LiveASR fed through resampled_chunks, and `python -m radnerf.live --pcm FILE
--pcm_rate ...` as a child process -- with the tiny wav2vec2 model of tests/golden/asr_tiny.npz.

The bound: a float32 fmaf chain of 2 W + 1 terms over coefficients rounded to float32 stays within (2 W + 3) 2^-24 sum |w x| of the
exact sum; it needs no measured constant.  Streaming and the routes are compared with torch.equal: the kernel runs one fixed chain
per output, whatever launch the output falls into."""
import io
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

import dataset_dir as dd
import resampleref64 as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "rad-nerf_amd")
GUARD = 512
SENTINEL = -777.25
TILE = 256
RATES = (48000, 44100, 22050, 11025, 8000)
FORMAT_IDS = {"u8": 0, "s16le": 1, "s24le": 2, "s32le": 3, "f32le": 4}
WIDTH = {"u8": 1, "s16le": 2, "s24le": 3, "s32le": 4, "f32le": 4}


# ---------------------------------------------------------------------------------------------------------------- rn_pcm_decode
def _extremes(fmt):
    """First-channel samples at the ends of the format's range and where the conversion rounds, as raw bytes."""
    if fmt == "u8":
        return np.array([0, 255, 128, 127, 129, 1], np.uint8).tobytes()
    if fmt == "s16le":
        return np.array([-32768, 32767, 0, -1, 1, 255, 256, -256], "<i2").tobytes()
    if fmt == "s24le":
        vals = [-(1 << 23), (1 << 23) - 1, 0, -1, 1, 0x7F, 0x80, 0xFF, 0x100, -0x100, 0x7FFF, 0x8000, -0x8000]
        return b"".join(int(v & 0xFFFFFF).to_bytes(3, "little") for v in vals)
    if fmt == "s32le":                  # 2^24 + 1, 2^24 + 3: ties to even; 2^31 - 65 .. 2^31 - 1: rounds up to 2^31
        vals = [-(1 << 31), (1 << 31) - 1, 0, -1, 1, (1 << 24) + 1, (1 << 24) + 3, -(1 << 24) - 1, (1 << 31) - 65, (1 << 31) - 64, (1 << 31) - 129]
        return np.array(vals, "<i4").tobytes()
    return np.array([np.inf, -np.inf, np.nan, -0.0, 0.0, 1e-45, -1e-45, 3.4028235e38, 1.17549435e-38, 1.0, -1.0], "<f4").tobytes()


def _frames(fmt, channels, n, rng):
    """n frames: the extremes first (as many as fit), random bytes after them and in every other channel."""
    w = WIDTH[fmt]
    if fmt == "f32le":
        body = rng.standard_normal(n * channels).astype("<f4").view(np.uint8).reshape(n, channels, w).copy()
    else:
        body = rng.integers(0, 256, (n, channels, w), dtype=np.uint8)
    ext = np.frombuffer(_extremes(fmt), np.uint8).reshape(-1, w)[:n]
    body[:len(ext), 0, :] = ext
    return body.tobytes()


@pytest.mark.parametrize("channels", [1, 2, 6])
@pytest.mark.parametrize("fmt", list(FORMAT_IDS))
def test_pcm_decode_bit_exact(hiplib, rng, fmt, channels):
    for n in (0, 1, TILE - 1, TILE, TILE + 1, 1000):
        raw = _frames(fmt, channels, n, rng)
        want = R.numpy_decode(raw, fmt, channels)
        for offset in (0, 1):                                                   # the input has byte alignment only
            src = torch.zeros(offset + len(raw) + 16, dtype=torch.uint8, device="cuda")
            src[offset:offset + len(raw)] = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda() if n else src[:0]
            view = src[offset:]
            assert view.data_ptr() % 2 == offset
            buf = torch.full((2 * GUARD + n,), SENTINEL, device="cuda")
            out = buf[GUARD:GUARD + n]
            hiplib.call("rn_pcm_decode", hiplib.ptr(view), n, channels, FORMAT_IDS[fmt], hiplib.ptr(out), hiplib.stream())
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32)), (n, offset)
            assert bool((buf[:GUARD] == SENTINEL).all() and (buf[GUARD + n:] == SENTINEL).all())


def test_resampler_decodes_on_the_device(hiplib, rng):
    from radnerf import resample as rs
    raw = _frames("s24le", 2, 777, rng)
    r = rs.Resampler(16000, 16000, "s24le", 2, device="cuda")
    got = torch.cat([r.push(raw[:1000]), r.push(raw[1000:1001]), r.push(raw[1001:]), r.flush()])
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), R.numpy_decode(raw, "s24le", 2)) and torch.equal(got, r.whole(raw))


# ------------------------------------------------------------------------------------------------------------------ rn_resample
_cases = {}


def cases_of(src):
    """{name: (x float32, y float64, bound)} per rate, computed once and shared."""
    if src not in _cases:
        L, M, W, _ = R.ratio(src)
        rng = np.random.default_rng(src)
        sig = {"one frame": 1, "W - 1 frames": W - 1, "2 W + 1 frames": 2 * W + 1}
        for k in (TILE - 1, TILE, TILE + 1):
            sig[f"n_out = {k}"] = -(-k * M // L)
        xs = {name: rng.uniform(-1, 1, n).astype(np.float32) for name, n in sig.items()}
        imp = np.zeros(src // 4, np.float32)
        imp[0], imp[-1] = 1.0, -0.75
        xs["impulses at both ends"] = imp
        xs["quarter second"] = rng.uniform(-1, 1, src // 4).astype(np.float32)
        out = {}
        for name, x in xs.items():
            y, b = R.resample(x, src)
            for a in (x, y, b):
                a.setflags(write=False)
            out[name] = (x, y, b)
        # going up in rate not every count occurs: the shortest input that gives at least k outputs gives k or k + 1 (8000 Hz: 256,
        # 256, 258; 11025 Hz: 255, 256, 258) -- at or just below the tile, exactly the tile, and past it either way
        counts = [len(out[f"n_out = {k}"][1]) for k in (TILE - 1, TILE, TILE + 1)]
        assert counts[0] in (TILE - 1, TILE) and counts[1] == TILE and counts[2] in (TILE + 1, TILE + 2), counts
        assert M < L or counts == [TILE - 1, TILE, TILE + 1]
        _cases[src] = out
    return _cases[src]


@pytest.mark.parametrize("src", RATES)
def test_resample_within_the_float32_bound(hiplib, src):
    from radnerf import resample as rs
    r = rs.Resampler(src, device="cuda")
    cpu = rs.Resampler(src)
    for name, (x, y, b) in cases_of(src).items():
        got = r.whole(x.copy())
        assert got.is_cuda and got.dtype == torch.float32 and got.numel() == len(y), name
        assert torch.equal(got, r.whole(x.copy())), name                                 # two calls, the same bits
        bound = R.f32_bound(src, 16000, b)
        err = np.abs(got.cpu().numpy().astype(np.float64) - y)
        host = cpu.whole(x.copy()).numpy().astype(np.float64)
        print(f"{src} Hz, {name}: {len(y)} outputs, max err {err.max() if len(y) else 0:.3e}, worst share of the bound "
              f"{np.max(err / np.maximum(bound, 1e-300)) if len(y) else 0:.3f}, device - cpu {np.abs(host - got.cpu().numpy()).max() if len(y) else 0:.3e}")
        assert np.all(err <= bound), name
        assert np.all(np.abs(host - y) <= bound) and np.all(np.abs(host - got.cpu().numpy()) <= 2 * bound), name
    x, y, _ = cases_of(src)["impulses at both ends"]
    assert np.abs(y[:8]).max() > 1e-3 and np.abs(y[-8:]).max() > 1e-3                   # the edges are not silent: zeros outside were read


@pytest.mark.parametrize("src", [48000, 44100, 8000])
def test_resample_entry_writes_its_outputs_only_and_ignores_the_launch(hiplib, src):
    """The entry point itself: guards around y, and the same bits for a sample whatever t0, origin or n_out its launch had."""
    from radnerf import resample as rs
    r = rs.Resampler(src, device="cuda")
    L, M, W = r.L, r.M, r.W
    x = torch.from_numpy(cases_of(src)["quarter second"][0].copy()).cuda()
    whole = r.whole(x)
    for t0, count in ((0, TILE + 1), (TILE - 1, 2), (TILE, 1), (3 * TILE - 7, 2 * TILE + 14), (whole.numel() - 1, 1)):
        first = max(0, (t0 * M) // L - W - 5)                                            # a buffer that starts just below the span
        last = min(x.numel(), ((t0 + count - 1) * M) // L + W + 3)
        part = x[first:last].contiguous()
        buf = torch.full((2 * GUARD + count,), SENTINEL, device="cuda")
        y = buf[GUARD:GUARD + count]
        hiplib.call("rn_resample", hiplib.ptr(part), part.numel(), first, hiplib.ptr(r.taps), L, M, W, t0, count, hiplib.ptr(y), hiplib.stream())
        torch.cuda.synchronize()
        assert torch.equal(y, whole[t0:t0 + count]), (t0, count)
        assert bool((buf[:GUARD] == SENTINEL).all() and (buf[GUARD + count:] == SENTINEL).all())


# -------------------------------------------------------------------------------------------------------------------- streaming
def _chunked(r, x, sizes):
    parts, at = [], 0
    for c in sizes:
        parts.append(r.push(x[at:at + c]))
        at += c
    assert at >= len(x)
    return torch.cat(parts + [r.flush()])


@pytest.mark.parametrize("src", [48000, 44100, 8000])
def test_streaming_equals_the_whole_file(hiplib, src):
    from radnerf import resample as rs
    L, M, W = rs.plan(src)
    x = cases_of(src)["quarter second"][0]
    new = lambda: rs.Resampler(src, device="cuda")
    short = x[:2 * W + 1 + 5 * M + 31]
    whole_short, whole = new().whole(short.copy()), new().whole(x.copy())
    for c in (1, 7, M):
        assert torch.equal(_chunked(new(), short, [c] * -(-len(short) // c)), whole_short), c
    for c in (round(src / 50), 4096):
        assert torch.equal(_chunked(new(), x, [c] * -(-len(x) // c)), whole), c
    cuts = np.sort(np.random.default_rng(7).integers(0, len(x), 9))
    assert torch.equal(_chunked(new(), x, list(np.diff(np.concatenate([[0], cuts, [len(x)]])))), whole)
    # one push up to just below output TILE, single frames across it, the rest (more than a tile) in one push
    before = W + ((TILE - 3) * M) // L
    assert torch.equal(_chunked(new(), x, [before] + [1] * (8 * -(-M // L)) + [len(x)]), whole)
    raw = (x * 32767).astype("<i2").tobytes()                                            # raw bytes, split inside a frame
    r = rs.Resampler(src, 16000, "s16le", 1, device="cuda")
    assert torch.equal(torch.cat([r.push(raw[:4097]), r.push(raw[4097:]), r.flush()]), r.whole(raw))


# ------------------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def tiny():
    from radnerf.asr import Wav2Vec2CTC
    z = np.load(os.path.join(HERE, "golden", "asr_tiny.npz"))
    sd = {k[3:]: torch.from_numpy(z[k]).float() for k in z.files if k.startswith("sd/")}
    cfg = json.loads(bytes(z["config"]).decode())
    return dict(sd=sd, cfg=cfg, model=Wav2Vec2CTC.from_state_dict(sd, cfg).cuda())


def _signal(rate, seconds, channels):
    """Interleaved float frames: channel 0 a modulated tone, the others something else (they must not be read)."""
    t = np.arange(int(rate * seconds)) / rate
    first = 0.3 * np.sin(2 * np.pi * 310 * t) * (1 + np.sin(2 * np.pi * 3 * t)) + 0.1 * np.sin(2 * np.pi * 2900 * t)
    return np.stack([first] + [0.5 * np.cos(2 * np.pi * 500 * (c + 1) * t) for c in range(1, channels)], axis=1)


def _pcm(frames, bits):
    v = np.round(frames * (2 ** (bits - 1) - 1)).astype(np.int64)
    if bits == 16:
        return v.astype("<i2").tobytes()
    return b"".join(int(s & 0xFFFFFF).to_bytes(3, "little") for s in v.reshape(-1))


def test_cli_features_from_any_wav(hiplib, tiny, tmp_path, monkeypatch):
    from radnerf import cli
    from radnerf.resample import samples_16k
    monkeypatch.setenv("RN_ASR", "hip")
    weights, config = tmp_path / "w2v.pth", tmp_path / "w2v.json"
    torch.save(tiny["sd"], str(weights))
    config.write_text(json.dumps(tiny["cfg"]))
    stub = type("AudioNet", (), dict(audio_in_dim=44))()
    quiet = lambda *a: None
    def features(path, *flags):
        opt = cli.parse(["d", "--test", "--aud_wav", str(path), "--asr_weights", str(weights), "--asr_config", str(config), "-l", "2", "-m", "6",
                         "-r", "2"] + list(flags))
        return cli.wav_features(opt, stub, torch.device("cuda"), quiet), opt
    seconds = 0.9
    f48 = tmp_path / "s24_48k.wav"
    f48.write_bytes(R.riff(1, 2, 48000, 24, _pcm(_signal(48000, seconds, 2), 24), extensible=True))
    got, opt = features(f48, "--resample")
    want = tiny["model"].features_from_samples(samples_16k(str(f48), "cuda"), 2, 6, 2, layout="FC16")
    assert got.is_cuda and opt.aud_features is got and torch.equal(got, want) and bool(got.abs().max() > 0)
    f16 = tmp_path / "s16_16k.wav"
    with wave.open(str(f16), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes(_pcm(_signal(16000, seconds, 1), 16))
    plain, _ = features(f16)
    same, _ = features(f16, "--resample")
    assert torch.equal(plain, same)                                                      # 16 kHz passes through with its bits
    assert got.shape == plain.shape and got.shape[0] > 8                                 # D seconds give D seconds' frames at any rate


def test_live_windows_from_a_44k_stream_equal_the_file_features(hiplib, tiny, monkeypatch):
    from radnerf import live
    from radnerf import resample as rs
    from radnerf.rays import get_audio_features
    monkeypatch.setenv("RN_ASR", "hip")
    lmr = (3, 12, 3)
    raw = _pcm(_signal(44100, 1.83, 2), 16)                                              # s16le stereo
    x16 = rs.Resampler(44100, 16000, "s16le", 2, device="cuda").whole(raw)
    feats = tiny["model"].features_from_samples(x16, *lmr, layout="FC16")
    source = live.block_reader(io.BytesIO(raw), 44100, "s16le", 2)
    read_chunk = live.resampled_chunks(source, rs.Resampler(44100, 16000, "s16le", 2, device="cuda"))
    lengths = []
    def counted():
        c = read_chunk()
        lengths.append(len(c))
        return c
    asr = live.LiveASR(tiny["model"], *lmr, ring_windows=8, tail="flush")
    got = [asr.next_window(k).clone() for k in live.schedule(asr, counted)]
    assert sum(lengths) == x16.numel() and all(n == 320 for n in lengths[:-1]) and lengths[-1] < 320
    assert asr.n_frames == len(got) == feats.shape[0] and asr.windows_run >= 4
    for k, w in enumerate(got):
        assert torch.equal(w, get_audio_features(feats, 2, k)), k


@pytest.fixture(scope="module")
def trained(tmp_path_factory, hiplib, tiny):
    """tests/dataset_dir.py's directory, 24 training iterations, the tiny model's files and 1.2 s of 48 kHz stereo s16le as a .wav
    and as raw frames."""
    from radnerf import cli
    root, ws = str(tmp_path_factory.mktemp("dataset")), str(tmp_path_factory.mktemp("workspace"))
    dd.write_dataset(root, 0)
    weights, config = os.path.join(root, "w2v.pth"), os.path.join(root, "w2v.json")
    torch.save(tiny["sd"], weights)
    with open(config, "w") as fh:
        fh.write(json.dumps(tiny["cfg"]))
    raw = _pcm(_signal(48000, 1.2, 2), 16)
    wav, pcm = os.path.join(root, "talk48.wav"), os.path.join(root, "talk48.pcm")
    with wave.open(wav, "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(48000)
        w.writeframes(raw)
    with open(pcm, "wb") as fh:
        fh.write(raw)
    base = [root, "--workspace", ws, "--num_rays", "256", "-O"]
    cli.main(base + ["--iters", "24", "--ckpt", "scratch"], log=lambda *a: None, decode=dd.npy_decode)
    return dict(base=base + ["--pose", os.path.join(root, "clip.json"), "--asr_weights", weights, "--asr_config", config], wav=wav, pcm=pcm)


def test_live_from_a_raw_48k_stream_renders_the_frames_of_the_wav(trained):
    from radnerf import live
    lines = []
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("RN_ASR", "hip")
        by_wav = live.main(trained["base"] + ["--wav", trained["wav"], "--resample"], log=lambda *a: lines.append(" ".join(str(x) for x in a)),
                           decode=dd.npy_decode)
        frames_by_wav = np.load(by_wav["video"])
        os.remove(by_wav["video"])                                                       # what is loaded below is what the child wrote
        env = dict(os.environ, RN_ASR="hip", PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
        child = subprocess.run([sys.executable, "-m", "radnerf.live"] + trained["base"] + ["--pcm", trained["pcm"], "--pcm_rate", "48000",
                                "--pcm_format", "s16le", "--pcm_channels", "2"], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                               timeout=300)
    assert child.returncode == 0, child.stdout.decode(errors="replace")[-2000:]
    frames_by_pcm = np.load(by_wav["video"])
    assert frames_by_wav.dtype == np.uint8 and frames_by_wav.shape == (30, dd.H, dd.W, 3) and by_wav["n_frames"] == 30
    assert np.array_equal(frames_by_pcm, frames_by_wav)
    latency = "expected latency = 1.484021s"                                             # (50 + 10 + 14) / 50 + 193 / 48000
    assert any(latency in ln for ln in lines) and latency.encode() in child.stdout
