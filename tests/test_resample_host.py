"""radnerf/resample.py without a GPU: the plan and the table against the float64 restatement (resampleref64.py), the filter's quality
asserted on that restatement itself, scipy's own polyphase resampler as an independent construction, the torch-CPU path of Resampler
against the float32 bound, chunking invariance, read_audio, the parsers' new flags and the host-side checks of the two entry points."""
import ctypes
import struct
import wave

import numpy as np
import pytest
import scipy.signal
import torch

import resampleref64 as R

SIX = (8000, 11025, 22050, 32000, 44100, 48000)
EDGE = 400                                              # outputs ignored at each end of a 0.25 s signal
_ref = {}


def ref_of(key, make, src):
    """(x, y float64, bound) of a named signal at a rate, computed once and shared (never written to)."""
    if (key, src) not in _ref:
        x = make(src)
        y, b = R.resample(x, src)
        for a in (x, y, b):
            a.setflags(write=False)
        _ref[(key, src)] = (x, y, b)
    return _ref[(key, src)]


def uniform(src):
    return np.random.default_rng(src).uniform(-1.0, 1.0, src // 4).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------- plan and table
@pytest.mark.parametrize("src,L,M,W", [(8000, 2, 1, 64), (11025, 640, 441, 64), (22050, 320, 441, 89), (32000, 1, 2, 128),
                                       (44100, 160, 441, 177), (48000, 1, 3, 192), (96000, 1, 6, 384), (16000, 1, 1, 64)])
def test_plan_and_table(src, L, M, W):
    from radnerf import resample as rs
    assert rs.plan(src) == (L, M, W) == R.ratio(src)[:3]
    tab, l, m, w = rs.phase_table(src)
    assert (l, m, w) == (L, M, W) and tab.shape == (L, 2 * W + 1) and tab.dtype == np.float32
    ref = R.table(src)
    assert np.all(np.abs(tab.astype(np.float64) - ref) <= 2.0 ** -24 * np.abs(ref) + 1e-15)
    assert np.abs(tab.astype(np.float64).sum(axis=1) - 1.0).max() <= 2e-7
    for n in (0, 1, 2, M - 1, M, M + 1, 1000):
        assert rs.n_out(n, L, M) == (n * L) // M
        if src != 16000 and n <= 2:
            assert rs.Resampler(src).whole(np.zeros(n, np.float32)).numel() == (n * L) // M


def test_table_sizes_of_the_common_rates():
    from radnerf import resample as rs
    assert rs.phase_table(44100)[0].nbytes == 160 * 355 * 4 and rs.phase_table(11025)[0].nbytes == 640 * 129 * 4


def test_refusals_of_the_plan():
    from radnerf import resample as rs
    with pytest.raises(ValueError, match="16000 phases"):
        rs.plan(44101)
    with pytest.raises(ValueError, match="16000 phases"):
        rs.Resampler(44101)
    for src, dst in ((0, 16000), (-1, 16000), (16000, 0)):
        with pytest.raises(ValueError, match="positive"):
            rs.plan(src, dst)
    with pytest.raises(ValueError, match="format"):
        rs.Resampler(48000, format="s16be")
    with pytest.raises(ValueError, match="channels"):
        rs.Resampler(48000, channels=0)


# -------------------------------------------------------------------------------------------- quality, on the reference itself
@pytest.mark.parametrize("src", SIX)
def test_passband_and_stopband_of_the_reference(src):
    for f in (440, 3000, 7000):
        if f < src / 2:
            y = ref_of(("tone", f), lambda s, f=f: R.tone(f, s), src)[1]
            want = np.sin(2 * np.pi * f * np.arange(len(y)) / 16000.0)
            err = np.abs(y - want)[EDGE:-EDGE].max()
            print(f"passband {src} Hz, {f} Hz tone: {err:.3e}")
            assert len(y) > 3 * EDGE and err < 1e-5
    for f in (8600, 9000, 12000):
        if f < src / 2:
            y = ref_of(("tone", f), lambda s, f=f: R.tone(f, s), src)[1]
            amp = np.abs(y)[EDGE:-EDGE].max()
            print(f"stopband {src} Hz, {f} Hz tone: {amp:.3e}")
            assert amp < 1e-5


def two_tones(src):
    return 0.5 * R.tone(440, src) + 0.3 * R.tone(2500, src)


@pytest.mark.parametrize("src", SIX[1:])
def test_against_scipys_polyphase_resampler(src):
    """An independent construction of the same thing: resample_poly designs its own Kaiser low-pass.  8000 -> 16000 is left out:
    its filter differs there by 1.1e-4 on this signal."""
    x, y, _ = ref_of("two", two_tones, src)
    L, M = R.ratio(src)[:2]
    other = scipy.signal.resample_poly(x, L, M, window=("kaiser", 14.0))
    n = min(len(y), len(other))
    d = np.abs(y[:n] - other[:n])[EDGE:-EDGE].max()
    print(f"resample_poly {src} Hz: {d:.3e}")
    assert d < 2e-6


# ------------------------------------------------------------------------------------------------------------- the torch path
@pytest.mark.parametrize("src", SIX + (96000,))
def test_cpu_path_within_the_float32_bound(src):
    from radnerf import resample as rs
    x, y, b = ref_of("uniform", uniform, src)
    got = rs.Resampler(src).whole(x)
    assert got.dtype == torch.float32 and got.device.type == "cpu" and got.numel() == len(y)
    err = np.abs(got.numpy().astype(np.float64) - y)
    print(f"cpu path {src} Hz: max err {err.max():.3e}, worst share of the bound {np.max(err / np.maximum(R.f32_bound(src, 16000, b), 1e-300)):.3f}")
    assert np.all(err <= R.f32_bound(src, 16000, b))


def _chunked(r, x, sizes):
    parts, at = [], 0
    for c in sizes:
        parts.append(r.push(x[at:at + c]))
        at += c
    assert at >= len(x)
    parts.append(r.flush())
    assert r.flush().numel() == 0
    return torch.cat(parts)


@pytest.mark.parametrize("src", [8000, 44100, 48000])
def test_chunking_does_not_change_a_bit(src):
    from radnerf import resample as rs
    L, M, W = rs.plan(src)
    x = uniform(src)
    short = x[:2 * W + 1 + 5 * M + 31]
    whole_short, whole = rs.Resampler(src).whole(short), rs.Resampler(src).whole(x)
    assert whole_short.numel() == (len(short) * L) // M and whole.numel() == (len(x) * L) // M
    for c in (1, 7, M):
        assert torch.equal(_chunked(rs.Resampler(src), short, [c] * -(-len(short) // c)), whole_short), c
    for c in (round(src / 50), 4096):
        assert torch.equal(_chunked(rs.Resampler(src), x, [c] * -(-len(x) // c)), whole), c
    cuts = np.sort(np.random.default_rng(7).integers(0, len(x), 9))
    sizes = list(np.diff(np.concatenate([[0], cuts, [len(x)]])))
    assert torch.equal(_chunked(rs.Resampler(src), x, sizes), whole)
    r = rs.Resampler(src)
    head = r.push(x[:100])
    assert torch.equal(r.whole(x), whole)                       # whole() does not disturb a stream, nor the stream whole()
    assert torch.equal(torch.cat([head, r.push(x[100:]), r.flush()]), whole)
    with pytest.raises(RuntimeError, match="flushed"):
        r.push(x[:1])


def test_raw_frames_split_anywhere_and_the_same_rate():
    from radnerf import resample as rs
    rng = np.random.default_rng(3)
    raw = rng.integers(0, 256, 6 * 2000, dtype=np.uint8).tobytes()            # 2000 frames of s24le stereo
    r = rs.Resampler(48000, 16000, "s24le", 2)
    whole = r.whole(raw)
    assert torch.equal(whole, r.whole(rs.decode_numpy(raw, "s24le", 2))) and whole.numel() == 666
    parts, at = [], 0
    for c in (1, 5, 7, 1000, 11, 6000, 4000, 10 ** 6):
        parts.append(r.push(raw[at:at + c]))
        at += c
    assert torch.equal(torch.cat(parts + [r.flush()]), whole)
    same = rs.Resampler(16000, 16000, "s16le", 1)
    x = rng.integers(-32768, 32768, 999).astype("<i2")
    assert same.passthrough and same.latency == 0.0
    assert np.array_equal(same.whole(x.tobytes()).numpy(), x.astype(np.float32) / np.float32(32768))
    f = rng.standard_normal(50).astype(np.float32)
    assert np.array_equal(torch.cat([same.push(x.tobytes()[:7]), same.push(x.tobytes()[7:]), same.flush()]).numpy(), x.astype(np.float32) / np.float32(32768))
    assert np.array_equal(rs.Resampler(16000).whole(f).numpy().view(np.uint32), f.view(np.uint32))
    assert rs.Resampler(48000).latency == 193 / 48000


# ------------------------------------------------------------------------------------------------------------------ read_audio
riff, numpy_decode = R.riff, R.numpy_decode


BODIES = {"u8": (1, 8), "s16le": (1, 16), "s24le": (1, 24), "s32le": (1, 32), "f32le": (3, 32)}


@pytest.mark.parametrize("fmt", list(BODIES))
def test_read_audio_round_trips_every_format(tmp_path, capsys, fmt):
    from radnerf import resample as rs
    tag, bits = BODIES[fmt]
    rng = np.random.default_rng(bits)
    for channels, extensible in ((1, False), (2, True), (6, True)):
        if fmt == "f32le":
            body = rng.standard_normal(40 * channels).astype("<f4").tobytes()
        else:
            body = rng.integers(0, 256, 40 * channels * bits // 8, dtype=np.uint8).tobytes()
        path = tmp_path / f"{fmt}_{channels}.wav"
        path.write_bytes(riff(tag, channels, 44100, bits, body, extensible=extensible))
        assert rs.check_audio(str(path)) == (44100, channels, fmt, 40) and capsys.readouterr().out == ""
        rate, ch, name, raw = rs.read_audio(str(path))
        out = capsys.readouterr().out
        assert (rate, ch, name, raw) == (44100, channels, fmt, body)
        assert out.count("[WARN]") == (channels > 1) and (channels == 1 or f"{channels} channels" in out)
        got = rs.decode_numpy(raw, name, ch)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), numpy_decode(body, fmt, channels).view(np.uint32))


def test_read_audio_walks_the_chunks(tmp_path):
    from radnerf import resample as rs
    body = np.arange(-5, 6, dtype="<i2").tobytes() + b"\x07"             # 11 frames and a stray byte: an odd data chunk
    odd = [(b"LIST", b"INFOabc"), (b"junk", b"")]                        # an odd-sized chunk (padded) and an empty one in front
    p = tmp_path / "list.wav"
    p.write_bytes(riff(1, 1, 22050, 16, body, before=odd))
    assert rs.read_audio(str(p)) == (22050, 1, "s16le", body[:22])
    p.write_bytes(riff(1, 2, 48000, 16, body[:18], data_size=4000))      # the data chunk says more than the file holds
    assert rs.check_audio(str(p)) == (48000, 2, "s16le", 4) and rs.read_audio(str(p))[3] == body[:16]
    p.write_bytes(riff(1, 1, 48000, 16, body[:22], data_size=10, riff_pad=b"tail"))      # ... or less: only the chunk is read
    assert rs.read_audio(str(p))[3] == body[:10]
    x = rs.samples_16k(str(p))
    assert x.dtype == torch.float32 and x.numel() == 1
    with wave.open(str(p), "wb") as w:                                   # what the wave module writes is read alike
        w.setnchannels(1); w.setsampwidth(3); w.setframerate(8000)
        w.writeframes(bytes(range(30)))
    assert rs.read_audio(str(p)) == (8000, 1, "s24le", bytes(range(30)))


@pytest.mark.parametrize("field,blob", [
    ("format tag 2", riff(2, 1, 16000, 4, b"\0" * 8)), ("format tag 7", riff(7, 1, 8000, 8, b"\0" * 8)),
    ("bits per sample = 64", riff(3, 1, 16000, 64, b"\0" * 16)), ("sample rate = 0", riff(1, 1, 0, 16, b"\0" * 8)),
    ("channels = 0", struct.pack("<4sI4s4sIHHIIHH4sI", b"RIFF", 36, b"WAVE", b"fmt ", 16, 1, 0, 16000, 0, 0, 16, b"data", 0)),
    ("bits per sample = 12", riff(1, 1, 16000, 12, b"\0" * 8)), ("block align", riff(1, 2, 16000, 16, b"\0" * 8)[:32] + b"\x02" + riff(1, 2, 16000, 16, b"\0" * 8)[33:]),
    ("format tag 2", riff(2, 1, 16000, 16, b"\0" * 8, extensible=True)), ("not a RIFF/WAVE", b"RIFX" + b"\0" * 40), ("no data chunk", riff(1, 1, 16000, 16, b"")[:36])])
def test_read_audio_refusals_name_the_field(tmp_path, field, blob):
    from radnerf import resample as rs
    p = tmp_path / "bad.wav"
    p.write_bytes(blob)
    for fn in (rs.check_audio, rs.read_audio):
        with pytest.raises(ValueError, match=field):
            fn(str(p))


# --------------------------------------------------------------------------------------------------------------------- parsers
@pytest.fixture
def files(tmp_path):
    f48 = tmp_path / "f48.wav"
    f48.write_bytes(riff(3, 2, 48000, 32, np.zeros(2 * 960, "<f4").tobytes()))
    bad = tmp_path / "odd.wav"
    bad.write_bytes(riff(1, 1, 44101, 16, b"\0" * 8))
    w16 = tmp_path / "a.wav"
    w16.write_bytes(riff(1, 1, 16000, 16, b"\0" * 640))
    weights = tmp_path / "w.pth"
    weights.write_bytes(b"")
    return dict(f48=str(f48), bad=str(bad), w16=str(w16), weights=str(weights), dir=str(tmp_path))


def test_cli_parse_with_resample_touches_no_gpu(files, capsys, monkeypatch):
    from radnerf import cli
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("a GPU call was made"))
    def refused(argv, text):
        with pytest.raises(SystemExit) as e:
            cli.parse(["d"] + argv)
        assert e.value.code == 2 and text in capsys.readouterr().err
    asr = ["--asr_weights", files["weights"]]
    refused(["--aud_wav", files["f48"]] + asr, "not a PCM")                   # today's refusals stand without the flag
    opt = cli.parse(["d", "--test", "--aud_wav", files["f48"], "--resample"] + asr)
    assert opt.resample and opt.aud_wav == files["f48"] and capsys.readouterr().out == ""
    refused(["--aud_wav", files["bad"], "--resample"] + asr, "16000 phases")
    refused(["--aud_wav", files["weights"], "--resample"] + asr, "not a RIFF/WAVE")
    refused(["--aud_wav", files["f48"], "--resample"], "--asr_weights")
    with_flag, without = cli.parse(["d", "--aud_wav", files["w16"], "--resample"] + asr), cli.parse(["d", "--aud_wav", files["w16"]] + asr)
    assert {k: v for k, v in vars(with_flag).items() if k != "resample"} == {k: v for k, v in vars(without).items() if k != "resample"}
    assert cli.parse(["d"]).resample is False


def test_live_parse_with_the_new_flags_touches_no_gpu(files, capsys, monkeypatch):
    from radnerf import live
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("a GPU call was made"))
    base = ["d", "--workspace", files["dir"], "-O", "--pose", files["dir"] + "/clip.json", "--asr_weights", files["weights"]]
    def refused(argv, text):
        with pytest.raises(SystemExit) as e:
            live.parse(base + argv)
        assert e.value.code == 2 and text in capsys.readouterr().err
    plain = live.parse(base + ["--pcm", "-"])
    assert (plain.pcm_rate, plain.pcm_format, plain.pcm_channels, plain.pcm_resample, plain.resample) == (16000, "s16le", 1, False, False)
    named = live.parse(base + ["--pcm", "-", "--pcm_rate", "16000", "--pcm_format", "s16le", "--pcm_channels", "1"])
    assert vars(named) == vars(plain)                                          # the defaults are today's path
    opt = live.parse(base + ["--pcm", "-", "--pcm_rate", "48000", "--pcm_format", "f32le", "--pcm_channels", "2"])
    assert (opt.pcm_rate, opt.pcm_format, opt.pcm_channels, opt.pcm_resample) == (48000, "f32le", 2, True)
    assert live.parse(base + ["--pcm", "-", "--pcm_channels", "2"]).pcm_resample
    assert live.parse(base + ["--wav", files["f48"], "--resample"]).resample
    refused(["--wav", files["f48"]], "not a PCM")
    refused(["--wav", files["w16"], "--pcm_rate", "48000"], "--pcm_rate")
    refused(["--wav", files["w16"], "--pcm_channels", "2"], "--pcm_rate")
    refused(["--pcm", "-", "--pcm_format", "s16be"], "invalid choice")
    refused(["--pcm", "-", "--pcm_rate", "44101"], "16000 phases")
    refused(["--pcm", "-", "--pcm_rate", "0"], "positive")
    refused(["--pcm", "-", "--pcm_channels", "0"], "at least one channel")
    refused(["--wav", files["bad"], "--resample"], "16000 phases")


def test_the_video_track_stays_the_file_when_the_avi_writer_reads_it(files, tmp_path):
    from radnerf import cli, video
    lines = []
    log = lambda *a: lines.append(" ".join(str(x) for x in a))
    p24 = tmp_path / "p24.wav"
    p24.write_bytes(riff(1, 2, 48000, 24, bytes(range(48))))
    assert cli.resampled_track(str(p24), lambda: pytest.fail("the signal was asked for"), log) is None and lines == []
    assert video.read_wav(str(p24))[:3] == (48000, 2, 3)                     # integer PCM at any rate: the user's file, as before
    x = torch.tensor([0.0, 0.5, -1.0, 1.0, 1e-5, -2.0, 3.0 / 65536])
    track = cli.resampled_track(files["f48"], x, log)
    assert track[:3] == (16000, 1, 2) and list(np.frombuffer(track[3], "<i2")) == [0, 16384, -32768, 32767, 0, -32768, 2]
    assert len(lines) == 1 and lines[0].startswith("[INFO]") and "PCM16" in lines[0]
    with video.AviWriter(str(tmp_path / "a.avi"), 16, 16, 25, audio=track) as avi:
        assert avi.audio == track


# ---------------------------------------------------------------------------------------------------------- resampled_chunks
@pytest.mark.parametrize("n_frames", [0, 1, 441, 882 * 3, 882 * 11 + 5, 44100 // 4])
def test_resampled_chunks_hand_out_whole_chunks_and_one_short(n_frames):
    import io
    from radnerf import live
    from radnerf import resample as rs
    raw = np.random.default_rng(n_frames).integers(-3000, 3000, 2 * n_frames).astype("<i2").tobytes()       # s16le stereo at 44.1 kHz
    want = rs.Resampler(44100, 16000, "s16le", 2).whole(raw)
    reads = []
    source = live.block_reader(io.BytesIO(raw), 44100, "s16le", 2)
    def counted():
        reads.append(source())
        return reads[-1]
    read_chunk = live.resampled_chunks(counted, rs.Resampler(44100, 16000, "s16le", 2))
    chunks = []
    while True:
        chunks.append(read_chunk())
        if len(chunks[-1]) < 320:
            break
    assert all(len(c) == 320 for c in chunks[:-1]) and torch.equal(torch.cat(chunks), want)
    assert all(len(r) == 882 * 4 for r in reads[:-1]) and len(reads[-1]) < 882 * 4
    assert len(read_chunk()) == 0 and len(reads) == n_frames // 882 + 1         # nothing is read past the end of the source


# ------------------------------------------------------------------------------------------------------------------------- ABI
def test_abi_entries_refuse_on_the_host(hiplib):
    lib, err = hiplib._lib, hiplib.last_error
    assert lib.rn_pcm_decode(None, 10, 1, 1, None, None) == -1 and "null pointer" in err()
    assert lib.rn_pcm_decode(16, 10, 1, 99, 16, None) == -1 and "format 99" in err()
    assert lib.rn_pcm_decode(16, 10, 1, -1, 16, None) == -1 and "format -1" in err()
    assert lib.rn_pcm_decode(16, 10, 0, 1, 16, None) == -1 and "channels" in err()
    assert lib.rn_pcm_decode(None, 0, 2, 2, None, None) == 0
    good = dict(L=1, M=3, W=192)
    def call(x=16, n_buf=100, origin=0, table=16, t0=0, n_out=10, y=16, **change):
        a = dict(good, **change)
        return lib.rn_resample(x, n_buf, origin, table, a["L"], a["M"], a["W"], t0, n_out, y, None)
    for null in ("x", "table", "y"):
        assert call(**{null: None}) == -1 and "null pointer" in err()
    for zero in ("L", "M", "W"):
        assert call(**{zero: 0}) == -1 and "at least 1" in err()
    assert call(origin=-1) == -1 and "negative" in err()
    assert call(t0=-1) == -1 and "negative" in err()
    assert call(M=200) == -1 and "LDS" in err()                       # 255 * 200 + 2 W + 2 floats: past 64 KiB
    assert call(t0=2 ** 62) == -1 and "int64" in err()
    assert call(n_out=0) == 0 and call(x=None, table=None, y=None, n_out=0) == 0
    assert {hiplib.abi.RN_PCM_U8, hiplib.abi.RN_PCM_S16LE, hiplib.abi.RN_PCM_S24LE, hiplib.abi.RN_PCM_S32LE, hiplib.abi.RN_PCM_F32LE} == set(range(5))
