"""radnerf/live.py without a GPU: LiveASR on a CPU module (the ring by indexing, the model by forward_torch) against a restatement of
the reference's run_step / get_next_feat loop, tail="flush" against the features of the whole file, and the argument checks.

The bits: both sides call the model once per window on the same [1, S] samples and everything else is copies, so tail="reference"
is held to the last bit.  tail="flush" is compared with features_from_samples, whose torch path batches the windows of one length
and so sums in another order: those cases get 2 x 8 x the fixture's err_f32_cpu (each side within 8 x of float64, the bound of
test_gpu_asr_cli.py), and torch.equal wherever every window of the file stands alone in its batch.
"""
import json
import os
import wave

import numpy as np
import pytest
import torch

import asrref64 as R
from test_cli_host import test_refused_flags_say_they_are_not_built  # noqa: F401  (cli.parse still refuses --asr*)

HERE = os.path.dirname(os.path.abspath(__file__))
CHUNK = 320


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(HERE, "golden", "asr_tiny.npz"))
    cfg = json.loads(bytes(z["config"]).decode())
    sd = {k[3:]: torch.from_numpy(z[k]).float() for k in z.files if k.startswith("sd/")}
    return dict(cfg=cfg, sd=sd, yard=float(z["err_f32_cpu"]))


@pytest.fixture(scope="module")
def module(golden):
    from radnerf.asr import Wav2Vec2CTC
    return Wav2Vec2CTC.from_state_dict(golden["sd"], golden["cfg"])


def _samples(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.1 * torch.randn(n, generator=g) * (1.0 + torch.sin(torch.arange(n) / 300.0))).float().numpy()


def _reference_loop(model, x, l, m, r, ring_windows=4):
    """nerf/asr.py in file mode as nerf/gui.py drives it, restated: warm_up_steps run_steps, then per frame two run_steps and one
    get_next_feat until the step that finds the stream empty.  -> the [8, C, 16] window of every frame."""
    C, size, rows = model.vocab_size, l + m + r, ring_windows * m
    st = dict(frames=[np.zeros(CHUNK, np.float32)] * l, idx=0, terminated=False, slot=0, front=rows - 8, tail=8,
              att=[np.zeros((C, 16), np.float32)] * 4)
    ring = np.zeros((rows, C), np.float32)

    def run_step():
        if st["terminated"]:
            return
        if st["idx"] < len(x):
            st["frames"].append(x[st["idx"]:st["idx"] + CHUNK])
            st["idx"] += CHUNK
            if len(st["frames"]) < size:
                return
        else:
            st["terminated"] = True
        inputs = np.concatenate(st["frames"])
        if not st["terminated"]:
            st["frames"] = st["frames"][-(l + r):]
        with torch.no_grad():
            logits = model.forward_torch(torch.from_numpy(inputs)[None])[0].numpy()
        right = logits.shape[0] if st["terminated"] else min(logits.shape[0], logits.shape[0] - r + 1)
        feats = logits[max(0, l):right]
        if not st["terminated"]:
            ring[st["slot"] * m:st["slot"] * m + feats.shape[0]] = feats            # in place: the views kept in `att` see it
            st["slot"] = (st["slot"] + 1) % ring_windows

    def next_feat():
        while len(st["att"]) < 8:
            f, t = st["front"], st["tail"]
            feat = ring[f:t] if f < t else np.concatenate([ring[f:], ring[:t]])     # a view of the ring, or (wrapping) a copy
            st["front"], st["tail"] = (f + 2) % rows, (t + 2) % rows
            st["att"].append(feat.T)                                               # permute keeps a view a view
            assert (feat.base is ring) == (f < t)
        out = np.stack(st["att"])                                                  # the views are read here, every frame
        st["att"] = st["att"][1:]
        return out

    for _ in range(m + r + 8 + 2 * 3):
        run_step()
    outs = []
    while not st["terminated"]:
        run_step()
        run_step()
        outs.append(next_feat())
    return outs


def _live_windows(module, x, l, m, r, ring_windows, tail):
    from radnerf import live
    asr = live.LiveASR(module, l, m, r, ring_windows=ring_windows, tail=tail)
    assert asr.n_frames is None and asr.frames_ready() == 0
    outs = [asr.next_window(k).clone() for k in live.schedule(asr, live.chunks_of(x))]
    return asr, outs


@pytest.mark.parametrize("n,lmr", [(260 * CHUNK + 123, (10, 50, 10)), (60 * CHUNK, (2, 6, 2))])
def test_reference_tail_equals_the_reference_loop_to_the_last_bit(module, n, lmr):
    """260 chunks + 123 samples at 10/50/10: five full windows, the write slot wraps; 60 chunks at 2/6/2: a ring of 24 rows that
    the writer laps (the reference's overwrite regime: a carried slice is a view and shows the rows written since, the wrapping slice
    is a copy and does not), the terminal window never written."""
    x = _samples(n, n % 1000)
    want = _reference_loop(module, x, *lmr)
    asr, got = _live_windows(module, x, *lmr, 4, "reference")
    assert len(got) == len(want) == asr.n_frames and len(got) >= 20
    assert asr.warm_up_chunks == lmr[1] + lmr[2] + 14
    for k, (a, b) in enumerate(zip(got, want)):
        assert tuple(a.shape) == (8, module.vocab_size, 16) and np.array_equal(a.numpy(), b), k
    assert np.count_nonzero(want[0][:4]) == 0 and np.count_nonzero(want[-1]) > 0


def _file_window(feats, k):
    """get_audio_features(feats, 2, k).  That function cuts its zero padding out of the rows it kept (zeros_like(auds[:pad])), so
    for a file of fewer than 4 frames, which has fewer rows than the padding, it hands back a short stack; there the same window is
    written out here: slices k - 4 .. k + 3, zeros outside the file."""
    from radnerf.rays import get_audio_features
    if feats.shape[0] >= 4:
        return get_audio_features(feats, 2, k)
    return torch.stack([feats[s] if 0 <= s < feats.shape[0] else torch.zeros_like(feats[0]) for s in range(k - 4, k + 4)])


FLUSH = [(1 * CHUNK, (10, 50, 10), 4), (2 * CHUNK, (10, 50, 10), 4), (59 * CHUNK, (10, 50, 10), 4), (60 * CHUNK, (10, 50, 10), 4),
         (61 * CHUNK, (10, 50, 10), 4), (150 * CHUNK, (10, 50, 10), 4), (399 * CHUNK, (10, 50, 10), 4), (83323, (10, 50, 10), 4),
         (91 * CHUNK, (3, 12, 3), 8)]


@pytest.mark.parametrize("n,lmr,ring_windows", FLUSH)
def test_flush_tail_equals_the_features_of_the_whole_file(module, golden, n, lmr, ring_windows):
    from radnerf.asr import _windows
    x = _samples(n, 7 + n % 1000)
    feats = module.features_from_samples(x, *lmr, layout="FC16")
    asr, got = _live_windows(module, x, *lmr, ring_windows, "flush")
    M = sum(min(T, right) - min(left, right) for _, _, T, left, right in _windows(n, *lmr, module.config) if T >= 1)
    assert asr.n_frames == len(got) == feats.shape[0] == M // 2 + 1 and asr.rows_written == M
    want = torch.stack([_file_window(feats, k) for k in range(len(got))])
    got = torch.stack(got)
    lengths = [w[1] for w in _windows(n, *lmr, module.config)]
    if len(set(lengths)) == len(lengths):                # every window alone in its batch: the same single-window calls
        assert torch.equal(got, want)
    else:
        e = R.err(got, want)
        print(f"{n} samples at {lmr}: live against the batched file pass {e:.3e}, bound {2 * 8.0 * golden['yard']:.3e}")
        assert e <= 2 * 8.0 * golden["yard"]


def test_push_takes_any_number_of_samples(module):
    """The chunking is LiveASR's: one push of everything, and pushes of 1, 7, 500, ... samples, give the windows of the loop."""
    from radnerf import live
    x = _samples(330 * CHUNK + 77, 5)
    whole = live.LiveASR(module, 10, 50, 10)
    whole.push(x)
    whole.finish()
    parts = live.LiveASR(module, 10, 50, 10)
    at, step = 0, 1
    while at < len(x):
        parts.push(x[at:at + step])
        at += step
        step = step * 7 % 2003 + 1
    assert parts.frames_ready() > 0 and parts.n_frames is None
    parts.finish()
    assert whole.n_frames == parts.n_frames == whole.frames_ready() and whole.windows_run == parts.windows_run == 7
    _, loop = _live_windows(module, x, 10, 50, 10, 4, "flush")
    for k in range(whole.n_frames - 60, whole.n_frames):         # the frames whose rows the ring still holds
        a, b = whole.next_window(k).clone(), parts.next_window(k).clone()
        assert torch.equal(a, b) and torch.equal(a, loop[k])
    with pytest.raises(RuntimeError, match="overwritten"):
        whole.next_window(0)


def test_argument_checks(module):
    from radnerf import live
    with pytest.raises(ValueError, match=r"2 m \+ r \+ 48"):
        live.LiveASR(module, 2, 11, 2, ring_windows=4)
    live.LiveASR(module, 2, 11, 2, ring_windows=4, tail="reference")
    live.LiveASR(module, 3, 12, 3, ring_windows=8)
    with pytest.raises(ValueError, match="at most 96"):
        live.LiveASR(module, 10, 78, 10)
    live.LiveASR(module, 10, 77, 10, ring_windows=5)
    with pytest.raises(ValueError, match="tail"):
        live.LiveASR(module, tail="zeros")
    asr = live.LiveASR(module)
    asr.push(np.zeros(1000, np.float32))
    with pytest.raises(RuntimeError, match="not ready"):
        asr.next_window(0)
    asr.finish()
    with pytest.raises(RuntimeError, match="finished"):
        asr.push(np.zeros(10, np.float32))
    for att in (0, 1):
        with pytest.raises(ValueError, match=f"--att {att}"):
            live.LiveScene(None, None, type("O", (), dict(att=att))(), "cpu", asr)


@pytest.fixture
def files(tmp_path):
    wav = tmp_path / "a.wav"
    with wave.open(str(wav), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(np.zeros(640, "<i2").tobytes())
    weights = tmp_path / "w.pth"
    weights.write_bytes(b"")
    return ["d", "--workspace", str(tmp_path), "-O", "--pose", str(tmp_path / "clip.json"), "--asr_weights", str(weights)], str(wav)


def test_parse_touches_no_gpu_and_names_what_it_refuses(files, capsys, monkeypatch):
    from radnerf import live
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("a GPU call was made"))
    base, wav = files
    opt = live.parse(base + ["--wav", wav, "--video", "--realtime"])
    assert opt.test and opt.smooth_lips and opt.exp_eye and opt.att == 2 and (opt.l, opt.m, opt.r) == (10, 50, 10)
    assert opt.wav == wav and opt.pcm == "" and opt.fps == 50 and opt.tail == "flush" and opt.ring_windows == 4 and opt.video and opt.realtime
    assert live.parse(base + ["--pcm", "-", "--raw_out", "-"]).raw_out == "-"

    def refused(argv, text):
        with pytest.raises(SystemExit) as e:
            live.parse(argv)
        assert e.value.code == 2
        assert text in capsys.readouterr().err
    refused(base + ["--wav", wav, "--pcm", "-"], "give one")
    refused(base, "--wav FILE or --pcm -")
    refused(base + ["--wav", wav, "--fps", "25"], "--fps 25")
    refused(base + ["--wav", wav, "--att", "0"], "--att 0")
    refused(base + ["--wav", wav, "--att", "1"], "--att 1")
    refused(base + ["--wav", wav, "-m", "78"], "at most 96")
    refused(base + ["--wav", wav, "-l", "2", "-m", "11", "-r", "2"], "2 m + r + 48")
    refused(base + ["--wav", wav, "--asr"], "not built here")
    refused(base[:-2] + ["--wav", wav], "--asr_weights FILE")
    refused(base + ["--wav", str(wav) + ".missing"], "is not a file")
    assert live.parse(base + ["--wav", wav, "-l", "2", "-m", "11", "-r", "2", "--tail", "reference"]).tail == "reference"
