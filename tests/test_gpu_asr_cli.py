"""--aud_wav end to end on tests/dataset_dir.py's directory with the tiny wav2vec2 model of tests/golden/asr_tiny.npz saved to a file:
`python -m radnerf.asr` writes the feature file, a --test render driven by that file equals the --test render driven by the wav
itself in every byte of the frames, and with --video the AVI carries the wav.  The runs that are compared byte for byte go through
the kernels (RN_ASR=hip: their bits do not depend on the batching or the call); the switch's default path is held to the bound."""
import json
import os
import sys
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dataset_dir as dd  # noqa: E402
import jpegref64 as J  # noqa: E402

SAMPLES = 19200                 # 1.2 s: windows (22400, 69, 10, 60) (6400, 19, 10, 19) -> 59 rows -> 30 audio frames


@pytest.fixture(scope="module")
def runs(tmp_path_factory, hiplib):
    from radnerf import asr, cli
    root = str(tmp_path_factory.mktemp("dataset"))
    ws = str(tmp_path_factory.mktemp("workspace"))
    dd.write_dataset(root, 0)
    z = np.load(os.path.join(HERE, "golden", "asr_tiny.npz"))
    weights, config = os.path.join(root, "w2v.pth"), os.path.join(root, "w2v.json")
    torch.save({k[3:]: torch.from_numpy(z[k]).float() for k in z.files if k.startswith("sd/")}, weights)
    with open(config, "w") as fh:
        fh.write(bytes(z["config"]).decode())
    wav = os.path.join(root, "intro.wav")
    t = np.arange(SAMPLES)
    pcm = np.round(6000 * np.sin(t / 9.0) * (1 + np.sin(t / 800.0)) + 500 * ((t * 37) % 11 - 5)).astype("<i2").tobytes()
    with wave.open(wav, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(pcm)
    quiet = lambda *a: None
    feats_file = os.path.join(root, "intro_eo.npy")
    default_feats = asr.main(["--wav", wav, "--weights", weights, "--config", config, "--out", os.path.join(root, "default.npy")], log=quiet)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("RN_ASR", "hip")
        return _runs(root, ws, wav, weights, config, feats_file, default_feats, pcm, quiet)


def _runs(root, ws, wav, weights, config, feats_file, default_feats, pcm, quiet):
    from radnerf import asr, cli
    feats = asr.main(["--wav", wav, "--weights", weights, "--config", config, "--out", feats_file], log=quiet)
    base = [root, "--workspace", ws, "--num_rays", "256", "-O"]
    cli.main(base + ["--iters", "24", "--ckpt", "scratch"], log=quiet, decode=dd.npy_decode)
    clip = ["--test", "--pose", os.path.join(root, "clip.json")]
    by_file = cli.main(base + clip + ["--aud", feats_file], log=quiet, decode=dd.npy_decode)
    frames_by_file = np.load(by_file["video"])                      # the next run writes the same file names
    lines = []
    by_wav = cli.main(base + clip + ["--aud_wav", wav, "--asr_weights", weights, "--asr_config", config, "--video"],
                      log=lambda *a: lines.append(" ".join(str(x) for x in a)), decode=dd.npy_decode)
    return dict(root=root, frames_by_file=frames_by_file, default_feats=default_feats, feats=feats, feats_file=feats_file, by_file=by_file, by_wav=by_wav, pcm=pcm, lines=lines, wav=wav,
                weights=weights, config=config, base=base, clip=clip)


def test_the_module_writes_the_feature_file(runs):
    saved = np.load(runs["feats_file"])
    assert saved.dtype == np.float32 and saved.shape == (30, 16, 44) and np.array_equal(saved, runs["feats"])
    assert np.isfinite(saved).all() and np.count_nonzero(saved[0, :8]) == 0 and np.count_nonzero(saved[0, 8:]) > 0


def test_the_default_path_agrees_within_the_bound(runs):
    import asrref64 as R
    z = np.load(os.path.join(HERE, "golden", "asr_tiny.npz"))
    assert runs["default_feats"].shape == runs["feats"].shape
    assert R.err(runs["default_feats"], runs["feats"]) <= 2 * 8.0 * float(z["err_f32_cpu"])      # each within 8 x of float64


def test_a_render_from_the_wav_equals_a_render_from_its_feature_file(runs):
    a, b = runs["frames_by_file"], np.load(runs["by_wav"]["video"])
    assert a.dtype == np.uint8 and a.shape == (30, dd.H, dd.W, 3) and np.array_equal(a, b)
    assert runs["by_wav"]["evals"] == [] and runs["by_file"]["avi"] is None
    assert any("30 audio frames of width 44" in ln for ln in runs["lines"])


def test_the_video_carries_the_wav(runs):
    done = runs["by_wav"]
    assert done["avi"] and os.path.isfile(done["avi"])
    avi = J.read_avi(open(done["avi"], "rb").read())
    assert avi["avih"]["total_frames"] == 30 and len(avi["streams"]) == 2
    assert b"".join(c[2] for c in avi["movi"] if c[0] == b"01wb") == runs["pcm"]


def test_a_logit_width_the_audio_net_does_not_take_is_named(runs, tmp_path):
    from radnerf import cli
    z = json.load(open(runs["config"]))
    z["vocab_size"] = 32
    sd = torch.load(runs["weights"], weights_only=True)
    sd["lm_head.weight"], sd["lm_head.bias"] = sd["lm_head.weight"][:32].clone(), sd["lm_head.bias"][:32].clone()
    torch.save(sd, str(tmp_path / "w32.pth"))
    (tmp_path / "w32.json").write_text(json.dumps(z))
    with pytest.raises(ValueError, match=r"width 32.*takes 44"):
        cli.main(runs["base"] + runs["clip"] + ["--aud_wav", runs["wav"], "--asr_weights", str(tmp_path / "w32.pth"), "--asr_config",
                                                  str(tmp_path / "w32.json")], log=lambda *a: None, decode=dd.npy_decode)
