"""radnerf/asr.py without a GPU: the float64 restatement against the golden logits of transformers' own model, the torch path,
the window plan, the loaders, read_wav, the command line's parse rules and the host-side checks of the rn_asr_* entry points."""
import ctypes
import json
import os
import struct
import sys
import wave

import numpy as np
import pytest
import torch

import asrref64 as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FACTOR = 8.0

# the table of the issue: what the reference's loop returns, run with a tiny random Wav2Vec2ForCTC
FULL, SMALL = (22400, 69, 10, 60), (3200, 9, 2, 8)
TABLE = [
    (48137, (10, 50, 10), [FULL, FULL, (19337, 60, 10, 60)], 150, 76),
    (22400, (10, 50, 10), [FULL, (9600, 29, 10, 29)], 69, 35),
    (19200, (10, 50, 10), [FULL, (6400, 19, 10, 19)], 59, 30),
    (8001, (2, 6, 2), [SMALL, SMALL, SMALL, (2881, 8, 2, 7), (961, 2, 2, 2)], 23, 12),
    (5000, (10, 50, 10), [(8200, 25, 10, 25)], 15, 8),
    (4480, (2, 6, 2), [SMALL, SMALL, (1280, 3, 2, 3)], 13, 7),
]


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(HERE, "golden", "asr_tiny.npz"))
    cfg = json.loads(bytes(z["config"]).decode())
    sd = {k[3:]: torch.from_numpy(z[k]).float() for k in z.files if k.startswith("sd/")}
    return dict(cfg=cfg, sd=sd, windows=[torch.from_numpy(z[f"window{i}"]) for i in range(2)],
                logits=[torch.from_numpy(z[f"logits{i}"]) for i in range(2)], yard=float(z["err_f32_cpu"]))


@pytest.fixture(scope="module")
def module(golden):
    from radnerf.asr import Wav2Vec2CTC
    return Wav2Vec2CTC.from_state_dict(golden["sd"], golden["cfg"])


def test_fixture_is_what_the_issue_asks_for(golden):
    assert golden["cfg"] == R.TINY and os.path.getsize(os.path.join(HERE, "golden", "asr_tiny.npz")) < 700 * 1024
    assert [w.numel() for w in golden["windows"]] == [22400, 961] and [tuple(l.shape) for l in golden["logits"]] == [(69, 44), (2, 44)]
    assert all(l.dtype == torch.float64 for l in golden["logits"]) and 1e-7 < golden["yard"] < 1e-5
    assert set(golden["sd"]) == set(R.shapes(R.TINY))


def test_asrref64_reproduces_the_golden_logits(golden):
    for w, want in zip(golden["windows"], golden["logits"]):
        assert R.err(R.forward(golden["sd"], golden["cfg"], w[None])[0], want) < 1e-12


def test_asrref64_against_transformers_on_a_second_config():
    """Three heads, K / G = 16 / 3, vocab 32, the older weight_g / weight_v spelling."""
    pytest.importorskip("transformers")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_asr_golden as G
    cfg = dict(R.TINY, hidden_size=192, num_attention_heads=3, num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=3, vocab_size=32)
    sd = R.random_state_dict(cfg, seed=9, old_names=True)
    w = 0.1 * torch.randn(3200, generator=torch.Generator().manual_seed(1))
    want = G.hf_logits(G.hf_model(cfg, sd, torch.float64), w, torch.float64)
    assert want.shape == (9, 32) and R.err(R.forward(sd, cfg, w[None])[0], want) < 1e-12


def test_torch_path(golden, module):
    for w, want in zip(golden["windows"], golden["logits"]):
        got = module(w[None])
        assert got.dtype == torch.float32 and R.err(got[0], want) <= FACTOR * golden["yard"]
        assert R.err(module(w[None].double())[0], want) < 1e-12
    with pytest.raises(ValueError, match="receptive field"):
        module(torch.zeros(1, 399))
    with pytest.raises(ValueError, match=r"\[B,S\]"):
        module(torch.zeros(400))


@pytest.mark.parametrize("n,lmr,windows,M,F", TABLE)
def test_plan_windows(n, lmr, windows, M, F):
    from radnerf.asr import plan_windows
    got = plan_windows(n, *lmr)
    assert got == windows
    assert sum(max(0, right - left) for _, _, left, right in got) == M and M // 2 + 1 == F


def test_plan_windows_edges():
    from radnerf.asr import frames_of, plan_windows, receptive_field, supported, LARGE
    c = supported(LARGE)
    assert receptive_field(c) == 400 and [frames_of(c, s) for s in (399, 400, 719, 720, 22400)] == [0, 1, 1, 2, 69]
    assert plan_windows(0, 0, 5, 0) == []
    assert plan_windows(100, 1, 5, 1) == [(420, 1, 1, 1)]                   # one logit row, cut away by l: no rows kept
    assert plan_windows(50, 0, 5, 1) == [(50, 0, 0, 0)]                     # below the receptive field: no rows
    with pytest.raises(ValueError):
        plan_windows(100, 1, 0, 1)


@pytest.mark.parametrize("n,lmr,windows,M,F", [TABLE[0], TABLE[3], TABLE[5]])
def test_batched_features_equal_the_sequential_loop(golden, module, n, lmr, windows, M, F):
    x = 0.1 * torch.randn(n, generator=torch.Generator().manual_seed(n), dtype=torch.float64)
    want, seen = R.features(golden["sd"], golden["cfg"], x.numpy(), *lmr)
    assert seen == windows and want.shape == (F, 16, 44)
    for max_batch in (None, 2):
        got = module.features_from_samples(x, *lmr, max_batch=max_batch)
        assert got.shape == want.shape and got.dtype == torch.float64 and R.err(got, want) < 1e-12
    fc16 = module.features_from_samples(x, *lmr, max_batch=2, layout="FC16")       # the same launches as `got`
    assert fc16.shape == (F, 44, 16) and fc16.is_contiguous() and torch.equal(fc16.permute(0, 2, 1), got)
    assert R.err(module.features_from_samples(x.float(), *lmr), want) <= FACTOR * golden["yard"]


# ----------------------------------------------------------------------------------------------------------------- loaders
def test_both_key_spellings_and_the_ignored_key(golden, module, tmp_path):
    from radnerf.asr import Wav2Vec2CTC
    new = module.hf_state_dict()
    assert R.POS + ".parametrizations.weight.original1" in new and R.POS + ".weight_v" not in new
    new["wav2vec2.masked_spec_embed"] = torch.zeros(128)
    w = golden["windows"][1][None]
    assert torch.equal(Wav2Vec2CTC.from_state_dict(new, golden["cfg"])(w), module(w))
    assert set(module.hf_state_dict(old_names=True)) == set(golden["sd"])
    torch.save(new, str(tmp_path / "w2v.pth"))
    (tmp_path / "config.json").write_text(json.dumps(golden["cfg"]))
    assert torch.equal(Wav2Vec2CTC.from_files(str(tmp_path / "w2v.pth"), str(tmp_path / "config.json"))(w), module(w))


def test_loader_refusals(golden):
    from radnerf.asr import Wav2Vec2CTC
    sd, cfg = golden["sd"], golden["cfg"]
    missing = {k: v for k, v in sd.items() if k != "lm_head.bias"}
    with pytest.raises(KeyError, match="lm_head.bias"):
        Wav2Vec2CTC.from_state_dict(missing, cfg)
    with pytest.raises(KeyError, match="wav2vec2.adapter.x"):
        Wav2Vec2CTC.from_state_dict(dict(sd, **{"wav2vec2.adapter.x": torch.zeros(1)}), cfg)
    with pytest.raises(ValueError, match=r"lm_head.weight.*\(32, 128\).*\(44, 128\)"):
        Wav2Vec2CTC.from_state_dict(dict(sd, **{"lm_head.weight": torch.zeros(32, 128)}), cfg)


@pytest.mark.parametrize("field,change", [
    ("feat_extract_norm", dict(feat_extract_norm="group")), ("do_stable_layer_norm", dict(do_stable_layer_norm=False)),
    ("num_conv_pos_embeddings", dict(num_conv_pos_embeddings=7)), ("add_adapter", dict(add_adapter=True)),
    ("num_attention_heads", dict(num_attention_heads=4)), ("conv_bias", dict(conv_bias=False)), ("hidden_act", dict(hidden_act="relu")),
    ("num_conv_pos_embedding_groups", dict(num_conv_pos_embedding_groups=5)), ("conv_dim", dict(conv_dim=[30] * 7))])
def test_unsupported_variants_name_the_field(field, change):
    from radnerf.asr import supported
    with pytest.raises(ValueError, match=field):
        supported(dict(R.TINY, **change))


def test_the_two_real_shapes_are_supported():
    from radnerf.asr import LARGE, supported, tensor_names, tensor_shapes
    for vocab in (44, 32):
        c = supported(dict(LARGE, vocab_size=vocab))
        assert (c["hidden_size"], c["num_attention_heads"], c["intermediate_size"], c["num_hidden_layers"]) == (1024, 16, 4096, 24)
        assert len(tensor_names(c)) == len(tensor_shapes(c)) == 4 * 7 + 11 + 16 * 24
        assert 3.1e8 < sum(int(np.prod(s)) for s in tensor_shapes(c)) < 3.2e8


# ---------------------------------------------------------------------------------------------------------------- read_wav
def _write_wav(path, data, rate=16000, channels=1):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels); w.setsampwidth(2); w.setframerate(rate)
        w.writeframes(np.asarray(data, dtype="<i2").tobytes())


def test_read_wav(tmp_path, capsys):
    from radnerf.asr import read_wav
    mono = np.array([0, 1, -1, 32767, -32768, 16384], dtype=np.int16)
    _write_wav(tmp_path / "mono.wav", mono)
    x = read_wav(str(tmp_path / "mono.wav"))
    assert x.dtype == np.float32 and np.array_equal(x, mono.astype(np.float32) / 32768) and capsys.readouterr().out == ""
    stereo = np.stack([mono, mono[::-1]], axis=1)
    _write_wav(tmp_path / "stereo.wav", stereo, channels=2)
    assert np.array_equal(read_wav(str(tmp_path / "stereo.wav")), x)
    out = capsys.readouterr().out
    assert out.count("[WARN]") == 1 and "2 channels" in out
    _write_wav(tmp_path / "slow.wav", mono, rate=8000)
    with pytest.raises(ValueError, match="8000 Hz.*resample"):
        read_wav(str(tmp_path / "slow.wav"))
    body = np.zeros(4, dtype="<f4").tobytes()                                  # format tag 3: IEEE float, not PCM
    fmt = struct.pack("<HHIIHH", 3, 1, 16000, 64000, 4, 32)
    riff = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(body)) + body
    (tmp_path / "float.wav").write_bytes(b"RIFF" + struct.pack("<I", len(riff)) + riff)
    with pytest.raises(ValueError, match="not a PCM"):
        read_wav(str(tmp_path / "float.wav"))


# --------------------------------------------------------------------------------------------------------------------- CLI
def test_cli_parse_rules_end_before_any_gpu_call(tmp_path, capsys, monkeypatch):
    from radnerf import cli
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("a GPU call was made"))
    wav, weights = tmp_path / "a.wav", tmp_path / "w.pth"
    _write_wav(wav, np.zeros(1600, dtype=np.int16))
    weights.write_bytes(b"")
    def refused(argv, text):
        with pytest.raises(SystemExit) as e:
            cli.main(["d"] + argv)
        assert e.value.code == 2 and text in capsys.readouterr().err
    refused(["--aud_wav", str(wav)], "--asr_weights")
    refused(["--aud_wav", str(wav), "--asr_weights", str(weights), "--aud", "x.npy"], "--aud")
    refused(["--aud_wav", str(tmp_path / "none.wav"), "--asr_weights", str(weights)], "is not a file")
    refused(["--aud_wav", str(wav), "--asr_weights", str(tmp_path / "none.pth")], "is not a file")
    refused(["--aud_wav", str(wav), "--asr_weights", str(weights), "--asr_config", str(tmp_path / "none.json")], "is not a file")
    refused(["--asr_weights", str(weights)], "--aud_wav")
    _write_wav(tmp_path / "slow.wav", np.zeros(800, dtype=np.int16), rate=8000)
    refused(["--aud_wav", str(tmp_path / "slow.wav"), "--asr_weights", str(weights)], "resample")
    opt = cli.parse(["d", "--test", "--aud_wav", str(wav), "--asr_weights", str(weights), "-l", "2", "-m", "6", "-r", "2"])
    assert (opt.aud_wav, opt.asr_weights, opt.asr_config, opt.l, opt.m, opt.r) == (str(wav), str(weights), "", 2, 6, 2)
    plain = cli.parse(["d"])
    assert (plain.aud_wav, plain.asr_weights, plain.asr_config, plain.l, plain.m, plain.r) == ("", "", "", 10, 50, 10)
    for flag in ("--asr", "--asr_wav=x.wav", "--emb", "--gui"):              # still refused, as test_cli_host.py pins
        refused([flag], "not built here")


# --------------------------------------------------------------------------------------------------------------------- ABI
def _config(hiplib, **change):
    from radnerf.asr import Wav2Vec2CTC
    cfg = Wav2Vec2CTC(R.TINY).c_config()
    for k, v in change.items():
        setattr(cfg, k, v)
    return cfg


def test_abi_entries_refuse_on_the_host(hiplib):
    lib, err = hiplib._lib, hiplib.last_error
    good = _config(hiplib)
    assert lib.rn_asr_image_floats(ctypes.byref(good)) >= sum(int(np.prod(s)) for s in R.shapes(R.TINY).values())
    assert lib.rn_asr_workspace(ctypes.byref(good), 3, 22400) > 0
    assert lib.rn_asr_workspace(ctypes.byref(good), 1, 399) == 0 and lib.rn_asr_workspace(ctypes.byref(good), 0, 3200) == 0
    assert lib.rn_asr_workspace(ctypes.byref(good), 1, 400 + 320 * 96) == 0          # 97 steps
    assert lib.rn_asr_image_floats(None) == 0
    for change, text in ((dict(heads=4), "hidden_size / num_attention_heads"), (dict(pos_taps=7), "num_conv_pos_embeddings"),
                         (dict(n_conv=9), "n_conv"), (dict(intermediate=130), "intermediate_size"), (dict(pos_groups=5), "groups")):
        bad = _config(hiplib, **change)
        assert lib.rn_asr_image_floats(ctypes.byref(bad)) == 0 and lib.rn_asr_workspace(ctypes.byref(bad), 1, 3200) == 0
        assert lib.rn_asr_pack(ctypes.byref(bad), None, 0, None, None) == -1 and text in err()
        assert lib.rn_asr_forward(ctypes.byref(bad), None, None, 0, None, 1, 3200, None, None) == -1 and text in err()
    assert lib.rn_asr_pack(ctypes.byref(good), None, 71, None, None) == -1 and "null pointer" in err()
    ptrs = (ctypes.c_void_p * 71)(*([8] * 71))
    assert lib.rn_asr_pack(ctypes.byref(good), ptrs, 70, 16, None) == -1 and "70 tensors, this config has 71" in err()
    ptrs[5] = None
    assert lib.rn_asr_pack(ctypes.byref(good), ptrs, 71, 16, None) == -1 and "tensor 5" in err()
    assert lib.rn_asr_forward(ctypes.byref(good), None, None, 0, None, 1, 3200, None, None) == -1 and "null pointer" in err()
    assert lib.rn_asr_forward(ctypes.byref(good), 16, 16, 0, 16, 1, 399, 16, None) == -1 and "unsupported shape" in err()
    assert lib.rn_asr_forward(ctypes.byref(good), 16, 16, 64, 16, 1, 3200, 16, None) == -1 and "rn_asr_workspace asks for" in err()
    seg = (ctypes.c_uint32 * 5)(0, 2, 9, 2, 8)
    assert lib.rn_asr_features(None, 18, 44, seg, 1, None, 7, None) == -1 and "null pointer" in err()
    assert lib.rn_asr_features(16, 17, 44, seg, 1, 16, 7, None) == -1 and "ends past" in err()
    assert lib.rn_asr_features(16, 18, 44, seg, 1, 16, 8, None) == -1 and "unfold to 7" in err()
    assert lib.rn_asr_features(16, 18, 44, seg, 5, 16, 7, None) == -1 and "n_segments" in err()
    seg[3] = 9; seg[4] = 8
    assert lib.rn_asr_features(16, 18, 44, seg, 1, 16, 7, None) == -1 and "keeps rows" in err()
