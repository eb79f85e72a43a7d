"""Writes tests/golden/asr_tiny.npz from `transformers`' own Wav2Vec2ForCTC in float64 on the CPU, built from a Wav2Vec2Config
(nothing is fetched):

    python tools/make_asr_golden.py [--out tests/golden/asr_tiny.npz]

    config        JSON of the tiny config (tests/asrref64.TINY)
    sd/<key>      the state dict, float16 values (exact in every wider type); the model computes with exactly these
    window0/1     two windows of 22400 and 961 samples, float32
    logits0/1     their float64 logits, model(window.double()[None]) after the processor's normalisation
    err_f32_cpu   max-normalised error of the same model run by torch in fp32 on the CPU against those logits (the larger of
                  the two windows'): the yardstick of the device tests
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import asrref64 as R  # noqa: E402


def hf_model(cfg, sd, dtype):
    from transformers import Wav2Vec2Config, Wav2Vec2ForCTC
    model = Wav2Vec2ForCTC(Wav2Vec2Config(**cfg, feat_extract_activation="gelu", hidden_act="gelu", mask_time_prob=0.0)).eval()
    own = model.state_dict()
    new = R.POS + ".parametrizations.weight.original0" in own
    load = dict(sd)
    if new and R.POS + ".weight_g" in load:
        load[R.POS + ".parametrizations.weight.original0"] = load.pop(R.POS + ".weight_g")
        load[R.POS + ".parametrizations.weight.original1"] = load.pop(R.POS + ".weight_v")
    if "wav2vec2.masked_spec_embed" in own:
        load["wav2vec2.masked_spec_embed"] = own["wav2vec2.masked_spec_embed"]
    model.load_state_dict({k: v.to(torch.float32) for k, v in load.items()}, strict=True)
    return model.to(dtype)


def hf_logits(model, window, dtype):
    x = torch.as_tensor(window).to(dtype)
    x = (x - x.mean()) / torch.sqrt(x.var(unbiased=False) + 1e-7)           # Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm
    with torch.no_grad():
        return model(x[None]).logits[0]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "asr_tiny.npz"))
    opt = p.parse_args()
    cfg = R.TINY
    sd = R.random_state_dict(cfg, seed=20, old_names=True)
    g = torch.Generator().manual_seed(21)
    windows = [(0.1 * torch.randn(n, generator=g) * (1.0 + torch.sin(torch.arange(n) / 700.0))).float() for n in (22400, 961)]
    m64, m32 = hf_model(cfg, sd, torch.float64), hf_model(cfg, sd, torch.float32)
    out = {"config": np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8)}
    for k, v in sd.items():
        out["sd/" + k] = v.half().numpy()
    worst = 0.0
    for i, w in enumerate(windows):
        want = hf_logits(m64, w, torch.float64)
        worst = max(worst, R.err(hf_logits(m32, w, torch.float32), want))
        out[f"window{i}"], out[f"logits{i}"] = w.numpy(), want.numpy()
        print(f"window {i}: {w.numel()} samples -> logits {tuple(want.shape)}, asrref64 differs by {R.err(R.forward(sd, cfg, w[None])[0], want):.3e}")
    out["err_f32_cpu"] = np.float64(worst)
    print(f"err_f32_cpu = {worst:.3e}")
    np.savez_compressed(opt.out, **out)
    print(f"wrote {opt.out}: {os.path.getsize(opt.out)} bytes")


if __name__ == "__main__":
    main()
