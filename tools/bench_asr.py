"""What audio features from a .wav cost on one GPU (radnerf/asr.py: Wav2Vec2CTC at the real shape, 24 layers, random weights).

    python tools/bench_asr.py [--seconds 60] [--repeats 5] [--out profiles/asr_bench.json] [--kernel-stats FILE.csv]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_asr.py --profile-pass

forms, alternating in ONE process (every form sees the same machine), `--repeats` windows of one features_from_samples call each,
host clock around a call ending in a synchronise, median [min, max]:
    hip_batched     the kernels (RN_ASR=hip), all windows of one length through the model together
    hip_one_window  the kernels, one window per call (max_batch = 1): the reference's data flow
    torch_batched   RN_ASR=torch, batched
--profile-pass: one warm-up and one hip_batched call, nothing else (the run to put under rocprofv3).
--kernel-stats: the *_kernel_stats.csv of such a run; its rows are copied into the record and the GEMM's rate is worked out from
    the floating-point operations of one call's matrix products (counted here from the shapes) against 157 TF.

Prints one JSON object (and writes it to --out).  Needs a GPU.  A record: nothing on the parent commit to compare with.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rad-nerf_amd"))

import torch  # noqa: E402

FORMS = ("hip_batched", "hip_one_window", "torch_batched")
PEAK_TF = 157.0


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), runs=xs)


def random_module(layers):
    from radnerf.asr import LARGE, Wav2Vec2CTC
    m = Wav2Vec2CTC(dict(LARGE, num_hidden_layers=layers)).cuda()
    g = torch.Generator(device="cuda").manual_seed(0)
    with torch.no_grad():
        for name, t in zip(m.names, m._tensors()):
            if name.endswith("layer_norm.weight") or name.endswith("weight_g"):
                t.copy_(1.0 + 0.1 * torch.randn(t.shape, generator=g, device="cuda"))
            elif name.endswith(".bias"):
                t.copy_(0.1 * torch.randn(t.shape, generator=g, device="cuda"))
            else:
                t.copy_(torch.randn(t.shape, generator=g, device="cuda") * (1.5 / (t[0].numel() ** 0.5)))
    return m


def gemm_flops(c, windows):
    """2 M N K over the matrix products of one features call (conv layers 1.., projection, positional conv, layers, head)."""
    from radnerf.asr import frames_of
    total = 0
    for samples, T, _, _ in windows:
        if T < 1:
            continue
        t, cin = samples, 1
        for i, (d, k, s) in enumerate(zip(c["conv_dim"], c["conv_kernel"], c["conv_stride"])):
            t = (t - k) // s + 1
            if i:
                total += 2 * t * d * k * cin
            cin = d
        H, I, K, G = c["hidden_size"], c["intermediate_size"], c["num_conv_pos_embeddings"], c["num_conv_pos_embedding_groups"]
        assert t == T == frames_of(c, samples)
        total += 2 * T * H * cin + 2 * T * H * K * (H // G)
        total += c["num_hidden_layers"] * (2 * T * 3 * H * H + 2 * T * H * H + 4 * T * H * I)
        total += 2 * T * c["vocab_size"] * H
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--profile-pass", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_asr: needs a GPU (a CPU timing says nothing about the kernels)")
    from radnerf.asr import plan_windows
    m = random_module(args.layers)
    n = int(args.seconds * 16000)
    g = torch.Generator().manual_seed(1)
    x = (0.1 * torch.randn(n, generator=g) * (1.0 + torch.sin(torch.arange(n) / 4000.0))).cuda()
    windows = plan_windows(n, 10, 50, 10, m.config)

    def call(form):
        os.environ["RN_ASR"] = "torch" if form.startswith("torch") else "hip"
        out = m.features_from_samples(x, 10, 50, 10, max_batch=1 if form == "hip_one_window" else None)
        torch.cuda.synchronize()
        return out

    if args.profile_pass:
        call("hip_batched")
        call("hip_batched")
        return
    outs = {f: call(f) for f in FORMS}                                     # warm-up: the weight image, the workspaces, the BLAS plans
    ms = {f: [] for f in FORMS}
    for _ in range(args.repeats):
        for f in FORMS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call(f)
            ms[f].append((time.perf_counter() - t0) * 1e3)
    flops = gemm_flops(m.config, windows)
    rec = {"tool": "bench_asr", "device": torch.cuda.get_device_name(0), "seconds_of_audio": args.seconds, "layers": args.layers,
           "windows": len(windows), "features": list(outs["hip_batched"].shape), "matrix_product_flop_per_call": flops,
           "ms_per_call": {f: spread(ms[f]) for f in FORMS},
           "matrix_product_tf_whole_call": {f: flops / (statistics.median(ms[f]) * 1e-3) / 1e12 for f in FORMS},
           "one_window_equals_batched_bits": bool(torch.equal(outs["hip_batched"], outs["hip_one_window"])),
           "torch_difference_of_max": float((outs["hip_batched"] - outs["torch_batched"]).abs().max() / outs["torch_batched"].abs().max())}
    if args.kernel_stats:
        with open(args.kernel_stats) as fh:
            rows = [dict(name=r["Name"], calls=int(r["Calls"]), total_ms=int(r["TotalDurationNs"]) / 1e6, percent=float(r["Percentage"]))
                    for r in csv.DictReader(fh)]
        rec["kernel_stats_two_calls"] = rows
        gemm = [r for r in rows if "asr::k_gemm" in r["name"]]
        if gemm:
            rec["gemm_tf"] = 2 * flops / (sum(r["total_ms"] for r in gemm) * 1e-3) / 1e12
            rec["gemm_fraction_of_157_tf"] = rec["gemm_tf"] / PEAK_TF
    os.environ.pop("RN_ASR", None)
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
