"""What live mode costs on one GPU (radnerf/live.py; Wav2Vec2CTC at the real shape, 24 layers, random weights).

    python tools/bench_live.py [--repeats 5] [--seconds 12] [--size 512] [--out profiles/live_bench.json]
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_live.py --profile-pass --tile 32     (and --tile 128)
    python tools/bench_live.py --traces TRACE_32.csv TRACE_128.csv --out profiles/live_gemm_by_shape.json

(a) one window of 22400 samples, the forms alternating in ONE process, `--repeats` windows, median [min, max]:
        tile128 | tile32 | auto   the kernels (RN_ASR=hip) under RN_ASR_TILE, called as LiveASR calls them (one workspace, one output)
        torch                     RN_ASR=torch
    per call: host_ms (the call returns: every launch is enqueued), wall_ms (host clock to the synchronise behind it) and device_ms
    (HIP events on the stream around the call); launches per pass are counted from the model's structure.
(b) the live loop on the synthetic benchmark scene, fused engine: warm-up pushes, then per frame two pushes, the window, the frame,
    and a synchronise (a frame's latency is the point); frames per second over the loop, per-frame p50 / p99 / max, the frames that
    carried a window pass listed apart; forms live_auto | live_128 | file (ClipScene over the whole file's features, the loop of
    cli.render_clip; its feature pass is timed apart) in one rotation, `--rotations` times.
--profile-pass: one warm-up and `--repeats` one-window passes under --tile, nothing else (the run to put under rocprofv3).
--traces: the *_kernel_trace.csv of two such runs (tile 32, tile 128): the matrix products of a pass by launch order, so that
    product p of one trace is product p of the other; per shape (M, N, K, groups) the median duration under each tiling and what
    pick_tile (restated here) chooses for it on 256 compute units.

Prints one JSON object (and writes it to --out).  Needs a GPU except for --traces.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rad-nerf_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

WINDOW = 22400


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), runs=[round(x, 4) for x in xs])


def products(c, samples, B=1):
    """(M, N, K, groups) of every matrix product of one forward pass, in launch order."""
    out, t, cin = [], samples, 1
    for i, (d, k, s) in enumerate(zip(c["conv_dim"], c["conv_kernel"], c["conv_stride"])):
        t = (t - k) // s + 1
        if i:
            out.append((B * t, d, k * cin, 1))
        cin = d
    H, I, K, G = c["hidden_size"], c["intermediate_size"], c["num_conv_pos_embeddings"], c["num_conv_pos_embedding_groups"]
    M = B * t
    out += [(M, H, cin, 1), (M, H // G, K * (H // G), G)]
    for _ in range(c["num_hidden_layers"]):
        out += [(M, 3 * H, H, 1), (M, H, H, 1), (M, I, H, 1), (M, H, I, 1)]
    return out + [(M, c["vocab_size"], H, 1)]


def launches(c):
    """Kernel launches of one forward pass: normalize, conv0, (GEMM + LN) per further conv layer, LN + projection, pad + positional
    conv, 7 per encoder layer, LN + head."""
    return 2 + 2 * (len(c["conv_dim"]) - 1) + 2 + 2 + 7 * c["num_hidden_layers"] + 2


def pick_tile(M, N, K, groups, cus):
    """csrc/rn_asr_dev.h: pick_tile, restated."""
    wg128 = -(-M // 128) * -(-N // 128) * groups
    waves32 = -(-M // 32) * -(-N // 32) * groups
    return 32 if wg128 < cus and waves32 <= 4 * cus else 128


def read_trace(path):
    """The rn::asr GEMM launches of a kernel trace, in start order: [(kernel, microseconds)]."""
    rows = []
    with open(path) as fh:
        for r in csv.DictReader(fh):
            name = r.get("Kernel_Name", "")
            if "asr" in name and "k_gemm" in name:
                rows.append((int(r["Start_Timestamp"]), "k_gemm32" if "k_gemm32" in name else "k_gemm",
                             (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    rows.sort()
    return [(k, us) for _, k, us in rows]


def by_shape(trace32, trace128, layers, cus=256):
    from radnerf.asr import LARGE
    prods = products(dict(LARGE, num_hidden_layers=layers), WINDOW)
    t32, t128 = read_trace(trace32), read_trace(trace128)
    n = len(prods)
    assert len(t32) % n == 0 and len(t128) % n == 0 and t32 and t128, (len(t32), len(t128), n)
    assert all(k == "k_gemm32" for k, _ in t32) and all(k == "k_gemm" for k, _ in t128)
    shapes = {}
    for trace, key in ((t32, "us_32"), (t128, "us_128")):
        for i, (_, us) in enumerate(trace[n:]):                   # the first pass is the warm-up
            shapes.setdefault(prods[i % n], {"us_32": [], "us_128": []})[key].append(us)
    rows = []
    for (M, N, K, G), d in shapes.items():
        a, b = statistics.median(d["us_32"]), statistics.median(d["us_128"])
        rows.append(dict(M=M, N=N, K=K, groups=G, products_per_pass=sum(1 for p in prods if p == (M, N, K, G)), launches=len(d["us_32"]),
                         median_us_32=round(a, 1), min_us_32=round(min(d["us_32"]), 1), max_us_32=round(max(d["us_32"]), 1),
                         median_us_128=round(b, 1), min_us_128=round(min(d["us_128"]), 1), max_us_128=round(max(d["us_128"]), 1),
                         auto_picks=pick_tile(M, N, K, G, cus),
                         auto_never_slower=bool(max(d["us_32"]) <= min(d["us_128"])) if pick_tile(M, N, K, G, cus) == 32 else True))
    per_pass = {k: sum(r["median_us_" + k] * r["products_per_pass"] for r in rows) for k in ("32", "128")}
    per_pass["auto"] = sum(r["median_us_%d" % r["auto_picks"]] * r["products_per_pass"] for r in rows)
    return dict(note="rn::asr::k_gemm32 / k_gemm per product of one 22400-sample window pass (rocprofv3 --kernel-trace, one run per tiling, "
                     "the warm-up pass dropped); auto_never_slower: the slowest 32-row launch against the fastest 128-row one",
                compute_units=cus, layers=layers, gemm_us_per_pass=per_pass, shapes=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rotations", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=12.0)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--profile-pass", action="store_true")
    ap.add_argument("--tile", default="auto", choices=("auto", "32", "128"))
    ap.add_argument("--traces", nargs=2, default=None, metavar=("TRACE_32", "TRACE_128"))
    ap.add_argument("--skip-loop", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    def emit(rec):
        text = json.dumps(rec, indent=1)
        print(text)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(text + "\n")

    if args.traces:
        return emit(by_shape(args.traces[0], args.traces[1], args.layers))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_live: needs a GPU (a CPU timing says nothing about the kernels)")
    from bench_asr import random_module
    from radnerf import live
    m = random_module(args.layers)
    C = m.vocab_size
    g = torch.Generator().manual_seed(1)
    n = int(args.seconds * 16000)
    x = (0.1 * torch.randn(n, generator=g) * (1.0 + torch.sin(torch.arange(n) / 4000.0)))
    w = x[:WINDOW].cuda()[None].contiguous()
    T = (WINDOW - 400) // 320 + 1
    ws = torch.empty(m.workspace_bytes(1, WINDOW), dtype=torch.uint8, device="cuda")
    out = torch.empty(1, T, C, device="cuda")

    def one_window(form):
        os.environ["RN_ASR"] = "torch" if form == "torch" else "hip"
        os.environ["RN_ASR_TILE"] = form[4:] if form.startswith("tile") else "auto"
        with torch.no_grad():
            return m.forward_torch(w) if form == "torch" else m.forward_hip(w, out=out, workspace=ws)

    if args.profile_pass:
        for _ in range(1 + args.repeats):
            one_window("tile" + args.tile if args.tile != "auto" else "auto")
            torch.cuda.synchronize()
        return

    forms = ("tile128", "tile32", "auto", "torch")
    outs = {}
    for f in forms:                                                      # warm-up: the weight image, the BLAS plans
        outs[f] = one_window(f).clone()
        torch.cuda.synchronize()
    ms = {f: dict(host_ms=[], wall_ms=[], device_ms=[]) for f in forms}
    for _ in range(args.repeats):
        for f in forms:
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            one_window(f)
            b.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            ms[f]["host_ms"].append((t1 - t0) * 1e3)
            ms[f]["wall_ms"].append((t2 - t0) * 1e3)
            ms[f]["device_ms"].append(a.elapsed_time(b))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    prods = products(m.config, WINDOW)
    rec = {"tool": "bench_live", "device": torch.cuda.get_device_name(0), "compute_units": cus, "layers": args.layers,
           "one_window": {"samples": WINDOW, "rows": T, "launches_per_pass": launches(m.config), "matrix_products_per_pass": len(prods),
                          "products_auto_runs_on_32_row_tiles": sum(1 for p in prods if pick_tile(*p, cus) == 32),
                          "ms": {f: {k: spread(v) for k, v in ms[f].items()} for f in forms},
                          "tile32_equals_tile128_bits": bool(torch.equal(outs["tile32"], outs["tile128"])),
                          "auto_equals_tile128_bits": bool(torch.equal(outs["auto"], outs["tile128"])),
                          "torch_difference_of_max": float((outs["tile128"] - outs["torch"]).abs().max() / outs["torch"].abs().max())}}

    if not args.skip_loop:
        import numpy as np
        from radnerf.clip import ClipScene
        from radnerf.parallel import FrameParallelRenderer
        from radnerf.scene import SyntheticScene, default_opt
        size = args.size
        syn = SyntheticScene(H=size, W=size, n_frames=250, device="cuda", opt=default_opt(engine="fused"))
        base = dict(H=size, W=size, poses=syn.poses.cpu().numpy(), intrinsics=syn.intrinsics, eye_area=np.full((250, 1), 0.25, np.float32),
                    bg=np.full((size, size, 3), 255, np.uint8))
        xs = x.numpy()

        def stats(frame_ms, carried, total_s, extra=None):
            s = sorted(frame_ms)
            plain = [t for t, c in zip(frame_ms, carried) if not c]
            d = dict(frames=len(s), fps=len(s) / total_s, p50_ms=s[len(s) // 2], p99_ms=s[min(len(s) - 1, int(0.99 * len(s)))], max_ms=s[-1],
                     frames_without_a_window_p50_ms=statistics.median(plain) if plain else None,
                     window_frames_ms=[round(t, 3) for t, c in zip(frame_ms, carried) if c])
            d.update(extra or {})
            return d

        def run_live(tile):
            os.environ["RN_ASR"], os.environ["RN_ASR_TILE"] = "hip", tile
            asr = live.LiveASR(m)
            scene = live.LiveScene(syn.model, SimpleNamespace(auds=np.zeros((1, C, 16), np.float32), **base), syn.opt, "cuda", asr)
            renderer = FrameParallelRenderer(scene, rank=0, world=1, dist=None)
            syn.model.enc_a = None
            frame_ms, carried = [], []
            torch.cuda.synchronize()
            t_begin = t0 = time.perf_counter()
            seen = 0
            with torch.no_grad():
                for k in live.schedule(asr, live.chunks_of(xs)):
                    if k == 0:                                   # the warm-up pushes (and their window) are latency, not frame time
                        torch.cuda.synchronize()
                        t_begin = t0 = time.perf_counter()
                        seen = asr.windows_run
                    renderer.step(k)
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    frame_ms.append((t1 - t0) * 1e3)
                    carried.append(asr.windows_run > seen)
                    seen, t0 = asr.windows_run, t1
            renderer.finish()
            return stats(frame_ms, carried, time.perf_counter() - t_begin, dict(windows=asr.windows_run))

        def run_file():
            os.environ["RN_ASR"], os.environ["RN_ASR_TILE"] = "hip", "auto"
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            feats = m.features_from_samples(xs, layout="FC16")
            torch.cuda.synchronize()
            feature_ms = (time.perf_counter() - t0) * 1e3
            scene = ClipScene(syn.model, SimpleNamespace(auds=feats, **base), syn.opt, "cuda")
            renderer = FrameParallelRenderer(scene, rank=0, world=1, dist=None)
            syn.model.enc_a = None
            frame_ms = []
            torch.cuda.synchronize()
            t_begin = t0 = time.perf_counter()
            with torch.no_grad():
                for k in range(scene.n_frames):
                    renderer.step(k)
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    frame_ms.append((t1 - t0) * 1e3)
                    t0 = t1
            renderer.finish()
            return stats(frame_ms, [False] * len(frame_ms), time.perf_counter() - t_begin, dict(feature_pass_ms=feature_ms))

        loop_forms = {"live_auto": lambda: run_live("auto"), "live_128": lambda: run_live("128"), "file": run_file}
        for f in loop_forms.values():
            f()                                                           # warm-up
        runs = {f: [] for f in loop_forms}
        for _ in range(args.rotations):
            for name, f in loop_forms.items():
                runs[name].append(f())
        rec["live_loop"] = {"size": size, "seconds_of_audio": args.seconds, "per_frame": "two pushes, the window, the frame, one synchronise",
                            "forms": {name: dict(fps=spread([r["fps"] for r in rs]), p50_ms=spread([r["p50_ms"] for r in rs]),
                                                 p99_ms=spread([r["p99_ms"] for r in rs]), max_ms=spread([r["max_ms"] for r in rs]),
                                                 rotations=rs) for name, rs in runs.items()}}
    os.environ.pop("RN_ASR", None)
    os.environ.pop("RN_ASR_TILE", None)
    emit(rec)


if __name__ == "__main__":
    main()
