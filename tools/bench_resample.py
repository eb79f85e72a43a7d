"""What the resampling stage costs on one GPU (radnerf/resample.py, csrc/rn_resample.hip).  A record: the parent has no such stage.

    python tools/bench_resample.py [--windows 5] [--seconds 60] [--live-seconds 8] [--size 512] [--out profiles/resample_bench.json]

(a) `--seconds` of stereo s16le at 48 kHz and at 44.1 kHz -> 16 kHz mono float32, the forms alternating in ONE process, `--windows`
    windows, median [min, max]:
        device     rn_pcm_decode + rn_resample on bytes that are already on the device, by HIP events around the two launches
        upload     the host-to-device copy of the raw bytes alone (pageable memory, as Resampler.whole does it), by HIP events
        whole      Resampler.whole(bytes): upload, decode and filter, host clock to the synchronise behind it
        scipy      scipy.signal.resample_poly on the host for the same first channel as float32 -- what a user would otherwise run
    and what the stage needs by its shapes: bytes in, bytes out, 2 (2 W + 1) flops per output.
(b) tools/bench_live.py's loop (warm-up pushes, then per frame two pushes, the window, the frame and a synchronise) on the synthetic
    scene, fed at 48 kHz stereo s16le through live.resampled_chunks against the same loop fed the 16 kHz signal through live.chunks_of
    (the path without this stage), in one rotation, `--rotations` times; frames per second, whether the difference lies inside the
    16 kHz form's own spread, and the launches and host copies the stage adds per 20 ms block.

Prints one JSON object (and writes it to --out).  Needs a GPU.
"""
import argparse
import io
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rad-nerf_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), runs=[round(x, 4) for x in xs])


def stereo_s16(rate, seconds):
    import numpy as np
    t = np.arange(int(rate * seconds)) / rate
    first = 0.3 * np.sin(2 * np.pi * 220 * t) * (1 + np.sin(2 * np.pi * 0.7 * t)) + 0.05 * np.sin(2 * np.pi * 5100 * t)
    second = 0.4 * np.cos(2 * np.pi * 330 * t)
    return np.round(32767 * np.stack([first, second], axis=1)).astype("<i2")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--rotations", type=int, default=5)
    ap.add_argument("--live-seconds", type=float, default=8.0)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--skip-loop", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import scipy.signal
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample: needs a GPU (a CPU timing says nothing about the kernels)")
    import radnerf_hip as hip
    from radnerf import live
    from radnerf import resample as rs

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), out

    rec = {"tool": "bench_resample", "device": torch.cuda.get_device_name(0), "whole_file": {}}
    for rate in (48000, 44100):
        frames = stereo_s16(rate, args.seconds)
        raw = frames.tobytes()
        r = rs.Resampler(rate, 16000, "s16le", 2, device="cuda")
        n = len(frames)
        count = rs.n_out(n, r.L, r.M)
        host = torch.frombuffer(bytearray(raw), dtype=torch.uint8)
        dev = host.cuda()
        x = torch.empty(n, dtype=torch.float32, device="cuda")
        y = torch.empty(count, dtype=torch.float32, device="cuda")
        first = frames[:, 0].astype(np.float32) / np.float32(32768)

        def device():
            hip.call("rn_pcm_decode", hip.ptr(dev), n, 2, 1, hip.ptr(x), hip.stream())
            hip.call("rn_resample", hip.ptr(x), n, 0, hip.ptr(r.taps), r.L, r.M, r.W, 0, count, hip.ptr(y), hip.stream())

        def whole():
            t0 = time.perf_counter()
            out = r.whole(raw)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, out

        def scipy_host():
            t0 = time.perf_counter()
            out = scipy.signal.resample_poly(first, r.L, r.M)
            return (time.perf_counter() - t0) * 1e3, out

        forms = {"device": lambda: events(device)[0], "upload": lambda: events(lambda: host.cuda())[0], "whole": lambda: whole()[0],
                 "scipy": lambda: scipy_host()[0]}
        for f in forms.values():
            f()                                                           # warm-up: code objects, the allocator, scipy's filter design
        ms = {name: [] for name in forms}
        for _ in range(args.windows):
            for name, f in forms.items():
                ms[name].append(f())
        got = whole()[1]
        other = scipy_host()[1]
        k = min(got.numel(), len(other))
        rec["whole_file"][str(rate)] = {
            "seconds": args.seconds, "frames_in": n, "samples_out": count, "L": r.L, "M": r.M, "taps": 2 * r.W + 1, "table_bytes": r.taps.numel() * 4,
            "bytes_in": len(raw), "bytes_out": 4 * count, "flops": 2 * (2 * r.W + 1) * count, "launches": 2,
            "ms": {name: spread(v) for name, v in ms.items()},
            "device_equals_whole_bits": bool(torch.equal(y, got)),
            "max_difference_from_scipy_interior": float(np.abs(got.cpu().numpy()[400:k - 400] - other[400:k - 400]).max())}

    if not args.skip_loop:
        from bench_asr import random_module
        from radnerf.parallel import FrameParallelRenderer
        from radnerf.scene import SyntheticScene, default_opt
        m = random_module(args.layers)
        C = m.vocab_size
        size = args.size
        syn = SyntheticScene(H=size, W=size, n_frames=250, device="cuda", opt=default_opt(engine="fused"))
        base = dict(H=size, W=size, poses=syn.poses.cpu().numpy(), intrinsics=syn.intrinsics, eye_area=np.full((250, 1), 0.25, np.float32),
                    bg=np.full((size, size, 3), 255, np.uint8), auds=np.zeros((1, C, 16), np.float32))
        raw48 = stereo_s16(48000, args.live_seconds).tobytes()
        x16 = rs.Resampler(48000, 16000, "s16le", 2, device="cuda").whole(raw48).cpu().numpy()
        os.environ["RN_ASR"], os.environ["RN_ASR_TILE"] = "hip", "auto"
        pushes = []

        def run(form):
            asr = live.LiveASR(m)
            if form == "fed_48k":
                r = rs.Resampler(48000, 16000, "s16le", 2, device="cuda")
                read_chunk = live.resampled_chunks(live.block_reader(io.BytesIO(raw48), 48000, "s16le", 2), r)
            else:
                read_chunk = live.chunks_of(x16)
            scene = live.LiveScene(syn.model, SimpleNamespace(**base), syn.opt, "cuda", asr)
            renderer = FrameParallelRenderer(scene, rank=0, world=1, dist=None)
            syn.model.enc_a = None
            frame_ms = []
            torch.cuda.synchronize()
            t_begin = t0 = time.perf_counter()
            with torch.no_grad():
                for k in live.schedule(asr, read_chunk):
                    if k == 0:                                   # the warm-up pushes (and their window) are latency, not frame time
                        torch.cuda.synchronize()
                        t_begin = t0 = time.perf_counter()
                    renderer.step(k)
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    frame_ms.append((t1 - t0) * 1e3)
                    t0 = t1
            renderer.finish()
            s = sorted(frame_ms)
            return dict(frames=len(s), fps=len(s) / (time.perf_counter() - t_begin), p50_ms=s[len(s) // 2], p99_ms=s[min(len(s) - 1, int(0.99 * len(s)))],
                        max_ms=s[-1], windows=asr.windows_run)

        forms = ("fed_16k", "fed_48k")
        for f in forms:
            run(f)                                                        # warm-up
        runs = {f: [] for f in forms}
        for _ in range(args.rotations):
            for f in forms:
                runs[f].append(run(f))
        fps = {f: spread([r["fps"] for r in runs[f]]) for f in forms}
        delta = fps["fed_48k"]["median"] - fps["fed_16k"]["median"]
        # one 20 ms block through Resampler.push alone, as the loop calls it: the host's share (the calls return) and the device's
        r = rs.Resampler(48000, 16000, "s16le", 2, device="cuda")
        block = 960 * 4
        host_us, dev_us = [], []
        for i in range(0, min(len(raw48), 400 * block), block):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            r.push(raw48[i:i + block])
            b.record()
            host_us.append((time.perf_counter() - t0) * 1e6)
            torch.cuda.synchronize()
            dev_us.append(a.elapsed_time(b) * 1e3)
        rec["live_loop"] = {
            "size": size, "seconds_of_audio": args.live_seconds, "layers": args.layers, "per_frame": "two pushes, the window, the frame, one synchronise",
            "forms": {f: dict(fps=fps[f], p50_ms=spread([r["p50_ms"] for r in runs[f]]), p99_ms=spread([r["p99_ms"] for r in runs[f]]),
                              rotations=runs[f]) for f in forms},
            "fps_difference_48k_minus_16k": delta,
            "inside_the_16k_forms_own_spread": bool(fps["fed_16k"]["min"] - fps["fed_16k"]["median"] <= delta <= fps["fed_16k"]["max"] - fps["fed_16k"]["median"]),
            "per_20ms_block": {"work": "one host-to-device copy of 3840 bytes, rn_pcm_decode, one concatenation with the kept tail, rn_resample; "
                                       "resampled_chunks adds one concatenation and two slices per chunk handed out",
                               "blocks": len(host_us) - 5,
                               "push_host_us": {k: v for k, v in spread(host_us[5:]).items() if k != "runs"},
                               "push_events_us": {k: v for k, v in spread(dev_us[5:]).items() if k != "runs"}}}
        os.environ.pop("RN_ASR", None)
        os.environ.pop("RN_ASR_TILE", None)
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
