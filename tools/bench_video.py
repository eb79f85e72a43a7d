"""What the Motion-JPEG write-out (radnerf/video.py over csrc/rn_jpeg.hip) costs on one GPU, beside the other ways to get frames off it.

    python tools/bench_video.py [--windows 5] [--out profiles/video_bench.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_video.py --kernels-only
    python tools/bench_video.py --merge-kernel-stats DIR/.../*_kernel_stats.csv --kernels-run RUN.json --out profiles/video_bench.json
                                                     (no GPU needed; RUN.json: what the --kernels-only run printed)

Frames: 512^2 and 450^2 renders of the benchmark's synthetic scene (SyntheticScene, the fused engine's uint8 output), quality 90,
4:2:0, batches of 1, 8 and 32.  One process; per batch size the forms alternate, `--windows` windows each; median [min, max]:
    device_encode_ms_per_frame   HIP events around the coefficient and entropy passes of a window's batches
    raw_read_back_ms_per_frame   HIP events around the copy of the same uint8 frames to pinned memory, nothing encoded
    pil_16_threads_ms_per_frame  host clock: PIL's encoder (same quality, subsampling, optimize=False) over the frames on 16 threads
    bytes_per_frame              the scans' sizes plus the header and EOI
render: frames per second of render_clip's loop (render, keep the frame) over `--render-frames` frames with and without the
    VideoSink (batch 8, an AVI in a temporary directory), host clock around a window that ends with the file closed.
--ablate: the same loop at 512^2 with the sink cut down to its staging copy, to staging + kernels, and whole: where its cost goes.
kernels (after --merge-kernel-stats): per-kernel times of the profiler's own run, the bytes each kernel must move computed from the
    shapes, and the bound that puts it against.  Whatever was not measured is written as "not measured".
Needs a GPU (except --merge-kernel-stats).
"""
import argparse
import csv
import io
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rad-nerf_amd"))

QUALITY, SUB, BATCHES, SIZES = 90, "420", (1, 8, 32), (512, 450)
HBM_BYTES_PER_S = 8e12             # MI355X peak; the kernels' traffic is a small multiple of the batch and mostly stays in L2


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), runs=xs)


def rendered_frames(torch, size, n):
    from radnerf.scene import SyntheticScene, default_opt
    sc = SyntheticScene(H=size, W=size, n_frames=max(n, 8), device="cuda", opt=default_opt(engine="fused"))
    with torch.no_grad():
        frames = torch.stack([sc.render(i, want_u8=True)["image_u8"].reshape(size, size, 3).clone() for i in range(n)])
    return sc, frames


def event_window(torch, fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def pil_window(frames_host, pool):
    from PIL import Image

    def one(f):
        buf = io.BytesIO()
        Image.fromarray(f).save(buf, "JPEG", quality=QUALITY, subsampling=2, optimize=False)
        return buf.tell()
    t0 = time.perf_counter()
    sizes = list(pool.map(one, frames_host))
    return (time.perf_counter() - t0) * 1e3 / len(frames_host), sizes


def sink_ablation(torch, sc, enc, size, n, windows, tmp):
    """Frames per second of the render loop with parts of the sink taken out: where what the sink costs goes."""
    from radnerf.video import AviWriter, VideoSink

    class StageOnly(VideoSink):                      # the per-frame copy into the batch's staging tensor, nothing else
        def _encode(self):
            self._n = 0

    class KernelsOnly(VideoSink):                    # + the coefficient and entropy passes; no side stream, no copy, no file
        def _encode(self):
            self.encoder.encode_device(self._stage[:self._n])
            self._n = 0

    def loop(cls, k):
        sink = cls(AviWriter(os.path.join(tmp, f"ablate_{size}_{k}.avi"), size, size, 25), enc, batch=8) if cls else None
        kept = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            for i in range(n):
                kept.append(sc.render(i, want_u8=True)["image_u8"].reshape(size, size, 3).clone())
                if sink is not None:
                    sink.push(kept[-1])
        if sink is not None:
            sink.finish()
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0)
    forms = (("no_sink", None), ("staging_copy_only", StageOnly), ("staging_and_kernels", KernelsOnly), ("whole_sink", VideoSink))
    for _, c in forms:
        loop(c, 0)
    runs = {name: [] for name, _ in forms}
    for k in range(windows):
        for name, c in forms:
            runs[name].append(loop(c, k))
    return {name: spread(v) for name, v in runs.items()}


def kernel_bytes(size, batch, stream_bytes):
    """Bytes each kernel of one batch must read and write at least, from the shapes (420: 1.5 samples per pixel)."""
    mcus = (-(-size // 16)) ** 2
    blocks = mcus * 6 * batch
    coef = blocks * 128
    words = blocks * 208
    return {"k_jpeg_coefficients": size * size * 3 * batch + coef, "k_jpeg_block_bits": coef + blocks * 4, "k_jpeg_scan": blocks * 8,
            "k_jpeg_pack": coef + blocks * 4 + stream_bytes, "k_jpeg_ff_count": stream_bytes, "k_jpeg_stuff": 2 * stream_bytes,
            "fillBufferAligned": words}                        # the memset of the unstuffed stream, sized by the worst case


def merge_kernel_stats(path, rec, shape):
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r["Name"]
            if "jpeg" in name or "fillBuffer" in name:
                rows[name.split("(")[0]] = dict(calls=int(r["Calls"]), average_us=float(r["AverageNs"]) / 1e3, min_us=float(r["MinNs"]) / 1e3,
                                                max_us=float(r["MaxNs"]) / 1e3)
    need = kernel_bytes(shape["size"], shape["batch"], shape["stream_bytes"])
    rec["kernels_run"] = shape
    for name, row in rows.items():
        for k, b in need.items():
            if name.endswith(k):
                row["bytes_at_least"] = b
                row["achieved_GB_per_s"] = b / row["average_us"] / 1e3
                share = b / HBM_BYTES_PER_S * 1e6 / row["average_us"]
                row["share_of_hbm_peak"] = share
                row["bound"] = "memory" if share > 0.5 else "not memory: instruction issue and latency (its bytes would take %.2f us at the HBM peak)" % (
                    b / HBM_BYTES_PER_S * 1e6)
    rec["kernels"] = rows or "not measured"
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--render-frames", type=int, default=512, help="per window: long enough that setting a sink up (pinned memory) is not what is timed")
    ap.add_argument("--ablate", action="store_true", help="only the render loop at 512^2 with parts of the sink taken out")
    ap.add_argument("--kernels-only", action="store_true", help="the profiler's run: batches of 8 at 512^2, nothing timed")
    ap.add_argument("--merge-kernel-stats", default=None, help="a rocprofv3 *_kernel_stats.csv of a --kernels-only run, merged into --out")
    ap.add_argument("--kernels-run", default=None, help="the JSON line a --kernels-only run printed")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.merge_kernel_stats:
        with open(args.out) as f:
            rec = json.load(f)
        with open(args.kernels_run) as f:
            shape = json.loads(f.read().strip().splitlines()[-1])
        text = json.dumps(merge_kernel_stats(args.merge_kernel_stats, rec, shape), indent=1)
        with open(args.out, "w") as f:
            f.write(text + "\n")
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_video: needs a GPU (a CPU timing says nothing about the kernels)")
    from radnerf.video import AviWriter, JpegEncoder, VideoSink
    if args.ablate:
        sc, _ = rendered_frames(torch, 512, 8)
        rec = dict(tool="bench_video --ablate", size=512, frames_per_window=args.render_frames,
                   render_frames_per_s=sink_ablation(torch, sc, JpegEncoder(512, 512, QUALITY, SUB), 512, args.render_frames, args.windows,
                                                     tempfile.mkdtemp(prefix="bench_video_")))
        print(json.dumps(rec, indent=1))
        return
    if args.kernels_only:
        _, frames = rendered_frames(torch, 512, 8)
        enc = JpegEncoder(512, 512, QUALITY, SUB)
        for _ in range(20):
            buf = enc.encode_device(frames)
        torch.cuda.synchronize()
        sizes = buf[:32].cpu().numpy().view("uint32")
        print(json.dumps(dict(size=512, batch=8, stream_bytes=int(sizes.sum()))))
        return
    try:
        import PIL  # noqa: F401
        have_pil = True
    except ImportError:
        have_pil = False
    rec = {"tool": "bench_video", "device": torch.cuda.get_device_name(0), "quality": QUALITY, "subsampling": SUB, "windows": args.windows,
           "sizes": {}, "kernels": "not measured", "played_in_ffmpeg_or_vlc": "not measured"}
    pool = ThreadPoolExecutor(16)
    for size in SIZES:
        sc, frames = rendered_frames(torch, size, max(BATCHES))
        enc = JpegEncoder(size, size, QUALITY, SUB)
        out = {"raw_bytes_per_frame": size * size * 3, "batches": {}}
        for B in BATCHES:
            batch = frames[:B].contiguous()
            pinned = torch.empty(batch.shape, dtype=torch.uint8).pin_memory()
            host = batch.cpu().numpy()
            calls = max(1, 64 // B)
            data, sizes = enc.encode(batch)                                             # warm-up, and the sizes
            pinned.copy_(batch, non_blocking=True)
            dev, raw, pil = [], [], []
            for _ in range(args.windows):                                               # the forms alternate
                dev.append(event_window(torch, lambda: enc.encode_device(batch), calls) / B)
                raw.append(event_window(torch, lambda: pinned.copy_(batch, non_blocking=True), calls) / B)
                if have_pil:
                    pil.append(pil_window(list(host) * (16 if B == 1 else 2), pool)[0])
            out["batches"][str(B)] = dict(device_encode_ms_per_frame=spread(dev), raw_read_back_ms_per_frame=spread(raw),
                                          pil_16_threads_ms_per_frame=spread(pil) if have_pil else "not measured",
                                          bytes_per_frame=float(sizes.mean()) + len(enc.header) + 2, calls_per_window=calls)
        # render_clip's loop with and without the sink
        n = args.render_frames
        tmp = tempfile.mkdtemp(prefix="bench_video_")

        def render_loop(with_sink, k):
            sink = VideoSink(AviWriter(os.path.join(tmp, f"{size}_{k}.avi"), size, size, 25), enc, batch=8) if with_sink else None
            kept = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.no_grad():
                for i in range(n):
                    kept.append(sc.render(i, want_u8=True)["image_u8"].reshape(size, size, 3).clone())
                    if sink is not None:
                        sink.push(kept[-1])
            if sink is not None:
                sink.finish()
            torch.cuda.synchronize()
            return n / (time.perf_counter() - t0)
        render_loop(True, 0), render_loop(False, 0)                                     # warm-up
        plain, sunk = [], []
        for k in range(args.windows):
            plain.append(render_loop(False, k))
            sunk.append(render_loop(True, k))
        out["render_frames_per_s"] = dict(without_sink=spread(plain), with_sink=spread(sunk), frames_per_window=n,
                                          avi_bytes=os.path.getsize(os.path.join(tmp, f"{size}_0.avi")))
        rec["sizes"][f"{size}^2"] = out
        del sc, frames
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
