"""What preparing a dataset directory (radnerf/prepare.py over csrc/rn_prep.hip) costs on one GPU, stage by stage, beside the reference's
data flow on the host.

    python tools/bench_prepare.py [--windows 5] [--out profiles/prepare_bench.json]

Inputs are synthetic: 512^2 portrait label maps that sway from frame to frame (tests/prepref.py), frames of smooth colour with noise;
64 frames for the plate, 256 for the layers.  One process, `--windows` windows each, median [min, max]:
    kernels    HIP events: rn_prep_plate_accumulate over the 64 frames in one batch, rn_prep_plate_fill, rn_prep_layers per batch of 64
    stages     decode (the default decoder on the decode pool, JPEG frame + PNG parsing + labels, host clock), upload (HIP events),
               encode (JpegEncoder.files: kernels and the read-back, host clock), torso read-back, PNG writes on the pool, JPEG file
               writes -- each alone, per frame
    tasks      host clock around prepare.extract_background (every 4th of 256 frames) and prepare.extract_torso_and_gt (256 frames)
               on a directory in a temporary folder
    host       the reference's data flow on the same inputs in this process: sklearn's k-d tree per plate frame when sklearn
               imports (else the brute force of tests/prepref.py at the reduced size the JSON states), and prepref's lexsort / unique
               numpy form per layer frame
This is a record: nothing exists on the parent commit to compare with.  Needs a GPU.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rad-nerf_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZE, PLATE_FRAMES, LAYER_FRAMES, BATCH, STRIDE = 512, 64, 256, 64, 4


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), runs=xs)


def synthetic(np, R, n, size):
    rng = np.random.default_rng(4242)
    yy, xx = np.mgrid[0:size, 0:size]
    maps = [R.portrait_labels(size, size, np.random.default_rng(k), holes=0.002, jag=6) for k in range(8)]
    frames = np.empty((n, size, size, 3), dtype=np.uint8)
    labels = np.empty((n, size, size), dtype=np.uint8)
    for i in range(n):
        labels[i] = np.roll(maps[(i // 8) % 8], int(round(size / 16 * np.sin(i / 9))), axis=1)
        base = np.stack([(yy // 2 + i) % 256, (xx // 2 + 60 * (labels[i] == R.HEAD)) % 256, ((yy + xx) // 4 + 90 * (labels[i] == R.TORSO)) % 256], -1)
        frames[i] = (base + rng.integers(0, 6, base.shape)).clip(0, 255)
    return frames, labels


def event_ms(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def host_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def write_directory(np, R, root, frames, labels):
    from PIL import Image
    for sub in ("ori_imgs", "parsing"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)

    def one(i):
        Image.fromarray(frames[i]).save(os.path.join(root, "ori_imgs", f"{i}.jpg"), "JPEG", quality=95)
        Image.fromarray(R.parsing_from_labels(labels[i])).save(os.path.join(root, "parsing", f"{i}.png"), "PNG")
    with ThreadPoolExecutor(16) as pool:
        list(pool.map(one, range(frames.shape[0])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_prepare: needs a GPU (a CPU timing says nothing about the kernels)")
    import prepref as R
    import radnerf_hip as hip
    from radnerf import prepare
    from radnerf.datafiles import decode_workers, default_decoder
    from radnerf.video import JpegEncoder

    frames, labels = synthetic(np, R, LAYER_FRAMES, SIZE)
    rec = {"tool": "bench_prepare", "device": torch.cuda.get_device_name(0), "size": SIZE, "plate_frames": PLATE_FRAMES,
           "layer_frames": LAYER_FRAMES, "batch": BATCH, "windows": args.windows, "decode_workers": decode_workers()}
    plate_ids = list(range(0, LAYER_FRAMES, STRIDE))
    pf, pl = torch.from_numpy(frames[plate_ids]).cuda(), torch.from_numpy(labels[plate_ids]).cuda()
    lf, ll = torch.from_numpy(frames[:BATCH]).cuda(), torch.from_numpy(labels[:BATCH]).cuda()

    # ---- kernels
    def accumulate():
        b = prepare.PlateBuilder(SIZE, SIZE)
        b.add(pf, pl)
        return b
    builder = accumulate()
    plate = builder.finish()
    prepare.layers(lf, ll, plate)
    ws = torch.empty(int(hip._lib.rn_prep_workspace(PLATE_FRAMES, SIZE, SIZE)), dtype=torch.uint8, device="cuda")
    n_sure = torch.zeros(1, dtype=torch.int32, device="cuda")
    acc, fill, lay = [], [], []
    for _ in range(args.windows):
        b = prepare.PlateBuilder(SIZE, SIZE)
        acc.append(event_ms(torch, lambda: hip.call("rn_prep_plate_accumulate", hip.ptr(pf), hip.ptr(pl), PLATE_FRAMES, SIZE, SIZE, 0,
                                                    hip.ptr(b.best_d2), hip.ptr(b.best_id), hip.ptr(b.plate), hip.ptr(ws), hip.stream()))[0])
        p2 = b.plate.clone()
        fill.append(event_ms(torch, lambda: hip.call("rn_prep_plate_fill", hip.ptr(b.best_d2), hip.ptr(p2), SIZE, SIZE, 25, hip.ptr(n_sure),
                                                     hip.ptr(ws), hip.stream()))[0])
        lay.append(event_ms(torch, lambda: prepare.layers(lf, ll, plate))[0])
    rec["kernels_ms"] = dict(plate_accumulate_64_frames=spread(acc), plate_fill=spread(fill), layers_batch_of_64=spread(lay),
                             layers_includes="two output allocations and the upload of the 53-entry darken table",
                             sure_pixels=int(builder.n_sure))

    # ---- stages, per frame
    tmp = tempfile.mkdtemp(prefix="bench_prepare_")
    write_directory(np, R, tmp, frames, labels)
    decode, write = default_decoder(), prepare.default_png_writer()
    enc = JpegEncoder(SIZE, SIZE, 95, "420")
    out_dir = os.path.join(tmp, "stage_out")
    os.makedirs(out_dir)
    pool = ThreadPoolExecutor(decode_workers())
    reader = prepare._Reader(tmp, [str(i) for i in range(BATCH)], BATCH, decode, pool)
    gt, torso = prepare.layers(lf, ll, plate)
    enc.files(gt)
    st = {k: [] for k in ("decode", "upload", "encode_and_read_back", "torso_read_back", "png_writes", "jpeg_file_writes")}
    for _ in range(args.windows):
        ms, (_, hf, hl) = host_ms(lambda: next(iter(reader)))
        st["decode"].append(ms / BATCH)
        st["upload"].append(event_ms(torch, lambda: (torch.from_numpy(hf).cuda(), torch.from_numpy(hl).cuda()))[0] / BATCH)
        ms, files = host_ms(lambda: enc.files(gt))
        st["encode_and_read_back"].append(ms / BATCH)
        ms, th = host_ms(lambda: torso.cpu().numpy())
        st["torso_read_back"].append(ms / BATCH)
        st["png_writes"].append(host_ms(lambda: list(pool.map(lambda k: write(os.path.join(out_dir, f"{k}.png"), th[k]), range(BATCH))))[0] / BATCH)

        def jpeg_writes():
            for k, data in enumerate(files):
                with open(os.path.join(out_dir, f"{k}.jpg"), "wb") as fh:
                    fh.write(data)
        st["jpeg_file_writes"].append(host_ms(jpeg_writes)[0] / BATCH)
    rec["stages_ms_per_frame"] = {k: spread(v) for k, v in st.items()}
    rec["stages_ms_per_frame"]["kernels_layers"] = spread([v / BATCH for v in lay])
    rec["stages_ms_per_frame"]["kernels_plate"] = spread([v / PLATE_FRAMES for v in acc])
    rec["stages_note"] = ("decode and png_writes run on the pool, so these are wall-clock per frame at decode_workers threads; upload is pageable memory")

    # ---- whole tasks
    quiet = lambda *a: None
    t5, t6 = [], []
    prepare.extract_background(tmp, STRIDE, BATCH, log=quiet)
    for _ in range(args.windows):
        t5.append(host_ms(lambda: (prepare.extract_background(tmp, STRIDE, BATCH, log=quiet), torch.cuda.synchronize()))[0])
        t6.append(host_ms(lambda: (prepare.extract_torso_and_gt(tmp, BATCH, log=quiet), torch.cuda.synchronize()))[0])
    rec["tasks_ms"] = dict(task_5_64_frames=spread(t5), task_6_256_frames=spread(t6),
                           task_5_ms_per_frame=statistics.median(t5) / PLATE_FRAMES, task_6_ms_per_frame=statistics.median(t6) / LAYER_FRAMES)

    # ---- the reference's data flow on the host, same inputs
    host = {}
    try:
        from sklearn.neighbors import NearestNeighbors
        all_xys = np.mgrid[0:SIZE, 0:SIZE].reshape(2, -1).transpose()

        def tree(i):
            fg = np.stack(np.nonzero(labels[i] != R.BACKGROUND)).transpose(1, 0)
            return NearestNeighbors(n_neighbors=1, algorithm="kd_tree").fit(fg).kneighbors(all_xys)[0]
        host["plate_kd_tree_ms_per_frame"] = spread([host_ms(lambda: tree(plate_ids[k]))[0] for k in range(args.windows)])
        host["plate_form"] = f"sklearn k-d tree, one {SIZE}^2 frame per window"
    except ImportError:
        small = 64
        host["plate_brute_force_ms_per_frame"] = spread([host_ms(lambda: R.squared_distances(labels[plate_ids[k]][::SIZE // small, ::SIZE // small]))[0]
                                                         for k in range(args.windows)])
        host["plate_form"] = f"sklearn does not import: tests/prepref.py brute force at the reduced size {small}^2"
    plate_host = plate.cpu().numpy()
    host["layers_numpy_ms_per_frame"] = spread([host_ms(lambda: R.layers(frames[k], labels[k], plate_host))[0] for k in range(args.windows)])
    host["layers_form"] = f"tests/prepref.py (lexsort / unique / fancy indexing, integer blur), one {SIZE}^2 frame per window, one thread"
    rec["host_reference"] = host
    got = prepare.layers(lf[:1], ll[:1], plate)
    want = R.layers(frames[0], labels[0], plate_host)
    rec["layers_equal_host_reference_on_frame_0"] = bool(np.array_equal(got[0][0].cpu().numpy(), want[0]) and np.array_equal(got[1][0].cpu().numpy(), want[1]))

    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
