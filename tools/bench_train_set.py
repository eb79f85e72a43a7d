"""What the device-resident training set costs (radnerf/dataset.py, csrc/rn_train_batch.hip), on one GPU.

    python tools/bench_train_set.py [--size 512] [--rays 4096] [--frames 64] [--out profiles/train_set_bench.json]
    python tools/bench_train_set.py --mode rect [--rect 96]       (or --mode patch [--patch 16]): the lip fine-tuning batches

1. Microseconds per DeviceTrainSet.batch(): the one-launch kernel against the class's own torch path on the device (the parent
   has no data-set path to compare with), same arrays, same run, alternating, `--repeats` windows of `--calls` calls each after a
   warm-up.  Two clocks per window: HIP events around the window (what the stream sees) and the host clock around the window
   ending in a synchronise (what the caller pays, enqueue included).
2. GraphedTrainer steps/s fed by ds.batch() cycling the frames, against a second, identically seeded model and trainer fed by
   SyntheticTrainStream (one frame, float table), same process, alternating windows of `--steps` steps after both are past their
   first grid refreshes.  Host clock around each window, ending in a synchronise.  `--feeds` picks the feeds (one alone for a
   profiler run of its own: rocprofv3 --kernel-trace --stats -- python tools/bench_train_set.py --skip-batch --feeds device_train_set).

--mode rect / patch time DeviceTrainSet.batch_rect() on a centred `--rect` x `--rect` square and batch_patch() with `--rays`
rays in `--patch` x `--patch` patches the same way (part 1 only: a captured step does not take these batches), and count the
device launches of one call of either path with the profiler.

Prints one JSON object (and writes it to --out).  Needs a GPU: there is no CPU timing worth reporting.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rad-nerf_amd"))

import torch  # noqa: E402


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), runs=xs)


def time_calls(fn, calls):
    """(event us per call, host us per call) of `calls` back-to-back calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    return a.elapsed_time(b) * 1e3 / calls, (t1 - t0) * 1e6 / calls


def count_launches(fn):
    """Device activities (kernels, copies, fills) of one call, counted with the profiler's device events."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type is not None and "cuda" in str(e.device_type).lower())


def bench_batch(ds, args):
    oracle = ds.clone(kernel="torch")
    frames = list(range(ds.F))
    state = {"k": 0}

    if args.mode == "rect":
        lo_r, lo_c = (ds.H - args.rect) // 2, (ds.W - args.rect) // 2
        rect = (lo_r, lo_r + args.rect, lo_c, lo_c + args.rect)
        one = lambda s, index: s.batch_rect(index, rect=rect)
        n = args.rect * args.rect
    elif args.mode == "patch":
        one = lambda s, index: s.batch_patch(index, args.patch)
        n = ds.num_rays
    else:
        one = lambda s, index: s.batch(index)
        n = ds.num_rays

    def call(s):
        def fn():
            state["k"] += 1
            one(s, [frames[state["k"] % len(frames)]])
        return fn
    paths = {"kernel": call(ds), "torch": call(oracle)}
    for fn in paths.values():
        for _ in range(args.warmup_calls):
            fn()
    res = {name: {"event_us": [], "host_us": []} for name in paths}
    for _ in range(args.repeats):
        for name, fn in paths.items():                      # alternating: both see the same machine
            ev, host = time_calls(fn, args.calls)
            res[name]["event_us"].append(ev)
            res[name]["host_us"].append(host)
    ds.check()
    out = {name: {k: spread(v) for k, v in r.items()} for name, r in res.items()}
    out["torch_over_kernel_event"] = out["torch"]["event_us"]["median"] / out["kernel"]["event_us"]["median"]
    out["torch_over_kernel_host"] = out["torch"]["host_us"]["median"] / out["kernel"]["host_us"]["median"]
    out["calls_per_window"], out["windows"] = args.calls, args.repeats
    out["mode"], out["rays_per_call"] = args.mode, n
    if args.mode != "batch":
        out["launches_per_call"] = {name: count_launches(fn) for name, fn in paths.items()}
    out["bytes_per_call"] = dict(written=n * 15 * 4 + n * 8, gathered=n * 10)    # packed + inds_out; 3 + 4 + 3 image bytes per pixel
    return out


def bench_trainers(ds, scene_ds, args):
    """Feeds: `device_train_set` (ds.batch cycling the frames), `synthetic_stream` (SyntheticTrainStream, one frame) and, to tell
    the cost of the launch from the cost of data that CHANGES, `device_train_set_one_frame` (ds.batch of frame 0 every step: the
    trainer's index upload and the frame-to-frame swing of the marcher's budget fall away).  One identically seeded model and
    trainer per feed."""
    from radnerf.scene import SyntheticScene
    from radnerf.train import GraphedTrainer, SyntheticTrainStream
    feeds, trainers = {}, {}
    for name in args.feeds.split(","):
        scene = scene_ds if not trainers else SyntheticScene(H=args.size, W=args.size, n_frames=args.frames, device="cuda", opt=scene_ds.opt)
        if name == "synthetic_stream":
            stream = SyntheticTrainStream(scene, n_rays=args.rays)
            nxt = lambda k, stream=stream: stream.batch()
        elif name in ("device_train_set", "device_train_set_one_frame"):
            own = ds.clone()
            own.install(scene.model)
            nxt = (lambda k, own=own: own.batch([k % own.F])) if name == "device_train_set" else (lambda k, own=own: own.batch([0]))
        else:
            raise SystemExit(f"bench_train_set: unknown feed {name!r}")
        trainer = trainers[name] = GraphedTrainer(scene.model, scene.opt)
        count = {"k": 0}

        def step(trainer=trainer, nxt=nxt, count=count):
            count["k"] += 1
            trainer.step(nxt(count["k"]))
        feeds[name] = step
    for fn in feeds.values():
        for _ in range(max(args.warmup, 33)):               # past the first two grid refreshes, as bench.py warms up
            fn()
    rates = {name: [] for name in feeds}
    captured = {name: trainers[name].captures for name in feeds}
    for _ in range(args.repeats):
        for name, fn in feeds.items():                      # alternating: every feed sees the same machine
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize()
            rates[name].append(args.steps / (time.perf_counter() - t0))
    out = {name: dict(steps_per_s=spread(v), captures=trainers[name].captures, captures_in_timed_windows=trainers[name].captures - captured[name],
                      replays=trainers[name].replays) for name, v in rates.items()}
    for name, tr in trainers.items():                       # the marcher's own count over the last 16 steps: the work a step did
        out[name]["samples_per_step"] = float(tr.model.step_counter[:, 0].float().mean().item())
    if "synthetic_stream" in rates:
        for name in rates:
            if name != "synthetic_stream":
                out[name]["ratio_to_stream_median"] = out[name]["steps_per_s"]["median"] / out["synthetic_stream"]["steps_per_s"]["median"]
                out[name]["ratio_to_stream_per_window"] = [a / b for a, b in zip(rates[name], rates["synthetic_stream"])]
    out["steps_per_window"], out["windows"], out["warmup_steps"] = args.steps, args.repeats, max(args.warmup, 33)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("batch", "rect", "patch"), default="batch")
    ap.add_argument("--rect", type=int, default=96, help="--mode rect: side of the centred square")
    ap.add_argument("--patch", type=int, default=16, help="--mode patch: patch_size (--rays must be a multiple of its square)")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--warmup-calls", type=int, default=50)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-trainers", action="store_true")
    ap.add_argument("--skip-batch", action="store_true")
    ap.add_argument("--feeds", default="device_train_set,synthetic_stream,device_train_set_one_frame")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_set: needs a GPU (a CPU timing says nothing about the kernel)")
    from radnerf.dataset import DeviceTrainSet
    from radnerf.scene import SyntheticScene, default_opt
    opt = default_opt(engine="ops", torso=False, smooth_lips=False)
    scene = SyntheticScene(H=args.size, W=args.size, n_frames=args.frames, device="cuda", opt=opt)
    ds = DeviceTrainSet.from_scene(scene, args.frames, num_rays=args.rays)
    rec = {"tool": "bench_train_set", "device": torch.cuda.get_device_name(0), "size": args.size, "rays": args.rays, "frames": args.frames,
           "set_bytes": int(ds.images.numel() + ds.torso_img.numel() + ds.bg_img.numel())}
    if not args.skip_batch:
        rec["batch"] = bench_batch(ds, args)
    if not args.skip_trainers and args.mode == "batch":
        rec["graphed_trainer"] = bench_trainers(ds, scene, args)
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
