"""Eager forward + backward of NeRFNetwork.forward_torso on the synthetic scene: the per-operator path (default) against the
fused training kernels (RN_TORSO_TRAIN=fused, csrc/rn_train_torso.hip), alternating in one process.

    python tools/bench_torso_train.py [--P 1311 20972] [--iters 200] [--warmup 20] [--runs 3] [--out profiles/torso_train_bench.json]
    python tools/bench_torso_train.py --only fused --P 1311 --runs 1 --iters 50      # one path alone, e.g. under a kernel trace
    python tools/bench_torso_train.py --summarise DIR --steps 71 [--out FILE]         # launches / step and per-kernel us of a trace
                                                                                      # (steps of the traced run: warmup + 1 + runs x iters)

    python tools/bench_torso_train.py --step [--rays 4096] [--size 64] [--iters 200] [--runs 3] [--out profiles/torso_step_bench.json]
    python tools/bench_torso_train.py --step --only graph --runs 1 --iters 50         # one path alone, e.g. under a kernel trace

--step times whole steps of a torso-training Trainer (radnerf/train.py) on the synthetic scene, four paths alternating in one
process: `default` (per-operator layer, PyTorch loss), `fused_host` (RN_TORSO_TRAIN=fused RN_TORSO_STEP=host: the fused layer on the
index list the host asks for), `resident` (RN_TORSO_TRAIN=fused: covered pixels, layer and loss on a device-side count, eager) and
`graph` (the same under GraphedTrainer).  Per path: per-step time of every run, median, spread (max - min), the calls that cross the
C ABI in one step (radnerf_hip.call; none when replayed -- a kernel trace + --summarise counts the launches themselves).

P = 1311 and 20972 are 0.32 (the covered share of the background) of a 4096-ray and a 65536-ray batch.  A run is
`iters` steps followed by one synchronise, timed on the host clock (the step is bound by launches, so the host side counts); per
path and size: the per-step time of every run, their median and their spread (max - min).
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rad-nerf_amd"))
sys.path.insert(0, ROOT)


def summarise(trace_dir, steps):
    """Kernels of a kernel trace that ran at least once per step: launches per step and mean duration."""
    if steps <= 0:
        raise SystemExit("--summarise needs --steps N > 0: the number of steps the traced run made (warm-up + runs x iters)")
    rows = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                d = rows.setdefault(r["Kernel_Name"], [])
                d.append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    kernels = {}
    for name, ds in rows.items():
        if len(ds) >= steps:
            kernels[name.split("(")[0][:96]] = dict(per_step=round(len(ds) / steps, 2), mean_us=round(statistics.mean(ds), 2))
    return dict(steps=steps, launches_per_step=round(sum(k["per_step"] for k in kernels.values()), 2),
                kernel_us_per_step=round(sum(k["per_step"] * k["mean_us"] for k in kernels.values()), 1), kernels=kernels)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, nargs="+", default=[1311, 20972])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--only", choices=["default", "fused"] + [p for p in STEP_PATHS if p != "default"])
    ap.add_argument("--step", action="store_true", help="time whole training steps of a torso Trainer (four paths)")
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--summarise")
    ap.add_argument("--steps", type=int, default=0)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.summarise:
        res = summarise(args.summarise, args.steps)
    elif args.step:
        if args.only == "fused":
            raise SystemExit("--step --only takes one of: " + ", ".join(STEP_PATHS))
        res = measure_steps(args)
    else:
        if args.only not in (None, "default", "fused"):
            raise SystemExit(f"--only {args.only} names a path of --step")
        res = measure(args)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


# --step: (RN_TORSO_TRAIN, RN_TORSO_STEP, replayed from a graph) of the four ways to run a torso training step
STEP_PATHS = {"default": (None, None, False), "fused_host": ("fused", "host", False), "resident": ("fused", "device", False),
              "graph": ("fused", "device", True)}


def _select_step_path(path):
    for name, value in zip(("RN_TORSO_TRAIN", "RN_TORSO_STEP"), STEP_PATHS[path][:2]):
        if value is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = value


def measure_steps(args):
    """Whole steps (zero_grad -> train_step -> backward -> Adam, the occupancy refresh every 16th) of a torso-training Trainer per
    path, each on its own copy of the same scene; the paths alternate run by run."""
    import torch
    import radnerf_hip as hip
    from radnerf import occupancy
    from radnerf.scene import SyntheticScene, default_opt
    from radnerf.train import GraphedTrainer, SyntheticTrainStream, Trainer
    paths = [args.only] if args.only else list(STEP_PATHS)
    warmup = max(args.warmup, 40)           # past the first refresh window: the graph is captured from step 17 on
    real_call, calls = hip.call, []

    def counting_call(fn, *a, **k):
        calls.append(fn)
        return real_call(fn, *a, **k)
    state, out = {}, dict(mode="step", rays=args.rays, size=args.size, iters=args.iters, warmup=warmup, runs=args.runs, paths={})
    for path in paths:
        _select_step_path(path)
        torch.manual_seed(0)
        scene = SyntheticScene(H=args.size, W=args.size, n_frames=8, device="cuda", opt=default_opt(engine="ops", torso=True, smooth_lips=False))
        stream = SyntheticTrainStream(scene, n_rays=args.rays)
        trainer = (GraphedTrainer if STEP_PATHS[path][2] else Trainer)(scene.model, scene.opt)
        batches = [stream.batch() for _ in range(8)]
        for i in range(warmup):
            trainer.step(batches[i % 8])
        while trainer.global_step % 16 == 0:           # the counted step is not one with an occupancy refresh
            trainer.step(batches[0])
        del calls[:]
        hip.call = counting_call
        try:
            trainer.step(batches[0])
        finally:
            hip.call = real_call
        torch.cuda.synchronize()
        m = scene.model
        thresh = min(m.density_thresh_torso, m.mean_density_torso)
        covered = int(occupancy.torso_pixels(m, batches[0]["bg_coords"].reshape(-1, 2), thresh).numel())
        info = dict(c_abi_calls_per_step=len(calls), torso_calls=sorted(set(c for c in calls if "torso" in c)), covered_pixels=covered)
        if STEP_PATHS[path][2]:
            assert trainer.captures >= 1 and trainer.replays > 0 and not calls, (trainer.captures, trainer.replays, calls)
            info.update(captures=trainer.captures, c_abi_calls_per_step=0, note="replayed: no call crosses the C ABI during a step")
        want = {"default": "rn_torso_mask", "fused_host": "rn_torso_mask", "resident": "rn_torso_select", "graph": None}[path]
        assert want is None or calls.count(want) == 1, f"{path}: {calls.count(want)} calls of {want} in one step"
        assert ("rn_train_torso_forward" in calls) == (path in ("fused_host", "resident")), (path, info["torso_calls"])
        state[path] = (trainer, batches, [], info)
    for _ in range(args.runs):
        for path in paths:                              # alternate the paths: drift of the machine lands on all of them
            _select_step_path(path)
            trainer, batches, times, _ = state[path]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.iters):
                trainer.step(batches[i % 8])
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) / args.iters * 1e6)
    for name in ("RN_TORSO_TRAIN", "RN_TORSO_STEP"):
        os.environ.pop(name, None)
    for path in paths:
        trainer, _, ts, info = state[path]
        med = statistics.median(ts)
        out["paths"][path] = dict(runs_us=[round(t, 1) for t in ts], median_us=round(med, 1), spread_us=round(max(ts) - min(ts), 1),
                                  steps_per_s=round(1e6 / med, 1), steps_made=trainer.global_step, **info)
    if "default" in out["paths"] and "graph" in out["paths"]:
        d, g = out["paths"]["default"], out["paths"]["graph"]
        out["graph_vs_default"] = dict(gain_us=round(d["median_us"] - g["median_us"], 1), spread_us=round(d["spread_us"] + g["spread_us"], 1),
                                       beats_default_by_more_than_the_spread=bool(d["median_us"] - g["median_us"] > d["spread_us"] + g["spread_us"]))
    return out


def measure(args):
    import torch
    from radnerf.scene import SyntheticScene, default_opt
    torch.manual_seed(0)
    scene = SyntheticScene(H=16, W=16, n_frames=8, device="cuda", opt=default_opt(engine="ops", smooth_lips=False))
    m = scene.model
    m.train()
    poses = scene.poses6[0:1].contiguous()
    g = torch.Generator(device="cuda").manual_seed(0)
    paths = [args.only] if args.only else ["default", "fused"]
    from radnerf import train_torso
    import radnerf_hip as hip
    entry, real_call, calls = "rn_train_torso_forward", hip.call, []

    def counting_call(fn, *a, **k):
        if fn == entry:
            calls.append(fn)
        return real_call(fn, *a, **k)
    out = dict(iters=args.iters, warmup=args.warmup, runs=args.runs, sizes={})
    for P in args.P:
        xy = (torch.rand(P, 2, device="cuda", generator=g) * 2 - 1).contiguous()
        up = [torch.randn(P, 1, device="cuda", generator=g), torch.randn(P, 3, device="cuda", generator=g),
              torch.randn(P, 2, device="cuda", generator=g)]

        def step():
            for p in m.parameters():
                p.grad = None
            code = m.individual_codes_torso[0] if m.individual_dim_torso else None
            a, c, dx = m.forward_torso(xy, poses, None, code)
            ((a * up[0]).sum() + (c * up[1]).sum() + (dx * up[2]).sum()).backward()

        def select(path):
            if path == "fused":
                os.environ["RN_TORSO_TRAIN"] = "fused"
            else:
                os.environ.pop("RN_TORSO_TRAIN", None)
        times = {p: [] for p in paths}
        for path in paths:
            select(path)
            # a "fused" column that quietly ran the per-operator path would report a tie: check the gate and count the
            # entry once, outside the timed region
            assert train_torso.usable(m, xy) == (path == "fused"), f"{path}: train_torso.usable() is {not (path == 'fused')}"
            del calls[:]
            hip.call = counting_call
            try:
                step()
            finally:
                hip.call = real_call
            assert len(calls) == (1 if path == "fused" else 0), f"{path}: {len(calls)} calls of {entry} in one step"
            for _ in range(args.warmup):
                step()
        torch.cuda.synchronize()
        for _ in range(args.runs):
            for path in paths:                      # alternate the paths: drift of the machine lands on both
                select(path)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.iters):
                    step()
                torch.cuda.synchronize()
                times[path].append((time.perf_counter() - t0) / args.iters * 1e6)
        os.environ.pop("RN_TORSO_TRAIN", None)
        out["sizes"][str(P)] = {p: dict(runs_us=[round(t, 1) for t in ts], median_us=round(statistics.median(ts), 1),
                                        spread_us=round(max(ts) - min(ts), 1)) for p, ts in times.items()}
    return out


if __name__ == "__main__":
    main()
