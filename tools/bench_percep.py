"""What the perceptual criterion (radnerf/percep.py: PerceptualAlex) costs on one GPU, kernels (RN_PERCEP=hip, csrc/rn_percep.hip)
against the same arithmetic in plain torch (RN_PERCEP=torch, unfold + matmul).

    python tools/bench_percep.py [--calls 200] [--repeats 5] [--lips-steps 40] [--out profiles/percep_bench.json]

criterion: forward + backward of 0.01 * criterion(pred, target).mean() for two shapes, one 96 x 96 image (a lips rect) and four
    32 x 32 patches (4 096 rays), on the seeded weights of the tests.  Both paths alternate in ONE process (every path sees the same
    machine): after a warm-up, `--repeats` windows of `--calls` calls each, timed twice over -- HIP events around the window, and the
    host clock around the same window ending in a synchronise.  Median [min, max] of the per-call times.
launches: device activities (kernels, copies, fills) of one forward + backward of each path, counted with the profiler.
lips_step: steps/s of the eager Trainer on the lips schedule (a rect step on even steps, a pixel step on odd ones, as
    radnerf.train.lips_schedule alternates them) of a 64 x 64 scene with a 32 x 32 rect, with each path, in the same rotation.

Prints one JSON object (and writes it to --out).  Needs a GPU.
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

SHAPES = {"rect_1x96x96": (1, 96, 96), "patches_4x32x32": (4, 32, 32)}
PATHS = ("hip", "torch")


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), runs=xs)


def seeded_module():
    """The weights of tests/percepref64.py (seed 7): He-scaled convolutions, small biases, non-negative lin vectors."""
    from radnerf.percep import LAYERS, PerceptualAlex
    g = torch.Generator().manual_seed(7)
    ws, bs = [], []
    for cin, cout, k, _, _ in LAYERS:
        ws.append(torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5)
        bs.append(torch.randn(cout, generator=g) * 0.1)
    lins = [torch.rand(1, cout, 1, 1, generator=g) / cout for _, cout, _, _, _ in LAYERS]
    return PerceptualAlex(ws, bs, lins).cuda()


def count_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type is not None and "cuda" in str(e.device_type).lower())


def bench_criterion(args, crit):
    out = {}
    for name, (P, h, w) in SHAPES.items():
        g = torch.Generator().manual_seed(1)
        pred = torch.rand(P, 3, h, w, generator=g).cuda().requires_grad_()
        target = torch.rand(P, 3, h, w, generator=g).cuda()

        def call(path):
            os.environ["RN_PERCEP"] = path
            pred.grad = None
            (0.01 * crit(pred, target).mean()).backward()
            return pred.grad

        grads = {}
        for path in PATHS:
            for _ in range(args.warmup):
                grads[path] = call(path).clone()
        diff = float((grads["hip"] - grads["torch"]).abs().max() / grads["torch"].abs().max())
        ev_ms, host_ms = {p: [] for p in PATHS}, {p: [] for p in PATHS}
        for _ in range(args.repeats):
            for path in PATHS:                                # ONE rotation: both paths see the same machine
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                a.record()
                for _ in range(args.calls):
                    call(path)
                b.record()
                torch.cuda.synchronize()
                host_ms[path].append((time.perf_counter() - t0) * 1e3 / args.calls)
                ev_ms[path].append(a.elapsed_time(b) / args.calls)
        rec = {path: dict(event_ms_per_call=spread(ev_ms[path]), host_ms_per_call=spread(host_ms[path]),
                          launches=count_launches(lambda path=path: call(path))) for path in PATHS}
        rec["torch_over_hip_per_window"] = [t / k for t, k in zip(host_ms["torch"], host_ms["hip"])]
        rec["hip_ahead_in_every_window"] = all(r > 1.0 for r in rec["torch_over_hip_per_window"])
        rec["gradient_difference_of_max"] = diff
        rec["calls_per_window"], rec["windows"] = args.calls, args.repeats
        out[name] = rec
    return out


def bench_lips_step(args, crit):
    from radnerf.dataset import DeviceTrainSet
    from radnerf.scene import SyntheticScene, default_opt
    from radnerf.train import Trainer
    forms = {}
    for path in PATHS:
        torch.manual_seed(0)
        scene = SyntheticScene(H=64, W=64, n_frames=8, device="cuda", opt=default_opt(engine="ops", torso=False, smooth_lips=False))
        ds = DeviceTrainSet.from_scene(scene, 8, num_rays=1024, seed=1)
        forms[path] = (Trainer(ds.install(scene.model), scene.opt, patch_criterion=crit), ds)

    def run(path, n, at):
        os.environ["RN_PERCEP"] = path
        tr, ds = forms[path]
        for s in range(at, at + n):
            tr.step(ds.batch_rect([s % 8], rect=(16, 48, 16, 48)) if s % 2 == 0 else ds.batch([s % 8]))
        return at + n

    at = {p: run(p, max(args.warmup, 34), 0) for p in PATHS}
    rates = {p: [] for p in PATHS}
    for _ in range(args.repeats):
        for path in PATHS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            at[path] = run(path, args.lips_steps, at[path])
            torch.cuda.synchronize()
            rates[path].append(args.lips_steps / (time.perf_counter() - t0))
    out = {path: dict(steps_per_s=spread(rates[path])) for path in PATHS}
    out["hip_over_torch_per_window"] = [k / t for k, t in zip(rates["hip"], rates["torch"])]
    out["steps_per_window"], out["windows"], out["rect"] = args.lips_steps, args.repeats, [32, 32]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--lips-steps", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_percep: needs a GPU (a CPU timing says nothing about the kernels)")
    crit = seeded_module()
    rec = {"tool": "bench_percep", "device": torch.cuda.get_device_name(0), "criterion": bench_criterion(args, crit)}
    if args.lips_steps > 0:
        rec["lips_step"] = bench_lips_step(args, crit)
    os.environ.pop("RN_PERCEP", None)
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
