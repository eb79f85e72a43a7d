"""What the reference's schedule around the training step costs (radnerf/train.py: lr_gamma, ema_decay; csrc/rn_train.hip:
rn_adam_step_sched), on one GPU, on the benchmark's training scene (4096 rays of a 512 x 512 frame, head model).

    python tools/bench_train_schedule.py [--steps 300] [--repeats 5] [--out profiles/train_schedule_bench.json]
    python tools/bench_train_schedule.py --mode evaluate [--frames 16]

--mode step (default): one identically seeded model and trainer per form, windows of `--steps` steps in ONE rotation (every form sees
the same machine), `--repeats` passes each, host clock around a window ending in a synchronise:
    a  host_lambda_lr    GraphedTrainer as the parent has it: the host rewrites param_groups[i]["lr"] before every step (LambdaLR), and
                         refresh_lr() uploads the rates before every replay
    b  device_schedule   GraphedTrainer(lr_gamma=0.1): the begin kernel computes the rates from the device-side step counter
    c  ema_1000          b + ema_decay=0.95 at interval 1000 (the reference's setting)
    d  ema_1             b + the EMA at interval 1: every step pays the two extra streams over the tables
    e  eager_host_ema    eager Trainer(lr_gamma=0.1) and ParamEma.update() after each step: torch_ema's three launches per tensor
    f  eager_device_ema  eager Trainer(lr_gamma=0.1, ema interval 1): e's comparison partner, the EMA inside the Adam launches
and the device activities (kernels, copies, fills) of one step of each, counted with the profiler.

--mode evaluate: Trainer.evaluate over `--frames` frames of a DeviceTrainSet (fused engine, one read-back) against the
host-synchronous form of the reference's loop (nerf/utils.py:1233-1298): ema.store / copy_to / restore by torch copies, and per frame
the render, loss.item() and PSNRMeter's numpy arithmetic on .cpu() arrays.  Same model, alternating, `--repeats` passes.

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

import numpy as np  # noqa: E402
import torch  # noqa: E402

GAMMA, ITERS = 0.1, 200000


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), runs=xs)


def count_launches(fn):
    """Device activities (kernels, copies, fills) of one call, counted with the profiler's device events."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type is not None and "cuda" in str(e.device_type).lower())


def make_forms(args):
    from radnerf.ema import ParamEma
    from radnerf.scene import SyntheticScene, default_opt
    from radnerf.train import GraphedTrainer, SyntheticTrainStream, Trainer
    forms = {}
    for name in args.forms.split(","):
        scene = SyntheticScene(H=args.size, W=args.size, n_frames=8, device="cuda", opt=default_opt(engine="ops", torso=False, smooth_lips=False))
        stream = SyntheticTrainStream(scene, n_rays=args.rays)
        m = scene.model
        if name == "host_lambda_lr":
            tr = GraphedTrainer(m, scene.opt, iters=ITERS)

            def step(tr=tr, stream=stream):
                for g in tr.optimizer.param_groups:                 # LambdaLR.step(): the rate after global_step scheduler steps
                    g["lr"] = g["initial_lr"] * GAMMA ** (tr.global_step / ITERS)
                tr.step(stream.batch())
        elif name in ("device_schedule", "ema_1000", "ema_1"):
            kw = {} if name == "device_schedule" else dict(ema_decay=0.95, ema_update_interval=1000 if name == "ema_1000" else 1)
            tr = GraphedTrainer(m, scene.opt, iters=ITERS, lr_gamma=GAMMA, **kw)
            step = lambda tr=tr, stream=stream: tr.step(stream.batch())
        elif name == "eager_host_ema":
            tr = Trainer(m, scene.opt, iters=ITERS, lr_gamma=GAMMA)
            host_ema = ParamEma(m.parameters(), 0.95, 1)
            host_ema.restrict([p for g in tr.optimizer.param_groups for p in g["params"]])

            def step(tr=tr, stream=stream, host_ema=host_ema):
                tr.step(stream.batch())
                host_ema.update()
        elif name == "eager_device_ema":
            tr = Trainer(m, scene.opt, iters=ITERS, lr_gamma=GAMMA, ema_decay=0.95, ema_update_interval=1)
            step = lambda tr=tr, stream=stream: tr.step(stream.batch())
        else:
            raise SystemExit(f"bench_train_schedule: unknown form {name!r}")
        forms[name] = (tr, step)
    return forms


def bench_steps(args):
    forms = make_forms(args)
    warm = max(args.warmup, 33)                              # past the first two grid refreshes, as bench.py warms up
    for _, step in forms.values():
        for _ in range(warm):
            step()
    rates = {name: [] for name in forms}
    windows = {name: [] for name in forms}
    for _ in range(args.repeats):
        for name, (tr, step) in forms.items():              # ONE rotation: every form sees the same machine
            first = tr.global_step + 1
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            torch.cuda.synchronize()
            rates[name].append(args.steps / (time.perf_counter() - t0))
            windows[name].append([first, tr.global_step])
    out = {}
    for name, (tr, step) in forms.items():
        ema = tr.ema
        rec = dict(steps_per_s=spread(rates[name]), windows=windows[name], captures=getattr(tr, "captures", None),
                   lr_uploads=getattr(tr.optimizer, "uploads", None), ema_updates=None if ema is None else ema.num_updates)
        if ema is not None:
            k = ema.update_interval
            rec["windows_with_an_update_step"] = [any(s % k == 0 for s in range(a, b + 1)) for a, b in windows[name]]
        rec["launches_per_step"] = count_launches(step)
        out[name] = rec
    base = out.get("host_lambda_lr")
    if base is not None:
        a = base["steps_per_s"]
        out["spread_of_host_lambda_lr"] = (a["max"] - a["min"]) / a["median"]
        for name in forms:
            if name != "host_lambda_lr":
                out[name]["ratio_to_host_lambda_lr_median"] = out[name]["steps_per_s"]["median"] / a["median"]
                out[name]["ratio_to_host_lambda_lr_per_window"] = [x / y for x, y in zip(rates[name], rates["host_lambda_lr"])]
    out["steps_per_window"], out["passes"], out["warmup_steps"] = args.steps, args.repeats, warm
    return out


def bench_evaluate(args):
    from radnerf.dataset import DeviceTrainSet
    from radnerf.scene import SyntheticScene, default_opt
    from radnerf.train import Trainer
    scene = SyntheticScene(H=args.size, W=args.size, n_frames=max(args.frames, 8), device="cuda",
                           opt=default_opt(engine="fused", torso=False, smooth_lips=False))
    ds = DeviceTrainSet.from_scene(scene, max(args.frames, 8), num_rays=args.rays)
    m = ds.install(scene.model)
    tr = Trainer(m, scene.opt, ema_decay=0.95, ema_update_interval=1000)
    ema, indices, H, W = tr.ema, list(range(args.frames)), ds.H, ds.W
    with torch.no_grad():
        for _, s in ema.pairs():
            s.mul_(1.001)

    def device_form():
        return tr.evaluate(ds, indices)

    def host_form():
        m.eval()
        total, psnrs = 0.0, []
        with torch.no_grad():
            ema.store()
            ema.copy_to()
            for i in indices:
                f = ds.frame(i)
                out = m.render(f["rays_o"], f["rays_d"], f["auds"], f["bg_coords"], f["poses"], eye=f["eye"], index=f["index"], staged=True,
                               bg_color=f["bg_color"], perturb=False, dt_gamma=scene.opt.dt_gamma, max_steps=scene.opt.max_steps)
                pred, truth = out["image"].reshape(1, H, W, 3), f["images"]
                total += torch.nn.functional.mse_loss(pred, truth).item()
                p, t = pred.detach().cpu().numpy(), truth.detach().cpu().numpy()
                psnrs.append(-10 * np.log10(np.mean((p - t) ** 2)))
            ema.restore()
        return dict(loss=total / len(indices), psnr=float(np.mean(psnrs)))
    forms = {"evaluate": device_form, "host_synchronous": host_form}
    last = {name: fn() for name, fn in forms.items()}         # warm-up, and the two forms' numbers side by side
    ms = {name: [] for name in forms}
    for _ in range(args.repeats):
        for name, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    out = {name: dict(ms_per_pass=spread(v), loss=last[name]["loss"], psnr=last[name]["psnr"]) for name, v in ms.items()}
    out["host_over_evaluate_median"] = out["host_synchronous"]["ms_per_pass"]["median"] / out["evaluate"]["ms_per_pass"]["median"]
    out["frames"], out["passes"] = args.frames, args.repeats
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("step", "evaluate", "both"), default="both")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--forms", default="host_lambda_lr,device_schedule,ema_1000,ema_1,eager_host_ema,eager_device_ema")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_schedule: needs a GPU (a CPU timing says nothing about the kernels)")
    rec = {"tool": "bench_train_schedule", "device": torch.cuda.get_device_name(0), "size": args.size, "rays": args.rays,
           "gamma": GAMMA, "iters": ITERS}
    if args.mode in ("step", "both"):
        rec["step"] = bench_steps(args)
    if args.mode in ("evaluate", "both"):
        rec["evaluate"] = bench_evaluate(args)
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
