"""The --train_camera training step through the fused head against the per-operator chain (RN_TRAIN_HEAD = fused | ops), config 2
(4096 rays, hash grid T = 2^19, eager Trainer, occupancy refresh every 16 steps inside the timed region).

    python tools/bench_train_camera.py [--repeats 5] [--cycles 16] [--out DIR]      # alternates fused / ops child processes
    python tools/bench_train_camera.py --one fused --cycles 16                      # one run, prints one JSON line

Each run is a fresh process (the head is chosen by an environment variable that the model caches its answer to).  A run warms up
for 33 steps (past the first two refreshes), then times whole 16-step refresh cycles with a host clock around one synchronise per
cycle; the sample count of every step stays on the device until the end.  Reported per head: steps/s of every repeat, their
spread, and ms per step of the cycles grouped by their samples per step (the budget moves with the refresh, so a run has a phase
of large steps and a phase of small ones).  The JSON goes to DIR/train_camera.json (default DIR: profiles).

    python tools/bench_train_camera.py --compare-pose [--parent DIR] [--repeats 5]
the pose code of the step instead of its head: RN_TRAIN_CAMERA = torch | fused (radnerf/train_camera.py), each eager and under
GraphedTrainer (--graph), as alternating child processes (`--one fused --pose P [--graph]`); --parent DIR adds the eager run of
another checkout's copy of this tool (the parent commit, built in DIR) to the rotation.  Written under the key "pose" of the
same JSON, with the launches per step of tools/train_step_launches.py --train-camera for both pose codes.

    python tools/bench_train_camera.py --kernel-stats KERNEL_TRACE.csv [--samples 62000]
folds the kernel-trace CSV of `rocprofv3 --kernel-trace --stats -- python tools/bench_train_camera.py --one fused` into the JSON: the
new kernel's average time over the launches of the large-step phase and its rate on algorithmic bytes (1 024 B gathered + 128 B feature gradients + 24 B written per sample).
"""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rad-nerf_amd"))
sys.path.insert(0, ROOT)

KERNEL = "k_train_input_grads"
BYTES_PER_SAMPLE = 1024 + 128 + 24


def one(head, cycles, rays, size, train_camera=True, pose="torch", graph=False):
    os.environ["RN_TRAIN_HEAD"] = head
    os.environ["RN_TRAIN_LOSS"] = "fused" if head == "fused" else "torch"
    os.environ["RN_TRAIN_CAMERA"] = pose
    import torch
    from bench import GRIDS
    from radnerf.scene import SyntheticScene, default_opt
    from radnerf.train import GraphedTrainer, SyntheticTrainStream, Trainer
    scene = SyntheticScene(H=size, W=size, n_frames=8, device="cuda",
                           opt=default_opt(engine="ops", torso=False, smooth_lips=False, train_camera=train_camera, **GRIDS["hash19"]))
    stream = SyntheticTrainStream(scene, n_rays=rays)
    trainer = (GraphedTrainer if graph else Trainer)(scene.model, scene.opt)
    m = scene.model
    for _ in range(33 + (16 - 33 % 16) % 16):          # warm-up ends on a cycle boundary: every timed cycle starts with a refresh
        trainer.step(stream.batch())
    counts = torch.zeros(cycles, 16, dtype=torch.int64, device="cuda")
    cycle_ms = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for c in range(cycles):
        t = time.perf_counter()
        for i in range(16):
            trainer.step(stream.batch())
            counts[c, i] = m.step_counter[(m.local_step - 1) % 16, 0]
        torch.cuda.synchronize()
        cycle_ms.append((time.perf_counter() - t) * 1e3 / 16)
    elapsed = time.perf_counter() - t0
    per_cycle = counts.double().mean(1).tolist()
    cam = float(m.camera_dT[stream.frame].abs().max()) if train_camera else None
    extra = dict(captures=trainer.captures, replays=trainer.replays) if graph else {}
    return dict(head=head, pose=pose, graph=graph, **extra, train_camera=train_camera, steps=16 * cycles, steps_per_s=16 * cycles / elapsed, ms_per_step=elapsed / (16 * cycles) * 1e3,
                cycle_ms_per_step=cycle_ms, cycle_samples_per_step=per_cycle, camera_dT_moved=cam)


def phases(runs):
    """ms per step of the cycles above / below the midpoint of the samples-per-step range of all runs of one head."""
    pts = [(s, t) for r in runs for s, t in zip(r["cycle_samples_per_step"], r["cycle_ms_per_step"])]
    lo, hi = min(p[0] for p in pts), max(p[0] for p in pts)
    if hi < 1.5 * lo:
        return [dict(samples_per_step=sum(p[0] for p in pts) / len(pts), ms_per_step=sum(p[1] for p in pts) / len(pts), cycles=len(pts))]
    mid, out = (lo + hi) / 2, []
    for grp in ([p for p in pts if p[0] >= mid], [p for p in pts if p[0] < mid]):
        out.append(dict(samples_per_step=sum(p[0] for p in grp) / len(grp), ms_per_step=sum(p[1] for p in grp) / len(grp), cycles=len(grp)))
    return out


def kernel_stats(path, samples):
    """path: a rocprofv3 kernel-trace CSV (one row per dispatch).  The launches of the large-step phase are those in the upper
    half of the kernel's duration range; `samples`: that phase's samples per step."""
    with open(path, newline="") as f:
        us = sorted((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in csv.DictReader(f) if KERNEL in r.get("Kernel_Name", ""))
    if not us:
        return dict(kernel=KERNEL, average_us="not measured")
    mid = (us[0] + us[-1]) / 2
    big = [u for u in us if u >= mid] if us[-1] > 1.5 * us[0] else us
    avg_us = sum(big) / len(big)
    return dict(kernel=KERNEL, calls=len(us), calls_in_large_phase=len(big), average_us=avg_us, min_us=big[0], max_us=big[-1],
                average_us_all_calls=sum(us) / len(us), samples_per_call=samples, algorithmic_bytes_per_sample=BYTES_PER_SAMPLE,
                algorithmic_GB_per_s=samples * BYTES_PER_SAMPLE / (avg_us * 1e-6) / 1e9,
                held_against="the rate at which L2 / Infinity Cache deliver lines, not HBM bytes: the 1 024 B are 64 loads of 16 B (x-pairs of "
                             "8-B rows), each of which moves a 128-B line -- 8 KB of line traffic per sample; HBM sees only the 152 B of "
                             "streamed gradients and outputs per sample")


def _child(cmd, cwd=None, last_line=True):
    """The JSON a child process printed (its last line, or all of its output)."""
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=cwd)
    if r.returncode != 0:                              # a failed run ends the measurement: nothing more is started on the device
        sys.stderr.write(r.stdout + r.stderr)
        sys.exit(r.returncode or 1)
    return json.loads(r.stdout.strip().splitlines()[-1] if last_line else r.stdout)


def compare_pose(args, path):
    """Alternating runs of the step with each pose code, eager and graphed (and the parent checkout's eager step)."""
    me, size = os.path.abspath(__file__), ["--cycles", str(args.cycles), "--rays", str(args.rays), "--size", str(args.size)]
    variants = {f"{pose}_{'graph' if graph else 'eager'}": ([sys.executable, me, "--one", "fused", "--pose", pose] + (["--graph"] if graph else []) + size, None)
                for graph in (False, True) for pose in ("torch", "fused")}
    if args.parent:
        variants = {"parent_eager": ([sys.executable, os.path.join(os.path.abspath(args.parent), "tools", "bench_train_camera.py"), "--one", "fused"] + size,
                                     os.path.abspath(args.parent)), **variants}
    runs = {k: [] for k in variants}
    for rep in range(args.repeats):
        for name, (cmd, cwd) in variants.items():
            runs[name].append(_child(cmd, cwd))
            print(f"repeat {rep} {name}: {runs[name][-1]['steps_per_s']:.1f} steps/s", flush=True)
    rec = json.load(open(path)) if os.path.exists(path) else {}
    out = {"workload": f"config 2 with --train_camera, fused head: {args.rays} rays of a {args.size}x{args.size} frame, hash grid T=2^19, "
                       f"{16 * args.cycles} timed steps per run after warm-up, occupancy refresh every 16 steps inside the timed region",
           "repeats": args.repeats}
    for name, rs in runs.items():
        v = [r["steps_per_s"] for r in rs]
        out[name] = dict(steps_per_s=v, mean=sum(v) / len(v), ms_per_step=[r["ms_per_step"] for r in rs], phases=phases(rs),
                         camera_dT_moved=[r["camera_dT_moved"] for r in rs])
        if rs[0].get("graph"):
            out[name]["captures"] = [r["captures"] for r in rs]
    launches = os.path.join(ROOT, "tools", "train_step_launches.py")
    for pose in ("torch", "fused"):
        os.environ["RN_TRAIN_CAMERA"] = pose
        step = _child([sys.executable, launches, "--train-camera", "--rays", str(args.rays), "--size", str(args.size)], last_line=False)
        out[f"{pose}_eager"]["launches_per_step"] = dict(launches=step["launches"], kernels=step["kernels"], gpu_us=step["gpu_us"], samples=step["samples"])
    rec["pose"] = out
    json.dump(rec, open(path, "w"), indent=1)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", choices=["fused", "ops"])
    ap.add_argument("--no-camera", action="store_true", help="--one: the same step without --train_camera")
    ap.add_argument("--pose", choices=["torch", "fused"], default="torch", help="--one: the pose code (RN_TRAIN_CAMERA)")
    ap.add_argument("--graph", action="store_true", help="--one: the step under GraphedTrainer")
    ap.add_argument("--compare-pose", action="store_true")
    ap.add_argument("--parent", help="--compare-pose: a built checkout of the parent commit")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cycles", type=int, default=16, help="timed 16-step refresh cycles per run (16 = 256 steps)")
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--kernel-stats")
    ap.add_argument("--samples", type=int, default=62000)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "train_camera.json")
    if args.one:
        print(json.dumps(one(args.one, args.cycles, args.rays, args.size, not args.no_camera, args.pose, args.graph)))
        return
    if args.compare_pose:
        compare_pose(args, path)
        return
    if args.kernel_stats:
        rec = json.load(open(path)) if os.path.exists(path) else {}
        big = max((p["samples_per_step"] for p in rec.get("fused", {}).get("phases", [])), default=None)
        rec["input_grads_kernel"] = kernel_stats(args.kernel_stats, int(big) if big else args.samples)
        json.dump(rec, open(path, "w"), indent=1)
        print(json.dumps(rec["input_grads_kernel"]))
        return
    runs = {"fused": [], "ops": []}
    for rep in range(args.repeats):
        for head in ("fused", "ops"):
            cmd = [sys.executable, os.path.abspath(__file__), "--one", head, "--cycles", str(args.cycles), "--rays", str(args.rays), "--size", str(args.size)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:                      # a failed run ends the measurement: nothing more is started on the device
                sys.stderr.write(r.stdout + r.stderr)
                sys.exit(r.returncode or 1)
            runs[head].append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(f"repeat {rep} {head}: {runs[head][-1]['steps_per_s']:.1f} steps/s", flush=True)
    rec = {"workload": f"config 2 with --train_camera: {args.rays} rays of a {args.size}x{args.size} frame, hash grid T=2^19, eager Trainer, "
                       f"{16 * args.cycles} timed steps per run after warm-up, whole 16-step refresh cycles, host clock around one synchronise per cycle",
           "repeats": args.repeats}
    for head, rs in runs.items():
        v = [r["steps_per_s"] for r in rs]
        rec[head] = dict(steps_per_s=v, mean=sum(v) / len(v), spread=(max(v) - min(v)) / (sum(v) / len(v)), phases=phases(rs),
                         camera_dT_moved=[r["camera_dT_moved"] for r in rs])
    f, o = rec["fused"], rec["ops"]
    rec["speedup"] = f["mean"] / o["mean"]
    rec["faster_by_more_than_the_spread"] = min(f["steps_per_s"]) > max(o["steps_per_s"])
    if os.path.exists(path) and "pose" in (kept := json.load(open(path))):
        rec["pose"] = kept["pose"]                    # --compare-pose's record lives in the same file
    json.dump(rec, open(path, "w"), indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
