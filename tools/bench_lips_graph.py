"""What replaying lip fine-tuning steps from captured graphs buys on one GPU: the eager Trainer against
GraphedTrainer(lips_graphs=...) on the same build, in ONE process, with PerceptualAlex on the seeded weights of the tests as the
patch criterion (tools/bench_percep.py's set-up).

    python tools/bench_lips_graph.py [--windows 5] [--steps 300] [--out profiles/lips_graph_bench.json]

rect_64: the 64 x 64 scene of bench_percep.py's `lips_step` with its 32 x 32 rect, so the rates stand next to the ones recorded there.
rect_512: a 512 x 512, 64-frame set (DeviceTrainSet.from_scene) whose lips rects are replaced by squares of even side, the side
    drawn per frame from 80 ... 112 with a fixed seed -- a STAND-IN for a landmark track (a real one gives a few dozen shapes too,
    provider.py:492-500), not one.
patch_512: the same set; 4 096 rays as four 32 x 32 patches in the rect's place.

Schedule: radnerf.train.lips_schedule's alternation -- the rect (or the patches) on even steps, random pixels on odd ones -- with
the frame moving on every second step, so that every frame's rect is visited.  A warm-up pass takes the first window and then visits
every frame once (its wall time is recorded: for the captured form it holds the captures); then `--windows` windows of `--steps`
steps per form, the forms alternating within one rotation, each window timed by the host clock around work that ends in a
synchronise.  Recorded: steps/s per window and form, their ratio per window pair, the graphs captured (in the warm-up and in every
window: a budget that moves to a new row capacity captures again), and the growth of torch.cuda.memory_reserved() from before the
captured form's first step to after its last window.

Prints one JSON object (and writes it to --out).  Needs a GPU.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rad-nerf_amd"))

import torch  # noqa: E402

FORMS = ("eager", "captured")
SIDES = tuple(range(80, 113, 2))            # 17 even sides


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), runs=xs)


def stand_in_rects(rects, H, W, seed=5):
    """Squares of even side around the centres of `rects` ([F][4] = xmin, xmax, ymin, ymax), the side drawn per frame from SIDES
    and the square clipped at the image border, as provider.py:492-500 clips."""
    rng = np.random.default_rng(seed)
    out = []
    for (xmin, xmax, ymin, ymax), side in zip(rects, rng.choice(SIDES, size=len(rects))):
        cx, cy, half = (xmin + xmax) // 2, (ymin + ymax) // 2, int(side) // 2
        out.append([max(0, cx - half), min(int(H), cx + half), max(0, cy - half), min(int(W), cy + half)])
    return out


def seeded_module():
    """The weights of tests/percepref64.py (seed 7), as tools/bench_percep.py builds them."""
    from radnerf.percep import LAYERS, PerceptualAlex
    g = torch.Generator().manual_seed(7)
    ws, bs = [], []
    for cin, cout, k, _, _ in LAYERS:
        ws.append(torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5)
        bs.append(torch.randn(cout, generator=g) * 0.1)
    lins = [torch.rand(1, cout, 1, 1, generator=g) / cout for _, cout, _, _, _ in LAYERS]
    return PerceptualAlex(ws, bs, lins).cuda()


def make_forms(size, n_frames, num_rays, crit, slots_of, shared=None, stand_in=False):
    """{form: (trainer, set)}: one scene and model per form from the same seed, the set's arrays shared between the forms."""
    from radnerf.dataset import DeviceTrainSet
    from radnerf.scene import SyntheticScene, default_opt
    from radnerf.train import GraphedTrainer, Trainer
    forms = {}
    for form in FORMS:
        torch.manual_seed(0)
        scene = SyntheticScene(H=size, W=size, n_frames=n_frames, device="cuda", opt=default_opt(engine="ops", torso=False, smooth_lips=False))
        if shared is None:
            shared = DeviceTrainSet.from_scene(scene, n_frames, num_rays=num_rays, seed=1)
            if stand_in:
                lips = stand_in_rects(shared.lips_rect, size, size)
                shared = DeviceTrainSet(shared.images, shared.torso_img, shared.bg_img, shared.poses, shared.intrinsics, shared.auds,
                                        shared.face_rect, eye_area=shared.eye_area, opt=shared.opt, num_rays=num_rays, seed=1,
                                        device=shared.device, lips_rect=lips)
        ds = shared.clone(num_rays=num_rays)
        m = ds.install(scene.model)
        if form == "eager":
            forms[form] = (Trainer(m, scene.opt, patch_criterion=crit), ds)
        else:
            forms[form] = (GraphedTrainer(m, scene.opt, patch_criterion=crit, lips_graphs=slots_of(ds)), ds)
    return forms, shared


def bench_schedule(args, forms, lips_batch):
    """lips_batch(ds, frame) -> the batch of an even step."""
    F = forms["eager"][1].F

    def run(form, n, at):
        tr, ds = forms[form]
        for s in range(at, at + n):
            frame = (s // 2) % F
            tr.step(lips_batch(ds, frame) if s % 2 == 0 else ds.batch([frame]))
        return at + n

    def timed(form, n, at):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        at = run(form, n, at)
        torch.cuda.synchronize()
        return at, time.perf_counter() - t0

    graphed = forms["captured"][0]
    at, warm_s, rates = {}, {}, {f: [] for f in FORMS}
    reserved_before = torch.cuda.memory_reserved()
    warm = 32 + 2 * F                                           # the first windows (the refresh at step 16 sets the budget), then every frame
    for form in ("captured", "eager"):
        at[form], warm_s[form] = timed(form, warm, 0)
    captures = [graphed.captures]
    for _ in range(args.windows):
        for form in FORMS:                                      # ONE rotation: both forms see the same machine
            at[form], dt = timed(form, args.steps, at[form])
            rates[form].append(args.steps / dt)
        captures.append(graphed.captures)
    grown = torch.cuda.memory_reserved() - reserved_before
    rec = {form: dict(steps_per_s=spread(rates[form]), warmup_wall_s=warm_s[form]) for form in FORMS}
    rec["captured_over_eager_per_window"] = [c / e for c, e in zip(rates["captured"], rates["eager"])]
    rec["captured_ahead_in_every_window"] = all(r > 1.0 for r in rec["captured_over_eager_per_window"])
    rec["captures_after_warmup"] = captures[0]
    rec["captures_per_window"] = [b - a for a, b in zip(captures, captures[1:])]
    rec["graphs"] = dict(plain=len(graphed.capture_log), lips=graphed.lips_captures, lips_slots=graphed.lips_graphs,
                         lips_held=len(graphed._lips.graphs), plain_held=len(graphed._plain.graphs),
                         capacities=sorted({c for _, _, c in graphed.capture_log} | {e[2] for e in graphed.lips_capture_log}))
    rec["memory_reserved_growth_mib"] = grown / 2 ** 20
    rec["memory_reserved_growth_mib_per_graph"] = grown / 2 ** 20 / max(graphed.captures, 1)
    rec["warmup_steps"], rec["steps_per_window"], rec["windows"] = warm, args.steps, args.windows
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--frames", type=int, default=64, help="frames of the 512 x 512 set")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lips_graph: needs a GPU (a CPU timing says nothing about a replayed graph)")
    crit = seeded_module()
    rec = {"tool": "bench_lips_graph", "device": torch.cuda.get_device_name(0),
           "schedule": "lips rect (or patches) on even steps, random pixels on odd ones; the frame moves every second step"}

    forms, _ = make_forms(64, 8, 1024, crit, lambda ds: 4)
    rec["rect_64"] = bench_schedule(args, forms, lambda ds, f: ds.batch_rect([f], rect=(16, 48, 16, 48)))
    rec["rect_64"]["rect"] = [32, 32]
    del forms
    torch.cuda.empty_cache()

    forms, shared = make_forms(512, args.frames, 4096, crit, lambda ds: 3 * len(ds.lips_shapes()), stand_in=True)
    shapes = shared.lips_shapes()
    rec["rect_512"] = bench_schedule(args, forms, lambda ds, f: ds.batch_rect([f]))
    rec["rect_512"]["lips_rects"] = ("a STAND-IN for a landmark track: squares of even side 80 ... 112, drawn per frame with a fixed seed, "
                                     "around the centres of from_scene's lips rects")
    rec["rect_512"]["shapes"] = {f"{h}x{w}": n for (h, w), n in sorted(shapes.items())}
    rec["rect_512"]["n_shapes"], rec["rect_512"]["frames"] = len(shapes), args.frames
    del forms
    torch.cuda.empty_cache()

    forms, _ = make_forms(512, args.frames, 4096, crit, lambda ds: 2, shared=shared)
    rec["patch_512"] = bench_schedule(args, forms, lambda ds, f: ds.batch_patch([f], 32))
    rec["patch_512"]["patch_size"], rec["patch_512"]["num_rays"] = 32, 4096

    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
