"""Launch-to-launch determinism of the fused network kernels (all three arithmetic variants): N launches on the same
inputs must agree bit for bit.  Written after the f16 kernels, built on v_mfma_f32_32x32x16_f16, were found to return
slightly different results from launch to launch with two waves per SIMD.

    python tools/check_determinism.py [--launches 16] [--samples 20000]

--train: run-to-run determinism of TRAINING with RN_TRAIN_DETERMINISTIC=1 (set here unless the caller set it: with 0 the table
gradients are sums of float atomics and the digests differ).  N steps of the synthetic head scene, the product's default jitter,
in two fresh child processes one after the other, each under its own `timeout`; the second starts only if the first exits 0.
Each prints a SHA-256 over all parameters and Adam moments; the digests must be equal.

    python tools/check_determinism.py --train [--steps 40] [--graphed] [--timeout 300]"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rad-nerf_amd"))


def train_child(steps, graphed):
    """One run: prints {"digest": ..., "loss": ...} as its last line."""
    import random

    import torch
    from radnerf.scene import SyntheticScene, default_opt
    from radnerf.train import GraphedTrainer, SyntheticTrainStream, Trainer
    torch.manual_seed(0)
    random.seed(0)
    scene = SyntheticScene(H=64, W=64, n_frames=8, device="cuda", opt=default_opt(engine="ops", smooth_lips=False, torso=False))
    stream = SyntheticTrainStream(scene, n_rays=1024, seed=4)
    trainer = (GraphedTrainer if graphed else Trainer)(scene.model, scene.opt)
    for _ in range(steps):
        loss = trainer.step(stream.batch())
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for name, p in scene.model.named_parameters():
        h.update(name.encode())
        h.update(p.detach().cpu().numpy().tobytes())
        st = trainer.optimizer.state.get(p, {})
        for key in ("exp_avg", "exp_avg_sq"):
            if key in st:
                h.update(st[key].detach().cpu().numpy().tobytes())
    print(json.dumps({"digest": h.hexdigest(), "loss": float(loss), "steps": steps, "graphed": bool(graphed)}), flush=True)


def train_parent(args):
    env = dict(os.environ)
    env.setdefault("RN_TRAIN_DETERMINISTIC", "1")
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--train-child", "--steps", str(args.steps)]
    cmd += ["--graphed"] if args.graphed else []
    digests = []
    for run in range(2):
        r = subprocess.run(cmd, env=env, capture_output=True, text=True)
        if r.returncode != 0:                     # nothing more is started on the device after a run that did not end well
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
            sys.exit(f"run {run} exited with status {r.returncode}")
        out = json.loads(r.stdout.strip().splitlines()[-1])
        print(f"run {run}: {out}")
        digests.append(out["digest"])
    same = digests[0] == digests[1]
    print(f"RN_TRAIN_DETERMINISTIC={env['RN_TRAIN_DETERMINISTIC']}: {'same' if same else 'DIFFERENT'} bits after {args.steps} steps")
    sys.exit(0 if same else 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=16)
    ap.add_argument("--samples", type=int, default=20000)
    ap.add_argument("--train", action="store_true", help="two training runs in child processes must end with the same bits")
    ap.add_argument("--train-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--graphed", action="store_true", help="--train with GraphedTrainer")
    ap.add_argument("--timeout", type=int, default=300, help="seconds each --train run may take")
    args = ap.parse_args()
    if args.train_child:
        return train_child(args.steps, args.graphed)
    if args.train:
        return train_parent(args)
    import torch
    from radnerf import fused
    from radnerf.scene import SyntheticScene, default_opt
    M = args.samples
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.rand(M, 3, device="cuda", generator=g) * 1.4 - 0.7
    d = torch.nn.functional.normalize(torch.randn(M, 3, device="cuda", generator=g), dim=1)
    enc_a = torch.randn(1, 64, device="cuda", generator=g)
    eye = torch.tensor([[0.25]], device="cuda")
    bad = 0
    for mlp in ("f32", "f32x2", "f16"):
        scene = SyntheticScene(H=16, W=16, n_frames=8, device="cuda", opt=default_opt(engine="fused", mlp_dtype=mlp))
        m = scene.model
        c = m.individual_codes[0].detach()
        with torch.no_grad():
            outs = [[t.clone() for t in fused.network_forward(m, x, d, enc_a, c, eye)] for _ in range(args.launches)]
        diffs = [sum(int((a != b).sum()) for a, b in zip(outs[0], o)) for o in outs[1:]]
        print(f"{mlp:6s} elements differing from launch 0: {diffs}")
        bad += sum(diffs)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
