"""What loading a dataset directory costs (radnerf/datafiles.py), and that nothing changes behind it, on one GPU.

    python tools/bench_datafiles.py [--size 512] [--frames 64] [--rays 4096] [--out profiles/datafiles_load.json]

Writes a synthetic `--size`^2, `--frames`-frame directory into a temporary folder (JPEG frames, PNG torso layers, landmark files,
an audio-feature file, transforms files, a background at twice the size), then times

1. DeviceTrainSet.from_directory: decode (the default decoder in the loader's thread pool) + landmarks + upload, wall clock, and
   load_split alone (the host part);
2. ds.batch() of that set against the same call on a DeviceTrainSet.from_scene set of the same shape -- the set
   tools/bench_train_set.py measures -- same process, alternating windows, its two clocks (HIP events and the host clock): the
   launch is the same one, so the two must sit together;
3. ClipScene.frame(i, lazy_rays=True): the host work per rendered frame (window cut, two slices, a dict).

A record, not a gate: the parent commit has no loader to compare a load time with.  Prints one JSON object (and writes it to --out).
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rad-nerf_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_train_set import spread, time_calls  # noqa: E402


def write_directory(root, size, frames, opt):
    from PIL import Image
    from radnerf.rays import intrinsics_from_fovy, orbit_pose
    rng = np.random.default_rng(0)
    for sub in ("gt_imgs", "torso_imgs", "ori_imgs"):
        os.makedirs(os.path.join(root, sub))
    rr = np.arange(size, dtype=np.float32)[:, None] / (size - 1)
    cc = np.arange(size, dtype=np.float32)[None, :] / (size - 1)
    listed = []
    for f in range(frames):
        img = np.stack([255 * (0.2 + 0.6 * rr * np.ones_like(cc)), 255 * (0.3 + 0.5 * cc * np.ones_like(rr)),
                        np.full((size, size), 40.0 + 2 * f)], -1) + rng.integers(0, 24, (size, size, 3))
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(os.path.join(root, "gt_imgs", f"{f}.jpg"), quality=95)
        torso = np.zeros((size, size, 4), dtype=np.uint8)
        torso[int(0.6 * size):, int(0.1 * size):int(0.9 * size)] = (150, 90, 96, 255)
        Image.fromarray(torso).save(os.path.join(root, "torso_imgs", f"{f}.png"))
        lms = np.round(0.25 * size + 0.5 * size * rng.random((68, 2)), 1)
        lms[48:60] = np.round(0.45 * size + 0.19 * size * rng.random((12, 2)), 1)
        np.savetxt(os.path.join(root, "ori_imgs", f"{f}.lms"), lms, fmt="%.1f")
        pose = orbit_pose(opt.radius, 8.0 * np.sin(0.25 * f), 4.0 * np.cos(0.4 * f))
        raw = np.zeros((4, 4), dtype=np.float32)
        for new, old in ((0, 1), (1, 2), (2, 0)):
            raw[old] = [pose[new, 0], -pose[new, 1], -pose[new, 2], pose[new, 3] / 4]
        raw[3, 3] = 1
        listed.append(dict(img_id=f, aud_id=f, transform_matrix=raw.tolist()))
    head = dict(focal_len=float(intrinsics_from_fovy(size, size, opt.fovy)[0]), cx=size / 2, cy=size / 2)
    for name, part in (("train", listed), ("val", listed[:8])):
        with open(os.path.join(root, f"transforms_{name}.json"), "w") as fh:
            json.dump(dict(head, frames=part), fh)
    np.save(os.path.join(root, "aud_eo.npy"), (3.0 * rng.standard_normal((frames, 16, 44))).astype(np.float32))
    Image.fromarray(rng.integers(0, 256, (2 * size, 2 * size, 3), dtype=np.uint8)).save(os.path.join(root, "bc.jpg"), quality=95)
    return sum(os.path.getsize(os.path.join(dp, f)) for dp, _, fs in os.walk(root) for f in fs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_datafiles: needs a GPU")
    from radnerf import datafiles
    from radnerf.clip import ClipScene
    from radnerf.dataset import DeviceTrainSet
    from radnerf.scene import SyntheticScene, default_opt
    opt = default_opt(engine="fused", torso=False, smooth_lips=False)
    rec = {"tool": "bench_datafiles", "device": torch.cuda.get_device_name(0), "size": args.size, "frames": args.frames, "rays": args.rays,
           "decode_workers": datafiles.decode_workers(), "decoder": "cv2" if datafiles._cv2() is not None else "PIL"}
    with tempfile.TemporaryDirectory() as root:
        rec["directory_bytes"] = write_directory(root, args.size, args.frames, opt)
        opt.path = root
        loads, hosts = [], []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ds = DeviceTrainSet.from_directory(root, opt, "train", num_rays=args.rays)
            torch.cuda.synchronize()
            loads.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            datafiles.load_split(root, opt, "train")
            hosts.append(time.perf_counter() - t0)
        rec["from_directory_s"], rec["load_split_s"] = spread(loads), spread(hosts)
        rec["set_bytes"] = int(ds.images.numel() + ds.torso_img.numel() + ds.bg_img.numel())
        clip = datafiles.LoadedClip(H=ds.H, W=ds.W, poses=ds.loaded.poses, intrinsics=ds.loaded.intrinsics, auds=ds.loaded.auds,
                                    eye_area=ds.loaded.eye_area, bg=ds.loaded.bg)
    scene = SyntheticScene(H=args.size, W=args.size, n_frames=args.frames, device="cuda", opt=opt)
    ref = DeviceTrainSet.from_scene(scene, args.frames, num_rays=args.rays)
    sets = {"from_directory": ds, "from_scene": ref}
    k = {"k": 0}

    def call(s):
        def fn():
            k["k"] += 1
            s.batch([k["k"] % s.F])
        return fn
    fns = {name: call(s) for name, s in sets.items()}
    for fn in fns.values():
        for _ in range(50):
            fn()
    res = {name: {"event_us": [], "host_us": []} for name in fns}
    for _ in range(args.repeats):
        for name, fn in fns.items():
            ev, host = time_calls(fn, args.calls)
            res[name]["event_us"].append(ev)
            res[name]["host_us"].append(host)
    rec["batch"] = {name: {c: spread(v) for c, v in r.items()} for name, r in res.items()}
    rec["batch"]["calls_per_window"], rec["batch"]["windows"] = args.calls, args.repeats

    cs = ClipScene(scene.model, clip, opt, "cuda")
    cs.frame(0, lazy_rays=True)
    times = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.calls):
            cs.frame(i, lazy_rays=True)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e6 / args.calls)
    rec["clip_scene_frame_us"] = spread(times)
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
