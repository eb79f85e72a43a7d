"""What the mesh export (radnerf/mesh.py over csrc/rn_mesh.hip) costs on one GPU, beside the only other way this tree can do it.

    python tools/bench_mesh.py [--calls 5] [--repeats 5] [--out profiles/mesh_bench.json]

device: at 128^3 and 256^3 on the synthetic scene's model, `field` = extract_fields (lattice ranges + the fused kernel's sigma
    branch, nothing read back) and `surface` = isosurface (count, the one read-back of the totals, emit) at the median of the field
    (a random network has no surface at the reference's threshold 10).  After a warm-up, `--repeats` windows of `--calls` calls,
    timed twice over: HIP events around the window, and the host clock around the same window ending in a synchronise.  Median
    [min, max] of the per-call times.
other_way: the reference's data flow with this tree's parts -- `model.density` through the PyTorch layers in blocks of 64^3 points (128^3 in
    the reference; 2^18 points stay below the 2^19 the occupancy refresh's PyTorch route feeds these layers at once), every block
    read back to the host (nerf/utils.py:369-384) -- at the same resolutions, host clock, one export per window; and
    the numpy marching tetrahedra of tests/mesh_reference.py (the tests' reference, not a product path) on the 64^3 field.

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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), runs=xs)


def windows(fn, calls, repeats):
    """(event ms per call, host ms per call) of `repeats` windows of `calls` calls."""
    ev, host = [], []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e3 / calls)
        ev.append(a.elapsed_time(b) / calls)
    return dict(event_ms_per_call=spread(ev), host_ms_per_call=spread(host), calls_per_window=calls, windows=repeats)


def density_with_read_back(model, lo, hi, R, enc_a, eye, S=64):
    """nerf/utils.py:369-384 with the network's audio code and eye value: blocks of S^3 points, each read back."""
    import numpy as np
    axes = [torch.linspace(float(lo[a]), float(hi[a]), R).split(S) for a in range(3)]
    u = np.zeros([R, R, R], dtype=np.float32)
    with torch.no_grad():
        for xi, xs in enumerate(axes[0]):
            for yi, ys in enumerate(axes[1]):
                for zi, zs in enumerate(axes[2]):
                    xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing="ij")
                    pts = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1), zz.reshape(-1, 1)], dim=-1).cuda()
                    val = model.density(pts, enc_a, eye)["sigma"].reshape(len(xs), len(ys), len(zs)).cpu().numpy()
                    u[xi * S: xi * S + len(xs), yi * S: yi * S + len(ys), zi * S: zi * S + len(zs)] = val
    return u


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--resolutions", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh: needs a GPU (a CPU timing says nothing about the kernels)")
    from radnerf import mesh
    from radnerf.rays import get_audio_features
    from radnerf.scene import SyntheticScene, default_opt
    sc = SyntheticScene(H=32, W=32, n_frames=8, device="cuda", opt=default_opt(engine="fused", torso=False))
    m = sc.model
    eye = torch.tensor([[0.25]], device="cuda")
    with torch.no_grad():
        enc_a = m.encode_audio(get_audio_features(sc.aud_features, sc.opt.att, 3))
    lo, hi = m.aabb_infer[:3], m.aabb_infer[3:]
    lo_host, hi_host = lo.tolist(), hi.tolist()
    rec = {"tool": "bench_mesh", "device": torch.cuda.get_device_name(0), "device_export": {}, "other_way": {}}
    for R in args.resolutions:
        field = mesh.extract_fields(m, lo, hi, R, enc_a, eye)
        threshold = float(field.median())
        for _ in range(args.warmup):
            mesh.extract_fields(m, lo, hi, R, enc_a, eye)
            verts, tris = mesh.isosurface(field, threshold, lo, hi)
        rec["device_export"][f"{R}^3"] = dict(
            threshold=threshold, vertices=int(verts.shape[0]), triangles=int(tris.shape[0]),
            workspace_bytes=int(mesh._lib.rn_mesh_workspace(R, R, R)),
            field=windows(lambda: mesh.extract_fields(m, lo, hi, R, enc_a, eye), args.calls, args.repeats),
            surface=windows(lambda: mesh.isosurface(field, threshold, lo, hi), args.calls, args.repeats))
        density_with_read_back(m, lo_host, hi_host, R, enc_a, eye)                          # warm-up
        host = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            u = density_with_read_back(m, lo_host, hi_host, R, enc_a, eye)
            host.append((time.perf_counter() - t0) * 1e3)
        rel = float((torch.from_numpy(u).cuda() - field).abs().max() / field.abs().max())
        rec["other_way"][f"{R}^3"] = dict(field_model_density_with_read_back_host_ms=spread(host), difference_of_max_to_the_device_field=rel)
        del field, verts, tris
    import mesh_reference
    field64 = mesh.extract_fields(m, lo, hi, 64, enc_a, eye)
    thr64 = float(field64.median())
    u64 = field64.cpu().numpy()
    host = []
    for _ in range(min(args.repeats, 3)):
        t0 = time.perf_counter()
        v, t = mesh_reference.marching_tetrahedra(u64, thr64, lo_host, hi_host)
        host.append((time.perf_counter() - t0) * 1e3)
    dv, dt = mesh.isosurface(field64, thr64, lo, hi)
    rec["other_way"]["64^3"] = dict(surface_numpy_reference_of_the_tests_host_ms=spread(host), vertices=len(v), triangles=len(t),
                                    equals_the_device_surface=bool(mesh_reference.same_bits(dv.cpu().numpy(), v)
                                                                   and (dt.cpu().numpy() == t).all()),
                                    surface_device=windows(lambda: mesh.isosurface(field64, thr64, lo, hi), args.calls, args.repeats))
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
