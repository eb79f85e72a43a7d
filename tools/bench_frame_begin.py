"""Where the frame prologue's time goes: rn_frame_begin alone (HIP events around single launches) on the benchmark's first pose, with
grids and boxes that take the occupancy walk apart.

    python tools/bench_frame_begin.py [--size 512] [--rounds 200]

    head          the synthetic head, rn_head_t.occ_box = NULL: every ray tests every cell from near to far
    head+box      the same with the occupied box: rays test cells only inside it
    empty         no bit set, NULL: every ray tests ~74 empty cells and emits nothing
    empty+box     no bit set, with its (empty) box: nobody tests a cell -- everything the launch does besides the walk
    full          every bit set, NULL: every ray that meets the cube emits at its first lattice point
Prints one JSON line: median / minimum microseconds per launch and the lattice points a ray visits."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rad-nerf_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=200)
    args = ap.parse_args()
    import numpy as np
    import torch
    import radnerf_hip as hip
    from radnerf_hip import abi
    from radnerf.scene import SyntheticScene, default_opt
    S = args.size
    scene = SyntheticScene(H=S, W=S, n_frames=8, device="cuda", opt=default_opt(engine="fused"))
    m, N = scene.model, S * S
    head = m.density_bitfield.clone()
    grids = {"head": head, "empty": torch.zeros_like(head), "full": torch.full_like(head, 255)}
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device="cuda")
    bufs = dict(rays_o=z(N, 3), rays_d=z(N, 3), nears=z(N), fars=z(N), weights_sum=z(N), depth=z(N), image=z(N, 3), rays_t=z(N), xyzs=z(N, 3),
                dirs=z(N, 3), deltas=z(N, 2), sigmas=z(N), rgbs=z(N, 3), rays_alive_a=z(N, dtype=torch.int32), rays_alive_b=z(N, dtype=torch.int32),
                state=z(abi.RN_HEAD_STATE_INTS, dtype=torch.int32), block_counts=z(3 * ((N + 255) // 256 + 1), dtype=torch.int32),
                live_slots=z(N, dtype=torch.int32))
    pose = scene.poses[0].reshape(-1, 4)[:4].contiguous().float()
    fx, fy, cx, cy = (float(v) for v in scene.intrinsics)
    out = {"size": S, "rounds": args.rounds}
    for name, grid, with_box in (("head", "head", False), ("head+box", "head", True), ("empty", "empty", False), ("empty+box", "empty", True),
                                 ("full", "full", False)):
        bits = grids[grid]
        box = torch.zeros(8, dtype=torch.int32, device="cuda")
        hip.call("rn_occ_box", hip.ptr(bits), int(m.cascade), int(m.grid_size), hip.ptr(box), hip.stream())
        h = abi.HeadT(N=N, aabb=hip.ptr(m.aabb_infer), min_near=float(m.min_near), bitfield=hip.ptr(bits), bound=float(m.bound),
                      dt_gamma=float(scene.opt.dt_gamma), max_steps=int(scene.opt.max_steps), cascade=int(m.cascade), grid_size=int(m.grid_size),
                      T_thresh=1e-4, order_w=S, occ_box=hip.ptr(box) if with_box else None, **{k: hip.ptr(v) for k, v in bufs.items()})
        times = []
        for r in range(args.rounds + 10):
            bufs["state"].zero_()                      # the prologue appends to the live list from state[6] on: start every launch at 0
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            hip.call("rn_frame_begin", C.byref(h), hip.ptr(pose), fx, fy, cx, cy, S, hip.stream())
            e1.record()
            e1.synchronize()
            if r >= 10:
                times.append(e0.elapsed_time(e1) * 1e3)
        hit = (bufs["nears"] < bufs["fars"]) & (bufs["fars"] < 3e38)
        points = float(((bufs["fars"] - bufs["nears"])[hit] / (2 * 3 ** 0.5 / int(m.grid_size))).mean())
        out[name] = dict(us_median=round(float(np.median(times)), 2), us_min=round(float(np.min(times)), 2),
                         live=int(bufs["state"][6]), rays_meeting_the_cube=int(hit.sum()), lattice_points_near_to_far=round(points, 1))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
