"""How the inference loop's marchers walk and where they put their samples (csrc/rn_head_loop.hip: k_frame_begin, k_head_march,
k_head_compact<true>, k_head_step<true>; their walk looks one lattice point ahead, their loads are issued early) against the
per-operator chain rn_march_rays / rn_composite_rays / rn_compact_rays, which keeps the plain walk and is pinned to the oracle by
tests/test_gpu_walk.py.  Row by row and word by word: any other way of writing the rows out has to pass the same file.

Scene: N near-parallel rays through a 128^3 grid; `alive` of them, at chosen places of the alive list, each pass through a column
of occupied cells of its own, whose depth (2 .. 40 cells, i.e. 1 .. 23 lattice points) the case chooses; every other ray meets
no occupied cell and dies in the first compositor.  T_thresh = 0, so a ray dies only by running out of samples: the live count
entering iteration 1 is exactly `alive`, its n_step is N // alive, and later iterations shrink the list and walk n_step up to 8.
Where `thin` is set the first 256 hit rays of the list have two-cell columns: they all die in iteration 1, so the first workgroup of
that compaction keeps nothing (an empty row range).  Sample buffers are NaN-filled on entry.

Bar, per iteration: live rows of xyzs / dirs / deltas bit-equal to the chain's (raw words), dead rows deltas == 0, the live list
sorted == the rows with deltas[0] != 0, the state words, both alive lists' live prefix, rays_t, and at the end image / depth /
weights_sum, the per-iteration live-ray counts and the iteration / live-sample / slot counters.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import occ_box_cases as ob
import walk_cases as wc

pytestmark = pytest.mark.gpu

DEV = "cuda"
H = 128
MAX_STEPS = 32          # <= H: constant dt, the loop's usual walk
ITERS = 12              # iterations enqueued: step grows by n_step >= 1, every case is over or well into n_step = 8 by then


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def raw(x):
    a = x.detach().cpu().numpy()
    return a.view(np.int32) if a.dtype == np.float32 else a


def alive_order(n, order_w):
    """rn_ray_dev.h alive_order: the ray at place n of the initial alive list."""
    if not order_w:
        return n
    tile, within, tiles_x = n >> 6, n & 63, order_w >> 3
    return ((tile // tiles_x) * 8 + (within >> 3)) * order_w + (tile % tiles_x) * 8 + (within & 7)


# (W, Hh, alive, thin): n_step of iteration 1 = min(W * Hh // alive, 8) takes every value 1 .. 8; alive counts 1, 63, 64, 255, 256,
# 257, 513 (wave and workgroup edges, a last partial workgroup); 20 x 17 and 21 x 19 take the plain list order
CASES = {
    "n1_a513": (32, 24, 513, False),
    "n2_a257_thin": (24, 24, 257, True),
    "n3_a256": (32, 28, 256, False),
    "n4_a255": (32, 32, 255, False),
    "n5_a64_plain": (20, 17, 64, False),
    "n6_a63_plain": (21, 19, 63, False),
    "n7_a513_thin": (64, 60, 513, True),
    "n8_a1": (16, 16, 1, False),
    "n8_a257": (48, 48, 257, False),
}


class Scene:
    def __init__(self, name):
        W, Hh, alive, thin = CASES[name]
        self.N = N = W * Hh
        self.order_w = W if (W % 8 == 0 and Hh % 8 == 0) else 0
        self.alive = alive
        rng = np.random.default_rng(sum(name.encode()))
        places = np.sort(rng.choice(N, alive, replace=False))          # places of the hit rays in the initial alive list
        self.hit_rays = np.array([alive_order(int(p), self.order_w) for p in places])
        depth = rng.integers(2, 41, alive)
        if thin:
            depth[:256] = 2
        d = np.float32([1e-3, 2e-3, 1.0])
        d /= np.linalg.norm(d)
        cell = 2.0 / H
        z0 = 40                                                        # first occupied cell of every column
        o = np.zeros((N, 3), np.float32)
        # misses: over the empty half x > 0
        o[:, 0] = rng.uniform(0.2, 0.8, N)
        o[:, 1] = rng.uniform(-0.8, 0.8, N)
        o[:, 2] = -1.5
        # hits: a column each (every second cell of the half x < 0), the ray through the column's centre at mid depth
        cols = rng.choice(32 * 64, alive, replace=False)
        cx, cy = 2 * (cols % 32), 2 * (cols // 32)
        cells = []
        for j, r in enumerate(self.hit_rays):
            zc = (z0 + depth[j] / 2) * cell - 1.0
            c = np.array([(cx[j] + 0.5) * cell - 1.0, (cy[j] + 0.5) * cell - 1.0])
            o[r, :2] = c - d[:2] / d[2] * (zc + 1.5)
            cells += [[cx[j], cy[j], z0 + k] for k in range(depth[j])]
        self.o, self.d = o, np.tile(d, (N, 1)).astype(np.float32)
        self.bits = ob.bits_from_cells(cells, H)


@pytest.fixture(scope="module")
def net(hiplib):
    """Network inputs of the loop (grids, packed weights, one frame's bias block) from a small synthetic model."""
    from radnerf import fused
    from radnerf.scene import SyntheticScene, default_opt
    torch.manual_seed(0)
    scene = SyntheticScene(H=16, W=16, n_frames=8, device=DEV, opt=default_opt(engine="fused"))
    m = scene.model
    st = fused._state(m)
    st.refresh()
    enc_a = torch.randn(m.audio_dim, device=DEV) * 0.1
    bias = fused._frame_bias(st, enc_a, scene.eye, m.individual_codes[0]).clone()
    torch.cuda.synchronize()
    return dict(scene=scene, st=st, bias=bias)


_scenes = {}


def scene_of(name):
    if name not in _scenes:
        _scenes[name] = Scene(name)
    return _scenes[name]


class Loop:
    """One frame of the device loop through the C ABI, a call at a time."""

    def __init__(self, net, sc, box, live_list=True):
        import radnerf_hip as hip
        from radnerf_hip import abi
        self.hip, self.abi, self.net, self.sc = hip, abi, net, sc
        N = sc.N
        self.keep = [t(sc.o), t(sc.d), t(sc.bits), t(np.float32([-1] * 3 + [1] * 3)), box]
        z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=DEV)
        nan = lambda *shape: torch.full(shape, float("nan"), device=DEV)
        self.b = dict(nears=z(N), fars=z(N), weights_sum=z(N), depth=z(N), image=z(N, 3), rays_t=z(N), xyzs=nan(N, 3), dirs=nan(N, 3),
                      deltas=nan(N, 2), sigmas=z(N), rgbs=z(N, 3), rays_alive_a=z(N, dtype=torch.int32), rays_alive_b=z(N, dtype=torch.int32),
                      state=z(abi.RN_HEAD_STATE_INTS, dtype=torch.int32), block_counts=z(3 * ((N + 255) // 256 + 1), dtype=torch.int32))
        self.live_slots = z(N, dtype=torch.int32) if live_list else None
        o, d, bits, aabb, _ = self.keep
        self.h = abi.HeadT(rays_o=hip.ptr(o), rays_d=hip.ptr(d), N=N, aabb=hip.ptr(aabb), min_near=wc.MIN_NEAR, bitfield=hip.ptr(bits), bound=1.0,
                           dt_gamma=1 / 256, max_steps=MAX_STEPS, cascade=1, grid_size=H, T_thresh=0.0, order_w=sc.order_w,
                           occ_box=hip.ptr(box), live_slots=hip.ptr(self.live_slots), **{k: hip.ptr(v) for k, v in self.b.items()})

    def begin(self):
        self.hip.call("rn_frame_begin", C.byref(self.h), None, 0.0, 0.0, 0.0, 0.0, 0, self.hip.stream())

    def iterate(self, first, n, flags):
        st = self.net["st"]
        self.hip.call("rn_head_iterate_ex", C.byref(self.h), C.byref(st.gx), C.byref(st.gw), self.hip.ptr(st.packed), self.hip.ptr(self.net["bias"]),
                      first, n, st.mlp_dtype, flags, self.hip.stream())

    def get(self, k):
        torch.cuda.synchronize()
        return self.b[k].cpu().numpy().copy()

    def bank(self, it):
        return self.get("state")[(it & 1) * 8:(it & 1) * 8 + 8]

    def check_samples(self, it, ref):
        """The sample buffers hold iteration `it`'s rows: against the chain's snapshot of that iteration."""
        bank = self.bank(it)
        assert bank[:5].tolist() == [ref["n_alive"], ref["step"], ref["n_step"], ref["M"], 1], (it, bank)
        M = ref["M"]
        deltas = self.get("deltas")[:M]
        live = ref["live"]
        dead = np.setdiff1d(np.arange(M), live)
        assert np.array_equal(np.nonzero(deltas[:, 0] != 0)[0], live), it
        assert not deltas[dead].view(np.int32).any(), it                       # dead rows: deltas == (+0, +0)
        for k in ("xyzs", "dirs", "deltas"):
            assert np.array_equal(self.get(k)[:M][live].view(np.int32), ref[k]), (it, k)
        if self.live_slots is not None:
            assert bank[6] == live.size, it
            assert np.array_equal(np.sort(self.live_slots.cpu().numpy()[:live.size]), live), it

    def check_after(self, it, ref):
        """Iteration `it` is composited and compacted: rays_t, the next list's live prefix, the next bank."""
        assert np.array_equal(self.get("rays_t").view(np.int32), ref["rays_t"]), it
        nxt = self.get("rays_alive_a" if (it + 1) % 2 == 0 else "rays_alive_b")
        assert np.array_equal(nxt[:ref["n_next"]], ref["list_next"]), it
        assert self.bank(it + 1)[0] == ref["n_next"], it

    def check_end(self, end):
        state = self.get("state")
        A = self.abi
        for k in ("image", "depth", "weights_sum"):
            assert np.array_equal(self.get(k).view(np.int32), end[k]), k
        n = len(end["hist"])
        assert state[A.RN_HEAD_ST_HIST:A.RN_HEAD_ST_HIST + n].tolist() == end["hist"]
        assert state[A.RN_HEAD_ST_ITERS:A.RN_HEAD_ST_SLOTS + 1].tolist() == end["counters"]
        assert state[A.RN_HEAD_ST_STALLED] == 0


def chain_and_single(net, sc, box, live_list=True):
    """The loop one iteration per call (k_frame_begin, then k_head_march) in lockstep with the per-operator chain, which composites
    with the loop's own network outputs of the iteration (same rows, so the same samples).  Returns the chain's snapshots."""
    import radnerf_hip as hip
    from radnerf_hip import abi
    N = sc.N
    lp = Loop(net, sc, box, live_list)
    o, d, bits, aabb, _ = lp.keep
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=DEV)
    nears, fars, ws, depth, image = z(N), z(N), z(N), z(N), z(N, 3)
    hip.call("rn_near_far_from_aabb", hip.ptr(o), hip.ptr(d), hip.ptr(aabb), N, wc.MIN_NEAR, hip.ptr(nears), hip.ptr(fars), hip.stream())
    rays_t = nears.clone()
    alive = t(np.array([alive_order(n, sc.order_w) for n in range(N)], np.int32))
    n_alive, step, snaps, hist, live_total, slots = N, 0, [], [], 0, 0
    lp.begin()
    for it in range(ITERS):
        if n_alive == 0 or step >= MAX_STEPS:
            break
        n_step = max(min(N // n_alive, 8), 1)
        M = n_alive * n_step
        xyzs, dirs, deltas = z(M, 3), z(M, 3), z(M, 2)
        hip.call("rn_march_rays", n_alive, n_step, hip.ptr(alive), hip.ptr(rays_t), hip.ptr(o), hip.ptr(d), 1.0, 1 / 256, MAX_STEPS, 1, H,
                 hip.ptr(bits), hip.ptr(nears), hip.ptr(fars), hip.ptr(xyzs), hip.ptr(dirs), hip.ptr(deltas), None, None, hip.stream())
        dl = deltas.cpu().numpy()
        live = np.nonzero(dl[:, 0] != 0)[0]
        ref = dict(n_alive=n_alive, step=step, n_step=n_step, M=M, live=live, deltas=raw(deltas)[live], xyzs=raw(xyzs)[live], dirs=raw(dirs)[live],
                   per_ray=(dl[:, 0] != 0).reshape(n_alive, n_step).sum(1))
        lp.iterate(it, 1, abi.RN_LOOP_FIRST_MARCHED if it == 0 else 0)
        lp.check_samples(it, ref)
        sig, rgb = lp.b["sigmas"][:M].clone(), lp.b["rgbs"][:M].clone()
        hip.call("rn_composite_rays", n_alive, n_step, 0.0, hip.ptr(alive), hip.ptr(rays_t), hip.ptr(sig), hip.ptr(rgb), hip.ptr(deltas), hip.ptr(ws),
                 hip.ptr(depth), hip.ptr(image), None, hip.stream())
        out, n_out = z(N, dtype=torch.int32), z(1, dtype=torch.int32)
        wsp = hip.workspace(hip.workspace_bytes("rn_compact_rays_workspace", n_alive), torch.device(DEV))
        hip.call("rn_compact_rays", hip.ptr(alive), n_alive, None, hip.ptr(out), hip.ptr(n_out), hip.ptr(wsp), hip.stream())
        torch.cuda.synchronize()
        n_next = int(n_out.item())
        ref.update(rays_t=raw(rays_t).copy(), n_next=n_next, list_next=out.cpu().numpy()[:n_next].copy())
        lp.check_after(it, ref)
        snaps.append(ref)
        hist.append(n_alive)
        live_total += live.size
        slots += M
        alive, n_alive, step = out, n_next, step + n_step
    over = n_alive == 0 or step >= MAX_STEPS
    hist.append(0 if over else n_alive)
    end = dict(image=raw(image).copy(), depth=raw(depth).copy(), weights_sum=raw(ws).copy(), hist=hist, counters=[len(snaps), live_total, slots], over=over)
    lp.check_end(end)
    return snaps, end


def run_grouped(net, sc, box, snaps, end, group, coop=False, live_list=True):
    """The same frame with `group` iterations per call: every iteration of a call but its first is marched by the compaction
    (k_head_compact<true>; k_head_step<true> with coop), and the samples a call leaves behind are its last iteration's."""
    from radnerf_hip import abi
    lp = Loop(net, sc, box, live_list)
    lp.begin()
    n = len(snaps)
    for first in range(0, n, group):
        cnt = min(group, n - first)
        flags = (abi.RN_LOOP_FIRST_MARCHED if first == 0 else 0) | (abi.RN_LOOP_COOP if coop else 0)
        if first + cnt == n and end["over"]:
            flags |= abi.RN_LOOP_CLOSE_FRAME
        lp.iterate(first, cnt, flags)
        last = first + cnt - 1
        if not (flags & abi.RN_LOOP_CLOSE_FRAME):       # (closing the frame zeroes the live-sample counters check_samples reads)
            lp.check_samples(last, snaps[last])
        lp.check_after(last, snaps[last])
    lp.check_end(end)
    assert lp.get("state")[abi.RN_HEAD_ST_UNFINISHED] == 0


def mixed_wave(snap):
    """Does a wave of this iteration hold a ray that emits nothing, one that emits some and one that emits all n_step samples?"""
    k, per_ray = snap["n_step"], snap["per_ray"]
    return k > 1 and any((w == 0).any() and (w == k).any() and ((w > 0) & (w < k)).any() for w in np.split(per_ray, range(64, per_ray.size, 64)))


def _box_of(sc):
    import radnerf_hip as hip
    box = torch.zeros(8, dtype=torch.int32, device=DEV)
    hip.call("rn_occ_box", hip.ptr(t(sc.bits)), 1, H, hip.ptr(box), hip.stream())
    torch.cuda.synchronize()
    return box


@pytest.mark.parametrize("name", sorted(CASES))
def test_loop_rows_equal_the_per_operator_chain(hiplib, net, name):
    sc = scene_of(name)
    box = _box_of(sc)
    snaps, end = chain_and_single(net, sc, box)
    assert snaps[1]["n_alive"] == sc.alive and snaps[1]["n_step"] == min(sc.N // sc.alive, 8)
    if CASES[name][3]:                                   # the first workgroup of iteration 1's compaction keeps nothing, the others do
        assert snaps[1]["n_next"] > 0 and not np.isin(snaps[1]["list_next"], sc.hit_rays[:256]).any()
    if name == "n7_a513_thin":                           # rays that emit none, some and all of their n_step samples within one wave
        assert any(mixed_wave(s) for s in snaps[2:])
    for group in (2, 3, len(snaps)):                     # a call's last iteration is checked row by row: 1, 3, ..; 2, 5, ..; the last one
        run_grouped(net, sc, box, snaps, end, group)


@pytest.mark.parametrize("name", ["n3_a256", "n7_a513_thin", "n6_a63_plain"])
def test_without_the_box_and_without_a_live_list(hiplib, net, name):
    sc = scene_of(name)
    for box, live_list in ((None, True), (_box_of(sc), False), (None, False)):
        snaps, end = chain_and_single(net, sc, box, live_list)
        run_grouped(net, sc, box, snaps, end, 2, live_list=live_list)
        run_grouped(net, sc, box, snaps, end, len(snaps), live_list=live_list)


def test_one_launch_loop_step(hiplib, net):
    """RN_LOOP_COOP: k_head_step<true> shares the compaction's march."""
    sc = scene_of("n7_a513_thin")
    box = _box_of(sc)
    snaps, end = chain_and_single(net, sc, box)
    run_grouped(net, sc, box, snaps, end, 2, coop=True)
    run_grouped(net, sc, box, snaps, end, len(snaps), coop=True)
