"""The occupied box on the GPU: rn_occ_box against numpy, and the inference loop with rn_head_t.occ_box against the same loop with
NULL -- every marcher of csrc/rn_head_loop.hip (k_frame_begin, k_head_march, k_head_compact<true>, k_head_step<true>).

Bar: bit equality (the raw 32-bit words) between the two loops, iteration by iteration: the live-slot lists (as sets: their order is
the workgroups' arrival order), xyzs / dirs / deltas on the live slots, both alive lists, the state words, and at the end image,
depth, weights_sum, the per-iteration live-ray counts (RN_HEAD_ST_HIST) and the iteration / sample counters.  Scenes: every family
of tests/walk_cases.py, and camera views (at most 96 x 96 rays) of the synthetic head, a blob touching a face of the box, two
blobs, a camera inside the occupied box, the diagonal views, a two-cascade model.  tests/test_occ_box.py holds the CPU argument.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import occ_box_cases as ob
import walk_cases as wc

pytestmark = pytest.mark.gpu

DEV = "cuda"


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def raw(x):
    """The raw words of a tensor: float32 compared as int32, so NaNs and signed zeros count."""
    a = x.detach().cpu().numpy()
    return a.view(np.int32) if a.dtype == np.float32 else a


# ------------------------------------------------------------------------------------------------ rn_occ_box

def _grids():
    from radnerf.scene import ellipsoid_bitfield
    return {
        "ellipsoid": (ellipsoid_bitfield(128, 1.0, (0.40, 0.42, 0.40))[0], 1, 128),
        "empty": (np.zeros(128 ** 3 // 8, np.uint8), 1, 128),
        "full": (np.full(128 ** 3 // 8, 255, np.uint8), 1, 128),
        "cell_0": (ob.bits_from_cells([[0, 0, 0]], 128), 1, 128),
        "cell_top": (ob.bits_from_cells([[127, 127, 127]], 128), 1, 128),
        "h64": (ob.blob_bits(64, (0.3, -0.2, 0.1), (0.2, 0.3, 0.25)), 1, 64),
        # the box is cascade 0's: bits of the second cascade do not widen it
        "two_cascades": (np.concatenate([ob.bits_from_cells([[5, 100, 7], [9, 3, 64]], 128), np.full(128 ** 3 // 8, 255, np.uint8)]), 2, 128),
    }


@pytest.mark.parametrize("name", ["ellipsoid", "empty", "full", "cell_0", "cell_top", "h64", "two_cascades"])
def test_occ_box_matches_numpy(hiplib, name):
    import radnerf_hip as hip
    bits, Cc, H = _grids()[name]
    want = ob.box_words(bits, H)
    if name == "empty":
        assert want.tolist() == [H, H, H, -1, -1, -1, 0, 0]
    if name == "cell_top":
        assert want.tolist() == [127] * 6 + [0, 0]
    g = t(bits)
    box = torch.full((8,), 77, dtype=torch.int32, device=DEV)
    for _ in range(2):                                     # a rebuild into a used box starts over
        hip.call("rn_occ_box", hip.ptr(g), Cc, H, hip.ptr(box), hip.stream())
        torch.cuda.synchronize()
        assert box.cpu().numpy().tolist() == want.tolist()


# ------------------------------------------------------------------------------------------------ the loop, with and without

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


class Scene:
    def __init__(self, o, d, bits, bound=1.0, C=1, H=128, max_steps=16, dt_gamma=1 / 256):
        self.o, self.d, self.bits = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32), bits
        self.bound, self.C, self.H, self.max_steps, self.dt_gamma = float(bound), C, H, max_steps, dt_gamma
        self.N = self.o.shape[0]


def _camera(yaw, pitch, fovy, size=96, radius=3.35):
    from radnerf.rays import get_rays, intrinsics_from_fovy, orbit_pose
    pose = torch.from_numpy(orbit_pose(radius, yaw, pitch))[None]
    r = get_rays(pose, intrinsics_from_fovy(size, size, fovy), size, size, -1)
    return r["rays_o"][0].numpy(), r["rays_d"][0].numpy()


def _scene(name, po):
    from radnerf.scene import ellipsoid_bitfield
    head = ellipsoid_bitfield(128, 1.0, (0.40, 0.42, 0.40))[0]
    if name in wc.FAMILIES:
        c = wc.family(name, po)
        return Scene(c.o, c.d, c.bits, *c.march_args[:1], C=c.C, H=c.H, max_steps=c.max_steps, dt_gamma=c.dt_gamma)
    if name == "head":
        return Scene(*_camera(6.0, -3.0, 21.24), head)
    if name == "blob_on_a_face":                       # cells up to x = H - 1 and down to z = 0: two sides of the box have no face
        return Scene(*_camera(20.0, 10.0, 40.0), ob.blob_bits(128, (0.85, 0.1, -0.9), (0.16, 0.3, 0.2)))
    if name == "two_blobs":
        bits = ob.blob_bits(128, (-0.5, 0.2, 0.0), (0.2, 0.2, 0.2)) | ob.blob_bits(128, (0.45, -0.3, 0.3), (0.15, 0.25, 0.2))
        return Scene(*_camera(-10.0, 5.0, 35.0), bits)
    if name == "camera_inside":
        rng = np.random.default_rng(5)
        d = rng.standard_normal((96 * 96, 3))
        d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
        d[:300] = np.eye(3, dtype=np.float32)[rng.integers(0, 3, 300)] * rng.choice([-1.0, 1.0], (300, 1)).astype(np.float32)   # axis-parallel
        return Scene(np.tile(np.float32([[0.05, 0.1, -0.1]]), (d.shape[0], 1)), d, head)
    if name.startswith("diagonal_view"):               # the optical axis on / beside the cube's diagonal: rays on both sides of the 0.58 seam
        pitch = math.degrees(math.asin(1 / math.sqrt(3)))
        return Scene(*_camera(45.0 + float(name[-2:]), pitch, 4.0), head)
    if name == "two_cascade_model":                    # C = 2, constant dt: the span must be inert
        rng = np.random.default_rng(6)
        bits = np.concatenate([head, rng.integers(0, 256, 128 ** 3 // 8).astype(np.uint8) & rng.integers(0, 256, 128 ** 3 // 8).astype(np.uint8)])
        return Scene(*_camera(6.0, -3.0, 30.0), bits, bound=2.0, C=2)
    raise KeyError(name)


SCENES = tuple(wc.FAMILIES) + ("head", "blob_on_a_face", "two_blobs", "camera_inside", "diagonal_view+0", "diagonal_view+1", "diagonal_view-1",
                               "two_cascade_model")


def _loop(net, sc, box, mode):
    """One frame of the loop through the C ABI; returns the list of snapshots (dicts of numpy arrays).
    mode: "whole"   rn_frame_begin + one rn_head_iterate_ex for all iterations (k_frame_begin, k_head_compact<true>)
          "coop"    the same with RN_LOOP_COOP (k_head_step<true>)
          "pairs"   two iterations per call: the samples left behind are those k_head_compact<true> marched
          "single"  one iteration per call: k_head_march marches every iteration but the first"""
    import radnerf_hip as hip
    from radnerf_hip import abi
    st = net["st"]
    N = sc.N
    o, d, bits = t(sc.o), t(sc.d), t(sc.bits)
    aabb = t(np.array([-sc.bound] * 3 + [sc.bound] * 3, np.float32))
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=DEV)
    bufs = dict(nears=z(N), fars=z(N), weights_sum=z(N), depth=z(N), image=z(N, 3), rays_t=z(N), xyzs=z(N, 3), dirs=z(N, 3), deltas=z(N, 2),
                sigmas=z(N), rgbs=z(N, 3), rays_alive_a=z(N, dtype=torch.int32), rays_alive_b=z(N, dtype=torch.int32),
                state=z(abi.RN_HEAD_STATE_INTS, dtype=torch.int32), block_counts=z(3 * ((N + 255) // 256 + 1), dtype=torch.int32),
                live_slots=z(N, dtype=torch.int32))
    h = abi.HeadT(rays_o=hip.ptr(o), rays_d=hip.ptr(d), N=N, aabb=hip.ptr(aabb), min_near=wc.MIN_NEAR, bitfield=hip.ptr(bits), bound=sc.bound,
                  dt_gamma=sc.dt_gamma, max_steps=sc.max_steps, cascade=sc.C, grid_size=sc.H, T_thresh=1e-4, order_w=0,
                  occ_box=hip.ptr(box), **{k: hip.ptr(v) for k, v in bufs.items()})
    iters = min(sc.max_steps, 16)                     # the loop's step grows by n_step >= 1 per iteration: 16 cover max_steps = 16; beyond, a prefix

    def iterate(first, n, flags):
        hip.call("rn_head_iterate_ex", C.byref(h), C.byref(st.gx), C.byref(st.gw), hip.ptr(st.packed), hip.ptr(net["bias"]), first, n,
                 st.mlp_dtype, flags, hip.stream())

    def snap(it):
        """What iteration `it` left behind: its state bank, its samples on the live slots, its live list, both alive lists."""
        torch.cuda.synchronize()
        state = bufs["state"].cpu().numpy().copy()
        bank = state[(it & 1) * 8:(it & 1) * 8 + 8]
        out = dict(bank=bank[:5].copy(), alive_a=raw(bufs["rays_alive_a"]).copy(), alive_b=raw(bufs["rays_alive_b"]).copy(),
                   rays_t=raw(bufs["rays_t"]).copy())
        if bank[4]:
            M = int(bank[3])
            dl = raw(bufs["deltas"])[:M]
            live = np.nonzero(bufs["deltas"][:M, 0].cpu().numpy() != 0)[0]
            out.update(live=live, deltas=dl[live].copy(), xyzs=raw(bufs["xyzs"])[:M][live].copy(), dirs=raw(bufs["dirs"])[:M][live].copy())
            if mode != "coop" and mode != "whole":
                # the marchers' list holds exactly the live slots (any order); its count stays in the bank until the frame closes
                assert np.array_equal(np.sort(bufs["live_slots"].cpu().numpy()[:int(bank[6])]), live)
        return out

    snaps = []
    hip.call("rn_frame_begin", C.byref(h), None, 0.0, 0.0, 0.0, 0.0, 0, hip.stream())
    snaps.append(snap(0))
    if mode in ("whole", "coop"):
        flags = abi.RN_LOOP_FIRST_MARCHED | abi.RN_LOOP_CLOSE_FRAME | (abi.RN_LOOP_COOP if mode == "coop" else 0)
        iterate(0, iters, flags)
    elif mode == "pairs":
        for it in range(0, iters, 2):
            iterate(it, 2, abi.RN_LOOP_FIRST_MARCHED if it == 0 else 0)
            snaps.append(snap(it + 1))
    else:
        for it in range(iters):
            iterate(it, 1, abi.RN_LOOP_FIRST_MARCHED if it == 0 else 0)
            snaps.append(snap(it))
    torch.cuda.synchronize()
    state = bufs["state"].cpu().numpy()
    snaps.append(dict(image=raw(bufs["image"]), depth=raw(bufs["depth"]), weights_sum=raw(bufs["weights_sum"]), nears=raw(bufs["nears"]),
                      fars=raw(bufs["fars"]), hist=state[abi.RN_HEAD_ST_HIST:].copy(), counters=state[abi.RN_HEAD_ST_ITERS:abi.RN_HEAD_ST_UNFINISHED + 1].copy(),
                      stalled=state[abi.RN_HEAD_ST_STALLED:abi.RN_HEAD_ST_STALLED + 1].copy()))
    return snaps


def _same(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.keys() == y.keys(), i
        for k in x:
            assert x[k].shape == y[k].shape and np.array_equal(x[k], y[k]), (i, k)


def _box_of(sc):
    import radnerf_hip as hip
    g = t(sc.bits)
    box = torch.zeros(8, dtype=torch.int32, device=DEV)
    hip.call("rn_occ_box", hip.ptr(g), sc.C, sc.H, hip.ptr(box), hip.stream())
    torch.cuda.synchronize()
    assert box.cpu().numpy().tolist() == ob.box_words(sc.bits, sc.H).tolist()
    return box


@pytest.mark.parametrize("name", SCENES)
def test_loop_with_the_box_equals_the_loop_without(po, hiplib, net, name):
    sc = _scene(name, po)
    assert sc.N <= 96 * 96
    box = _box_of(sc)
    use, _, _ = ob.span(sc.o, sc.d, *ob.box_of(sc.bits, sc.H), sc.H, sc.bound, sc.C,
                        wc.Case("x", sc.o, sc.d, sc.bound, sc.C, sc.H, sc.max_steps).dt_min, wc.Case("x", sc.o, sc.d, sc.bound, sc.C, sc.H, sc.max_steps).dt_max)
    if name in ("two_cascade_model", "casc2", "casc3", "casc3_rec", "vardt_c1", "short", "needles"):
        assert not use.any()
    if name in ("head", "blob_on_a_face", "two_blobs", "plus_y"):
        assert use.all()
    if name == "camera_inside":                        # random directions: a few per cent lie within 0.58 of a diagonal
        assert use.sum() > 0.9 * sc.N and use[:300].all()
    if name.startswith("diagonal"):
        assert use.sum() >= 30 and (~use).sum() >= 30
    sampled = False
    for mode in ("whole", "pairs", "single", "coop"):
        with_box, without = _loop(net, sc, box, mode), _loop(net, sc, None, mode)
        _same(with_box, without)
        end = with_box[-1]
        assert end["counters"][3] == 0 or sc.max_steps > 16          # no frame flagged unfinished where all iterations were enqueued
        assert end["stalled"][0] == 0
        sampled = sampled or end["counters"][1] > 0
    assert sampled or name == "degenerate"


# ------------------------------------------------------------------------------------------------ FusedState keeps the box current

def _frame(scene):
    with torch.no_grad():
        out = scene.render(0)
    torch.cuda.synchronize()
    return {k: raw(out[k]).copy() for k in ("image", "depth")}, dict(scene.model.last_stats)


def test_fused_state_rebuilds_the_box_when_the_bitfield_changes(hiplib, monkeypatch):
    from radnerf import fused
    from radnerf.scene import SyntheticScene, default_opt
    scene = SyntheticScene(H=64, W=64, n_frames=8, device=DEV, opt=default_opt(engine="fused", smooth_lips=False))
    m = scene.model
    _frame(scene)
    st = fused._state(m)
    assert st.box_builds == 1
    _frame(scene)
    assert st.box_builds == 1                                            # same grid: built once
    assert st.box.cpu().numpy().tolist() == ob.box_words(m.density_bitfield.cpu().numpy(), 128).tolist()
    # an in-place edit: a second blob outside the first box
    extra = t(ob.blob_bits(128, (0.0, 0.75, -0.5), (0.15, 0.15, 0.2)))
    with torch.no_grad():
        m.density_bitfield.bitwise_or_(extra)
    got, stats = _frame(scene)
    assert st.box_builds == 2
    assert st.box.cpu().numpy().tolist() == ob.box_words(m.density_bitfield.cpu().numpy(), 128).tolist()
    monkeypatch.setenv("RN_OCC_BOX", "0")
    want, stats0 = _frame(scene)
    assert st.box_builds == 2
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert stats == stats0 and stats["live_samples"] > 0


def test_fused_state_rebuilds_the_box_after_a_grid_refresh(hiplib, monkeypatch):
    """update_extra_state rewrites the bitfield through its address; the refresh moves its version, so the next frame has a new box."""
    from radnerf import fused
    from radnerf.scene import SyntheticScene, default_opt
    scene = SyntheticScene(H=64, W=64, n_frames=8, device=DEV, opt=default_opt(engine="fused", smooth_lips=False, torso=False))
    m = scene.model
    m.aud_features = scene.aud_features
    m.eye_area = torch.full((scene.n_frames, 1), 0.25, device=DEV)
    _frame(scene)
    st = fused._state(m)
    assert st.box_builds == 1
    with torch.no_grad():
        m.density_grid.zero_()
        m.update_extra_state()
    got, stats = _frame(scene)
    assert st.box_builds == 2
    assert st.box.cpu().numpy().tolist() == ob.box_words(m.density_bitfield.cpu().numpy(), 128).tolist()
    monkeypatch.setenv("RN_OCC_BOX", "0")
    want, stats0 = _frame(scene)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert stats == stats0
