"""The rays' direction terms (rn_head_t.dir_term, RN_DIR_TERM): the fp32 network launch of loop iteration 0 stores the colour
net's first-layer accumulators after the bias and the SH(dir) steps per ray, the launches of the later iterations load them.

Bar: torch.equal on image, depth and weights_sum between a frame with the buffer and the same frame without it (RN_DIR_TERM=0,
or dir_term = NULL in the descriptor).  Scenes: the synthetic head, xyz hash grid with T = 2^14, max_steps = 16; a 64 x 64 frame
(4 096 rays, the alive list starts in 8 x 8 pixel blocks) and a 40 x 24 frame (960 rays: no multiple of 256, partial tiles), the
latter handed to the loop without an image width, so that its list starts in ray order (order_w = 0); the scene's own sigma row
(no ray ends on opacity), the row x 80 (bench.py's regime A: rays end on T < T_thresh, most of them within the second iteration) and
the row x 30 (rays end in different iterations, the lists shrink unevenly).
Every frame with the buffer starts from a buffer full of NaN: a row that is read before the frame wrote it shows.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
KEYS = ("image", "depth", "weights_sum")
SHAPES = {"64x64": (64, 64, True), "40x24": (24, 40, False)}      # H, W, hand the image width to the loop
_SCENES, _OFF = {}, {}


def _scene(shape):
    from radnerf.scene import SyntheticScene, default_opt
    if shape not in _SCENES:
        H, W, ordered = SHAPES[shape]
        torch.manual_seed(0)
        sc = SyntheticScene(H=H, W=W, n_frames=8, device=DEV,
                            opt=default_opt(engine="fused", xyz_grid="hashgrid", xyz_log2_hashmap_size=14, smooth_lips=False, max_steps=16))
        if not ordered:
            sc.model.ray_order_width = 0
        _SCENES[shape] = sc
    return _SCENES[shape]


class _sigma_row:
    """The sigma net's output row as the scene has it ("own") or made positive and x 80 ("x80", bench.py's regime A) / x 30 ("x30")."""

    def __init__(self, model, which):
        self.row, self.which = model.sigma_net.net[-1].weight, which

    def __enter__(self):
        self.keep = self.row.detach().clone()
        if self.which != "own":
            with torch.no_grad():
                self.row[0].abs_().mul_(float(self.which[1:]))

    def __exit__(self, *exc):
        with torch.no_grad():
            self.row.copy_(self.keep)


def _frame(scene, i, monkeypatch, on, poison=True):
    """Frame i through model.render -> what fused.render_frame returned (clones of KEYS) and the loop's statistics."""
    from radnerf import fused
    got = {}
    orig = fused.render_frame

    def spy(*a, **k):
        out = orig(*a, **k)
        got.update(out)
        return out

    monkeypatch.setenv("RN_DIR_TERM", "1" if on else "0")
    st = fused._state(scene.model)
    if on and poison:
        assert st._N                                          # the switch-off frame before this one made the state's scratch
        st.dir_terms().fill_(float("nan"))                    # allocated on first use with the switch on
    with monkeypatch.context() as mp:
        mp.setattr(fused, "render_frame", spy)
        with torch.no_grad():
            scene.render(i)
    torch.cuda.synchronize()
    return {k: got[k].clone() for k in KEYS}, dict(scene.model.last_stats)


def _off(shape, row, i, monkeypatch):
    """The frame without direction terms, rendered once per (shape, sigma row, frame) and shared."""
    key = (shape, row, i)
    if key not in _OFF:
        scene = _scene(shape)
        with _sigma_row(scene.model, row):
            _OFF[key] = _frame(scene, i, monkeypatch, on=False)
    return _OFF[key]


def _equal(got, want):
    for k in KEYS:
        assert bool(torch.isfinite(got[k]).all()), k
        assert torch.equal(got[k], want[k]), k


@pytest.mark.parametrize("row", ["own", "x30", "x80"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_frame_with_direction_terms_equals_the_frame_without(hiplib, monkeypatch, shape, row):
    """Frame shapes x sigma rows, from a poisoned buffer: finite and equal -- every ray alive after iteration 0 wrote its row first."""
    from radnerf import fused
    scene = _scene(shape)
    want, stats0 = _off(shape, row, 0, monkeypatch)
    with _sigma_row(scene.model, row):
        got, stats = _frame(scene, 0, monkeypatch, on=True)
    st = fused._state(scene.model)
    assert st.dir_term is not None and tuple(st.dir_term.shape) == (scene.H * scene.W, 64)
    _equal(got, want)
    assert stats == stats0 and stats["iterations"] >= (3 if row == "own" else 2) and stats["live_samples"] > 0   # some launch loaded rows
    assert bool(torch.isnan(st.dir_term).any()) and bool(torch.isfinite(st.dir_term).any())   # rows of rays that hit were written, no others
    if row == "x80":
        assert stats["live_samples"] < _off(shape, "own", 0, monkeypatch)[1]["live_samples"]   # rays did end on opacity


def test_buffer_reuse_two_frames_in_a_row(hiplib, monkeypatch):
    """Two frames with different poses and audio through one buffer, no poison in between: the second frame equals its own
    switch-off frame, so its rows were rewritten and nothing of the frame before was read."""
    scene = _scene("64x64")
    want0, want3 = _off("64x64", "x30", 0, monkeypatch)[0], _off("64x64", "x30", 3, monkeypatch)[0]
    assert not torch.equal(want0["image"], want3["image"])
    with _sigma_row(scene.model, "x30"):
        got0 = _frame(scene, 0, monkeypatch, on=True)[0]
        got3 = _frame(scene, 3, monkeypatch, on=True, poison=False)[0]
    _equal(got0, want0)
    _equal(got3, want3)


# ------------------------------------------------------------------------------------------------ the loop through the C ABI

def _loop(scene, rays, mode, with_terms, schedule=None):
    """One frame's loop over `rays` (o, d: [N,3]) through the C ABI with dir_term = a NaN-filled buffer or NULL.
    mode "whole": rn_frame_begin + one rn_head_iterate_ex for all iterations; "single": one iteration per call (first_iter > 0);
    "band": rn_head_begin, then rn_head_reschedule with schedule = (schedule_N, live rays of the whole frame) before iteration 0,
    so that iteration 0 runs with n_step > 1, then one iteration per call.  Returns KEYS and the state words."""
    import radnerf_hip as hip
    from radnerf import fused
    from radnerf_hip import abi
    m = scene.model
    st = fused._state(m)
    st.refresh()
    torch.manual_seed(5)
    enc_a = torch.randn(m.audio_dim, device=DEV) * 0.1
    bias = fused._frame_bias(st, enc_a, scene.eye, m.individual_codes[0]).clone()
    o, d = rays[0].contiguous(), rays[1].contiguous()
    N = o.shape[0]
    R = 1 if schedule is None else 8                      # sample slots per ray the scratch has room for
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=DEV)
    bufs = dict(nears=z(N), fars=z(N), weights_sum=z(N), depth=z(N), image=z(N, 3), rays_t=z(N), xyzs=z(R * N, 3), dirs=z(R * N, 3),
                deltas=z(R * N, 2), sigmas=z(R * N), rgbs=z(R * N, 3), rays_alive_a=z(N, dtype=torch.int32), rays_alive_b=z(N, dtype=torch.int32),
                state=z(abi.RN_HEAD_STATE_INTS, dtype=torch.int32), block_counts=z(3 * ((N + 255) // 256 + 1), dtype=torch.int32),
                live_slots=z(R * N, dtype=torch.int32))
    terms = torch.full((N, 64), float("nan"), device=DEV) if with_terms else None
    h = abi.HeadT(rays_o=hip.ptr(o), rays_d=hip.ptr(d), N=N, aabb=hip.ptr(m.aabb_infer), min_near=float(m.min_near),
                  bitfield=hip.ptr(m.density_bitfield), bound=float(m.bound), dt_gamma=1 / 256, max_steps=16, cascade=int(m.cascade),
                  grid_size=int(m.grid_size), T_thresh=1e-4, order_w=0, occ_box=None, dir_term=hip.ptr(terms),
                  **{k: hip.ptr(v) for k, v in bufs.items()})

    def iterate(first, n, flags):
        hip.call("rn_head_iterate_ex", C.byref(h), C.byref(st.gx), C.byref(st.gw), hip.ptr(st.packed), hip.ptr(bias), first, n,
                 st.mlp_dtype, flags, hip.stream())

    extra = {}
    if mode == "band":
        total = torch.tensor([schedule[1]], dtype=torch.int32, device=DEV)
        hip.call("rn_head_begin", C.byref(h), hip.stream())
        hip.call("rn_head_reschedule", C.byref(h), 0xFFFFFFFF, int(schedule[0]), hip.ptr(total), hip.stream())   # the bank of iteration 0
        iterate(0, 1, 0)
        torch.cuda.synchronize()
        extra["bank0"] = bufs["state"][:8].cpu().numpy().copy()
        for it in range(1, 16):
            iterate(it, 1, 0)
    else:
        hip.call("rn_frame_begin", C.byref(h), None, 0.0, 0.0, 0.0, 0.0, 0, hip.stream())
        if mode == "whole":
            iterate(0, 16, abi.RN_LOOP_FIRST_MARCHED | abi.RN_LOOP_CLOSE_FRAME)
        else:
            for it in range(16):
                iterate(it, 1, abi.RN_LOOP_FIRST_MARCHED if it == 0 else 0)
    torch.cuda.synchronize()
    state = bufs["state"].cpu().numpy()
    out = {k: bufs[k].clone() for k in KEYS}
    return out, dict(extra, iterations=int(state[abi.RN_HEAD_ST_ITERS]), live=int(state[abi.RN_HEAD_ST_LIVE]), terms=terms)


def _rays(scene, rows=None):
    f = scene.frame(0)
    o, d = f["rays_o"].reshape(-1, 3), f["rays_d"].reshape(-1, 3)
    if rows is not None:
        o, d = o[rows[0] * scene.W:rows[1] * scene.W], d[rows[0] * scene.W:rows[1] * scene.W]
    return o, d


def test_one_iteration_per_call_and_null_equal_the_one_call_loop(hiplib):
    """first_iter > 0: the call that runs iteration it >= 1 on its own still reads what iteration 0's call stored; and the
    descriptor with dir_term = NULL renders the same frame."""
    scene = _scene("40x24")
    with _sigma_row(scene.model, "x30"):
        rays = _rays(scene)
        whole, info = _loop(scene, rays, "whole", True)
        single, info1 = _loop(scene, rays, "single", True)
        null, info0 = _loop(scene, rays, "whole", False)
    assert info["iterations"] >= 2 and info["live"] > 0
    assert info["iterations"] == info1["iterations"] == info0["iterations"] and info["live"] == info1["live"] == info0["live"]
    _equal(whole, null)
    _equal(single, whole)
    assert torch.equal(torch.isnan(info["terms"]), torch.isnan(info1["terms"]))
    assert torch.equal(torch.nan_to_num(info["terms"]), torch.nan_to_num(info1["terms"]))


def test_band_of_the_tile_workload_with_more_than_one_step_in_iteration_0(hiplib):
    """A band of the 64 x 64 frame whose schedule is the whole frame's (rn_head_reschedule): iteration 0 runs with n_step = 2, so a
    ray's row is stored by each of its live samples there (the same bytes).  The band is the frame's top rows, where fewer than half
    of the rays meet the head: its live samples of iteration 0 fit the N entries a network launch takes."""
    scene = _scene("64x64")
    rays = _rays(scene, rows=(0, 24))
    N = rays[0].shape[0]
    with _sigma_row(scene.model, "x30"):
        on, info = _loop(scene, rays, "band", True, schedule=(2 * N, N))
        off, info0 = _loop(scene, rays, "band", False, schedule=(2 * N, N))
    for i in (info, info0):
        assert i["bank0"][2] == 2 and i["bank0"][3] == 2 * N and 0 < i["bank0"][6] <= N       # n_step, slots, live samples of iteration 0
    assert info["iterations"] >= 2 and info["iterations"] == info0["iterations"] and info["live"] == info0["live"] > 0
    _equal(on, off)
    assert bool(torch.isfinite(info["terms"]).any())
