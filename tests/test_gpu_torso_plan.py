"""The torso plan (csrc/rn_torso.hip: rn_torso_plan_bytes, rn_torso_plan_build, rn_torso_blend_frame_planned) and its owner
(radnerf.fused.FusedState.torso_plan).

A planned frame runs the covered pixels as dense 32-pixel tiles whose position encoding was built once, and blends the rest in
pixel-range workgroups.  Held here: uncovered pixels are bit-equal to rn_torso_blend_frame in image, depth, uint8 frame,
background, alpha and deform; covered ones are within 5e-5 of it -- and, since the plan feeds the same products to the same
sums in the same order, bit-equal too -- and within 5e-5 of the fp32 C oracle (the bar of
test_gpu_fused.py::test_torso_fused_matches_oracle on the background, applied to alpha and deform as well); nothing is written
outside a buffer.  The occupancy grids are the tests' own, G = 16, 0 / 1 quadrants with every pixel drawn at least 0.1 inside
one (the bilinear test reads four equal nodes there), so a case decides which pixels are covered.

The owner: a plan is built on the second call with one key, a changed occupancy grid drops it, after a changed weight or grid
the next frame equals a frame that never saw a plan, a key that changes every call builds nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_options import _np

pytestmark = pytest.mark.gpu

G = 16
THRESH = 0.5
PAD = 64
BAR = 5e-5
_SCENES = {}


def _scene(ind=8):
    from radnerf.scene import SyntheticScene, default_opt
    if ind not in _SCENES:
        torch.manual_seed(0)
        _SCENES[ind] = SyntheticScene(H=16, W=16, n_frames=8, device="cuda",
                                      opt=default_opt(engine="fused", ind_dim_torso=ind, smooth_lips=False))
    return _SCENES[ind]


def _quadrants():
    g = torch.zeros(G, G, device="cuda")
    g[:G // 2, :G // 2] = 1
    g[G // 2:, G // 2:] = 1
    return g.reshape(-1).contiguous()


def _pixels(mask, gen):
    """One coordinate per entry of `mask`, at least 0.1 inside a quadrant of _quadrants() of that value (the quadrants meet
    between nodes 7 and 8 of 16: |coordinate| < 0.067)."""
    n = mask.numel()
    u = torch.rand(n, 2, device="cuda", generator=gen) * 0.8 + 0.1
    s = torch.where(torch.rand(n, device="cuda", generator=gen) < 0.5, -1.0, 1.0)
    return torch.stack([s * u[:, 0], torch.where(mask, s, -s) * u[:, 1]], 1).contiguous()


def _masks(N, gen):
    """(name, covered [N] bool, thresh): none / all (through thresh = -1: the mask then holds for any grid) / only the last
    pixel / a covered count of 32 k + 1."""
    z = torch.zeros(N, dtype=torch.bool, device="cuda")
    out = [("none", z.clone(), THRESH), ("all", ~z, -1.0)]
    last = z.clone()
    last[N - 1] = True
    out.append(("last", last, THRESH))
    k32 = 32 * ((N - 1) // 32) + 1              # 1, 1, 33, 193
    pick = z.clone()
    pick[torch.randperm(N, device="cuda", generator=gen)[:k32]] = True
    out.append((f"count{k32}", pick, THRESH))
    return out


class _Guard:
    def __init__(self):
        self.full = []

    def new(self, n, *tail, dtype=torch.float32, src=None):
        mark = 165 if dtype == torch.uint8 else -77.0
        full = torch.full((n + 2 * PAD, *tail), mark, dtype=dtype, device="cuda")
        view = full[PAD:PAD + n]
        if src is not None:
            view.copy_(src)
        elif dtype != torch.uint8:
            view.fill_(float("nan"))
        self.full.append((full, n, mark))
        return view

    def check(self):
        for full, n, mark in self.full:
            assert bool((full[:PAD] == mark).all()) and bool((full[PAD + n:] == mark).all()), "write outside the buffer"


def _grid_desc(m, st, half):
    """(rn_grid_t of the torso table, the tensor it points into)."""
    import radnerf_hip as hip
    from radnerf import fused
    if not half:
        return st.gt, st.tables[2]
    table = hip.aligned(m.torso_encoder.embeddings.detach().half())
    return fused._grid_desc(m.torso_encoder, table), table


def _frame_inputs(N, gen):
    """What the head loop leaves for the epilogue: image, weights_sum, depth, nears, fars."""
    r = lambda *s: torch.rand(*s, device="cuda", generator=gen)   # noqa: E731
    nears = r(N) + 0.5
    return dict(image=r(N, 3) * 0.6, weights_sum=r(N), depth=r(N) * 2 + 0.3, nears=nears, fars=nears + 0.5 + r(N))


def _run(m, st, gt, xy, grid, thresh, poses, ct, bg, fr, planned, want):
    """rn_torso_blend_frame (+ rn_torso_fused for deform), or the planned call over a plan built here, on guarded copies.
    `want`: which nullable outputs are handed in.  Returns the tensors written (None where not asked for) and n_on."""
    import radnerf_hip as hip
    n = xy.shape[0]
    gd = _Guard()
    coords = gd.new(n, 2, src=xy)
    bg_in = gd.new(n, 3, src=bg) if bg is not None else None
    image, depth = gd.new(n, 3, src=fr["image"]), gd.new(n, src=fr["depth"])
    ws, nears, fars = gd.new(n, src=fr["weights_sum"]), gd.new(n, src=fr["nears"]), gd.new(n, src=fr["fars"])
    bg_out = gd.new(n, 3) if "bg" in want else None
    alpha = gd.new(n) if "alpha" in want else None
    deform = gd.new(n, 2) if "deform" in want else None
    u8 = gd.new(n, 3, dtype=torch.uint8) if "u8" in want else None
    p6 = poses.reshape(-1).contiguous().float()
    shrink = float(m.opt.torso_shrink)
    tail = (hip.ptr(image), hip.ptr(ws), hip.ptr(depth), hip.ptr(nears), hip.ptr(fars), hip.ptr(u8), hip.stream())
    n_on = None
    if planned:
        cnt = C.c_uint32(0xFFFFFFFF)
        nbytes = int(hip._lib.rn_torso_plan_bytes(n, 0))
        plan = gd.new(nbytes + 512, dtype=torch.uint8)
        plan = plan[(-plan.data_ptr()) % 256:][:nbytes]
        hip.call("rn_torso_plan_build", hip.ptr(coords), n, hip.ptr(grid), G, float(thresh), shrink, hip.ptr(plan), nbytes,
                 C.byref(cnt), hip.stream())
        n_on = int(cnt.value)
        need = int(hip._lib.rn_torso_plan_bytes(n, n_on))
        assert need == nbytes + ((n_on + 31) // 32) * 21 * 64 * 4
        if need > nbytes:
            plan = gd.new(need + 512, dtype=torch.uint8)
            plan = plan[(-plan.data_ptr()) % 256:][:need]
            hip.call("rn_torso_plan_build", hip.ptr(coords), n, hip.ptr(grid), G, float(thresh), shrink, hip.ptr(plan), need,
                     C.byref(cnt), hip.stream())
            assert int(cnt.value) == n_on
        hip.call("rn_torso_blend_frame_planned", hip.ptr(plan), plan.numel(), n, n_on, hip.ptr(p6), hip.ptr(ct), shrink, C.byref(st.tw),
                 hip.ptr(st.tpacked), C.byref(gt), hip.ptr(bg_in), hip.ptr(bg_out), hip.ptr(alpha), hip.ptr(deform), *tail)
    else:
        head = (hip.ptr(coords), n, hip.ptr(grid), G, float(thresh), hip.ptr(p6), hip.ptr(ct), shrink, C.byref(st.tw),
                hip.ptr(st.tpacked), C.byref(gt), hip.ptr(bg_in))
        hip.call("rn_torso_blend_frame", *head, hip.ptr(bg_out), hip.ptr(alpha), *tail)
        if deform is not None:
            scratch = torch.empty(n, device="cuda")
            hip.call("rn_torso_fused", *head, None, hip.ptr(scratch), hip.ptr(deform), hip.stream())
    torch.cuda.synchronize()
    gd.check()
    out = dict(image=image, depth=depth, bg=bg_out, alpha=alpha, deform=deform, u8=u8)
    for k, v in out.items():
        assert v is None or v.dtype == torch.uint8 or bool(torch.isfinite(v).all()), k
    return {k: (v.clone() if v is not None else None) for k, v in out.items()}, n_on


def _compare(got, ref, mask, what):
    """Uncovered pixels bit-equal in everything; covered ones within BAR (uint8: one step) -- and then bit-equal as well; depth
    never depends on the torso.  Returns the largest difference on covered pixels."""
    worst = 0.0
    off = ~mask
    assert torch.equal(got["depth"], ref["depth"]), what
    for k in ("image", "bg", "alpha", "deform", "u8"):
        if ref[k] is None:
            assert got[k] is None
            continue
        assert torch.equal(got[k][off], ref[k][off]), (what, k, "uncovered pixels differ")
        if not bool(mask.any()):
            continue
        if k == "u8":
            assert int((got[k][mask].int() - ref[k][mask].int()).abs().max()) <= 1, (what, k)
        else:
            err = float((got[k][mask].double() - ref[k][mask].double()).abs().max())
            worst = max(worst, err)
            assert err <= BAR, (what, k, err)
        assert torch.equal(got[k], ref[k]), (what, k, "covered pixels differ in some bit")
    if got["alpha"] is not None:
        assert torch.equal(got["alpha"] > 0, mask), what
    return worst


def _oracle(po, om, xy, mask, poses, ct, bg):
    n = xy.shape[0]
    alpha, deform = np.zeros(n, np.float32), np.zeros((n, 2), np.float32)
    out = bg.cpu().numpy().copy() if bg is not None else np.ones((n, 3), np.float32)
    mk = mask.cpu().numpy()
    if mk.any():
        ea, ec, edx = po.torso_forward(om, xy.cpu().numpy()[mk], poses.cpu().numpy(), _np(ct))
        alpha[mk], deform[mk] = ea[:, 0], edx
        out[mk] = ec * ea + out[mk] * (1 - ea)
    return dict(alpha=alpha, deform=deform, bg=out)


ALL = ("bg", "alpha", "deform", "u8")


@pytest.mark.parametrize("N", [1, 31, 33, 197])
@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_planned_frame_against_the_unplanned_one_and_the_oracle(po, hiplib, N, half):
    """Every mask case at N below, at and above a 32-pixel tile and at several tiles with a ragged one; bg_in given and white; all
    nullable outputs, then none.  The oracle bar is held with the fp32 table (the oracle reads fp32 rows)."""
    from radnerf import fused
    scene = _scene()
    m = scene.model
    st = fused._state(m)
    st.refresh()
    gt, keep = _grid_desc(m, st, half)
    poses, ct = scene.poses6[0:1].contiguous(), m.individual_codes_torso[0].detach().contiguous()
    om = po.model_from_module(m)
    gen = torch.Generator(device="cuda").manual_seed(7 * N + int(half))
    grid = _quadrants()
    worst = 0.0
    for name, mask, thresh in _masks(N, gen):
        xy = _pixels(mask, gen)
        fr = _frame_inputs(N, gen)
        for bg, want in ((torch.rand(N, 3, device="cuda", generator=gen), ALL), (None, ALL), (None, ())):
            what = (name, "bg_in" if bg is not None else "white", want)
            ref, _ = _run(m, st, gt, xy, grid, thresh, poses, ct, bg, fr, False, want)
            got, n_on = _run(m, st, gt, xy, grid, thresh, poses, ct, bg, fr, True, want)
            assert n_on == int(mask.sum()), what
            worst = max(worst, _compare(got, ref, mask, what))
            if want and not half:
                orc = _oracle(po, om, xy, mask, poses, ct, bg)
                for k in ("alpha", "deform", "bg"):
                    err = float(np.abs(got[k].cpu().numpy().astype(np.float64) - orc[k]).max())
                    assert err <= BAR, (what, k, "oracle", err)
    del keep
    print(f"torso plan N={N} {'f16' if half else 'f32'}: max |planned - unplanned| on covered pixels = {worst:.3e}")


def test_plan_build_refuses_a_capturing_stream_and_a_short_buffer(hiplib):
    import radnerf_hip as hip
    from radnerf import fused
    scene = _scene()
    st = fused._state(scene.model)
    st.refresh()
    N = 33
    xy = torch.rand(N, 2, device="cuda") * 2 - 1
    grid = _quadrants()
    nbytes = int(hip._lib.rn_torso_plan_bytes(N, 0))
    plan = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    cnt = C.c_uint32(0)
    args = (hip.ptr(xy), N, hip.ptr(grid), G, THRESH, 1.0, hip.ptr(plan))
    with pytest.raises(RuntimeError, match="plan_bytes"):
        hip.call("rn_torso_plan_build", *args, nbytes - 1, C.byref(cnt), hip.stream())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            rc = hip._lib.rn_torso_plan_build(*args, nbytes, C.byref(cnt), side.cuda_stream)
    assert rc != 0 and "capturing" in hip.last_error()
    torch.cuda.current_stream().wait_stream(side)


# ======================================================================================================= the owner
def _render(scene, i=0):
    with torch.no_grad():
        out = scene.render(i, want_u8=True)
    torch.cuda.synchronize()
    return {k: out[k].clone() for k in ("image", "depth", "image_u8", "torso_alpha", "torso_color")}


def _fresh(scene, monkeypatch, i=0):
    """The frame as a build without plans renders it."""
    monkeypatch.setenv("RN_TORSO_PLAN", "0")
    out = _render(scene, i)
    monkeypatch.delenv("RN_TORSO_PLAN")
    return out


def _same_frame(got, ref):
    on = ref["torso_alpha"].reshape(-1) > 0
    assert bool(on.any()) and not bool(on.all())
    for k in ("image", "depth", "torso_color", "image_u8", "torso_alpha"):
        assert torch.equal(got[k], ref[k]), k


def test_state_builds_once_per_view_and_follows_weights_and_grid(hiplib, monkeypatch):
    from radnerf import fused
    monkeypatch.delenv("RN_TORSO_PLAN", raising=False)
    scene = _scene()
    m = scene.model
    st = fused._state(m)
    slot = st.cache.plan
    slot.forget()
    b0 = st.plan_builds
    _render(scene)                                   # first sight of the key: no build
    assert slot.held is None and st.plan_builds == b0
    got = _render(scene)                             # seen on the call before: built and used
    assert slot.held is not None and slot.held.buf is not None and st.plan_builds == b0 + 1 and slot.held.n_on > 0
    before = _fresh(scene, monkeypatch)
    _same_frame(got, before)
    _same_frame(_render(scene, 3), _fresh(scene, monkeypatch, 3))     # another pose, the same plan
    assert st.plan_builds == b0 + 1
    # a first-layer weight changed in place: nothing of it is in the plan, the frame equals a frame without plans
    w = m.torso_deform_net.net[0].weight
    keep_w = w.detach().clone()
    with torch.no_grad():
        w.mul_(1.25)
    try:
        got = _render(scene)
        ref = _fresh(scene, monkeypatch)
        _same_frame(got, ref)
        assert not torch.equal(ref["torso_color"], before["torso_color"]) and st.plan_builds == b0 + 1
    finally:
        with torch.no_grad():
            w.copy_(keep_w)
    # the occupancy grid changed: the plan goes, the frame is an unplanned one, the next call builds for the new grid
    keep_g = m.density_grid_torso.clone()
    m.density_grid_torso.view(m.grid_size, m.grid_size)[:, : m.grid_size // 2] = 1.0
    try:
        builds = st.plan_builds
        got = _render(scene)
        assert slot.held is None and st.plan_builds == builds
        ref = _fresh(scene, monkeypatch)
        _same_frame(got, ref)
        assert int((ref["torso_alpha"] > 0).sum()) > int((before["torso_alpha"] > 0).sum())
        got = _render(scene)
        assert st.plan_builds == builds + 1
        _same_frame(got, ref)
    finally:
        m.density_grid_torso.copy_(keep_g)
    # the switch: no plan is looked at
    monkeypatch.setenv("RN_TORSO_PLAN", "0")
    builds = st.plan_builds
    _render(scene), _render(scene), _render(scene)
    assert st.plan_builds == builds


def test_a_key_that_changes_every_call_builds_nothing(hiplib, monkeypatch):
    from radnerf import fused
    monkeypatch.delenv("RN_TORSO_PLAN", raising=False)
    scene = _scene()
    m = scene.model
    st = fused._state(m)
    slot = st.cache.plan
    slot.forget()
    builds = st.plan_builds
    keep = scene.bg_coords
    try:
        for i in range(4):                           # new coordinates every call, as a patch batch hands them over
            scene.bg_coords = keep + 1e-3 * (i + 1)
            _render(scene)
            assert slot.held is None
        scene.bg_coords = keep.clone()
        for i in range(4):                           # one buffer written in place between calls
            scene.bg_coords.add_(1e-4)
            _render(scene)
            assert slot.held is None
    finally:
        scene.bg_coords = keep
    assert st.plan_builds == builds
