"""The torso layer pinned at the level of the head (test_gpu_options.py::test_fused_head_against_float64): the inference
kernel k_torso_fused (csrc/rn_torso.hip: rn_torso_fused, rn_torso_blend_frame, rn_torso_mask) and the training branch
(NeRFNetwork.forward_torso under autograd, NeRFRenderer._torso_layer) against the float64 restatement
netref64.Net64.forward_torso, with the fp32 C oracle (pyoracle.torso_forward) as the second opinion.

The occupancy mask is the tests' own: density_grid_torso is filled with 0 / 1 quadrants (threshold 0.5) and every pixel is
drawn well inside a quadrant of the wanted value, so a test decides which lanes of which 64-pixel tile are covered: ragged
last tiles, a single covered lane, a covered lane only in the ragged tail.  Every buffer handed to the kernel is cut out of
a larger one whose margins must come back untouched.  rn_torso_mask, the kernel's coverage (alpha > 0) and
F.grid_sample(align_corners=True) > thresh agree on every pixel of every case.

Bars: with the scene's own weights the standing absolute ones (deform, alpha 3e-5, blended background 5e-5).  Where a fixed
number is not known (last deformation layer scaled until the clamp is active; fp16 table; gradients) the error against
float64 may be at most 4 x that of the reference formulation against float64, plus 1e-6: e <= 4 e_ref + 1e-6."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import netref64
from test_gpu_options import _maxerr, _np

pytestmark = pytest.mark.gpu

G = 128            # NeRFRenderer.grid_size: density_grid_torso is [G * G], flat index [y * G + x]
THRESH = 0.5
PAD = 64           # rows of margin on either side of every buffer the kernels see
# factor on torso_deform_net.net[-1].weight at which float64 alone clamps 10 % .. 90 % of the covered pixels (the unscaled
# nets clamp 0 % / 0 % / 1.6 % of uniform pixels); with these the float64 reference on the CPU clamps 44 % / 47 % / 44 % of the
# pixels the inference tests draw and 46 % / 48 % / 45 % of uniform ones; the tests that use them assert the share
CLAMP_K = {8: 20.0, 3: 10.0, 0: 3.0}
EDGE_N = [1, 63, 64, 65, 127, 128, 129, 257, 4097]
_SCENES = {}


def _scene(ind=8, engine="fused", **kw):
    from radnerf.scene import SyntheticScene, default_opt
    key = (ind, engine, tuple(sorted(kw.items())))
    if key not in _SCENES:
        torch.manual_seed(0)
        opt = default_opt(engine=engine, ind_dim_torso=ind, smooth_lips=False, **kw)
        _SCENES[key] = SyntheticScene(H=16, W=16, n_frames=8, device="cuda", opt=opt)
        assert _SCENES[key].model.individual_dim_torso == ind
    return _SCENES[key]


def _code(m, row=0):
    return m.individual_codes_torso[row].detach() if m.individual_dim_torso else None


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


# ------------------------------------------------------------------------------------------------ occupancy of the tests
def _quadrants(dev="cuda"):
    g = torch.zeros(G, G, device=dev)
    g[:G // 2, :G // 2] = 1
    g[G // 2:, G // 2:] = 1
    return g


@contextlib.contextmanager
def _occupancy(m, grid):
    """The model's torso occupancy replaced by `grid` [G, G] and its threshold by THRESH; both restored afterwards."""
    keep = (m.density_grid_torso.clone(), m.density_thresh_torso, m.mean_density_torso)
    m.density_grid_torso.copy_(grid.reshape(-1))
    m.density_thresh_torso, m.mean_density_torso = THRESH, 1.0
    try:
        yield
    finally:
        m.density_grid_torso.copy_(keep[0])
        m.density_thresh_torso, m.mean_density_torso = keep[1], keep[2]


@contextlib.contextmanager
def _scaled_deform(m, k):
    """torso_deform_net.net[-1].weight *= k (in place: the packed weight images follow the version counter); restored."""
    w = m.torso_deform_net.net[-1].weight
    keep = w.detach().clone()
    with torch.no_grad():
        w.mul_(k)
    try:
        yield
    finally:
        with torch.no_grad():
            w.copy_(keep)


def _pixels(mask, gen):
    """One coordinate per entry of `mask`, at least 0.1 (6 grid cells) inside a quadrant of _quadrants() of that value."""
    n, dev = mask.numel(), mask.device
    u = torch.rand(n, 2, device=dev, generator=gen) * 0.8 + 0.1
    s = torch.where(torch.rand(n, device=dev, generator=gen) < 0.5, -1.0, 1.0)
    return torch.stack([s * u[:, 0], torch.where(mask, s, -s) * u[:, 1]], 1).contiguous()


def _patterns(N, gen):
    """(name, mask [N]) of the covered-lane patterns that exist at this N."""
    tile = 64 * (((N - 1) // 64) // 2)            # a tile in the middle of the launch
    one = lambda i: torch.zeros(N, dtype=torch.bool, device="cuda").index_fill_(0, torch.tensor([i], device="cuda"), True)  # noqa: E731
    out = [("all", torch.ones(N, dtype=torch.bool, device="cuda")), ("none", torch.zeros(N, dtype=torch.bool, device="cuda")),
           ("lane0", one(tile))]
    if tile + 63 < N:
        out.append(("lane63", one(tile + 63)))
    if N % 64:
        out.append(("tail", one(N - 1)))          # the only covered lane sits in the ragged last tile
    out.append(("half", torch.rand(N, device="cuda", generator=gen) < 0.5))
    return out


# -------------------------------------------------------------------------------------------------------- guarded buffers
class _Guard:
    """Buffers cut out of larger ones: PAD rows of a marker on either side, which check() wants back untouched (an index one
    past the end lands in memory of the test's own)."""

    def __init__(self):
        self.full = []

    def new(self, n, *tail, dtype=torch.float32, src=None):
        mark = 165 if dtype == torch.uint8 else -77.0
        full = torch.full((n + 2 * PAD, *tail), mark, dtype=dtype, device="cuda")
        view = full[PAD:PAD + n]
        if src is not None:
            view.copy_(src)
        elif dtype != torch.uint8:
            view.fill_(float("nan"))              # an output: every element must be written
        self.full.append((full, n, mark))
        assert view.is_contiguous()
        return view

    def check(self):
        for full, n, mark in self.full:
            assert bool((full[:PAD] == mark).all()) and bool((full[PAD + n:] == mark).all()), "write outside the buffer"


def _launch(m, coords, poses, ct, bg_in, bg_out, alpha, deform, blend=None):
    """rn_torso_fused, or rn_torso_blend_frame with blend = (image, weights_sum, depth, nears, fars, u8)."""
    import radnerf_hip as hip
    from radnerf import fused
    st = fused._state(m)
    st.refresh()
    p6 = poses.reshape(-1).contiguous().float()
    head = (hip.ptr(coords), coords.shape[0], hip.ptr(m.density_grid_torso), int(m.grid_size), THRESH, hip.ptr(p6), hip.ptr(ct),
            float(m.opt.torso_shrink), C.byref(st.tw), hip.ptr(st.tpacked), C.byref(st.gt), hip.ptr(bg_in), hip.ptr(bg_out), hip.ptr(alpha))
    if blend is None:
        hip.call("rn_torso_fused", *head, hip.ptr(deform), hip.stream())
    else:
        assert deform is None
        hip.call("rn_torso_blend_frame", *head, *(hip.ptr(t) for t in blend), hip.stream())


def _coverage(m, coords, alpha, mask):
    """rn_torso_mask == the kernel's coverage == F.grid_sample(...) > thresh == the mask the test asked for."""
    import radnerf_hip as hip
    n = coords.shape[0]
    got = torch.full((n + 2 * PAD,), 165, dtype=torch.uint8, device="cuda")
    hip.call("rn_torso_mask", hip.ptr(coords), n, hip.ptr(m.density_grid_torso), int(m.grid_size), THRESH, hip.ptr(got[PAD:PAD + n]),
             hip.stream())
    assert bool((got[:PAD] == 165).all()) and bool((got[PAD + n:] == 165).all())
    occ = F.grid_sample(m.density_grid_torso.view(1, 1, G, G), coords.view(1, -1, 1, 2), align_corners=True).view(-1)
    want = occ > THRESH
    assert torch.equal(want, mask)
    assert torch.equal(got[PAD:PAD + n] != 0, want)
    assert torch.equal(alpha.reshape(-1) > 0, want)


def _run(m, xy, mask, poses, ct, bg):
    """The kernel on guarded copies of xy / bg: dict(alpha [N], deform [N, 2], bg [N, 3]); coverage and margins checked, and what
    holds on every uncovered pixel: alpha and deform exactly 0, background passed through bit for bit."""
    n = xy.shape[0]
    gd = _Guard()
    coords, bg_in = gd.new(n, 2, src=xy), gd.new(n, 3, src=bg)
    bg_out, alpha, deform = gd.new(n, 3), gd.new(n, 1), gd.new(n, 2)
    _launch(m, coords, poses, ct, bg_in, bg_out, alpha, deform)
    gd.check()
    out = dict(alpha=alpha.reshape(-1).clone(), deform=deform.clone(), bg=bg_out.clone())
    for v in out.values():
        assert bool(torch.isfinite(v).all())
    _coverage(m, coords, alpha, mask)
    un = ~mask
    assert int(torch.count_nonzero(out["alpha"][un])) == 0 and int(torch.count_nonzero(out["deform"][un])) == 0
    assert torch.equal(out["bg"][un], bg[un])
    return out


# ------------------------------------------------------------------------------------------------------------ references
def _truth(ref, xy, mask, poses, ct, bg):
    """float64: alpha [N], deform [N, 2] (0 where uncovered), bg = color * alpha + bg_in * (1 - alpha) on covered pixels."""
    n = xy.shape[0]
    alpha = torch.zeros(n, dtype=torch.float64, device=xy.device)
    deform = torch.zeros(n, 2, dtype=torch.float64, device=xy.device)
    out = bg.double().clone()
    idx = torch.nonzero(mask).reshape(-1)
    if idx.numel():
        with torch.no_grad():
            a, c, dx = ref.forward_torso(xy[idx], poses, ct)
        alpha[idx], deform[idx] = a[:, 0], dx
        out[idx] = c * a + out[idx] * (1 - a)
    return dict(alpha=alpha, deform=deform, bg=out)


def _oracle(po, om, xy, mask, poses, ct, bg):
    """The same from the fp32 C restatement (blend in fp32, as test_torso_kernel_code_widths has it)."""
    n = xy.shape[0]
    alpha, deform, out = np.zeros(n, np.float32), np.zeros((n, 2), np.float32), bg.cpu().numpy().copy()
    mk = mask.cpu().numpy()
    if mk.any():
        ea, ec, edx = po.torso_forward(om, xy.cpu().numpy()[mk], poses.cpu().numpy(), _np(ct))
        alpha[mk], deform[mk] = ea[:, 0], edx
        out[mk] = ec * ea + out[mk] * (1 - ea)
    return {k: torch.from_numpy(v).cuda() for k, v in (("alpha", alpha), ("deform", deform), ("bg", out))}


def _standing_bars(got, want, what):
    for key, bar in (("deform", 3e-5), ("alpha", 3e-5), ("bg", 5e-5)):
        err = float((got[key].double() - want[key].double()).abs().max())
        assert err <= bar, (what, key, err)


def _ratio_bars(got, ref, truth, sel, what, keys=("deform", "alpha", "bg")):
    """e <= 4 e_ref + 1e-6 per output, max-normalised, over the pixels `sel`; returns the worst e / e_ref."""
    worst = 0.0
    for key in keys:
        e, e_ref = _maxerr(got[key][sel], truth[key][sel]), _maxerr(ref[key][sel], truth[key][sel])
        print(f"torso {what} {key}: e {e:.3e}  e_ref {e_ref:.3e}  ratio {e / (e_ref + 1e-12):.2f}")
        assert e <= 4 * e_ref + 1e-6, (what, key, e, e_ref)
        worst = max(worst, e / (e_ref + 1e-12))
    return worst


def _poses(scene):
    return scene.poses6[0:1].contiguous()


# ===================================================================================================== inference kernel
@pytest.mark.parametrize("ind,N", [(8, n) for n in EDGE_N] + [(i, n) for i in (0, 3) for n in (65, 4097)])
def test_torso_kernel_tile_edges(po, hiplib, ind, N):
    """Every covered-lane pattern at N around the 64-pixel tile: covered pixels against float64 and the oracle at the standing
    bars, uncovered ones exactly passed through, nothing written outside [0, N)."""
    scene = _scene(ind)
    m, poses, ct = scene.model, _poses(scene), _code(scene.model)
    ref, om = netref64.Net64(m), po.model_from_module(m)
    gen = _gen(100 * ind + N)
    with _occupancy(m, _quadrants()):
        for name, mask in _patterns(N, gen):
            xy = _pixels(mask, gen)
            bg = torch.rand(N, 3, device="cuda", generator=gen)
            out = _run(m, xy, mask, poses, ct, bg)
            assert name == "half" or int(mask.sum()) == {"all": N, "none": 0}.get(name, 1)
            _standing_bars(out, _truth(ref, xy, mask, poses, ct, bg), (name, "float64"))
            _standing_bars(out, _oracle(po, om, xy, mask, poses, ct, bg), (name, "oracle"))


def _stride_n():
    """One launch is capped at 2 workgroups of 8 waves per CU: the first N at which waves take a second, ragged, round of tiles."""
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count * 8 * 64 + 65


def test_torso_kernel_grid_stride_loop(po, hiplib):
    scene = _scene(8)
    m, poses, ct = scene.model, _poses(scene), _code(scene.model)
    N = _stride_n()
    gen = _gen(5)
    mask = torch.rand(N, device="cuda", generator=gen) < 0.5
    xy = _pixels(mask, gen)
    bg = torch.rand(N, 3, device="cuda", generator=gen)
    with _occupancy(m, _quadrants()):
        out = _run(m, xy, mask, poses, ct, bg)                   # coverage and the uncovered-pixel rules: all N pixels
        idx = torch.cat([torch.arange(128, device="cuda"), torch.arange(N - 193, N, device="cuda"),
                         torch.randint(0, N, (4096,), device="cuda", generator=gen)])
        sub = {k: v[idx] for k, v in out.items()}
        _standing_bars(sub, _truth(netref64.Net64(m), xy[idx], mask[idx], poses, ct, bg[idx]), "float64")
        _standing_bars(sub, _oracle(po, po.model_from_module(m), xy[idx], mask[idx], poses, ct, bg[idx]), "oracle")


def _clamp_share(m, xy, mask, truth):
    """Among the covered pixels, by float64 alone: (clamped [n] -- some coordinate of x * shrink + dx beyond +-1 --, near [n] --
    some coordinate within 2e-5 of +-1, where fp32 and float64 may clamp differently), indices of the covered pixels."""
    idx = torch.nonzero(mask).reshape(-1)
    un = xy[idx].double() * float(np.float32(m.opt.torso_shrink)) + truth["deform"][idx]
    return (un.abs() > 1).any(1), ((un.abs() - 1).abs() < 2e-5).any(1), idx


@pytest.mark.parametrize("ind", [8, 3, 0])
def test_torso_kernel_with_the_clamp_active(po, hiplib, ind):
    """x = clamp(x + dx, -1, 1) with a last deformation layer k times as large: float64 clamps 10 % .. 90 % of the covered
    pixels.  A fixed bar is not known for these weights: e_kernel <= 4 e_oracle + 1e-6 against float64, per output."""
    scene = _scene(ind)
    m, poses, ct = scene.model, _poses(scene), _code(scene.model)
    N = 4097
    gen = _gen(40 + ind)
    mask = torch.rand(N, device="cuda", generator=gen) < 0.5
    xy = _pixels(mask, gen)
    bg = torch.rand(N, 3, device="cuda", generator=gen)
    with _occupancy(m, _quadrants()), _scaled_deform(m, CLAMP_K[ind]):
        out = _run(m, xy, mask, poses, ct, bg)
        truth = _truth(netref64.Net64(m), xy, mask, poses, ct, bg)
        orc = _oracle(po, po.model_from_module(m), xy, mask, poses, ct, bg)
    clamped, near, idx = _clamp_share(m, xy, mask, truth)
    share = float(clamped.double().mean())
    print(f"torso clamp ind={ind} k={CLAMP_K[ind]}: float64 clamps {100 * share:.1f} % of {idx.numel()} covered pixels, "
          f"{int(near.sum())} within 2e-5 of +-1")
    assert 0.10 <= share <= 0.90, share
    assert int(near.sum()) <= idx.numel() // 100
    worst = _ratio_bars(out, orc, truth, idx[~near], f"clamp ind={ind}")
    print(f"torso clamp ind={ind}: worst e / e_oracle = {worst:.2f}")


def _exact_nodes():
    """Interior grid nodes k whose coordinate 2 k / (G - 1) - 1, rounded to fp32, is mapped back to exactly k by grid_sample's
    ((x + 1) / 2) * (G - 1) in fp32."""
    k = np.arange(1, G - 1, dtype=np.float32)
    x = (np.float32(2) * k / np.float32(G - 1) - np.float32(1)).astype(np.float32)
    back = ((x + np.float32(1)) / np.float32(2)) * np.float32(G - 1)
    return [(int(a), float(b)) for a, b in zip(k[back == k], x[back == k])]


def test_torso_kernel_borders_and_threshold(po, hiplib):
    """Pixels at (+-1, +-1) and on every edge (the x1 == G / y1 == G branches of the bilinear occupancy), and pixels exactly on
    a grid node whose occupancy EQUALS the threshold: the test is a strict `>`, so they are uncovered."""
    scene = _scene(8)
    m, poses, ct = scene.model, _poses(scene), _code(scene.model)
    gen = _gen(77)
    grid = torch.ones(G, G, device="cuda")
    grid[0, 0] = THRESH                                      # the node of pixel (-1, -1)
    on_node = [(-1.0, -1.0)]
    nodes = _exact_nodes()
    if nodes:
        (k, x) = nodes[len(nodes) // 2]
        grid[k, k] = THRESH
        on_node.append((x, x))
    t = (torch.rand(64, device="cuda", generator=gen) * 1.9 - 0.95).tolist()
    edges = [(1.0, v) for v in t[:16]] + [(-1.0, v) for v in t[16:32]] + [(v, 1.0) for v in t[32:48]] + [(v, -1.0) for v in t[48:]]
    pts = on_node + [(1.0, 1.0), (1.0, -1.0), (-1.0, 1.0)] + edges
    xy = torch.tensor(pts, dtype=torch.float32, device="cuda")
    mask = torch.ones(len(pts), dtype=torch.bool, device="cuda")
    mask[:len(on_node)] = False
    bg = torch.rand(len(pts), 3, device="cuda", generator=gen)
    with _occupancy(m, grid):
        out = _run(m, xy, mask, poses, ct, bg)
        _standing_bars(out, _truth(netref64.Net64(m), xy, mask, poses, ct, bg), "float64")
        _standing_bars(out, _oracle(po, po.model_from_module(m), xy, mask, poses, ct, bg), "oracle")


@pytest.mark.parametrize("N", [65, 4097])
def test_torso_kernel_optional_pointers(hiplib, N):
    """bg_in == NULL is a white background; bg_out == NULL (alpha only) and deform == NULL change nothing else: bit for bit."""
    scene = _scene(8)
    m, poses, ct = scene.model, _poses(scene), _code(scene.model)
    gen = _gen(N)
    mask = torch.rand(N, device="cuda", generator=gen) < 0.5
    xy = _pixels(mask, gen)

    def call(bg, want_bg=True, want_deform=True):
        gd = _Guard()
        coords = gd.new(N, 2, src=xy)
        bg_in = gd.new(N, 3, src=bg) if bg is not None else None
        bg_out, alpha, deform = gd.new(N, 3) if want_bg else None, gd.new(N, 1), gd.new(N, 2) if want_deform else None
        _launch(m, coords, poses, ct, bg_in, bg_out, alpha, deform)
        gd.check()
        _coverage(m, coords, alpha, mask)
        return bg_out, alpha, deform
    with _occupancy(m, _quadrants()):
        white = call(torch.ones(N, 3, device="cuda"))
        none = call(None)
        assert all(torch.equal(a, b) for a, b in zip(white, none))
        bg = torch.rand(N, 3, device="cuda", generator=gen)
        full = call(bg)
        assert not torch.equal(full[0], white[0])
        alpha_only = call(bg, want_bg=False, want_deform=False)
        assert torch.equal(alpha_only[1], full[1])
        no_deform = call(bg, want_deform=False)
        assert torch.equal(no_deform[0], full[0]) and torch.equal(no_deform[1], full[1])


@pytest.mark.parametrize("N", [65, 4097])
def test_torso_kernel_fp16_table(po, hiplib, monkeypatch, N):
    """The __half instantiation.  Truth: float64 on the fp16-rounded table.  The margin is measured: the project's fp16 grid
    operator (bit-exact to the oracle, test_gpu_ops.py::test_grid_forward_fp16_bit_exact) on float64's clamped coordinates
    rounded to fp32, its features through the float64 torso net, gives e_op; e_kernel <= 4 e_op + 1e-6."""
    import radnerf_hip as hip
    from radnerf import fused
    scene = _scene(8, half_tables=True)
    m, poses, ct = scene.model, _poses(scene), _code(scene.model)
    enc = m.torso_encoder
    gen = _gen(16 + N)
    mask = torch.rand(N, device="cuda", generator=gen) < 0.5
    xy = _pixels(mask, gen)
    bg = torch.rand(N, 3, device="cuda", generator=gen)
    ref = netref64.Net64(m)
    ref.P["torso_encoder.embeddings"] = enc.embeddings.detach().half().double()

    def grid_op(x, table, e, bound):
        assert e is enc and bound == 1.0
        xn = ((x.detach().float() + 1) / 2).contiguous()                       # netref64.grid_encode's fp32 normalisation
        feat = torch.empty(xn.shape[0], 32, dtype=torch.half, device="cuda")
        half = enc.half_table()
        hip.call("rn_grid_encode_forward", hip.ptr(xn), hip.ptr(half), hip.ptr(enc.offsets), hip.ptr(feat), xn.shape[0], 2, 2, 16,
                 float(np.log2(enc.per_level_scale)), int(enc.base_resolution), None, int(enc.gridtype_id), 0, 0, hip.RN_F16,
                 hip.RN_LAYOUT_BLC, hip.stream())
        return feat.double()
    with _occupancy(m, _quadrants()):
        out = _run(m, xy, mask, poses, ct, bg)
        assert fused._state(m).gt.dtype == hip.RN_F16
        truth = _truth(ref, xy, mask, poses, ct, bg)
        monkeypatch.setattr(netref64, "grid_encode", grid_op)
        op = _truth(ref, xy, mask, poses, ct, bg)
    assert float((out["deform"].double() - truth["deform"]).abs().max()) <= 3e-5      # upstream of the table
    worst = _ratio_bars(out, op, truth, torch.nonzero(mask).reshape(-1), f"fp16 table N={N}", keys=("alpha", "bg"))
    print(f"torso fp16 table N={N}: worst e / e_op = {worst:.2f}")


@pytest.mark.parametrize("N", [63, 64, 65, 4097, "stride"])
def test_torso_blend_frame_equals_torso_then_blend(hiplib, N):
    """rn_torso_blend_frame (BLEND = true: the frame epilogue in the torso pass) against rn_torso_fused followed by
    rn_blend_frame on the same frame buffers: image, depth, the uint8 frame, alpha and bg_out bit for bit."""
    import radnerf_hip as hip
    scene = _scene(8)
    m, poses, ct = scene.model, _poses(scene), _code(scene.model)
    N = _stride_n() if N == "stride" else N
    gen = _gen(N % 1000)
    mask = torch.rand(N, device="cuda", generator=gen) < 0.5
    xy = _pixels(mask, gen)
    r = lambda *s: torch.rand(*s, device="cuda", generator=gen)  # noqa: E731
    # image + (1 - weights_sum) * bg leaves [0, 1] on part of the pixels (the clamp works); depth - near goes negative on some
    src = dict(bg=r(N, 3), image=r(N, 3) * 1.2 - 0.1, weights_sum=r(N), depth=r(N) * 3, nears=r(N) + 0.5, fars=r(N) + 2.5)

    def frame(merged):
        gd = _Guard()
        coords, bg_in = gd.new(N, 2, src=xy), gd.new(N, 3, src=src["bg"])
        image, wsum, depth = gd.new(N, 3, src=src["image"]), gd.new(N, src=src["weights_sum"]), gd.new(N, src=src["depth"])
        nears, fars = gd.new(N, src=src["nears"]), gd.new(N, src=src["fars"])
        u8, bg_out, alpha = gd.new(N, 3, dtype=torch.uint8), gd.new(N, 3), gd.new(N, 1)
        if merged:
            _launch(m, coords, poses, ct, bg_in, bg_out, alpha, None, blend=(image, wsum, depth, nears, fars, u8))
        else:
            _launch(m, coords, poses, ct, bg_in, bg_out, alpha, None)
            hip.call("rn_blend_frame", hip.ptr(image), hip.ptr(wsum), hip.ptr(bg_out), hip.ptr(depth), hip.ptr(nears), hip.ptr(fars), N,
                     hip.ptr(u8), hip.stream())
        gd.check()
        _coverage(m, coords, alpha, mask)
        return dict(image=image, depth=depth, u8=u8, alpha=alpha, bg_out=bg_out)
    with _occupancy(m, _quadrants()):
        two, one = frame(False), frame(True)
    for key in two:
        assert torch.equal(one[key], two[key]), key
    assert bool(torch.isfinite(one["image"]).all()) and bool(torch.isfinite(one["depth"]).all())
    assert float(one["image"].max()) == 1.0 and float(one["depth"].min()) == 0.0        # both clamps were at work
    assert not torch.equal(one["image"], src["image"])


# ====================================================================================================== training branch
def _train_scene(ind):
    scene = _scene(ind, engine="ops")
    scene.model.train()
    return scene


def _smooth_pixels(m, xy, poses, ct, margin=2e-5):
    """Pixels at which forward_torso is smooth in its parameters, by the float64 reference alone (modelled on
    test_gpu_train_head.py::_stable_samples): no hidden pre-activation of either net within `margin` of 0, no clamped coordinate
    within `margin` (normalised) of a cell boundary of any of the 16 levels, no unclamped coordinate within `margin` of +-1.
    Returns (smooth [N], share of the pixels the ReLU rule alone keeps)."""
    pre = []

    def mlp(ws, x):
        for i, w in enumerate(ws):
            x = x @ w.t()
            if i != len(ws) - 1:
                pre.append(x)
                x = torch.relu(x)
        return x
    with pytest.MonkeyPatch.context() as mp, torch.no_grad():
        mp.setattr(netref64, "mlp", mlp)
        _, _, dx = netref64.Net64(m).forward_torso(xy, poses, ct)
    assert len(pre) == 4
    relu_ok = torch.stack([(z.abs() > margin).all(-1) for z in pre]).all(0)
    un = xy.double() * float(np.float32(m.opt.torso_shrink)) + dx
    edge_ok = ((un.abs() - 1).abs() > margin).all(-1)
    enc = m.torso_encoder
    S = float(np.log2(enc.per_level_scale))
    scales = torch.tensor([float(netref64.level_scale(l, S, int(enc.base_resolution))[0]) for l in range(16)], dtype=torch.float64,
                          device=xy.device)
    pos = ((un.clamp(-1, 1) + 1) / 2).unsqueeze(-1) * scales + 0.5                    # [N, 2, 16]
    frac = pos - pos.floor()
    cell_ok = ((frac > margin * scales) & (frac < 1 - margin * scales)).all(-1).all(-1)
    return relu_ok & edge_ok & cell_ok, float(relu_ok.double().mean())


def _smooth_batch(m, n, seed, poses, ct, inside=None):
    """Exactly n smooth pixels out of a uniform pool (as test_gpu_options.py::_stable_batch draws its samples); `inside`: the
    pool is drawn inside the covered quadrants of _quadrants() instead of over the whole image."""
    gen = _gen(seed)
    pool = 3 * n + 512
    if inside is None:
        xy = torch.rand(pool, 2, device="cuda", generator=gen) * 2 - 1
    else:
        xy = _pixels(torch.full((pool,), bool(inside), device="cuda"), gen)
    smooth, relu_share = _smooth_pixels(m, xy, poses, ct)
    share = float(smooth.double().mean())
    assert share > 0.40, (share, relu_share)
    idx = torch.nonzero(smooth).reshape(-1)[:n]
    assert idx.numel() == n
    return xy[idx].contiguous(), gen


def _grad_names(m):
    names = [n for n, _ in m.named_parameters() if n.startswith(("torso_deform_net.", "torso_net."))] + ["torso_encoder.embeddings"]
    assert len(names) == 7
    return names + (["individual_codes_torso"] if m.individual_dim_torso else [])


def _torso_loss(alpha, color, dx, up):
    return (alpha * up[0]).sum() + (color * up[1]).sum() + (dx * up[2]).sum()


@contextlib.contextmanager
def _spy():
    """Names of the C entry points called inside the block (radnerf_hip.call is the one door to the library)."""
    import radnerf_hip as hip
    names, real = [], hip.call

    def call(name, *a):
        names.append(name)
        return real(name, *a)
    hip.call = call
    try:
        yield names
    finally:
        hip.call = real


def _collect(m, names, row):
    out = {}
    for n in names:
        g = dict(m.named_parameters())[n].grad
        assert g is not None and bool(torch.isfinite(g).all()), n
        if n == "individual_codes_torso":
            assert int(torch.count_nonzero(g)) == int(torch.count_nonzero(g[row])), "a gradient in a row that was not picked"
            g = g[row]
        out[n] = g.detach().clone()
    return out


def _compare(g_hip, g_torch, g64, what):
    """Per tensor: e_hip <= 4 e_torch + 1e-6 against float64, and e_hip < 2e-3 wherever the torch formulation meets that bar (the
    rule of test_fused_head_against_float64).  Returns the worst e_hip / e_torch."""
    assert set(g_hip) == set(g_torch) == set(g64)
    worst = (0.0, None)
    for name in sorted(g64):
        assert g_hip[name].shape == g64[name].shape, name
        assert float(g64[name].abs().max()) > 0, name
        e_h, e_t = _maxerr(g_hip[name], g64[name]), _maxerr(g_torch[name], g64[name])
        assert e_h <= 4 * e_t + 1e-6, (what, name, e_h, e_t)
        assert e_h < 2e-3 or e_t >= 2e-3, (what, name, e_h, e_t)
        worst = max(worst, (e_h / (e_t + 1e-12), (name, e_h, e_t)), key=lambda t: t[0])
    print(f"torso gradients {what}: worst e_hip/e_torch = {worst[0]:.2f} ({worst[1][0]}: e_hip {worst[1][1]:.2e}, e_torch {worst[1][2]:.2e})")
    return worst[0]


GRAD_CASES = [(8, n, False) for n in (1023, 1024, 1025, 1055, 1056, 1057, 4099)] + \
             [(i, n, False) for i in (3, 0) for n in (1025, 4099)] + [(i, 4099, True) for i in (8, 3, 0)]


@pytest.mark.parametrize("ind,N,clamp", GRAD_CASES)
def test_forward_torso_gradients_against_float64(hiplib, monkeypatch, ind, N, clamp):
    """Outputs and every gradient of forward_torso (both nets, the torso table, the picked row of the codes) on exactly N smooth
    pixels: float64 truth, RN_MLP_TRAIN=torch, RN_MLP_TRAIN=hip.  forward_split takes the kernels from 1024 rows on: N sits on
    either side of that and on the 32-row tiles after it.  clamp: the last deformation layer scaled as in the inference test,
    so that clamped coordinates carry no gradient into the deformation net, on both sides."""
    scene = _train_scene(ind)
    m, poses, row = scene.model, _poses(scene), 3
    names = _grad_names(m)
    with _scaled_deform(m, CLAMP_K[ind] if clamp else 1.0):
        xy, gen = _smooth_batch(m, N, 2000 + N + ind, poses, _code(m, row))
        up = [torch.randn(N, 1, device="cuda", generator=gen), torch.randn(N, 3, device="cuda", generator=gen),
              torch.randn(N, 2, device="cuda", generator=gen)]
        ref = netref64.Net64(m)
        out64 = ref.forward_torso(xy, poses, ref.P["individual_codes_torso"][row] if ind else None)
        g64 = dict(zip(names, torch.autograd.grad(_torso_loss(*out64, [u.double() for u in up]), [ref.P[n] for n in names])))
        if ind:
            g64["individual_codes_torso"] = g64["individual_codes_torso"][row]
        if clamp:
            un = xy.double() * float(np.float32(m.opt.torso_shrink)) + out64[2].detach()
            share = float((un.abs() > 1).any(1).double().mean())
            assert 0.10 <= share <= 0.90, share
        runs = {}
        for mode in ("torch", "hip"):
            monkeypatch.setenv("RN_MLP_TRAIN", mode)
            for p in m.parameters():
                p.grad = None
            with _spy() as called:
                out = m.forward_torso(xy, poses, None, m.individual_codes_torso[row] if ind else None)
                _torso_loss(*out, up).backward()
            n_fwd, n_bwd = called.count("rn_mlp64_forward"), called.count("rn_mlp64_backward")
            if mode == "torch" or N < 1024:
                assert not [c for c in called if c.startswith("rn_mlp64_")], called
            else:
                assert (n_fwd, n_bwd) == (2, 2) and called.count("rn_mlp64_weight_grads") == 2, called
            runs[mode] = dict(_collect(m, names, row), **{f"out:{k}": v.detach() for k, v in zip(("alpha", "color", "dx"), out)})
    g64.update({f"out:{k}": v.detach() for k, v in zip(("alpha", "color", "dx"), out64)})
    _compare(runs["hip"], runs["torch"], g64, f"ind={ind} N={N} clamp={clamp}")


@pytest.mark.parametrize("N", [65, 4097])
def test_torso_layer_gather_and_index_copy(hiplib, monkeypatch, N):
    """NeRFRenderer._torso_layer under autograd on a random-half mask: the blended background and its gradients (parameters and
    the background itself) equal a float64 restatement in which uncovered pixels contribute exactly nothing; the gathered index
    list is the inference kernel's coverage."""
    from radnerf import occupancy
    scene = _train_scene(8)
    m, poses, row = scene.model, _poses(scene), 3
    names = _grad_names(m)
    gen = _gen(900 + N)
    mask = torch.rand(N, device="cuda", generator=gen) < 0.5
    idx = torch.nonzero(mask).reshape(-1)
    xy = _pixels(mask, gen)
    xy[idx], _ = _smooth_batch(m, idx.numel(), 901 + N, poses, _code(m, row), inside=True)
    bg = torch.rand(N, 3, device="cuda", generator=gen)
    up = torch.randn(N, 3, device="cuda", generator=gen)
    with _occupancy(m, _quadrants()):
        # coverage: the index list of the training formulation against the kernel's alpha > 0 (and grid_sample, and the mask)
        alpha = torch.empty(N, 1, device="cuda")
        _launch(m, xy, poses, _code(m, row), bg, torch.empty(N, 3, device="cuda"), alpha, None)
        _coverage(m, xy, alpha, mask)
        assert torch.equal(occupancy.torso_pixels(m, xy, THRESH), idx)
        ref = netref64.Net64(m)
        bg64 = bg.double().requires_grad_(True)
        a, c, _ = ref.forward_torso(xy[idx], poses, ref.P["individual_codes_torso"][row])
        out64 = bg64.index_put((idx,), c * a + bg64[idx] * (1 - a))
        g64 = dict(zip(names + ["background"], torch.autograd.grad((out64 * up.double()).sum(), [ref.P[n] for n in names] + [bg64])))
        g64["individual_codes_torso"] = g64["individual_codes_torso"][row]
        g64["out:bg"] = out64.detach()
        runs = {}
        for mode in ("torch", "hip"):
            monkeypatch.setenv("RN_MLP_TRAIN", mode)
            for p in m.parameters():
                p.grad = None
            bg_leaf = bg.clone().requires_grad_(True)
            res = {}
            with _spy() as called:
                out = m._torso_layer(xy, poses, None, row, bg_leaf, res)
                (out * up).sum().backward()
            kernels = mode == "hip" and idx.numel() >= 1024
            assert called.count("rn_mlp64_forward") == (2 if kernels else 0) and called.count("rn_torso_mask") == 1, called
            assert "rn_torso_fused" not in called
            un = ~mask
            assert torch.equal(out[un], bg[un]) and torch.equal(bg_leaf.grad[un], up[un])     # exactly nothing from uncovered pixels
            assert int(torch.count_nonzero(res["torso_alpha"][un])) == 0 and torch.equal(res["torso_alpha"].reshape(-1) > 0, mask)
            assert res["deform"].shape == (idx.numel(), 2)
            runs[mode] = dict(_collect(m, names, row), background=bg_leaf.grad.clone(), **{"out:bg": out.detach()})
    _compare(runs["hip"], runs["torch"], g64, f"_torso_layer N={N}")
