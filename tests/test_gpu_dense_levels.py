"""The dense image of the xyz table's coarser hashed levels (csrc/rn_grid.hip: rn_grid_dense_plan, rn_grid_dense_build) and its
owner (radnerf.fused.FusedState.frame_grid).

Held here, all of it exact: every image row is the table row the hash names for its lattice point (computed on the CPU in
uint32 arithmetic), untaken levels are copies and padding rows are zero, nothing is written outside the image; the three
inference network kernels give the same bits from the image descriptor as from the table descriptor, at tile edges, at
coordinates exactly on and outside the box, with fp32 and fp16 tables and for the sigma-only call; a rendered frame is the same
with the switch on and off; the image is built on the second frame call over one table, dropped when the table changes, and a
table that changes between calls never builds one.  The planner's own cases are in tests/test_dense_plan.py (no GPU)."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_dense_plan import S11, grid_desc, level_resolutions, plan, plan_ref, table_offsets

pytestmark = pytest.mark.gpu

PAD = 4096
_SCENE = []


# ------------------------------------------------------------------------------------------------------ image contents
def _hashed_rows(R, T):
    """Table row (within its level) of every lattice point of a hashed level, in image order x + y (R+1) + z (R+1)^2."""
    r1, m32 = R + 1, np.uint64(0xFFFFFFFF)
    i = np.arange(r1 ** 3, dtype=np.uint64)
    x, y, z = i % np.uint64(r1), (i // np.uint64(r1)) % np.uint64(r1), i // np.uint64(r1 * r1)
    h = (x ^ ((y * np.uint64(2654435761)) & m32) ^ ((z * np.uint64(805459861)) & m32)) & m32
    return (h % np.uint64(T)).astype(np.int64)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_image_rows_are_the_hashed_rows(hiplib, dtype):
    log2_T, T = 12, 2 ** 12
    off, res = table_offsets(3, 16, S11, log2_T), level_resolutions(16, S11)
    assert all((R + 1) ** 3 > T for R in res)                    # every level is hashed at T = 2^12
    row_bytes = 4 if dtype == torch.float16 else 8
    word = torch.int32 if dtype == torch.float16 else torch.int64           # one row, as bits
    gen = torch.Generator(device="cuda").manual_seed(5)
    table = (torch.rand(off[-1], 2, device="cuda", generator=gen) * 2 - 1).to(dtype).contiguous()
    off_dev = torch.tensor(off, dtype=torch.int32, device="cuda")
    g = grid_desc(hiplib, off, 16, S11, 1 if dtype == torch.float16 else 0, embeddings=table.data_ptr(), offsets_dev=off_dev.data_ptr())
    rows_0_2 = off[-1] + sum(((res[l] + 1) ** 3 + 7) // 8 * 8 - T for l in range(3))
    image_off, mask, nbytes = plan(hiplib, g, off, rows_0_2 * row_bytes)
    assert mask == 0b111 and nbytes == rows_0_2 * row_bytes and (image_off, mask, nbytes) == plan_ref(off, res, row_bytes, nbytes)

    full = torch.full((nbytes + 2 * PAD,), 165, dtype=torch.uint8, device="cuda")
    image = full[PAD:PAD + nbytes]
    oh, ih = (C.c_int32 * len(off))(*off), (C.c_int32 * len(off))(*image_off)
    hiplib.call("rn_grid_dense_build", C.byref(g), oh, ih, mask, hiplib.ptr(image), nbytes, hiplib.stream())
    torch.cuda.synchronize()
    assert bool((full[:PAD] == 165).all()) and bool((full[PAD + nbytes:] == 165).all()), "write outside the image"
    got = image.view(word).cpu()
    src = table.view(word).reshape(-1).cpu()
    for l in range(16):
        lvl = got[image_off[l]:image_off[l + 1]]
        if (mask >> l) & 1:
            n = (res[l] + 1) ** 3
            want = src[off[l] + torch.from_numpy(_hashed_rows(res[l], T))]
            assert torch.equal(lvl[:n], want), l
            assert lvl.numel() == (n + 7) // 8 * 8 and bool((lvl[n:] == 0).all()), l
        else:
            assert torch.equal(lvl, src[off[l]:off[l + 1]]), l

    # a build the plan does not back is refused before anything is launched
    with pytest.raises(RuntimeError, match="grid_dense_build"):
        hiplib.call("rn_grid_dense_build", C.byref(g), oh, ih, mask, hiplib.ptr(image), nbytes - row_bytes, hiplib.stream())
    with pytest.raises(RuntimeError, match="grid_dense_build"):
        hiplib.call("rn_grid_dense_build", C.byref(g), oh, ih, mask | 8, hiplib.ptr(image), nbytes, hiplib.stream())
    with pytest.raises(RuntimeError, match="grid_dense_build"):
        hiplib.call("rn_grid_dense_build", C.byref(g), oh, oh, mask, hiplib.ptr(image), nbytes, hiplib.stream())


# ------------------------------------------------------------------------------------------------------ kernel equality
def _scene():
    """64 x 64, xyz hash grid with T = 2^14 (levels 2.. are hashed), a 16 MiB budget: levels 2-5 become lattices (8.7 MiB)."""
    from radnerf.scene import SyntheticScene, default_opt
    if not _SCENE:
        torch.manual_seed(0)
        _SCENE.append(SyntheticScene(H=64, W=64, n_frames=8, device="cuda",
                                     opt=default_opt(engine="fused", xyz_grid="hashgrid", xyz_log2_hashmap_size=14, smooth_lips=False,
                                                     dense_budget_mb=16)))
    return _SCENE[0]


def _samples(bound):
    """1000 samples: the first ones exactly on corners and faces of the box, some outside it, the rest inside."""
    rng = np.random.default_rng(11)
    x = rng.uniform(-bound, bound, (1000, 3)).astype(np.float32)
    b = np.float32(bound)
    x[0] = (b, -b, b)
    x[1] = (-b, -b, -b)
    x[2] = (b, b, b)
    x[3] = (1.5 * b, 0.0, 0.0)
    x[4] = (0.25, np.nextafter(-b, np.float32(-2) * b), 0.0)
    x[5] = (-b, 0.3, b)
    x[40] = (0.0, 0.0, np.nextafter(b, np.float32(2) * b))
    x[41] = (b, 0.0, 0.0)
    d = rng.standard_normal((1000, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return torch.from_numpy(x).cuda(), torch.from_numpy(d).cuda()


def _forward(hip, st, gx, x, d, M, bound, sigma_only):
    sig = torch.full((M,), -77.0, device="cuda")
    rgb = None if sigma_only else torch.full((M, 3), -77.0, device="cuda")
    amb = None if sigma_only else torch.full((M, 2), -77.0, device="cuda")
    xs, ds = x[:M].contiguous(), None if sigma_only else d[:M].contiguous()
    hip.call("rn_nerf_fused_forward", hip.ptr(xs), hip.ptr(ds), None, M, None, C.byref(gx), C.byref(st.gw), hip.ptr(st.packed),
             hip.ptr(st.bias), float(bound), hip.ptr(sig), hip.ptr(rgb), hip.ptr(amb), st.mlp_dtype, hip.stream())
    torch.cuda.synchronize()
    return sig, rgb, amb


@pytest.mark.parametrize("half", [False, True], ids=["table32", "table16"])
@pytest.mark.parametrize("mlp", ["f32", "f32x2", "f16"])
def test_kernels_read_the_same_features_from_the_image(hiplib, mlp, half):
    from radnerf import fused
    scene = _scene()
    m = scene.model
    keep = (getattr(m.opt, "mlp_dtype", "f32"), getattr(m.opt, "half_tables", False))
    m.opt.mlp_dtype, m.opt.half_tables = mlp, half
    try:
        st = fused._state(m)
        st.refresh()
        assert st.tables[0].dtype == (torch.float16 if half else torch.float32)
        rng = np.random.default_rng(3)
        enc_a = torch.from_numpy(rng.standard_normal((1, m.audio_dim)).astype(np.float32)).cuda()
        fused._frame_bias(st, enc_a, scene.eye if m.exp_eye else None, m.individual_codes[0] if m.individual_dim > 0 else None)
        builds = st.dense_builds
        img = st._build_dense(None, st.tables[0], 16 << 20)
        assert img.buf is not None and st.dense_builds == builds + 1
        assert img.levels & 0b11 == 0 and bin(img.levels).count("1") >= 3          # levels 0, 1 are dense in the table already
        x, d = _samples(float(m.bound))
        for M in (1, 31, 33, 1000):
            for sigma_only in (False, True):
                ref = _forward(hiplib, st, st.gx, x, d, M, m.bound, sigma_only)
                got = _forward(hiplib, st, img.gx, x, d, M, m.bound, sigma_only)
                for name, a, b in zip(("sigma", "rgb", "ambient"), got, ref):
                    if b is None:
                        assert a is None
                        continue
                    assert torch.equal(a, b), (name, M, sigma_only)
                    assert not bool((b == -77.0).any()) and bool(torch.isfinite(b).all()), (name, M, sigma_only)
        # ... and it is the image they read: with its de-hashed levels cleared the same call gives other numbers
        ref = _forward(hiplib, st, st.gx, x, d, 1000, m.bound, False)
        lo = int(img.offsets[2].item()) * (4 if half else 8)
        img.buf[lo:].zero_()
        got = _forward(hiplib, st, img.gx, x, d, 1000, m.bound, False)
        assert not torch.equal(got[0], ref[0])
    finally:
        m.opt.mlp_dtype, m.opt.half_tables = keep
        fused._state(m).refresh()


# ------------------------------------------------------------------------------------------------------ frame and lifetime
def _render(scene, i):
    with torch.no_grad():
        out = scene.render(i, want_u8=True)
    torch.cuda.synchronize()
    return {k: out[k].clone() for k in ("image", "depth", "image_u8")}


def _off(scene, monkeypatch, i):
    """The frame as a build without dense images renders it."""
    monkeypatch.setenv("RN_DENSE_LEVELS", "0")
    out = _render(scene, i)
    monkeypatch.delenv("RN_DENSE_LEVELS")
    return out


def _same(got, ref):
    assert int((ref["image_u8"] < 255).sum()) > 100              # the head is in the frame
    for k in ("image_u8", "image", "depth"):
        assert torch.equal(got[k], ref[k]), k


def _forget(m):
    from radnerf import fused
    fused._caches(m).image.forget()


def test_frames_are_the_same_and_the_image_follows_the_table(hiplib, monkeypatch):
    from radnerf import fused
    monkeypatch.delenv("RN_DENSE_LEVELS", raising=False)
    scene = _scene()
    m = scene.model
    st = fused._state(m)
    slot = st.cache.image
    _forget(m)
    b0 = st.dense_builds
    on = [_render(scene, 0)]                                     # first sight of the table: no build
    assert slot.held is None and st.dense_builds == b0
    on.append(_render(scene, 1))                                 # seen on the call before: built and used
    img = slot.held
    assert img is not None and img.buf is not None and st.dense_builds == b0 + 1 and img.levels != 0
    on += [_render(scene, 2), _render(scene, 3)]
    assert slot.held is img and st.dense_builds == b0 + 1
    off = [_off(scene, monkeypatch, i) for i in range(4)]
    assert st.dense_builds == b0 + 1
    for a, b in zip(on, off):
        _same(a, b)
    assert not torch.equal(off[0]["image_u8"], off[3]["image_u8"])

    # the table changes in place: the image goes, that frame reads the table, the call after it builds for the new table
    emb = m.encoder.embeddings
    keep = emb.detach().clone()
    try:
        with torch.no_grad():
            emb.mul_(1.5)
        got = _render(scene, 1)
        assert slot.held is None and st.dense_builds == b0 + 1
        ref = _off(scene, monkeypatch, 1)
        _same(got, ref)
        assert not torch.equal(ref["image_u8"], off[1]["image_u8"])
        got = _render(scene, 1)
        assert st.dense_builds == b0 + 2 and slot.held is not None and slot.held is not img
        _same(got, ref)
        # the switch: no image is looked at, none is built
        monkeypatch.setenv("RN_DENSE_LEVELS", "0")
        _forget(m)
        _render(scene, 0), _render(scene, 0), _render(scene, 0)
        assert st.dense_builds == b0 + 2 and slot.held is None
        monkeypatch.delenv("RN_DENSE_LEVELS")
    finally:
        with torch.no_grad():
            emb.copy_(keep)
        _forget(m)


def test_a_table_that_changes_between_calls_builds_nothing(hiplib, monkeypatch):
    from radnerf import fused
    monkeypatch.delenv("RN_DENSE_LEVELS", raising=False)
    scene = _scene()
    m = scene.model
    st = fused._state(m)
    slot = st.cache.image
    _forget(m)
    builds = st.dense_builds
    emb = m.encoder.embeddings
    keep = emb.detach().clone()
    x, _ = _samples(float(m.bound))
    enc_a = torch.zeros(1, m.audio_dim, device="cuda")
    try:
        for i in range(4):                                       # density queries of an occupancy refresh between training steps
            with torch.no_grad():
                emb.add_(1e-3)
            fused.density_forward(m, x, enc_a, scene.eye if m.exp_eye else None)
            assert slot.held is None and st.dense_builds == builds
        for i in range(4):                                       # density queries over one table build nothing either
            fused.density_forward(m, x, enc_a, scene.eye if m.exp_eye else None)
        assert slot.held is None and st.dense_builds == builds
        for i in range(4):                                       # a validation frame after every step
            with torch.no_grad():
                emb.add_(1e-3)
            _render(scene, i)
            assert slot.held is None and st.dense_builds == builds
    finally:
        with torch.no_grad():
            emb.copy_(keep)
        _forget(m)


def test_a_second_stream_uses_what_the_first_built(hiplib, monkeypatch):
    """The plan and the image are the model's, not a stream's: a frame on a side stream builds neither, is ordered behind both
    builds once, and is the frame of a build without them."""
    from radnerf import fused
    monkeypatch.delenv("RN_DENSE_LEVELS", raising=False)
    monkeypatch.delenv("RN_TORSO_PLAN", raising=False)
    scene = _scene()
    m = scene.model
    assert m.torso
    st = fused._state(m)
    plan, image = st.cache.plan, st.cache.image
    plan.forget(), image.forget()
    try:
        _render(scene, 0), _render(scene, 1)                     # second sight: both are built, on the current stream
        assert plan.held is not None and plan.held.buf is not None and image.held is not None and image.held.buf is not None
        builds = (st.plan_builds, st.dense_builds)
        waited = (set(plan.held.waited), set(image.held.waited))
        assert waited == ({torch.cuda.current_stream().cuda_stream},) * 2
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            got = _render(scene, 2)
        assert (st.plan_builds, st.dense_builds) == builds
        assert side.cuda_stream in plan.held.waited and side.cuda_stream in image.held.waited
        grown = (set(plan.held.waited), set(image.held.waited))
        assert grown == tuple(w | {side.cuda_stream} for w in waited)
        monkeypatch.setenv("RN_TORSO_PLAN", "0")
        ref = _off(scene, monkeypatch, 2)
        monkeypatch.delenv("RN_TORSO_PLAN")
        _same(got, ref)
        with torch.cuda.stream(side):
            _render(scene, 3)
        assert (set(plan.held.waited), set(image.held.waited)) == grown and (st.plan_builds, st.dense_builds) == builds
    finally:
        plan.forget(), image.forget()
