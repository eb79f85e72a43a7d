"""The reference-side binding (radnerf_hip/compat_backend.py): `_backend` objects with the pybind modules'
function names and argument lists (raymarching.h:7-20, gridencoder.h:12-15, shencoder.h:9-10,
freqencoder.h:7-10), driven here exactly like the reference's Python wrappers drive them."""
import inspect

import numpy as np
import pytest
import torch

REFERENCE_SURFACE = {
    "raymarching_backend": {
        "near_far_from_aabb": 7, "sph_from_ray": 5, "morton3D": 3, "morton3D_invert": 3, "packbits": 4,
        "morton3D_dilation": 4, "march_rays_train": 18, "march_rays_train_backward": 8,
        "composite_rays_train_forward": 12, "composite_rays_train_backward": 17, "march_rays": 18, "composite_rays": 11},
    "gridencoder_backend": {"grid_encode_forward": 14, "grid_encode_backward": 16, "grad_total_variation": 13},
    "shencoder_backend": {"sh_encode_forward": 6, "sh_encode_backward": 7},
    "freqencoder_backend": {"freq_encode_forward": 6, "freq_encode_backward": 7},
}


def test_backend_objects_have_the_pybind_names_and_arities(hiplib):
    from radnerf_hip import compat_backend as cb
    for obj_name, fns in REFERENCE_SURFACE.items():
        obj = getattr(cb, obj_name)
        have = {n for n, f in vars(obj).items() if isinstance(f, staticmethod)}
        assert have == set(fns), (obj_name, have ^ set(fns))
        for fn, arity in fns.items():
            assert len(inspect.signature(getattr(obj, fn)).parameters) == arity, (obj_name, fn)


def _pybind_modules(hiplib):
    """The four pybind11 modules (csrc/bindings/radnerf_pybind.cpp), built on demand into rad-nerf_amd/lib/pybind/."""
    import importlib
    import importlib.util
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("rn_build", os.path.join(root, "rad-nerf_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    import sysconfig
    suffix = sysconfig.get_config_var("EXT_SUFFIX")
    d = mod.BINDINGS_DIR
    if os.environ.get("RN_REBUILD") == "1" or not all(os.path.exists(os.path.join(d, n + suffix)) for n in mod.BINDINGS_MODULES):
        d = mod.build_bindings()            # ~2.5 min of g++ on torch's headers; the built objects travel with the tree
    if d not in sys.path:
        sys.path.insert(0, d)
    return {name: importlib.import_module(name) for name in mod.BINDINGS_MODULES}


def test_pybind_modules_have_the_reference_names_and_arities(hiplib):
    """Module names of the reference's setup.py / bindings.cpp, every function, and the argument count pybind11 reports."""
    mods = _pybind_modules(hiplib)
    for mod_name, key in (("_raymarching_face", "raymarching_backend"), ("_gridencoder", "gridencoder_backend"),
                          ("_shencoder", "shencoder_backend"), ("_freqencoder", "freqencoder_backend")):
        have = {n for n in dir(mods[mod_name]) if not n.startswith("_")}
        assert have == set(REFERENCE_SURFACE[key]), (mod_name, have ^ set(REFERENCE_SURFACE[key]))
        for fn, arity in REFERENCE_SURFACE[key].items():
            sig = getattr(mods[mod_name], fn).__doc__.splitlines()[0]
            assert sig.count("arg") == arity, (mod_name, fn, sig)


@pytest.mark.gpu
@pytest.mark.parametrize("binding", ["ctypes", "pybind11"])
def test_reference_style_calls_through_the_backend(po, hiplib, rng, binding):
    if binding == "ctypes":
        from radnerf_hip.compat_backend import freqencoder_backend, gridencoder_backend, raymarching_backend, shencoder_backend
    else:
        mods = _pybind_modules(hiplib)
        raymarching_backend, gridencoder_backend = mods["_raymarching_face"], mods["_gridencoder"]
        shencoder_backend, freqencoder_backend = mods["_shencoder"], mods["_freqencoder"]
    from radnerf.scene import ellipsoid_bitfield
    from gridencoder.encoder import level_offsets
    dev = "cuda"
    N = 3000
    o = np.tile(np.array([[0.05, 3.3, -0.1]], np.float32), (N, 1))
    d = rng.uniform(-0.7, 0.7, (N, 3)).astype(np.float32) - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    aabb = np.array([-1, -0.5, -1, 1, 0.5, 1], np.float32)
    bits, _ = ellipsoid_bitfield(128, 1.0, (0.4, 0.42, 0.4))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731

    # raymarching/raymarching.py:37-45
    rays_o, rays_d, taabb = t(o), t(d), t(aabb)
    nears = torch.empty(N, device=dev); fars = torch.empty(N, device=dev)
    raymarching_backend.near_far_from_aabb(rays_o, rays_d, taabb, N, 0.05, nears, fars)
    en, ef = po.near_far_from_aabb(o, d, aabb, 0.05)
    assert np.array_equal(nears.cpu().numpy(), en) and np.array_equal(fars.cpu().numpy(), ef)

    # raymarching/raymarching.py:380-395 (march_rays) and :433 (composite_rays)
    n_alive, n_step = N, 2
    M = n_alive * n_step
    M += 128 - (M % 128)
    xyzs = torch.zeros(M, 3, device=dev); dirs = torch.zeros(M, 3, device=dev); deltas = torch.zeros(M, 2, device=dev)
    noises = torch.zeros(n_alive, device=dev)
    alive = torch.arange(N, dtype=torch.int32, device=dev); rays_t = nears.clone(); tbits = t(bits)
    raymarching_backend.march_rays(n_alive, n_step, alive, rays_t, rays_o, rays_d, 1.0, 1 / 256, 16, 1, 128, tbits, nears, fars,
                                   xyzs, dirs, deltas, noises)
    ex, ed, edl = po.march_rays(n_alive, n_step, np.arange(N, dtype=np.int32), en, o, d, 1.0, 1 / 256, 16, 1, 128, bits, en, ef,
                                np.zeros(N, np.float32), M=M)
    assert np.array_equal(xyzs.cpu().numpy(), ex) and np.array_equal(deltas.cpu().numpy(), edl)

    # gridencoder/grid.py:47-54 ([L,B,C] outputs) and :75-84 (backward)
    D, C, L = 3, 2, 16
    pls = np.exp2(np.log2(2048 / 16) / 15)
    offsets = level_offsets(D, L, pls, 16, 16, False)
    emb = rng.uniform(-0.5, 0.5, (int(offsets[-1]), C)).astype(np.float32)
    B = 2000
    x = rng.uniform(0, 1, (B, D)).astype(np.float32)
    tx, temb, toff = t(x), t(emb), t(offsets)
    outputs = torch.empty(L, B, C, device=dev)
    dy_dx = torch.empty(B, L * D * C, device=dev)
    S = np.log2(pls)
    gridencoder_backend.grid_encode_forward(tx, temb, toff, outputs, B, D, C, L, S, 16, dy_dx, 1, False, 0)
    eo, edy = po.grid_encode_forward(x, emb, offsets, B, D, C, L, float(S), 16, True, 1, False, 0)
    assert np.array_equal(outputs.cpu().numpy(), eo) and np.array_equal(dy_dx.cpu().numpy(), edy)
    grad = t(rng.standard_normal((L, B, C)).astype(np.float32))
    g_emb = torch.zeros_like(temb); g_in = torch.zeros(B, D, device=dev)
    gridencoder_backend.grid_encode_backward(grad, tx, temb, toff, g_emb, B, D, C, L, S, 16, dy_dx, g_in, 1, False, 0)
    ege, egi = po.grid_encode_backward(grad.cpu().numpy(), x, emb, offsets, B, D, C, L, float(S), 16, edy, 1, False, 0)
    np.testing.assert_allclose(g_emb.cpu().numpy(), ege, rtol=1e-4, atol=1e-4)
    assert np.array_equal(g_in.cpu().numpy(), egi)

    # shencoder/sphere_harmonics.py:24-32, freqencoder/freq.py:26-28
    v = t(d[:1000])
    sh = torch.empty(1000, 16, device=dev)
    shencoder_backend.sh_encode_forward(v, sh, 1000, 3, 4, None)
    np.testing.assert_allclose(sh.cpu().numpy(), po.sh_encode_forward(d[:1000], 4)[0], rtol=2e-6, atol=2e-6)
    fq = torch.empty(1000, 3 + 3 * 2 * 4, device=dev)
    freqencoder_backend.freq_encode_forward(v, 1000, 3, 4, 27, fq)
    np.testing.assert_allclose(fq.cpu().numpy(), po.freq_encode_forward(d[:1000], 4), rtol=0, atol=4e-5)


@pytest.mark.gpu
def test_all_19_pybind_functions_reproduce_the_reference_vectors(po, hiplib):
    """Every function of the four built pybind11 modules (raymarching/src/bindings.cpp:5-21, gridencoder/src/bindings.cpp,
    shencoder/src/bindings.cpp, freqencoder/src/bindings.cpp), called with CUDA tensors allocated the way the reference's
    wrappers allocate them (raymarching/raymarching.py:42-45, 231-244, 301-305, 323-326, 385-395; gridencoder/grid.py:47-54,
    77-84; shencoder/sphere_harmonics.py:24-32, 48-52; freqencoder/freq.py:26-28, 44-47), on the inputs of
    tests/golden/reference_ops.npz -- vectors those wrappers themselves produced (tests/golden/make_golden.py)."""
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(here, "golden"))
    import cases
    from radnerf.scene import SyntheticScene, default_opt
    mods = _pybind_modules(hiplib)
    rmb, geb, shb, fqb = mods["_raymarching_face"], mods["_gridencoder"], mods["_shencoder"], mods["_freqencoder"]
    gold = cases.load_golden("ops")
    flow = np.load(os.path.join(here, "golden", "reference_flow.npz"))
    dev = "cuda"
    T = lambda k: torch.from_numpy(gold[k]).to(dev)  # noqa: E731
    cpu = lambda t: t.detach().float().cpu().numpy() if t.dtype in (torch.float16, torch.float32) else t.detach().cpu().numpy()  # noqa: E731
    called = set()

    def call(mod, name, *a):
        called.add(name)
        getattr(mod, name)(*a)

    scene = SyntheticScene(H=32, W=32, n_frames=8, device=dev, opt=default_opt())
    m, opt = scene.model, scene.opt
    rays_o = torch.from_numpy(flow["rays_o"]).reshape(-1, 3).contiguous().to(dev)
    rays_d = torch.from_numpy(flow["rays_d"]).reshape(-1, 3).contiguous().to(dev)
    N = rays_o.shape[0]
    bits = m.density_bitfield
    # ---- _raymarching_face: 12 functions
    nears, fars = torch.empty(N, device=dev), torch.empty(N, device=dev)
    call(rmb, "near_far_from_aabb", rays_o, rays_d, m.aabb_infer, N, m.min_near, nears, fars)
    assert np.array_equal(cpu(nears), gold["nears"]) and np.array_equal(cpu(fars), gold["fars"])
    coords = torch.empty(N, 2, device=dev)
    call(rmb, "sph_from_ray", rays_o, rays_d, 2.0, N, coords)
    np.testing.assert_allclose(cpu(coords), po.sph_from_ray(cpu(rays_o), cpu(rays_d), 2.0), rtol=0, atol=2e-6)
    mc = T("morton_coords")
    idx = torch.empty(mc.shape[0], dtype=torch.int32, device=dev)
    call(rmb, "morton3D", mc, mc.shape[0], idx)
    assert np.array_equal(cpu(idx), gold["morton_indices"])
    back = torch.empty(mc.shape[0], 3, dtype=torch.int32, device=dev)
    call(rmb, "morton3D_invert", idx, mc.shape[0], back)
    assert np.array_equal(cpu(back), gold["morton_invert"])
    grid = T("occ_grid")
    Cc, H3 = grid.shape
    bitfield = torch.empty(Cc * H3 // 8, dtype=torch.uint8, device=dev)
    call(rmb, "packbits", grid, Cc * H3 // 8, 1.0, bitfield)          # N counts OUTPUT bytes (raymarching/raymarching.py:146-152)
    assert np.array_equal(cpu(bitfield), gold["occ_bits"])
    dil = torch.empty_like(grid)
    call(rmb, "morton3D_dilation", grid, Cc, int(round(H3 ** (1 / 3))), dil)
    assert np.array_equal(cpu(dil), gold["occ_dilated"])
    # march_rays (raymarching.py:380-395): M = n_alive * n_step, then M += 128 - M % 128; zero-initialised outputs
    alive3 = T("march3_alive")
    n_alive, n_step = alive3.shape[0], 3
    M = n_alive * n_step
    M += 128 - M % 128
    xyzs, dirs, deltas = torch.zeros(M, 3, device=dev), torch.zeros(M, 3, device=dev), torch.zeros(M, 2, device=dev)
    rays_t = nears.clone()
    call(rmb, "march_rays", n_alive, n_step, alive3, rays_t, rays_o, rays_d, m.bound, opt.dt_gamma, opt.max_steps, m.cascade, m.grid_size, bits,
         nears, fars, xyzs, dirs, deltas, torch.zeros(n_alive, device=dev))
    for got, key in ((xyzs, "march3_xyzs"), (dirs, "march3_dirs"), (deltas, "march3_deltas")):
        assert np.array_equal(cpu(got), gold[key]), key
    ws, dp, im = torch.zeros(N, device=dev), torch.zeros(N, device=dev), torch.zeros(N, 3, device=dev)
    alive_c = alive3.clone()
    call(rmb, "composite_rays", n_alive, n_step, 1e-4, alive_c, rays_t, T("comp_sigmas"), T("comp_rgbs"), deltas, ws, dp, im)
    assert np.array_equal(cpu(alive_c), gold["comp_rays_alive"]) and np.array_equal(cpu(rays_t), gold["comp_rays_t"])
    np.testing.assert_allclose(cpu(ws), gold["comp_weights_sum"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(cpu(im), gold["comp_image"], rtol=0, atol=2e-5)
    # march_rays_train, first epochs (raymarching.py:221-257): M = N * max_steps, outputs trimmed to counter[0] padded
    Mt = N * opt.max_steps
    xt, dt_, dlt = torch.zeros(Mt, 3, device=dev), torch.zeros(Mt, 3, device=dev), torch.zeros(Mt, 2, device=dev)
    rays = torch.empty(N, 3, dtype=torch.int32, device=dev)
    counter = torch.zeros(2, dtype=torch.int32, device=dev)
    call(rmb, "march_rays_train", rays_o, rays_d, bits, m.bound, opt.dt_gamma, opt.max_steps, N, m.cascade, m.grid_size, Mt, nears, fars, xt, dt_,
         dlt, rays, counter, torch.zeros(N, device=dev))
    mcount = int(counter[0].item())
    mcount += 128 - mcount % 128
    xt, dt_, dlt = xt[:mcount], dt_[:mcount], dlt[:mcount]
    for got, key in ((xt, "train_xyzs"), (dt_, "train_dirs"), (dlt, "train_deltas"), (rays, "train_rays")):
        assert np.array_equal(cpu(got), gold[key]), key
    g_o, g_d = torch.zeros(N, 3, device=dev), torch.zeros(N, 3, device=dev)
    call(rmb, "march_rays_train_backward", T("trainb_gx"), T("trainb_gd"), rays, dlt.contiguous(), N, mcount, g_o, g_d)
    np.testing.assert_allclose(cpu(g_o), gold["trainb_grad_rays_o"], rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(cpu(g_d), gold["trainb_grad_rays_d"], rtol=1e-5, atol=1e-3)
    sg, rg, am = T("ctrain_sigmas"), T("ctrain_rgbs"), T("ctrain_ambient")
    wsum, asum, dep, img = (torch.empty(N, device=dev), torch.empty(N, device=dev), torch.empty(N, device=dev), torch.empty(N, 3, device=dev))
    call(rmb, "composite_rays_train_forward", sg, rg, am, dlt.contiguous(), rays, mcount, N, 1e-4, wsum, asum, dep, img)
    for got, key, tol in ((wsum, "ctrain_weights_sum", 3e-5), (asum, "ctrain_ambient_sum", 3e-5), (dep, "ctrain_depth", 2e-4), (img, "ctrain_image", 3e-5)):
        np.testing.assert_allclose(cpu(got), gold[key], rtol=0, atol=tol, err_msg=key)
    gs, gr, ga = torch.zeros_like(sg), torch.zeros_like(rg), torch.zeros_like(am)
    call(rmb, "composite_rays_train_backward", T("ctrain_g_ws"), T("ctrain_g_as"), T("ctrain_g_im"), sg, rg, am, dlt.contiguous(), rays, wsum, asum,
         img, mcount, N, 1e-4, gs, gr, ga)
    for got, key in ((gs, "ctrain_grad_sigmas"), (gr, "ctrain_grad_rgbs"), (ga, "ctrain_grad_ambient")):
        np.testing.assert_allclose(cpu(got), gold[key], rtol=0, atol=2e-4, err_msg=key)
    # ---- _gridencoder: 3 functions (grid.py:27-89: [L,B,C] outputs, permuted by the wrapper; [L,B,C] gradients in)
    from gridencoder import GridEncoder
    for name, seed in (("hash3d", 100 + len("hash3d")), ("tiled2d", 100 + len("tiled2d"))):
        kw, x, grad = cases.grid_case(name)
        enc = cases.redraw_table(GridEncoder(**kw), seed).to(dev)
        D, L, C = kw["input_dim"], kw["num_levels"], kw["level_dim"]
        B = x.shape[0]
        S, Hb = float(np.log2(enc.per_level_scale)), enc.base_resolution
        xin = ((x + 1) / 2).to(dev).contiguous()                                   # GridEncoder.forward, bound = 1 (grid.py:151)
        emb = enc.embeddings.detach()
        out = torch.empty(L, B, C, device=dev)
        dy_dx = torch.empty(B, L * D * C, device=dev) if name == "tiled2d" else None
        call(geb, "grid_encode_forward", xin, emb, enc.offsets, out, B, D, C, L, S, Hb, dy_dx, enc.gridtype_id, False, 0)
        assert np.array_equal(cpu(out.permute(1, 0, 2).reshape(B, L * C)), gold[f"grid_{name}_out"]), name
        g = grad.to(dev).view(B, L, C).permute(1, 0, 2).contiguous()               # grid.py:75
        g_emb = torch.zeros_like(emb)
        g_in = torch.zeros(B, D, device=dev) if dy_dx is not None else None
        call(geb, "grid_encode_backward", g, xin, emb, enc.offsets, g_emb, B, D, C, L, S, Hb, dy_dx, g_in, enc.gridtype_id, False, 0)
        np.testing.assert_allclose(cpu(g_emb), gold[f"grid_{name}_grad_table"], rtol=1e-5, atol=1e-5)
        if g_in is not None:
            np.testing.assert_allclose(cpu(g_in) / 2, gold[f"grid_{name}_grad_inputs"], rtol=1e-5, atol=2e-4)   # d/dx of (x + 1) / 2
    kw, x, _ = cases.grid_case("tv3d")
    enc = cases.redraw_table(GridEncoder(**kw), 77).to(dev)
    g_tv = torch.zeros_like(enc.embeddings)
    xin = ((x + 1) / 2).to(dev).contiguous()
    call(geb, "grad_total_variation", xin, enc.embeddings.detach(), g_tv, enc.offsets, 1e-3, x.shape[0], 3, 2, kw["num_levels"],
         float(np.log2(enc.per_level_scale)), enc.base_resolution, enc.gridtype_id, False)
    np.testing.assert_allclose(cpu(g_tv), gold["grid_tv3d_grad"], rtol=1e-4, atol=1e-7)
    # ---- _shencoder, _freqencoder: 2 + 2 functions
    d, g = cases.dir_case()
    din, B = d.to(dev), d.shape[0]
    sh, dy = torch.empty(B, 16, device=dev), torch.empty(B, 3 * 16, device=dev)
    call(shb, "sh_encode_forward", din, sh, B, 3, 4, dy)
    np.testing.assert_allclose(cpu(sh), gold["sh_out"], rtol=0, atol=2e-6)
    g_in = torch.zeros(B, 3, device=dev)
    call(shb, "sh_encode_backward", g.to(dev), din, B, 3, 4, dy, g_in)
    np.testing.assert_allclose(cpu(g_in), gold["sh_grad_inputs"], rtol=1e-5, atol=2e-5)
    for D, deg in ((2, 10), (6, 4)):
        x, g = cases.freq_case(D, deg)
        xin, B, C = x.to(dev), x.shape[0], D + D * 2 * deg
        y = torch.empty(B, C, device=dev)
        call(fqb, "freq_encode_forward", xin, B, D, deg, C, y)
        np.testing.assert_allclose(cpu(y), gold[f"freq{D}_out"], rtol=0, atol=2e-6 * 2 ** deg)
        g_in = torch.zeros(B, D, device=dev)
        call(fqb, "freq_encode_backward", g.to(dev), y, B, D, deg, C, g_in)
        np.testing.assert_allclose(cpu(g_in), gold[f"freq{D}_grad_inputs"], rtol=1e-4, atol=2e-3 * 2 ** deg)
    want = {fn for fns in REFERENCE_SURFACE.values() for fn in fns}
    assert called == want and len(called) == 19, want ^ called
