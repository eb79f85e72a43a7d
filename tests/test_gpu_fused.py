"""GPU parity of the MI355X-native fused path (include/radnerf_fused.h) against the oracle and against the
per-operator engine.

Tolerances (fp32 everywhere; differences are summation order inside the MFMA tiles / folded bias vectors and
expf/tanhf implementations): per-sample sigma rel 2e-4, rgb / ambient abs 2e-5; frame |dRGB| <= 2e-3
(north-star bar; measured ~1e-6), integer loop statistics (iterations, live samples) exact.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _scene(size, engine, n_frames=8, **kw):
    from radnerf.scene import SyntheticScene, default_opt
    return SyntheticScene(H=size, W=size, n_frames=n_frames, device="cuda", opt=default_opt(engine=engine, **kw))


def test_symbols_of_fused_header_are_exported(hiplib):
    names = hiplib.exported_symbols()           # one table for the three headers: radnerf_fused.h's 54 functions are among its 105
    assert len(names) >= 105 and {"rn_nerf_fused_forward", "rn_head_iterate_ex", "rn_torso_blend_frame", "rn_adam_step_lr"} <= set(names)
    for name in names:
        assert hasattr(hiplib._lib, name), name


@pytest.mark.parametrize("mlp", ["f32", "f32x2"])      # fp32 MFMA / fp32-grade split products on the 16-bit MFMA: same bar
@pytest.mark.parametrize("M", [1, 63, 64, 65, 5000, 100003])
def test_fused_network_matches_oracle(po, hiplib, M, mlp):
    from radnerf import fused
    scene = _scene(16, "fused", mlp_dtype=mlp)
    m = scene.model
    rng = np.random.default_rng(M)
    x = rng.uniform(-0.7, 0.7, (M, 3)).astype(np.float32)
    if M > 10:
        x[3] = (1.5, 0.0, 0.0)   # outside [-bound, bound] -> enc_x = 0
    d = rng.standard_normal((M, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    enc_a = rng.standard_normal((1, 64)).astype(np.float32)
    eye = np.array([[0.25]], np.float32)
    c = m.individual_codes[0].detach()
    with torch.no_grad():
        sigma, color, amb = fused.network_forward(m, torch.from_numpy(x).cuda(), torch.from_numpy(d).cuda(),
                                                  torch.from_numpy(enc_a).cuda(), c, torch.from_numpy(eye).cuda())
    om = po.model_from_module(m)
    es, ec, ea = po.nerf_forward(om, x, d, enc_a, c.cpu().numpy(), eye)
    np.testing.assert_allclose(amb.cpu().numpy(), ea, rtol=0, atol=2e-5)
    np.testing.assert_allclose(sigma.cpu().numpy(), es, rtol=2e-4, atol=1e-6)
    np.testing.assert_allclose(color.cpu().numpy(), ec, rtol=0, atol=2e-5)


def test_fused_network_skips_dead_slots(po, hiplib):
    from radnerf import fused
    scene = _scene(16, "fused")
    m = scene.model
    rng = np.random.default_rng(5)
    M = 1000
    x = rng.uniform(-0.5, 0.5, (M, 3)).astype(np.float32)
    d = np.tile(np.array([[0.0, -1.0, 0.0]], np.float32), (M, 1))
    deltas = np.stack([np.full(M, 0.027), np.full(M, 3.0)], 1).astype(np.float32)
    dead = rng.uniform(size=M) < 0.5
    dead[64:192] = True  # two whole wave tiles dead
    deltas[dead] = 0
    enc_a = rng.standard_normal((1, 64)).astype(np.float32)
    eye = np.array([[0.25]], np.float32)
    c = m.individual_codes[0].detach()
    with torch.no_grad():
        sigma, color, _ = fused.network_forward(m, torch.from_numpy(x).cuda(), torch.from_numpy(d).cuda(),
                                                torch.from_numpy(enc_a).cuda(), c, torch.from_numpy(eye).cuda(),
                                                deltas=torch.from_numpy(deltas).cuda())
    es, ec, _ = po.nerf_forward(po.model_from_module(m), x, d, enc_a, c.cpu().numpy(), eye)
    np.testing.assert_allclose(sigma.cpu().numpy()[~dead], es[~dead], rtol=2e-4, atol=1e-6)
    np.testing.assert_allclose(color.cpu().numpy()[~dead], ec[~dead], rtol=0, atol=2e-5)


def _oracle_frame(po, scene, f, enc_a):
    m = scene.model
    om = po.model_from_module(m)
    rc = po.render_cfg_from_module(m, scene.opt.dt_gamma, scene.opt.max_steps)
    return po.render_frame(om, rc, f["rays_o"].cpu().numpy(), f["rays_d"].cpu().numpy(), enc_a.cpu().numpy(),
                           m.individual_codes[0].detach().cpu().numpy(), f["eye"].cpu().numpy(),
                           f["bg_coords"].cpu().numpy(), f["poses"].cpu().numpy(),
                           m.individual_codes_torso[0].detach().cpu().numpy(), f["bg_color"].reshape(-1, 3).cpu().numpy())


@pytest.mark.parametrize("mlp", ["f32", "f32x2"])
@pytest.mark.parametrize("size", [32, 64, 160])
def test_fused_frame_matches_oracle(po, hiplib, size, mlp):
    scene = _scene(size, "fused", mlp_dtype=mlp)
    for i in range(3):  # iteration hint adapts after the first frame; EMA state advances
        f = scene.frame(i)
        with torch.no_grad():
            out = scene.render(i)
        enc_a = scene.model.enc_a
        img, dep, stats = _oracle_frame(po, scene, f, enc_a)
        got = out["image"].reshape(-1, 3).cpu().numpy()
        st = scene.model.last_stats
        assert st["iterations"] == stats["iterations"]
        assert st["live_samples"] == stats["live_samples"]
        assert np.abs(got - img).max() <= 2e-3, np.abs(got - img).max()
        gd = out["depth"].reshape(-1).cpu().numpy()
        assert np.array_equal(np.isnan(gd), np.isnan(dep))
        ok = ~np.isnan(dep)
        assert np.abs(gd[ok] - dep[ok]).max() <= 1e-3


HASH19 = dict(xyz_grid="hashgrid", xyz_log2_hashmap_size=19)   # BASELINE config[1]


# ---- opt-in 16-bit matrix-core variant (opt.mlp_dtype = "f16", include/radnerf_fused.h) ---------------------------
# Checker: the oracle run under the same arithmetic (orc_nerf_forward_mp16: fp16 operands into the contractions, fp32
# accumulation).  Two independent implementations of that arithmetic differ only by fp32 summation order and by the
# rare fp16 rounding flip it causes (an activation that sits on a rounding boundary moves by one fp16 ulp, up to 2^-7
# for hidden values in [8, 16)): 99.9 % of the outputs agree to 1e-4 (sigma: rel 1e-3), every output to 1e-2 (sigma: rel 3e-2).
# Against the fp32 oracle the mode itself costs at most ~1e-2 per sample and <= 4e-3 (one 8-bit step) per rendered
# pixel -- stated here, measured ~1e-3.
def _close_up_to_rounding_flips(got, want, bulk_atol, rel=False):
    err = np.abs(got - want) / (np.abs(want) if rel else 1.0)
    assert float((err <= bulk_atol).mean()) >= 0.999, float((err <= bulk_atol).mean())
    assert float(err.max()) <= (3e-2 if rel else 1e-2), float(err.max())     # sigma = exp(raw) turns abs into rel


@pytest.mark.parametrize("M", [1, 64, 65, 5000, 100003])
@pytest.mark.parametrize("grid", ["tiled16", "hash19"])
def test_fused_f16_network_matches_mp16_oracle(po, hiplib, M, grid):
    from radnerf import fused
    kw = HASH19 if grid == "hash19" else {}
    scene = _scene(16, "fused", mlp_dtype="f16", **kw)
    m = scene.model
    rng = np.random.default_rng(M + 7)
    x = rng.uniform(-0.7, 0.7, (M, 3)).astype(np.float32)
    if M > 10:
        x[3] = (1.5, 0.0, 0.0)   # outside [-bound, bound] -> enc_x = 0
    d = rng.standard_normal((M, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    enc_a = rng.standard_normal((1, 64)).astype(np.float32)
    eye = np.array([[0.25]], np.float32)
    c = m.individual_codes[0].detach()
    with torch.no_grad():
        sigma, color, amb = fused.network_forward(m, torch.from_numpy(x).cuda(), torch.from_numpy(d).cuda(),
                                                  torch.from_numpy(enc_a).cuda(), c, torch.from_numpy(eye).cuda())
    om = po.model_from_module(m)
    es, ec, ea = po.nerf_forward(om, x, d, enc_a, c.cpu().numpy(), eye, mlp_dtype="f16")
    _close_up_to_rounding_flips(amb.cpu().numpy(), ea, 1e-4)
    _close_up_to_rounding_flips(sigma.cpu().numpy(), es, 1e-3, rel=True)
    _close_up_to_rounding_flips(color.cpu().numpy(), ec, 1e-4)
    fs, fc, fa = po.nerf_forward(om, x, d, enc_a, c.cpu().numpy(), eye)            # the fp32 truth
    assert np.abs(color.cpu().numpy() - fc).max() < 1e-2 and np.abs(amb.cpu().numpy() - fa).max() < 1e-2
    assert np.abs(sigma.cpu().numpy() / fs - 1).max() < 3e-2


@pytest.mark.parametrize("size", [64, 160])
def test_fused_f16_frame_within_one_8bit_step_of_fp32_oracle(po, hiplib, size):
    scene = _scene(size, "fused", mlp_dtype="f16")
    worst = 0.0
    for i in range(2):
        f = scene.frame(i)
        with torch.no_grad():
            out = scene.render(i)
        img, dep, stats = _oracle_frame(po, scene, f, scene.model.enc_a)
        got = out["image"].reshape(-1, 3).cpu().numpy()
        worst = max(worst, float(np.abs(got - img).max()))
        assert scene.model.last_stats["iterations"] == stats["iterations"]
    assert worst <= 4e-3, worst


def test_fused_f16_and_f32_share_one_model(hiplib):
    """Switching opt.mlp_dtype re-packs the weight image (FusedState.refresh keys on it)."""
    a = _scene(48, "fused")
    with torch.no_grad():
        i32 = a.render(0)["image"].clone()
        a.model.opt.mlp_dtype = "f16"
        a.model.enc_a = None
        i16 = a.render(0)["image"].clone()
        a.model.opt.mlp_dtype = "f32"
        a.model.enc_a = None
        back = a.render(0)["image"].clone()
    assert torch.equal(i32, back)
    d = (i32 - i16).abs().max().item()
    assert 0 < d <= 4e-3, d


@pytest.mark.parametrize("engine", ["fused", "fused-f32x2", "ops"])
def test_hash_grid_frame_matches_oracle(po, hiplib, engine):
    """BASELINE config[1] names an instant-ngp hash grid with T=2^19 for xyz: levels 5..15 go through fast_hash
    (gridencoder.cu:57-74, 98-99) instead of the tiled modulo."""
    mlp = "f32x2" if engine.endswith("x2") else "f32"
    engine = engine.split("-")[0]
    scene = _scene(64, engine, mlp_dtype=mlp, **HASH19)
    assert scene.model.encoder.gridtype == "hash" and scene.model.encoder.embeddings.shape[0] > 16 * 2 ** 16
    for i in range(2):
        f = scene.frame(i)
        with torch.no_grad():
            out = scene.render(i)
        img, dep, stats = _oracle_frame(po, scene, f, scene.model.enc_a)
        got = out["image"].reshape(-1, 3).cpu().numpy()
        assert np.abs(got - img).max() <= 2e-3, np.abs(got - img).max()
        if engine == "fused":
            st = scene.model.last_stats
            assert st["iterations"] == stats["iterations"] and st["live_samples"] == stats["live_samples"]


def test_hash_grid_fused_network_matches_oracle(po, hiplib):
    from radnerf import fused
    scene = _scene(16, "fused", **HASH19)
    m = scene.model
    rng = np.random.default_rng(19)
    M = 20011
    x = rng.uniform(-0.9, 0.9, (M, 3)).astype(np.float32)
    d = rng.standard_normal((M, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    enc_a = rng.standard_normal((1, 64)).astype(np.float32)
    eye = np.array([[0.4]], np.float32)
    c = m.individual_codes[1].detach()
    with torch.no_grad():
        sigma, color, amb = fused.network_forward(m, torch.from_numpy(x).cuda(), torch.from_numpy(d).cuda(),
                                                  torch.from_numpy(enc_a).cuda(), c, torch.from_numpy(eye).cuda())
    es, ec, ea = po.nerf_forward(po.model_from_module(m), x, d, enc_a, c.cpu().numpy(), eye)
    np.testing.assert_allclose(amb.cpu().numpy(), ea, rtol=0, atol=2e-5)
    np.testing.assert_allclose(sigma.cpu().numpy(), es, rtol=2e-4, atol=1e-6)
    np.testing.assert_allclose(color.cpu().numpy(), ec, rtol=0, atol=2e-5)


def test_fused_equals_ops_engine(hiplib):
    a, b = _scene(96, "fused", ray_engine="torch"), _scene(96, "ops")     # same rays for both (rn_get_rays differs by 1 ulp)
    for i in range(2):
        with torch.no_grad():
            ia = a.render(i)["image"]
            ib = b.render(i)["image"]
        assert (ia - ib).abs().max().item() <= 1e-4


def test_opaque_regime_early_termination(po, hiplib):
    """Regime A: sigma scaled up (x80: 10/50/90th percentile 22 / 67 / 287 inside the head) so rays terminate
    on T < T_thresh -- half the samples and 4 instead of 6 loop iterations of regime B; engine and oracle agree."""
    scene = _scene(64, "fused")
    with torch.no_grad():
        scene.model.sigma_net.net[-1].weight[0].abs_().mul_(80.0)
    f = scene.frame(0)
    with torch.no_grad():
        out = scene.render(0)
    img, dep, stats = _oracle_frame(po, scene, f, scene.model.enc_a)
    st = scene.model.last_stats
    assert stats["live_samples"] < 12000 and stats["iterations"] < 6      # regime B: 19 300 samples, 6 iterations
    assert st["iterations"] == stats["iterations"]
    assert abs(st["live_samples"] - stats["live_samples"]) <= 0.002 * stats["live_samples"] + 8  # knife-edge T tests
    assert np.abs(out["image"].reshape(-1, 3).cpu().numpy() - img).max() <= 2e-3


def test_torso_fused_matches_oracle(po, hiplib):
    import ctypes as C
    import radnerf_hip as hip
    import torch.nn.functional as F
    from radnerf import fused
    scene = _scene(80, "fused")
    m = scene.model
    st = fused._state(m)
    st.refresh()
    N = 80 * 80
    f = scene.frame(0)
    bg_coords = f["bg_coords"].reshape(-1, 2).contiguous()
    rng = np.random.default_rng(0)
    bg_in = torch.from_numpy(rng.uniform(0, 1, (N, 3)).astype(np.float32)).cuda()
    bg_out = torch.empty(N, 3, device="cuda")
    alpha = torch.empty(N, device="cuda")
    deform = torch.empty(N, 2, device="cuda")
    thresh = min(m.density_thresh_torso, m.mean_density_torso)
    poses = f["poses"].reshape(-1).contiguous()
    ict = m.individual_codes_torso[0].detach().contiguous()
    hip.call("rn_torso_fused", hip.ptr(bg_coords), N, hip.ptr(m.density_grid_torso), 128, float(thresh), hip.ptr(poses),
             hip.ptr(ict), float(m.opt.torso_shrink), C.byref(st.tw), hip.ptr(st.tpacked), C.byref(st.gt), hip.ptr(bg_in),
             hip.ptr(bg_out), hip.ptr(alpha), hip.ptr(deform), hip.stream())
    occ = F.grid_sample(m.density_grid_torso.view(1, 1, 128, 128), bg_coords.view(1, -1, 1, 2), align_corners=True).view(-1)
    mask = (occ > thresh).cpu().numpy()
    om = po.model_from_module(m)
    ea, ec, edx = po.torso_forward(om, bg_coords.cpu().numpy()[mask], poses.cpu().numpy(), ict.cpu().numpy())
    ga, gd = alpha.cpu().numpy(), deform.cpu().numpy()
    assert mask.sum() > 500
    assert not ga[~mask].any() and not gd[~mask].any()
    np.testing.assert_allclose(gd[mask], edx, rtol=0, atol=3e-5)
    np.testing.assert_allclose(ga[mask], ea[:, 0], rtol=0, atol=3e-5)
    exp_bg = bg_in.cpu().numpy().copy()
    exp_bg[mask] = ec * ea + exp_bg[mask] * (1 - ea)
    np.testing.assert_allclose(bg_out.cpu().numpy(), exp_bg, rtol=0, atol=5e-5)


@pytest.mark.parametrize("mlp", ["f32", "f32x2", "f16"])
def test_fused_kernels_are_deterministic(hiplib, mlp):
    """Same inputs, 12 launches, identical bits.  (Guards the finding recorded in DESIGN.md section 3: built on the
    double-rate v_mfma_f32_32x32x16_f16 the f16 kernels were not, with two waves per SIMD.)"""
    from radnerf import fused
    scene = _scene(16, "fused", mlp_dtype=mlp)
    m = scene.model
    M = 20000
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.rand(M, 3, device="cuda", generator=g) * 1.4 - 0.7
    d = torch.nn.functional.normalize(torch.randn(M, 3, device="cuda", generator=g), dim=1)
    enc_a = torch.randn(1, 64, device="cuda", generator=g)
    eye = torch.tensor([[0.25]], device="cuda")
    c = m.individual_codes[0].detach()
    with torch.no_grad():
        first = [t.clone() for t in fused.network_forward(m, x, d, enc_a, c, eye)]
        for _ in range(11):
            again = fused.network_forward(m, x, d, enc_a, c, eye)
            for a, b in zip(first, again):
                assert torch.equal(a, b)


def test_speculative_loop_length_is_flagged_when_too_small(po, hiplib):
    """set_loop_hint: frames rendered with enough iterations equal the full loop and are not flagged; a hint that is
    too small is flagged on the device (rn_head_check_done) so the caller can render again."""
    from radnerf import fused
    a, b = _scene(64, "fused"), _scene(64, "fused")
    with torch.no_grad():
        full = a.render(0)["image"].clone()
        need = a.model.last_stats["iterations"]
        b.render(1)                                   # creates the state
        b.model.enc_a = None
        fused.set_loop_hint(b.model, need + 1)
        b.model.enc_a = None
        again = _scene(64, "fused")
        fused._state(again.model)
        fused.set_loop_hint(again.model, need + 1)
        img = again.render(0)["image"]
        assert torch.equal(img, full) and fused.unfinished_frames(again.model) == 0
        fused.set_loop_hint(again.model, max(1, need - 2))
        again.model.enc_a = None
        again.render(0)
        assert fused.unfinished_frames(again.model) == 1
        fused.set_loop_hint(again.model, None)
        again.model.enc_a = None
        assert torch.equal(again.render(0)["image"], full) and fused.unfinished_frames(again.model) == 1


def test_frame_parallel_renderer_learns_the_loop_length(hiplib):
    from radnerf import fused
    from radnerf.parallel import FrameParallelRenderer
    ref, spec = _scene(64, "fused"), _scene(64, "fused")
    with torch.no_grad():
        want = [ref.render(i)["image"].clone() for i in range(6)]
        fpr = FrameParallelRenderer(spec, 0, 1, None, gather=False, speculate_loop=True)
        got = [fpr.step(i) for i in range(3)]
        fpr.finish()
        hint = fused._state(spec.model).loop_hint
        assert hint is not None and hint < spec.opt.max_steps
        got += [fpr.step(i) for i in range(3, 6)]
        fpr.finish()                                   # would raise LoopHintTooSmall
    for g, w in zip(got, want):
        assert torch.equal(g, (w.reshape(64, 64, 3) * 255).to(torch.uint8))


@pytest.mark.parametrize("mlp", ["f32", "f32x2", "f16"])
def test_block_ray_order_changes_no_pixel(hiplib, mlp):
    """rn_head_t.order_w (8 x 8 pixel blocks in the alive list) is a speed knob: rays are independent, so image, depth and
    the loop statistics are identical to the plain ray order -- bit for bit.  Also: a width the frame does not fit is ignored."""
    outs = []
    for width in (0, 64, 48):                 # 48: N / width is not an integer -> treated as 0
        scene = _scene(64, "fused", mlp_dtype=mlp)
        scene.model.ray_order_width = width
        with torch.no_grad():
            out = scene.render(1)
        outs.append((out["image"].clone(), out["depth"].clone(), dict(scene.model.last_stats)))
    for img, dep, st in outs[1:]:
        assert torch.equal(img, outs[0][0])
        assert torch.equal(torch.nan_to_num(dep, nan=-1.0), torch.nan_to_num(outs[0][1], nan=-1.0))
        assert st == outs[0][2]


def _recap_levels(enc, cap, seed):
    """Give every level of a GridEncoder at most `cap` rows (a multiple of 8 that is NOT a power of two) and re-draw the table:
    capped levels then need a true `index % rows` -- the "generic" level kind of the fused kernels' plans."""
    D = enc.input_dim
    S, H = float(np.log2(enc.per_level_scale)), enc.base_resolution
    offs = [0]
    for l in range(enc.num_levels):
        res = int(np.ceil(np.exp2(l * S) * H - 1.0)) + 1
        rows = min(cap, (res + 1) ** D)
        offs.append(offs[-1] + int(np.ceil(rows / 8) * 8))
    enc.offsets = torch.tensor(offs, dtype=enc.offsets.dtype, device=enc.offsets.device)
    g = torch.Generator().manual_seed(seed)
    enc.embeddings = torch.nn.Parameter(((torch.rand(offs[-1], enc.level_dim, generator=g) * 2 - 1) * 0.5).to(enc.offsets.device))


@pytest.mark.parametrize("mlp", ["f32", "f32x2"])
@pytest.mark.parametrize("grid", ["hashgrid", "tiledgrid"])
def test_fused_network_with_non_power_of_two_levels(po, hiplib, grid, mlp):
    """Row counts that are neither dense nor a power of two (not produced by the reference's own offsets, but legal for the
    C ABI): hashed AND tiled levels go through the plans' generic modulo and still match the oracle's `index % rows`."""
    from radnerf import fused
    scene = _scene(16, "fused", mlp_dtype=mlp, xyz_grid=grid, xyz_log2_hashmap_size=17)
    m = scene.model
    _recap_levels(m.encoder, 50000, 1)
    _recap_levels(m.encoder_ambient, 3000, 2)
    rng = np.random.default_rng(23)
    M = 6007
    x = rng.uniform(-0.9, 0.9, (M, 3)).astype(np.float32)
    d = rng.standard_normal((M, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    enc_a = rng.standard_normal((1, 64)).astype(np.float32)
    eye = np.array([[0.4]], np.float32)
    c = m.individual_codes[1].detach()
    with torch.no_grad():
        sigma, color, amb = fused.network_forward(m, torch.from_numpy(x).cuda(), torch.from_numpy(d).cuda(),
                                                  torch.from_numpy(enc_a).cuda(), c, torch.from_numpy(eye).cuda())
    es, ec, ea = po.nerf_forward(po.model_from_module(m), x, d, enc_a, c.cpu().numpy(), eye)
    np.testing.assert_allclose(amb.cpu().numpy(), ea, rtol=0, atol=2e-5)
    np.testing.assert_allclose(sigma.cpu().numpy(), es, rtol=2e-4, atol=1e-6)
    np.testing.assert_allclose(color.cpu().numpy(), ec, rtol=0, atol=2e-5)


@pytest.mark.parametrize("mlp", ["f32", "f32x2", "f16"])
def test_live_sample_list_changes_no_pixel(hiplib, mlp):
    """rn_head_t.live_slots (the marchers list the live sample slots, the network kernels skip the dead ones) against the
    plain walk over all n_alive * n_step slots (opt.live_list = False): same image, depth and loop statistics, bit for bit."""
    outs = []
    for live_list in (True, False):
        scene = _scene(96, "fused", mlp_dtype=mlp, live_list=live_list)
        with torch.no_grad():
            for i in range(2):
                out = scene.render(i)
        outs.append((out["image"].clone(), out["depth"].clone(), dict(scene.model.last_stats)))
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(torch.nan_to_num(outs[0][1], nan=-1.0), torch.nan_to_num(outs[1][1], nan=-1.0))
    assert outs[0][2] == outs[1][2]
    assert outs[0][2]["live_samples"] < outs[0][2]["sample_slots"]      # there ARE dead slots to skip


@pytest.mark.parametrize("mlp", ["f32", "f32x2", "f16"])
def test_frames_are_bit_stable_across_repeats(hiplib, mlp):
    """The live-sample list is filled in the workgroups' arrival order, which differs from run to run; every sample is
    computed on its own lane and written back to its slot, so the frame must not: 12 renders of one frame agree bit for bit."""
    scene = _scene(128, "fused", mlp_dtype=mlp, smooth_lips=False)     # no EMA state: every render sees the same audio code
    ref = None
    with torch.no_grad():
        for _ in range(12):
            out = scene.render(2)
            img, dep = out["image"].clone(), torch.nan_to_num(out["depth"], nan=-1.0).clone()
            if ref is None:
                ref = (img, dep)
            assert torch.equal(img, ref[0]) and torch.equal(dep, ref[1])


@pytest.mark.parametrize("mlp", ["f32", "f16"])
def test_merged_frame_kernels_change_no_pixel(hiplib, mlp):
    """The one-launch prologue (rays from the pose + near/far + initialisation + march of iteration 0), the loop's last
    compaction doing the check_done bookkeeping, and the torso pass with the blend folded in, against the kernel-per-stage
    sequence (opt.frame_kernels = "separate"): same image, depth, torso layer, uint8 frame and loop statistics, bit for bit --
    over three frames, so the live-sample counters the prologue relies on are seen to be left at zero."""
    a, b = _scene(96, "fused", mlp_dtype=mlp), _scene(96, "fused", mlp_dtype=mlp, frame_kernels="separate")
    for i in range(3):
        with torch.no_grad():
            oa, ob = a.render(i, want_u8=True), b.render(i, want_u8=True)
        for key in ("image", "torso_alpha", "torso_color", "image_u8"):
            assert torch.equal(oa[key], ob[key]), (i, key)
        assert torch.equal(torch.nan_to_num(oa["depth"], nan=-1.0), torch.nan_to_num(ob["depth"], nan=-1.0))
        assert dict(a.model.last_stats) == dict(b.model.last_stats)
    from radnerf import fused
    assert fused.unfinished_frames(a.model) == 0 and fused._state(a.model).state[[6, 14]].tolist() == [0, 0]


@pytest.mark.parametrize("size,kernels", [(96, "merged"), (96, "separate"), (512, "merged")])
def test_one_launch_loop_step_changes_no_pixel(hiplib, size, kernels):
    """opt.loop_launch = "coop" (compositor + compaction + next march of an iteration in one launch with a grid-wide
    barrier inside, RN_LOOP_COOP) against the default "split" (a launch each for the compositor and the compaction): same frames, same
    loop statistics, bit for bit; no workgroup ever gives up at the barrier.  512^2 = 1024 chunks of the alive list on 512
    workgroups: the chunk loops of both phases are exercised."""
    from radnerf import fused
    a = _scene(size, "fused", frame_kernels=kernels, loop_launch="coop")
    b = _scene(size, "fused", frame_kernels=kernels)
    assert fused.loop_flags(a.model) == fused.RN_LOOP_COOP and fused.loop_flags(b.model) == 0
    for i in range(3):
        with torch.no_grad():
            oa, ob = a.render(i, want_u8=True), b.render(i, want_u8=True)
        for key in ("image", "image_u8", "weights_sum"):
            if key in oa and key in ob:
                assert torch.equal(oa[key], ob[key]), (i, key)
        assert torch.equal(torch.nan_to_num(oa["depth"], nan=-1.0), torch.nan_to_num(ob["depth"], nan=-1.0))
        assert dict(a.model.last_stats) == dict(b.model.last_stats)
        assert torch.equal(fused.loop_history(a.model, 17), fused.loop_history(b.model, 17))
    assert fused.stalled_workgroups(a.model) == 0 and fused.unfinished_frames(a.model) == 0
    assert fused._state(a.model).state[[6, 14]].tolist() == [0, 0]


def test_audio_batches_equal_the_per_frame_audio_path(hiplib):
    """FrameParallelRenderer(audio_batch=K): codes, smoothing recurrence and bias blocks of K frames in four launches; the
    frames must be the ones the per-frame path renders (same kernels on the same numbers)."""
    from radnerf.parallel import FrameParallelRenderer
    for world, rank in ((1, 0), (3, 1)):
        a, b = _scene(64, "fused"), _scene(64, "fused")
        with torch.no_grad():
            fa = FrameParallelRenderer(a, rank, world, None, gather=False, audio_batch=4)
            fb = FrameParallelRenderer(b, rank, world, None, gather=False)
            for s in range(7):                                     # a full batch, then a partial one
                assert torch.equal(fa.step(s), fb.step(s)), (world, s)


def test_two_frames_in_flight_render_the_same_frames(hiplib):
    """FrameParallelRenderer(streams=2): consecutive frames alternate between two HIP streams (own loop state, scratch and ray
    buffers each); the frames are those of the one-stream renderer, bit for bit."""
    from radnerf.parallel import FrameParallelRenderer
    a, b = _scene(96, "fused"), _scene(96, "fused")
    with torch.no_grad():
        fa = FrameParallelRenderer(a, 0, 1, None, gather=False, audio_batch=4, streams=2, speculate_loop=True)
        fb = FrameParallelRenderer(b, 0, 1, None, gather=False, audio_batch=4)
        got = [fa.step(s) for s in range(6)]
        fa.finish()
        got += [fa.step(s) for s in range(6, 11)]          # after finish(): with the learned loop length
        fa.finish()
        want = [fb.step(s) for s in range(11)]
        fb.finish()
    torch.cuda.synchronize()
    for s, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g, w), s


@pytest.mark.parametrize("H,W", [(24, 40), (37, 53)])
def test_loop_with_a_partial_last_chunk(hiplib, H, W):
    """Frames whose ray count is no multiple of the loop's 256-ray chunk: 24 x 40 = 960 rays (block order usable, last chunk of
    192 lanes) and 37 x 53 = 1 961 rays (block order refused, last chunk of 169 lanes = two full waves + 41).  The loop's
    variants -- merged / separate prologue, one-launch / split step, block / plain ray order -- must agree on image, depth and
    the loop statistics bit for bit over two frames, no workgroup may give up at the barrier, and the frames must be those of
    the per-operator engine on the same rays (the bar of test_fused_equals_ops_engine)."""
    from radnerf import fused
    from radnerf.scene import SyntheticScene, default_opt

    def frames(order_w=W, engine="fused", **kw):
        scene = SyntheticScene(H=H, W=W, n_frames=8, device="cuda", opt=default_opt(engine=engine, **kw))
        scene.model.ray_order_width = order_w
        outs = []
        for i in range(2):
            with torch.no_grad():
                out = scene.render(i)
            outs.append((out["image"].clone(), torch.nan_to_num(out["depth"], nan=-1.0).clone(), dict(scene.model.last_stats)))
        if engine == "fused":
            assert fused.stalled_workgroups(scene.model) == 0 and fused.unfinished_frames(scene.model) == 0
        return outs

    assert H * W % 256 != 0
    base = frames()
    variants = {"separate prologue": frames(frame_kernels="separate"), "one-launch step": frames(loop_launch="coop"),
                "plain ray order": frames(order_w=0)}
    for name, outs in variants.items():
        for i, (got, want) in enumerate(zip(outs, base)):
            assert torch.equal(got[0], want[0]), (name, i, "image")
            assert torch.equal(got[1], want[1]), (name, i, "depth")
            assert got[2] == want[2], (name, i, got[2], want[2])
    same_rays, ops = frames(ray_engine="torch"), frames(engine="ops")
    for i in range(2):
        diff = (same_rays[i][0] - ops[i][0]).abs().max().item()
        print(f"{H}x{W} frame {i}: max |fused - ops| = {diff:.3e}")
        assert diff <= 1e-4
