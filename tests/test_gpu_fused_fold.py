"""The inference kernel's weight image folds sigma_net's geo_feat rows into color_net's first layer
(csrc/rn_nerf_image_dev.h: nerf_infer_image_elem): layout, accuracy against a float64 evaluation of the two-layer
module, re-pack when a weight changes in place, and sigma / ambient untouched by the fold.

Bars: the project's own (rgb / ambient abs 2e-5, sigma rel 2e-4 / abs 1e-6; tests/test_gpu_fused.py).  With both folded
layers scaled x8 the rgb bar is relative to what fp32 itself gives: the kernel's largest rgb error against the float64
truth is at most twice that of the two-layer form evaluated in fp32 (the factor covers summation order), by torch and by
the oracle, whose sums are sequential like the kernel's.  A folded element is a 64-term double sum rounded once, so it
may differ from numpy's by the order of the double additions: 1 fp32 ulp.

The float64 truth interpolates the grids on the lattice the kernels use: the level scale comes from libm's exp2f
(_level_scale), as in the kernels' host code.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import netref64

pytestmark = pytest.mark.gpu

GRIDS = {"tiled16": dict(xyz_grid="tiledgrid", xyz_log2_hashmap_size=16),
         "hash19": dict(xyz_grid="hashgrid", xyz_log2_hashmap_size=19)}

K_STEP = 128        # floats per MFMA step of a 64-row layer: [2 h][32 j][2 row tiles]


def _scene(**kw):
    from radnerf.scene import SyntheticScene, default_opt
    return SyntheticScene(H=16, W=16, n_frames=8, device="cuda", opt=default_opt(engine="fused", mlp_dtype="f32", **kw))


def rowmap(r, h):
    """Output row (within a 32-row tile) held by accumulator register r of lane half h (v_mfma_f32_32x32x2_f32)."""
    return (r & 3) + 8 * (r >> 2) + 4 * h


def kmap(s, h):
    """k (of 64) that lane half h feeds at step s of a layer whose input is the previous layer's accumulators."""
    return 32 * (s >> 4) + rowmap(s & 15, h)


def _mfma_block(src, n_steps, k_of):
    """[step][h][j][row tile] image of src [64, ld]: element = src[32 rt + j, k_of(step, h)]."""
    out = np.empty((n_steps, 2, 32, 2), src.dtype)
    for s in range(n_steps):
        for h in range(2):
            k = k_of(s, h)
            out[s, h, :, 0] = src[0:32, k]
            out[s, h, :, 1] = src[32:64, k]
    return out.reshape(-1)


def _valu_block(src):
    """[out][h][q] image of src [n_out, 64]: q = 16 rt + r -> src[o, 32 rt + rowmap(r, h)]."""
    out = np.empty((src.shape[0], 2, 32), src.dtype)
    for h in range(2):
        for q in range(32):
            out[:, h, q] = src[:, 32 * (q >> 4) + rowmap(q & 15, h)]
    return out.reshape(-1)


def _gather_k(s, h):
    return 4 * (s >> 1) + 2 * h + (s & 1)        # gather round s / 2: half h holds level 2 (s / 2) + h, steps = its 2 features


def _documented_image(ws):
    """(prefix, sigma row, colour L0 SH steps, folded steps in float64, colour L1) from the eight raw weights."""
    amb_w0, amb_w1, amb_w2, sig_w0, sig_w1, sig_w2, col_w0, col_w1 = ws
    prefix = np.concatenate([_mfma_block(amb_w0, 16, _gather_k), _mfma_block(amb_w1, 32, kmap), _valu_block(amb_w2),
                             _mfma_block(sig_w0, 32, _gather_k), _mfma_block(sig_w1, 32, kmap)])
    sigma_row = _valu_block(sig_w2[0:1])
    sh = _mfma_block(col_w0, 8, lambda s, h: 2 * s + h)
    folded64 = col_w0[:, 16:80].astype(np.float64) @ sig_w2[1:65].astype(np.float64)        # [64 colour rows, 64 hidden k]
    folded = _mfma_block(folded64, 32, kmap)
    return prefix, sigma_row, sh, folded, _valu_block(col_w1)


def test_packed_image_is_the_documented_layout_with_the_folded_block(hiplib):
    from radnerf import fused
    m = _scene().model
    st = fused._state(m)
    st.refresh()
    n = int(hiplib._lib.rn_nerf_packed_floats())
    assert n == 23936 - 32 * K_STEP
    got = st.packed[:n].cpu().numpy()
    ws = [w.detach().cpu().numpy() for w in fused.head_weights(m)]
    prefix, sigma_row, sh, folded, col1 = _documented_image(ws)
    assert prefix.size == 14464 and prefix.size + sigma_row.size + sh.size + folded.size + col1.size == n
    o = 0
    for name, want in (("prefix", prefix), ("sigma row", sigma_row), ("colour L0, SH steps", sh)):
        assert np.array_equal(got[o:o + want.size], want), name
        o += want.size
    want32 = folded.astype(np.float32)
    diff = np.abs(got[o:o + folded.size].astype(np.float64) - want32.astype(np.float64))
    ulp = np.spacing(np.abs(want32)).astype(np.float64)
    print(f"folded block: {int((diff > 0).sum())} of {folded.size} elements differ from numpy's, max {float((diff / ulp).max()):.2f} ulp")
    assert (diff <= ulp).all()
    o += folded.size
    assert np.array_equal(got[o:], col1), "colour L1"


def _inputs(m, M, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.9, 0.9, (M, 3)).astype(np.float32)
    d = rng.standard_normal((M, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    enc_a = rng.standard_normal((1, 64)).astype(np.float32)
    eye = np.array([[0.4]], np.float32)
    return (torch.from_numpy(x).cuda(), torch.from_numpy(d).cuda(), torch.from_numpy(enc_a).cuda(),
            m.individual_codes[1].detach(), torch.from_numpy(eye).cuda())


_exp2f = C.CDLL("libm.so.6").exp2f
_exp2f.restype, _exp2f.argtypes = C.c_float, [C.c_float]


def _level_scale(l, S, H):
    """(scale, resolution) of level l as the kernels' host code and the oracle compute them (rn_grid_dev.h, orc_grid.c):
    exp2f((float)l * S) * (float)H - 1.0f with libm's exp2f.  numpy's float32 exp2 is one ulp away from it on levels 1, 3,
    6, 9 and 12 of these grids, which moves the lattice position by up to 1e-4 of a cell and a feature by up to 9e-5: a
    different function, not an error of the kernel."""
    scale = np.float32(_exp2f(np.float32(l) * np.float32(S))) * np.float32(H) - np.float32(1)
    return scale, int(np.ceil(scale)) + 1


def _grid_encode(x, table, enc, bound):
    """GridEncoder(x, bound) [N, L*C] in float64 (netref64.grid_encode with _level_scale): lattice position, cell and
    fractional position in fp32 exactly as the kernels compute them, interpolation in float64."""
    D, L, H = int(enc.input_dim), int(enc.num_levels), int(enc.base_resolution)
    S = float(np.log2(enc.per_level_scale))
    gridtype = int(enc.gridtype_id)
    off = [int(v) for v in enc.offsets.tolist()]
    bound32 = torch.tensor(bound, dtype=torch.float32)
    xn32 = (x.float() + bound32) / (2 * bound32)
    inside = ((xn32 >= 0) & (xn32 <= 1)).all(-1, keepdim=True).to(torch.float64)
    outs = []
    for l in range(L):
        scale, res = _level_scale(l, S, H)
        pos32 = xn32 * torch.tensor(scale) + torch.tensor(np.float32(0.5))
        cell = torch.floor(pos32)
        fr = (pos32 - cell).double()
        p0 = cell.long()
        acc = 0
        for corner in range(1 << D):
            w = 1
            pg = p0.clone()
            for k in range(D):
                bit = (corner >> k) & 1
                w = w * (fr[:, k] if bit else 1 - fr[:, k])
                pg[:, k] += bit
            rows = off[l] + netref64.grid_rows(pg, gridtype, off[l + 1] - off[l], res)
            acc = acc + w.unsqueeze(-1) * table[rows]
        outs.append(acc)
    return torch.cat(outs, -1) * inside


def _torch_forward(model, x, d, enc_a, c, e, dtype):
    """NeRFNetwork.forward, two separate layers, on the CPU: grid features from _grid_encode (the kernels' fp32 lattice
    positions, float64 interpolation), then every MLP, activation and the SH basis in `dtype`."""
    ref = netref64.Net64(model, device="cpu")
    P = {k: v.detach() for k, v in ref.P.items()}
    x, d, enc_a, e = x.cpu().double(), d.cpu().double(), enc_a.cpu().to(dtype), e.cpu().to(dtype)
    c = c.cpu().to(dtype)
    n = x.shape[0]
    ws = lambda net: [w.detach().to(dtype) for w in ref._ws(net)]
    enc_x = _grid_encode(x, P["encoder.embeddings"], model.encoder, ref.bound).to(dtype)
    ambient = torch.tanh(netref64.mlp(ws("ambient_net"), torch.cat([enc_x, enc_a.reshape(1, -1).expand(n, -1)], -1)))
    enc_w = _grid_encode(ambient.double(), P["encoder_ambient.embeddings"], model.encoder_ambient, 1.0).to(dtype)
    h = netref64.mlp(ws("sigma_net"), torch.cat([enc_x, enc_w, e.reshape(1, -1).expand(n, -1)], -1))
    sigma = torch.exp(h[:, 0])
    cols = [netref64.sh4(d.to(dtype)), h[:, 1:], c.reshape(1, -1).expand(n, -1)]
    rgb = torch.sigmoid(netref64.mlp(ws("color_net"), torch.cat(cols, -1)))
    return sigma.double().numpy(), rgb.double().numpy(), ambient.double().numpy()


def _run(m, inputs):
    from radnerf import fused
    with torch.no_grad():
        return [t.cpu().numpy().astype(np.float64) for t in fused.network_forward(m, *inputs)]


def _scale_folded_layers(m, factor=8.0):
    """sigma_net's last and color_net's first weight, IN PLACE: nothing tells the engine but the tensors' _version."""
    with torch.no_grad():
        m.sigma_net.net[-1].weight.mul_(factor)
        m.color_net.net[0].weight.mul_(factor)


@pytest.mark.parametrize("grid", ["tiled16", "hash19"])
def test_folded_kernel_meets_the_project_bars_against_float64(hiplib, grid):
    m = _scene(**GRIDS[grid]).model
    inputs = _inputs(m, 20011, 19)
    gs, gc, ga = _run(m, inputs)
    ts, tc, ta = _torch_forward(m, *inputs, torch.float64)
    print(f"{grid}: max |rgb - f64| {np.abs(gc - tc).max():.3e}, |ambient - f64| {np.abs(ga - ta).max():.3e}, "
          f"sigma rel {(np.abs(gs - ts) / np.abs(ts)).max():.3e}")
    np.testing.assert_allclose(ga, ta, rtol=0, atol=2e-5)
    np.testing.assert_allclose(gs, ts, rtol=2e-4, atol=1e-6)
    np.testing.assert_allclose(gc, tc, rtol=0, atol=2e-5)


@pytest.mark.parametrize("grid", ["tiled16", "hash19"])
def test_in_place_weight_change_is_repacked(hiplib, grid):
    """No explicit re-pack call: FusedState.refresh keys on the parameters' _version.  After the x8 the kernel follows the
    float64 truth of the NEW weights to 64 x the rgb bar (an error entering the two scaled layers grows by at most 8 x 8),
    while the new truth is more than 1e-3 away from the old output."""
    m = _scene(**GRIDS[grid]).model
    inputs = _inputs(m, 20011, 19)
    _, gc, ga = _run(m, inputs)
    _scale_folded_layers(m)
    _, gc8, ga8 = _run(m, inputs)
    _, tc8, _ = _torch_forward(m, *inputs, torch.float64)
    assert np.abs(tc8 - gc).max() > 1e-3
    np.testing.assert_allclose(gc8, tc8, rtol=0, atol=64 * 2e-5)
    assert np.array_equal(ga8, ga)                       # the ambient net has none of the scaled weights


def _x8_errors(po, m, inputs):
    """Largest / rms rgb error against the float64 truth, both folded layers x8: (kernel, plain fp32 torch, fp32 oracle)."""
    _scale_folded_layers(m)
    _, gc8, _ = _run(m, inputs)
    _, tc8, _ = _torch_forward(m, *inputs, torch.float64)
    _, fc8, _ = _torch_forward(m, *inputs, torch.float32)
    x, d, enc_a, c, eye = [t.cpu().numpy() for t in inputs]
    _, oc8, _ = po.nerf_forward(po.model_from_module(m), x, d, enc_a, c, eye)
    errs = [np.abs(v.astype(np.float64) - tc8) for v in (gc8, fc8, oc8)]
    print("x8 rgb error against f64 (max / rms): " + "; ".join(
        f"{name} {e.max():.3e} / {np.sqrt((e ** 2).mean()):.3e}" for name, e in zip(("kernel", "fp32 torch", "fp32 oracle"), errs)))
    return [e.max() for e in errs]


@pytest.mark.parametrize("grid", ["tiled16", "hash19"])
def test_x8_rgb_error_within_twice_plain_fp32_torch(po, hiplib, grid):
    """Both folded layers x8: the kernel's largest rgb error against the float64 truth is at most twice that of a plain fp32
    torch evaluation of the two-layer form on the same inputs (the factor covers summation order).
    On the CPU the oracle's sequential two-layer sums stand at 2.6e-5 against 1.9e-5 for torch (tiled16)."""
    m = _scene(**GRIDS[grid]).model
    kernel, fp32_torch, _ = _x8_errors(po, m, _inputs(m, 20011, 19))
    assert kernel <= 2.0 * fp32_torch


@pytest.mark.parametrize("grid", ["tiled16", "hash19"])
def test_x8_rgb_error_within_twice_the_fp32_oracle(po, hiplib, grid):
    """The same bar against the two-layer form in the kernel's own kind of arithmetic: the oracle (oracle/orc_nerf.c) evaluates
    sigma_net's last layer and color_net's first one after the other in sequential fp32 sums.  Folding the two layers must not
    cost accuracy against float64 beyond summation order (factor 2)."""
    m = _scene(**GRIDS[grid]).model
    kernel, _, fp32_oracle = _x8_errors(po, m, _inputs(m, 20011, 19))
    assert kernel <= 2.0 * fp32_oracle


def _raw_forward(m, x, d, enc_a, c, eye, want_rgb, want_ambient):
    """rn_nerf_fused_forward with or without the colour branch (rgbs NULL = the density query)."""
    import radnerf_hip as hip
    from radnerf import fused
    st = fused._state(m)
    st.refresh()
    fused._frame_bias(st, enc_a, eye, c)
    M = x.shape[0]
    sigmas = torch.full((M,), float("nan"), device="cuda")
    rgbs = torch.full((M, 3), float("nan"), device="cuda") if want_rgb else None
    ambient = torch.full((M, 2), float("nan"), device="cuda") if want_ambient else None
    hip.call("rn_nerf_fused_forward", hip.ptr(x), hip.ptr(d), None, M, None, C.byref(st.gx), C.byref(st.gw), hip.ptr(st.packed),
             hip.ptr(st.bias), float(m.bound), hip.ptr(sigmas), hip.ptr(rgbs), hip.ptr(ambient), st.mlp_dtype, hip.stream())
    torch.cuda.synchronize()
    return sigmas, rgbs, ambient


@pytest.mark.parametrize("grid", ["tiled16", "hash19"])
def test_sigma_and_ambient_do_not_pass_through_the_fold(hiplib, grid):
    """sigma of the full forward is bit-equal to the density query's, ambient bit-equal with and without the colour branch."""
    from radnerf import fused
    m = _scene(**GRIDS[grid]).model
    x, d, enc_a, c, eye = _inputs(m, 20011, 7)
    with torch.no_grad():
        s_full, rgb, a_full = _raw_forward(m, x, d, enc_a, c, eye, True, True)
        s_dens, _, a_dens = _raw_forward(m, x, d, enc_a, c, eye, False, True)
        s_query = fused.density_forward(m, x, enc_a, eye)
    assert torch.isfinite(rgb).all() and torch.isfinite(s_full).all() and torch.isfinite(a_full).all()
    assert torch.equal(s_full, s_dens) and torch.equal(s_full, s_query)
    assert torch.equal(a_full, a_dens)
