"""The network off the default options (tests/golden/cases.py OPTION_SETS: no eye input and no individual codes; odd code
widths), on the CPU: the oracle and the float64 restatement tests/netref64.py against the outputs and smooth-sample gradients
that the unmodified reference generated (tests/golden/reference_options.npz), and netref64 against the oracle at the default
options.

Bars.  The oracle against the reference (two fp32 implementations): the output bars of reference_train_stable.npz in
test_golden_frames.py.  netref64 against the reference: the error of the reference's own fp32 formulation, measured -- outputs
<= 3.5e-5 (sigma, relative) / 2.6e-6 (rgb, ambient, torso); on the smooth samples the gradients of ambient_net and enc_a <=
1.6e-3 of their largest entry (a contribution upstream of the 2-D grid carries its ~2047 x table-difference derivative and the
contributions largely cancel in the sum, which magnifies fp32 rounding), every other gradient <= 1.2e-3 -- held at 5e-3 / 1e-5."""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

import netref64

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import cases  # noqa: E402
OUT_BARS = {"sigma": 2e-5, "rgb": 2e-6, "ambient": 2e-7}     # x max(1, max |ref|): oracle vs reference
REF64_BARS = {"sigma": 1e-4, "rgb": 1e-5, "ambient": 1e-5}   # netref64 vs reference


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(HERE, "golden", "reference_options.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _model(tag):
    from radnerf.scene import SyntheticScene, default_opt
    torch.manual_seed(0)
    return SyntheticScene(H=32, W=32, n_frames=8, device="cpu", opt=default_opt(**cases.OPTION_SETS[tag])).model


def _close(got, want, bar, name):
    err = float(np.abs(np.asarray(got, np.float64) - want).max())
    assert err <= bar * max(1.0, float(np.abs(want).max())), (name, err)


@pytest.mark.parametrize("tag", sorted(cases.OPTION_SETS))
def test_model_of_the_option_set_is_the_reference_model(gold, hiplib, tag):
    m = _model(tag)
    params = dict(m.named_parameters())
    flat = np.concatenate([params[n].detach().numpy().reshape(-1) for n in sorted(params)])
    assert hashlib.sha256(np.ascontiguousarray(flat).tobytes()).hexdigest() == str(gold[f"{tag}_params_sha256"])
    kw = cases.OPTION_SETS[tag]
    assert m.exp_eye == kw["exp_eye"] and m.individual_dim == kw["ind_dim"] and m.individual_dim_torso == kw["ind_dim_torso"]
    assert tuple(m.sigma_net.net[0].weight.shape) == (64, 64 + int(kw["exp_eye"]))
    assert tuple(m.color_net.net[0].weight.shape) == (64, 80 + kw["ind_dim"])
    assert tuple(m.torso_net.net[0].weight.shape) == (32, 128 + kw["ind_dim_torso"])


@pytest.mark.parametrize("tag", sorted(cases.OPTION_SETS))
def test_oracle_reproduces_reference_options(po, gold, hiplib, tag):
    m = _model(tag)
    om = po.model_from_module(m)
    c = m.individual_codes[0].detach().numpy() if m.individual_dim else np.zeros(0, np.float32)
    sigma, rgb, amb = po.nerf_forward(om, gold["x"], gold["d"], gold["enc_a"], c, gold["eye"])
    for name, got in (("sigma", sigma), ("rgb", rgb), ("ambient", amb)):
        _close(got, gold[f"{tag}_{name}"], OUT_BARS[name], name)
    ct = m.individual_codes_torso[0].detach().numpy() if m.individual_dim_torso else np.zeros(0, np.float32)
    ta, tc, tdx = po.torso_forward(om, gold["torso_xy"], gold[f"{tag}_torso_poses"], ct)
    for name, got in (("alpha", ta), ("color", tc), ("dx", tdx)):
        _close(got, gold[f"{tag}_torso_{name}"], 2e-6, "torso_" + name)


def reference_gradients(ref, m, x, d, enc_a, eye, up, mask, ind_index=0):
    """Outputs and float64 autograd gradients of netref64 under upstream gradients `up` (sigma, rgb, ambient) x mask:
    {parameter name: grad} + enc_a / eye / individual_codes (the row used)."""
    enc_a = enc_a.double().clone().requires_grad_(True)
    eye = eye.double().clone().requires_grad_(True) if m.exp_eye else None
    c = ref.P["individual_codes"][ind_index] if m.individual_dim else None
    sigma, rgb, amb = ref.forward(x, d, enc_a, c, eye)
    k = mask.double()
    loss = (sigma * up[0].double() * k).sum() + (rgb * up[1].double() * k[:, None]).sum() + (amb * up[2].double() * k[:, None]).sum()
    names = [n for n in ref.P if n.split(".")[0] in ("encoder", "encoder_ambient", "ambient_net", "sigma_net", "color_net")]
    leaves = [ref.P[n] for n in names] + [enc_a] + ([eye] if eye is not None else []) + ([ref.P["individual_codes"]] if c is not None else [])
    grads = torch.autograd.grad(loss, leaves)
    out = dict(zip(names + ["enc_a"] + (["eye"] if eye is not None else []) + (["individual_codes"] if c is not None else []), grads))
    return (sigma.detach(), rgb.detach(), amb.detach()), out


@pytest.mark.parametrize("tag", sorted(cases.OPTION_SETS))
def test_netref64_reproduces_reference_options(gold, hiplib, tag):
    m = _model(tag)
    ref = netref64.Net64(m)
    t = {k: torch.from_numpy(gold[k]) for k in ("x", "d", "enc_a", "eye", "up_sigma", "up_rgb", "up_ambient", "torso_xy")}
    mask = torch.from_numpy(gold[f"{tag}_mask"]).bool()
    assert 0.3 < float(mask.float().mean()) < 1.0
    outs, grads = reference_gradients(ref, m, t["x"], t["d"], t["enc_a"], t["eye"], (t["up_sigma"], t["up_rgb"], t["up_ambient"]), mask)
    for name, got in zip(("sigma", "rgb", "ambient"), outs):
        _close(got.numpy(), gold[f"{tag}_{name}"], REF64_BARS[name], name)
    keys = [k for k in gold if k.startswith(f"{tag}_grad::")]
    assert len(keys) == 9 + int(m.exp_eye) + int(m.individual_dim > 0)
    for key in keys:
        name = key.split("::")[1]
        got = grads[name].numpy()
        got = got[:1] if name == "individual_codes" else got
        want = gold[key]
        assert got.shape == want.shape, name
        assert np.abs(got - want).max() <= 5e-3 * np.abs(want).max(), (name, np.abs(got - want).max() / np.abs(want).max())
        assert float((got * want).sum() / (np.linalg.norm(got) * np.linalg.norm(want))) > 0.99999, name
    if m.individual_dim:
        assert float(grads["individual_codes"][1:].abs().max()) == 0.0
    for name in ("encoder", "encoder_ambient"):
        gt = grads[f"{name}.embeddings"]
        rows = torch.from_numpy(gold[f"{tag}_gradrows::{name}"]).long()
        want = gold[f"{tag}_gradvals::{name}"]
        assert np.abs(gt[rows].numpy() - want).max() <= 5e-3 * np.abs(want).max(), name
        s, sa, nz = gold[f"{tag}_gradsum::{name}"]
        assert abs(float(gt.abs().sum()) - sa) <= 1e-4 * sa, name
        assert int((gt.abs().sum(1) > 0).sum()) == int(nz), name
    with torch.no_grad():
        c = ref.P["individual_codes_torso"][0] if m.individual_dim_torso else None
        ta, tc, tdx = ref.forward_torso(t["torso_xy"], torch.from_numpy(gold[f"{tag}_torso_poses"]), c)
    for name, got in (("alpha", ta), ("color", tc), ("dx", tdx)):
        _close(got.numpy(), gold[f"{tag}_torso_{name}"], 1e-5, "torso_" + name)


@pytest.mark.parametrize("grid", ["tiledgrid16", "hashgrid19"])
def test_netref64_reproduces_the_oracle_at_default_options(po, hiplib, grid):
    from radnerf.scene import SyntheticScene, default_opt
    kw = dict(xyz_grid="hashgrid", xyz_log2_hashmap_size=19) if grid == "hashgrid19" else {}
    torch.manual_seed(0)
    scene = SyntheticScene(H=16, W=16, n_frames=8, device="cpu", opt=default_opt(**kw))
    m = scene.model
    inp = cases.options_inputs(seed=29)
    x, d, enc_a, eye = (inp[k].numpy() for k in ("x", "d", "enc_a", "eye"))
    c = m.individual_codes[0].detach()
    om = po.model_from_module(m)
    es, ec, ea = po.nerf_forward(om, x, d, enc_a, c.numpy(), eye)
    ref = netref64.Net64(m)
    with torch.no_grad():
        s, r, a = ref.forward(inp["x"], inp["d"], inp["enc_a"], c, inp["eye"])
    np.testing.assert_allclose(s.numpy(), es, rtol=2e-4, atol=1e-6)
    np.testing.assert_allclose(r.numpy(), ec, rtol=0, atol=2e-5)
    np.testing.assert_allclose(a.numpy(), ea, rtol=0, atol=2e-5)
    ct = m.individual_codes_torso[0].detach()
    xy = inp["torso_xy"]
    oa, oc, od = po.torso_forward(om, xy.numpy(), scene.poses6[0:1].numpy(), ct.numpy())
    with torch.no_grad():
        ta, tc, td = ref.forward_torso(xy, scene.poses6[0:1], ct)
    for got, want in ((ta, oa), (tc, oc), (td, od)):
        np.testing.assert_allclose(got.numpy(), want, rtol=0, atol=2e-5)
