"""RN_TRAIN_MLP=f16: the fused training head with 16-bit matrix products (csrc/rn_train_head_f16.hip, the *_h16 entries of
include/radnerf_train.h) -- the entry points and what the switch changes, every output and gradient against float64 with the
bound err_gpu <= 2 E_model + bar_f32 (E_model: the distance of the arithmetic model tests/netref16.py from float64; bar_f32: the
bar tests/test_gpu_train_head.py applies to the fp32 route, which tests/test_gpu_train_head_ref.py now backs with measurements: the fp32
route stands at most 1.2e-4 from float64 on a gradient and 6e-6 on an output), the per-tile gradient scaling, reproducibility, the live count, and
16 training steps eager and captured."""
import os
import random

import numpy as np
import pytest
import torch

import netref16
from head_cases import batch as _batch, direct as _direct, environment as _environment, head as _head, model as _model
from netref64 import Net64

pytestmark = pytest.mark.gpu

# the bars of tests/test_gpu_train_head.py::test_fused_head_matches_the_operator_path, as max-normalised errors
SIGMA_RTOL, SIGMA_ATOL, RGB_ATOL, AMBIENT_ATOL, GRAD_BAR = 2e-4, 1e-6, 2e-5, 2e-5, 2e-3
ENTRIES = ["rn_train_head_image_floats_h16", "rn_train_head_pack_h16", "rn_train_head_pack_row_h16", "rn_train_head_forward_h16",
           "rn_train_head_backward_h16"]


# --------------------------------------------------------------------------------------------------------- 1: the entry points
def test_entry_points_exist_and_the_switch_changes_only_the_matrix_products(hiplib, monkeypatch):
    from radnerf.switches import TABLE
    lib = hiplib._lib
    for name in ENTRIES:
        assert hasattr(lib, name), name
    assert int(lib.rn_train_head_image_floats_h16()) > int(lib.rn_train_head_image_floats())
    assert [row[1:3] for row in TABLE if row[0] == "RN_TRAIN_MLP"] == [("f32", ("f32", "f16"))]
    m, b = _model("default"), _batch("default", 95, 1500)
    f32, f16 = _direct(m, b, ""), _direct(m, b, "_h16")
    n32 = int(lib.rn_train_head_image_floats())
    assert torch.equal(f32["image"], f16["image"][:n32])                     # today's fp32 image, unchanged
    assert torch.equal(f32["xn"], f16["xn"])
    assert not torch.equal(f32["sigmas"], f16["sigmas"])
    assert float((f32["sigmas"] - f16["sigmas"]).abs().max() / f32["sigmas"].abs().max()) < 1e-2
    # the same through the switch (train_head._HeadTrain picks the entries); xn is bit for bit the fp32 route's, and wn = (ambient + 1) / 2
    # follows the ambient output, which the 16-bit products move
    outs = {}
    for mlp in ("f32", "f16"):
        _environment(monkeypatch, mlp)
        outs[mlp] = _head(m, b, b["up"])[0]
    assert torch.equal(outs["f32"]["sigma"], f32["sigmas"]) and torch.equal(outs["f16"]["sigma"], f16["sigmas"])
    assert torch.equal(f16["wn"], (f16["ambient"] + 1.0) / 2.0)


# ----------------------------------------------------------------------------------------------------- 2: against float64
FIGURES = {}


@pytest.mark.parametrize("case", range(len(netref16.CASES)))
def test_outputs_and_gradients_against_float64(hiplib, monkeypatch, case):
    """err_gpu(q) <= 2 E_model(q) + bar_f32(q) for every output and every gradient q (max-normalised; input gradients included),
    the gradients on samples whose ReLU masks a rounding of an operand cannot flip (netref16.Net16.unstable; the batch keeps at
    least two thirds of its samples).  The margin of 2: an activation within fp32 rounding of a half-precision rounding boundary may
    round the other way on the GPU than in float64; each such flip moves one operand by one half-precision ulp, the size of the
    roundings E_model consists of."""
    tag, M, live, row = netref16.CASES[case]
    m, b = _model(tag), _batch(tag, M, 1600 + case)
    n = M if live is None else live
    # holds by construction: netref16.stable_batch picked the rows from a pool with the model alone (the rule excludes 80 - 95 % of
    # uniformly drawn samples, tests/test_netref16.py), so the gradients below are compared on well-conditioned samples only
    assert 3 * int(b["excluded"][:n].sum()) <= n
    _environment(monkeypatch, "f16")
    out, (g,) = _head(m, b, b["up"], live=live, row=row, input_grads=True)
    ref_up = [u[:n] for u in b["up"]]
    o64, g64 = netref16.run_reference(Net64(m), b["xyzs"][:n], b["dirs"][:n], b["enc_a"], b["eye"], ref_up, input_grads=True)
    o16, g16 = netref16.run_reference(netref16.Net16(m), b["xyzs"][:n], b["dirs"][:n], b["enc_a"], b["eye"], ref_up, input_grads=True)
    bars = {"sigma": SIGMA_RTOL + SIGMA_ATOL / float(o64["sigma"].abs().max()), "rgb": RGB_ATOL / float(o64["rgb"].abs().max()),
            "ambient": AMBIENT_ATOL / float(o64["ambient"].abs().max())}
    rows, failed = [], []
    for name, got, r16, r64 in [(k, out[k], o16[k], o64[k]) for k in o64] + [(k, g.get(k), g16[k], g64[k]) for k in sorted(g64)]:
        assert got is not None and got.shape == r64.shape and torch.isfinite(got).all(), name
        e_model, e_gpu = netref16.max_normalised(r16, r64), netref16.max_normalised(got, r64)
        bar = bars.get(name, GRAD_BAR)
        rows.append(f"  {name:34s} E_model {e_model:.3e}  err_gpu {e_gpu:.3e}  bar_f32 {bar:.1e}  gpu-model {netref16.max_normalised(got, r16):.3e}")
        if not e_gpu <= 2 * e_model + bar:
            failed.append(rows[-1])
    assert set(g) == set(g64), set(g) ^ set(g64)
    print(f"\n{tag} M={M} live={live} row={row}: {int(b['excluded'][:n].sum())} excluded\n" + "\n".join(rows))
    assert not failed, "\n".join(failed)


def test_live_count_zero_writes_nothing_and_every_gradient_is_zero(hiplib, monkeypatch):
    m, b = _model("default"), _batch("default", 64, 1605)
    _environment(monkeypatch, "f16")
    _, (g,) = _head(m, b, b["up"], live=0, input_grads=True)
    assert {"encoder.embeddings", "encoder_ambient.embeddings", "sigma_net.net.0.weight", "enc_a", "eye", "xyzs"} <= set(g)
    for name, t in g.items():
        assert torch.isfinite(t).all() and float(t.abs().max()) == 0.0 if t.numel() else True, name


# -------------------------------------------------------------------------------------------------------- 3: gradient scaling
@pytest.mark.parametrize("tag", ["default", "hash19"])
def test_a_gradient_2_to_the_minus_20_smaller_gives_the_same_bits_scaled(hiplib, monkeypatch, tag):
    """Backward of g and of 2^-20 g through the same forward: only powers of two are involved, so every gradient of the second is
    2^-20 times the first bit for bit (the table gradients through the ordered sum: atomics add in an order of their own).  An
    implementation that rounds unscaled gradients to half fails this: 2^-20 g lies in half precision's subnormals or below.
    The middle tile's upstream gradients are zero: its rows come back zero, and nothing is NaN."""
    m, b = _model(tag), _batch(tag, 95, 1500)
    up = [u.clone() for u in b["up"]]
    for u in up:
        u[32:64] = 0
    _environment(monkeypatch, "f16", deterministic=True)
    _, (g1, g2) = _head(m, b, up, input_grads=True, backwards=2)
    assert set(g1) == set(g2) and len(g1) >= 14
    for name in sorted(g1):
        assert torch.isfinite(g1[name]).all() and float(g1[name].abs().max()) > 0, name
        assert torch.equal(g2[name], g1[name] * 2.0 ** -20), name
    assert float(g1["xyzs"][32:64].abs().max()) == 0.0 and float(g1["dirs"][32:64].abs().max()) == 0.0
    assert float(g1["xyzs"][64:].abs().max()) > 0.0
    # the feature gradients themselves, through the C ABI: zero rows for the zero tile, scaled bits for the others
    d1, d2 = _direct(m, b, "_h16", up=up), _direct(m, b, "_h16", up=[u * 2.0 ** -20 for u in up])
    for k in ("g_enc_x", "g_enc_w"):
        assert torch.isfinite(d1[k]).all() and float(d1[k][:, 32:64].abs().max()) == 0.0 and float(d1[k][:, :32].abs().max()) > 0.0
        assert torch.equal(d2[k], d1[k] * 2.0 ** -20), k


# ------------------------------------------------------------------------------------------------------ 4: reproducibility
@pytest.mark.parametrize("tag", ["default", "hash19"])
def test_two_runs_give_the_same_bits(hiplib, monkeypatch, tag):
    m, b = _model(tag), _batch(tag, 95, 1500)
    first, second = _direct(m, b, "_h16", up=b["up"]), _direct(m, b, "_h16", up=b["up"])
    for k in first:
        assert torch.equal(first[k].view(torch.int32), second[k].view(torch.int32)), k      # outputs, feature gradients, every workspace tile
    assert float(first["work"].abs().max()) > 0 and torch.isfinite(first["work"]).all()
    _environment(monkeypatch, "f16", deterministic=True)
    (o1, (g1,)), (o2, (g2,)) = (_head(m, b, b["up"], input_grads=True) for _ in range(2))
    for k in o1:
        assert torch.equal(o1[k], o2[k]), k
    for k in g1:
        assert torch.equal(g1[k].view(torch.int32), g2[k].view(torch.int32)), k


# ---------------------------------------------------------------------------------------------------------- 5: live count
@pytest.mark.parametrize("live", [0, 1, 40])
def test_rows_past_the_live_count_are_not_written_and_contribute_nothing(hiplib, monkeypatch, live):
    m, b = _model("default"), _batch("default", 64, 1605)
    M, sentinel = 64, -7.25
    cnt = torch.tensor([live, 0], dtype=torch.int32, device="cuda")
    capped = _direct(m, b, "_h16", m_dev=cnt, up=b["up"], sentinel=sentinel)
    for k in ("sigmas", "rgbs", "ambient", "amb_abs", "xn", "wn"):
        assert bool((capped[k][live:] == sentinel).all()), k
    for k in ("g_enc_x", "g_enc_w"):
        assert bool((capped[k][:, live:] == sentinel).all()), k
    if live:
        exact = _direct(m, b, "_h16", M=live, up=b["up"], sentinel=sentinel)
        for k in ("sigmas", "rgbs", "ambient", "amb_abs", "xn", "wn"):
            assert torch.equal(capped[k][:live], exact[k]), k
        for k in ("g_enc_x", "g_enc_w"):
            assert torch.equal(capped[k][:, :live], exact[k]), k
        # no contribution to any gradient: the capacity-64 run with a device count equals the run on the first `live` rows, with
        # the bar the fp32 kernels' live-count test applies (tests/test_gpu_train_head.py: 1e-4 of the maximum)
        _environment(monkeypatch, "f16")
        short = {k: (v[:live].contiguous() if k in ("xyzs", "dirs") else v) for k, v in b.items()}
        _, (g_a,) = _head(m, b, b["up"], live=live, input_grads=True)
        _, (g_b,) = _head(m, short, [u[:live] for u in b["up"]], input_grads=True)
        assert g_a.keys() == g_b.keys()
        for name in g_b:
            assert netref16.max_normalised(g_a[name], g_b[name]) < 1e-4, name


# ----------------------------------------------------------------------------------------------------------- 6: end to end
def _train(monkeypatch, mlp, deterministic, graphed, steps=16, want_bits=True):
    """`steps` optimizer steps on the 64 x 64 scene of the train tests (1024 rays, no occupancy refresh): three of the first
    window, then the budgeted step (the one a GraphedTrainer captures) -> (last loss, {parameter: bits})."""
    from radnerf.scene import SyntheticScene, default_opt
    from radnerf.train import GraphedTrainer, SyntheticTrainStream, Trainer
    for name in [n for n in os.environ if n.startswith("RN_")]:
        monkeypatch.delenv(name)
    monkeypatch.setenv("RN_TRAIN_NOISE", "torch")
    monkeypatch.setenv("RN_TRAIN_MLP", mlp)
    monkeypatch.setenv("RN_TRAIN_DETERMINISTIC", "1" if deterministic else "0")
    torch.backends.cuda.preferred_blas_library("cublas")     # as tests/test_gpu_train_deterministic.py: before the scene's first matrix product
    torch.manual_seed(0)
    random.seed(0)
    np.random.seed(0)
    scene = SyntheticScene(H=64, W=64, n_frames=8, device="cuda", opt=default_opt(engine="ops", torso=False, smooth_lips=False))
    stream = SyntheticTrainStream(scene, n_rays=1024, seed=4)
    trainer = (GraphedTrainer if graphed else Trainer)(scene.model, scene.opt, update_extra_interval=0)
    for _ in range(3):
        trainer.step(stream.batch())
    scene.model.mean_count = 12000
    for _ in range(steps - 3):
        loss = trainer.step(stream.batch())
    torch.cuda.synchronize()
    if graphed:
        assert trainer.captures == 1 and trainer.replays == steps - 3
    if not want_bits:
        return float(loss), None
    bits = {n: p.detach().cpu().numpy().reshape(-1).view(np.uint32).copy() for n, p in scene.model.named_parameters()}
    return float(loss), bits


_LOSS = {}
SPREAD_RUNS = 20


def test_sixteen_training_steps_eager_and_captured_end_with_the_same_bits(hiplib, monkeypatch):
    """RN_TRAIN_MLP=f16 with RN_TRAIN_DETERMINISTIC=1: 16 steps of Trainer and of GraphedTrainer (three eager steps of the first
    window, one capture, 13 replays) end with the same bits in every parameter and in the loss."""
    l_eager, p_eager = _train(monkeypatch, "f16", True, False)
    l_graph, p_graph = _train(monkeypatch, "f16", True, True)
    _LOSS["f16"] = l_eager
    assert np.isfinite(l_eager) and all(np.isfinite(v.view(np.float32)).all() for v in p_eager.values())
    differing = [n for n in p_eager if not np.array_equal(p_eager[n], p_graph[n])]
    assert not differing and l_eager == l_graph, differing


def test_loss_after_sixteen_steps_lies_within_the_fp32_routes_own_spread(hiplib, monkeypatch):
    """The loss after 16 steps with RN_TRAIN_MLP=f16 is no farther from the fp32 route's deterministic run than that route's own
    atomic runs get: |L_f16 - L_f32,det| <= max_i |L_f32,atomic,i - L_f32,det|, the spread measured here on the same scene from
    SPREAD_RUNS atomic runs, not fixed in advance.  One atomic run is one draw of the scatter's summation order, and a single
    draw decides nothing (the recorded draws span 1.2e-9 ... 4.8e-8); the largest of SPREAD_RUNS draws is a stable statistic of
    the fp32 route alone.  SPREAD_RUNS = 20: of nine recorded draws two lay in the upper quarter of their range, so twenty draws
    miss that quarter with probability (7/9)^20 = 0.7 % (DESIGN section 4 holds the draws and what the comparison means)."""
    l_f16 = _LOSS["f16"] if "f16" in _LOSS else _train(monkeypatch, "f16", True, False)[0]
    l_det, _ = _train(monkeypatch, "f32", True, False)
    draws = sorted(abs(_train(monkeypatch, "f32", False, False, want_bits=False)[0] - l_det) for _ in range(SPREAD_RUNS))
    print(f"\nloss after 16 steps: f16 {l_f16:.9g}  f32 deterministic {l_det:.9g}  |f16 - f32 det| {abs(l_f16 - l_det):.3e}"
          f"  |f32 atomic - f32 det| over {SPREAD_RUNS} runs: " + " ".join(f"{d:.2e}" for d in draws))
    assert draws[-1] > 0.0                                   # the atomic route does move from run to run: there is a spread to measure
    assert abs(l_f16 - l_det) <= draws[-1]
