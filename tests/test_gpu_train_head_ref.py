"""The default route of a training step -- RN_TRAIN_HEAD=fused with RN_TRAIN_MLP=f32: k_train_fwd, k_train_bwd,
k_train_input_grads, k_train_wgrad / k_train_wreduce / k_train_const of csrc/rn_train_head.hip -- against float64
(netref64.Net64Libm: Net64 with the level scales the library computes) at the tile, part and trip edges of those kernels.

Every output and every gradient q (head parameters, both tables, enc_a, eye, individual_codes, xyzs, dirs), max-normalised:

    err_fused(q) <= FACTOR * E_ops(q) + 2^-20        and        err_fused(q) <= the bar of tests/test_gpu_train_head.py

E_ops(q) is measured in the same test: the distance from that reference of the plain fp32 formulation of the network (head_cases.ops:
nn.Linear and torch activations under torch.autograd over the grid and SH operators, none of the head's kernels) on the same
batch and upstream gradients.  Both are fp32 evaluations of one expression which differ in summation order and in who
computes exp / tanh: their errors are two draws of the same size, FACTOR = 4 covers the spread of a maximum over many entries,
and 2^-20 covers a quantity the torch path happens to get exact.  The gradients are compared on samples picked with the model
alone to be away from every ReLU switch and cell boundary (tests/headref32.py); the outputs on every row.

The gradients of a batch of fewer than 1024 compared samples get a factor of their own.  Every gradient depends on the
ambient coordinate through the 2-D grid, which multiplies the coordinate's fp32 error (a few ulp, 1e-8 .. 1e-7, in either
evaluation) by up to scale_15 / 2 = 1023: what is left of a gradient's error is that product for the few samples with the
largest derivative, not a maximum over many entries.  With one compared sample err_fused / E_ops is the ratio of two centred
draws, whose tail is P(ratio > r) = 2 / (pi r): measured 648 for sigma_net.net.0.weight at M = 1 (the torch path's ambient
1.5 ulp from float64, the kernels' 8 ulp), and 4.2 .. 7.4 on three gradients at M = 33.  SINGLE_FACTOR = 1024, the grid's
own amplification, puts a false alarm at 1 in 1600 per draw; SMALL_FACTOR = 64 = 4 x 16 at 1 in 100 for a gradient that one
sample dominates.  Both bars stay far below what a lost or doubled row moves (1 / n >= 1 % of a gradient for n <= 95; the
whole gradient for n = 1), and the bars of tests/test_gpu_train_head.py cap them.  From 1024 compared samples on (every part
and trip case) the factor is 4 (measured ratios 0.3 .. 2.2) -- except for the gradients UPSTREAM of the 2-D grid (ambient_net's
weights, enc_a, the xyz table, xyzs), which keep 64 at every size (OWN_FACTOR): they carry the grid's derivative with respect
to the ambient coordinate, 1023 table differences of alternating sign per level, which depends on the other coordinate's
fraction and so on that coordinate's error; the per-sample terms largely cancel in the sum, and the handful of samples with
the largest uncancelled term decide the error at any batch size.  Measured at M = 4064: ambient_net.net.2.weight 4.8e-5
(a weight gradient: the same bits in every run) against E_ops 1.6e-5 .. 7.8e-6 depending on the BLAS library the torch path was
given by the tests before it, a ratio of 3 .. 6.2.

The sizes of the part and trip cases follow from W = RN_TRAIN_WPARTS as the library reads it (the parts of a weight-gradient job:
part p takes tiles p, p + W, ... through two register sets fetched two strides ahead, so each count of 0 .. 5 tiles per part
takes another path through csrc/rn_wgrad_dev.h's fetch / commit / break sequence) and from the device's CU count (the tile
loops of k_train_fwd / k_train_bwd take a second trip past 32 * 8 * CUs samples, k_train_input_grads' past 32 * 16 * CUs).

The float64 reference is evaluated 16384 rows at a time with the gradients summed (head_cases.reference64): every case up to
that size is a single pass, the larger ones are chunked -- every gradient is linear in the samples."""
import pytest
import torch

import netref16
from head_cases import batch32, direct, environment, head, model, ops, reference64, weight_grads, wparts

pytestmark = pytest.mark.gpu

SEED0 = 3200                      # the batch of netref16.CASES[i] has seed SEED0 + i (tests/test_headref32_host.py picks the same ones)
FACTOR, FLOOR = 4.0, 2.0 ** -20
SMALL_FACTOR, SINGLE_FACTOR, MANY = 64.0, 1024.0, 1024            # gradients of fewer than MANY / of one compared sample (see above)
# A quantity that needs more than FACTOR gets its own factor here, with the property of the arithmetic that explains it
_UPSTREAM = "upstream of the 2-D grid: its derivative (1023 x table differences) times the ambient error, few samples decide"
OWN_FACTOR = {name: (SMALL_FACTOR, _UPSTREAM) for name in ("ambient_net.net.0.weight", "ambient_net.net.1.weight", "ambient_net.net.2.weight",
                                                           "enc_a", "encoder.embeddings", "xyzs")}
# one number and four numbers: no maximum over many entries at any batch size, the ratio of two single draws (measured for eye at
# M = 131 105: 1.07e-5 against 1.8e-6, a ratio of 5.8; 10.4 at 8193 under the floor)
OWN_FACTOR["eye"] = (SINGLE_FACTOR, "a scalar: one draw against one draw, P(ratio > r) = 2 / (pi r)")
OWN_FACTOR["individual_codes"] = (SMALL_FACTOR, "four entries of one row: a few draws")
# the bars of tests/test_gpu_train_head.py::test_fused_head_matches_the_operator_path, as max-normalised errors: the upper cap
SIGMA_RTOL, SIGMA_ATOL, RGB_ATOL, AMBIENT_ATOL, GRAD_BAR = 2e-4, 1e-6, 2e-5, 2e-5, 2e-3
SENTINEL = -7.25


def _compare(monkeypatch, tag, M, seed, live=None, row=False, deterministic=False):
    m, b = model(tag), batch32(tag, M, seed)
    n = M if live is None else live
    # holds by construction (headref32.stable_batch32 picked the rows): what it still catches is a pick that went wrong
    assert 3 * int(b["excluded"][:n].sum()) <= n
    compared = n - int(b["excluded"][:n].sum())
    grad_factor = FACTOR if compared >= MANY else (SMALL_FACTOR if compared > 1 else SINGLE_FACTOR)
    environment(monkeypatch, "f32", deterministic)
    out, (g,) = head(m, b, b["up"], live=live, row=row, input_grads=True)
    o_ops, g_ops = ops(m, b, b["up"], monkeypatch, live=live)
    o64, g64 = reference64(m, b, b["up"], live=live)
    caps = {"sigma": SIGMA_RTOL + SIGMA_ATOL / float(o64["sigma"].abs().max()), "rgb": RGB_ATOL / float(o64["rgb"].abs().max()),
            "ambient": AMBIENT_ATOL / float(o64["ambient"].abs().max())}
    assert set(g) == set(g64), set(g) ^ set(g64)
    assert set(g_ops) == set(g64), set(g_ops) ^ set(g64)
    rows, failed = [], []
    for name, got, plain, r64 in [(k, out[k], o_ops[k], o64[k]) for k in o64] + [(k, g[k], g_ops[k], g64[k]) for k in sorted(g64)]:
        assert got.shape == r64.shape and plain.shape == r64.shape, name
        assert torch.isfinite(got).all() and torch.isfinite(plain).all() and torch.isfinite(r64).all(), name
        e_ops, e_fused = netref16.max_normalised(plain, r64), netref16.max_normalised(got, r64)
        factor, cap = (FACTOR if name in o64 else max(grad_factor, OWN_FACTOR.get(name, (FACTOR,))[0])), caps.get(name, GRAD_BAR)
        rows.append(f"  {name:34s} E_ops {e_ops:.3e}  err_fused {e_fused:.3e}  ratio {e_fused / (e_ops + 1e-300):8.2f}  bar {factor * e_ops + FLOOR:.3e}"
                    f"  cap {cap:.1e}")
        if not (e_fused <= factor * e_ops + FLOOR and e_fused <= cap):
            failed.append(rows[-1])
    print(f"\n{tag} M={M} live={live} row={row} deterministic={deterministic}: {int(b['excluded'][:n].sum())} excluded\n" + "\n".join(rows))
    assert not failed, "\n".join(failed)


# ---------------------------------------------------------------------------------------------- a: the cases of the f16 route
@pytest.mark.parametrize("case", range(len(netref16.CASES)))
def test_tile_edges_and_models_against_float64(hiplib, monkeypatch, case):
    """netref16.CASES: M = 1 / 31 / 32 / 33 / 95, a capacity of 64 with a device live count of 1 / 40, the 2^19 hash table, no
    eye and no code, audio_dim 32, the row-indexed code."""
    tag, M, live, row = netref16.CASES[case]
    _compare(monkeypatch, tag, M, SEED0 + case, live=live, row=row)


# --------------------------------------------------------------------------------------------------- b: part and trip edges
def _edge(name):
    """-> (M or capacity, live or None, row-indexed code)."""
    W, cus = wparts(), torch.cuda.get_device_properties(0).multi_processor_count
    return {"idle_part": (32 * (W - 1), None, False),              # one part without a tile: it writes a zero partial; last tile full
            "two_tiles": (32 * W + 1, None, False),                # part 0: two tiles, the second with one live row (31 zero rows staged)
            "three_tiles": (32 * 2 * W + 1, None, False),
            "four_tiles": (32 * 3 * W + 1, None, False),
            "five_tiles": (32 * 4 * W + 1, None, False),
            "live_tiles": (32 * 2 * W + 1, 32 * W + 1, True),      # the weight gradients follow the live tiles, not the capacity
            "second_trip": (32 * 8 * cus + 33, None, False),       # k_train_fwd / k_train_bwd: a second trip, the last tile partial
            "second_trip_input_grads": (32 * 16 * cus + 33, None, False)}[name]


EDGES = ["idle_part", "two_tiles", "three_tiles", "four_tiles", "five_tiles", "live_tiles", "second_trip", "second_trip_input_grads"]


@pytest.mark.parametrize("name", EDGES)
def test_part_and_trip_edges_against_float64(hiplib, monkeypatch, name):
    M, live, row = _edge(name)
    _compare(monkeypatch, "default", M, SEED0 + 100 + EDGES.index(name), live=live, row=row)


# ---------------------------------------------------------------------------------------------------- c: the deterministic route
def test_deterministic_route_against_float64(hiplib, monkeypatch):
    """RN_TRAIN_DETERMINISTIC=1 (the ordered table-gradient sum) under the same bars."""
    _compare(monkeypatch, "default", 95, SEED0 + 4, deterministic=True)


# ------------------------------------------------------------------------------------------------------------- d: live count
@pytest.mark.parametrize("live", [0, 1, 40])
def test_rows_past_the_live_count_keep_the_sentinel(hiplib, monkeypatch, live):
    """The fp32 entries on sentinel-filled buffers of capacity 64: rows past the device count are not written in any of the six
    outputs and both feature-gradient blocks, rows below it are bit-equal to a run on the first `live` rows alone, and with a
    count of 0 every gradient through autograd is exactly zero."""
    m, b = model("default"), batch32("default", 64, SEED0 + 5)
    cnt = torch.tensor([live, 0], dtype=torch.int32, device="cuda")
    capped = direct(m, b, "", m_dev=cnt, up=b["up"], sentinel=SENTINEL)
    for k in ("sigmas", "rgbs", "ambient", "amb_abs", "xn", "wn"):
        assert bool((capped[k][live:] == SENTINEL).all()), k
    for k in ("g_enc_x", "g_enc_w"):
        assert bool((capped[k][:, live:] == SENTINEL).all()), k
    if live:
        exact = direct(m, b, "", M=live, up=b["up"], sentinel=SENTINEL)
        for k in ("sigmas", "rgbs", "ambient", "amb_abs", "xn", "wn"):
            assert torch.equal(capped[k][:live], exact[k]) and bool((exact[k] != SENTINEL).all()), k
        for k in ("g_enc_x", "g_enc_w"):
            assert torch.equal(capped[k][:, :live], exact[k]) and bool((exact[k] != SENTINEL).all()), k
    else:
        environment(monkeypatch, "f32")
        _, (g,) = head(m, b, b["up"], live=0, input_grads=True)
        assert {"encoder.embeddings", "encoder_ambient.embeddings", "sigma_net.net.0.weight", "enc_a", "eye", "individual_codes", "xyzs"} <= set(g)
        for name, t in g.items():
            assert torch.isfinite(t).all() and (t.numel() == 0 or float(t.abs().max()) == 0.0), name


# ------------------------------------------------------------------------------------------------ e: a large code table, row form
@pytest.mark.parametrize("rows", [300, 16400])
def test_row_form_fills_one_row_of_a_large_code_gradient_table(hiplib, rows):
    """k_train_const in row form zero-fills the gradient table of individual_codes with min(ceil(rows * 4 / 1024), 64) extra
    workgroups of 256 threads: 300 rows = 1200 elements take two of them with a ragged end, 16 400 rows = 65 600 elements lie past
    the clamp at 64 (a grid-stride loop of more than one trip).  Row 0, a middle row and the last row: the row's gradient equals
    the code form's bit for bit, every other element of the sentinel-filled table comes back exactly zero, and every other
    gradient is the code form's."""
    m = netref16.head_scene("default", "cuda").model              # a model of this test's own: its code table is replaced
    m.train()
    gen = torch.Generator().manual_seed(rows)
    m.individual_codes = torch.nn.Parameter((torch.randn(rows, m.individual_dim, generator=gen) * 0.1).cuda())
    b = batch32("default", 95, SEED0 + 4)
    assert rows * m.individual_dim > 1024 and (rows * m.individual_dim) % 1024 != 0
    for r in (0, rows // 2, rows - 1):
        d = direct(m, b, "", up=b["up"], ind_row=r)
        code = weight_grads(m, b, d["work"], 95, r, False, SENTINEL)
        table = weight_grads(m, b, d["work"], 95, r, True, SENTINEL)
        got = table.pop("ind_code")
        want = code.pop("ind_code")
        assert got.shape == (rows, m.individual_dim) and torch.isfinite(want).all() and float(want.abs().min()) > 0 and bool((want != SENTINEL).all())
        assert torch.equal(got[r], want), r
        rest = got.clone()
        rest[r] = 0
        assert int((rest != 0).sum()) == 0, (r, int((rest == SENTINEL).sum()), int((rest != 0).sum()))
        for k in code:
            assert torch.equal(table[k], code[k]) and bool((code[k] != SENTINEL).all()), k
