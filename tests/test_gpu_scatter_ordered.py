"""The ordered table-gradient sum (rn_grid_scatter_ordered, csrc/rn_grid_scatter_ordered.hip) against the CPU oracle, BIT FOR BIT.

orc_grid_encode_backward adds every row's contributions level by level, samples ascending, corners ascending, in fp32 with
-ffp-contract=off; the ordered scatter keeps that order, so `==` on the uint32 views is the test.  The inputs make the order matter
(hundreds of contributions per coarse row, gradients over 24 binades): a precondition, asserted on the CPU, shows that the oracle
itself gives other bits when it sees the same samples in reversed order.  Rows past the live count are NaN: reading one would show.
"""
import numpy as np
import pytest
import torch

from scatter_ref import _bits, _contributions, _inputs, _jobs, _oracle, accumulate  # noqa: F401  (shared with test_gpu_scatter_atomic.py)

pytestmark = pytest.mark.gpu

CAP, LIVE = 777, 700
GRIDS = {
    "hash3": dict(input_dim=3, log2_hashmap_size=14, gridtype="hash"),
    "tiled3": dict(input_dim=3, log2_hashmap_size=14, gridtype="tiled"),
    "tiled2": dict(input_dim=2, log2_hashmap_size=12, gridtype="tiled"),
}
_CACHE = {}


def _encoder(name):
    from gridencoder import GridEncoder
    return GridEncoder(num_levels=16, level_dim=2, base_resolution=16, desired_resolution=2048, **GRIDS[name]).cuda()


def _case(po, name):
    """One grid's inputs, oracle result and device tensors, computed once and shared (nobody writes to them)."""
    if name not in _CACHE:
        enc = _encoder(name)
        x, g = _inputs(enc.input_dim, CAP, LIVE)
        _CACHE[name] = dict(enc=enc, x=x, g=g, want=_oracle(po, enc, x, g, LIVE), xd=torch.from_numpy(x).cuda(), gd=torch.from_numpy(g).cuda(),
                            cnt=torch.tensor([LIVE], dtype=torch.int32, device="cuda"))
    return _CACHE[name]


def _ordered(entries, M, cnt, short=0):
    """rn_grid_scatter_ordered on the current stream -> return code; `short`: bytes withheld from the workspace."""
    import radnerf_hip as hip
    arr, keep = _jobs(entries)
    need = int(hip._lib.rn_grid_scatter_ordered_workspace(arr, len(entries), M))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    rc = hip._lib.rn_grid_scatter_ordered(arr, len(entries), M, None if cnt is None else cnt.data_ptr(), ws.data_ptr(), need - short, hip.stream())
    torch.cuda.synchronize()
    return rc


def _run(case, M=CAP, cnt="case"):
    table = torch.zeros_like(case["enc"].embeddings)
    assert _ordered([(case["gd"], case["xd"], case["enc"], table)], M, case["cnt"] if cnt == "case" else cnt) == 0
    return table


@pytest.mark.parametrize("name", list(GRIDS))
def test_equals_the_oracle_bit_for_bit(po, hiplib, name):
    case = _case(po, name)
    want = case["want"]
    # precondition (CPU only): the oracle, given the same samples in reversed order, gives other bits in >= 500 elements -- so
    # equality below does tell one order from another
    rev = _oracle(po, case["enc"], np.ascontiguousarray(case["x"][:LIVE][::-1]), np.ascontiguousarray(case["g"][:, :LIVE][:, ::-1]), LIVE)
    changed = int((_bits(rev) != _bits(want)).sum())
    touched = int((want != 0).sum())
    print(name, "elements whose bits depend on the order:", changed, "of", touched, "touched")
    assert changed >= 500
    assert not np.isnan(want).any()
    got = _run(case)
    diff = int((_bits(got) != _bits(want)).sum())
    print(name, "elements differing from the oracle:", diff)
    assert diff == 0


def test_two_jobs_equal_the_two_single_jobs(po, hiplib):
    a, b = _case(po, "hash3"), _case(po, "tiled2")
    ta, tb = torch.zeros_like(a["enc"].embeddings), torch.zeros_like(b["enc"].embeddings)
    assert _ordered([(a["gd"], a["xd"], a["enc"], ta), (b["gd"], b["xd"], b["enc"], tb)], CAP, a["cnt"]) == 0
    assert np.array_equal(_bits(ta), _bits(_run(a))) and np.array_equal(_bits(tb), _bits(_run(b)))
    assert np.array_equal(_bits(ta), _bits(a["want"])) and np.array_equal(_bits(tb), _bits(b["want"]))


@pytest.mark.parametrize("M", [1, 31, 32, 33, 256, 257])
def test_row_counts_around_the_wave_and_the_workgroup(po, hiplib, M):
    """Every row live (no device count): M around 32 / 256, the sizes at which the key and the sum launches gain a wave or a
    workgroup; with M >= 33 the coarse rows' runs are longer than a wave (the whole-wave walk)."""
    enc = _case(po, "hash3")["enc"]
    x, g = _inputs(3, M, M, seed=100 + M)
    want = _oracle(po, enc, x, g, M)
    table = torch.zeros_like(enc.embeddings)
    assert _ordered([(torch.from_numpy(g).cuda(), torch.from_numpy(x).cuda(), enc, table)], M, None) == 0
    assert np.array_equal(_bits(table), _bits(want))


def test_a_live_count_of_zero_leaves_the_table_zero(po, hiplib):
    case = _case(po, "tiled3")
    got = _run(case, cnt=torch.zeros(1, dtype=torch.int32, device="cuda"))
    assert not _bits(got).any()


def test_a_workspace_one_byte_short_is_an_error_and_launches_nothing(po, hiplib):
    import radnerf_hip as hip
    case = _case(po, "hash3")
    table = torch.zeros_like(case["enc"].embeddings)
    rc = _ordered([(case["gd"], case["xd"], case["enc"], table)], CAP, case["cnt"], short=1)
    assert rc != 0 and "workspace" in hip.last_error()
    assert not _bits(table).any()


def test_two_calls_and_a_side_stream_give_the_same_bits(po, hiplib):
    case = _case(po, "hash3")
    first = _bits(_run(case))
    assert np.array_equal(first, _bits(_run(case)))
    # on a side stream, while a long kernel keeps the main stream busy
    side = torch.cuda.Stream()
    a = torch.randn(4096, 4096, device="cuda")
    torch.cuda.synchronize()
    busy = a @ a
    with torch.cuda.stream(side):
        got = _bits(_run(case))
    torch.cuda.synchronize()
    assert busy.shape == a.shape and np.array_equal(first, got)
    assert np.array_equal(first, _bits(case["want"]))


@pytest.mark.parametrize("name", ["hash3", "tiled2"])
def test_within_the_two_sum_bound_of_the_atomic_scatter(po, hiplib, name):
    """|ordered - rn_grid_scatter_jobs| <= 2 (n - 1) 2^-24 sum |v_i| per element: two fp32 sums of the same n terms each lie within
    (n - 1) u sum |v_i| of the exact sum (u = 2^-24).  n and sum |v_i| come from a float64 np.add.at of the oracle's contributions."""
    import radnerf_hip as hip
    case = _case(po, name)
    rows, vals = _contributions(case["enc"], case["x"], case["g"], LIVE)
    n, mag, exact = accumulate(rows, vals, case["want"].shape[0])
    bound = 2.0 * np.maximum(n - 1.0, 0.0)[:, None] * 2.0 ** -24 * mag
    # the restatement is the oracle's: same rows touched, and the oracle's fp32 sum within half that bound of the float64 one
    assert not (case["want"][n == 0] != 0).any()
    assert (np.abs(case["want"].astype(np.float64) - exact) <= bound / 2).all()
    ordered = _run(case).cpu().numpy()
    lbc = torch.zeros_like(case["enc"].embeddings)
    arr, keep = _jobs([(case["gd"], case["xd"], case["enc"], lbc)])
    hip.call("rn_grid_scatter_jobs", arr, 1, CAP, case["cnt"].data_ptr(), None, 0, hip.stream())
    torch.cuda.synchronize()
    err = np.abs(ordered.astype(np.float64) - lbc.cpu().numpy().astype(np.float64))
    print(name, "largest |ordered - atomic| / bound:", float((err / np.maximum(bound, 1e-300)).max()), "longest run:", int(n.max()))
    assert (err <= bound).all()
