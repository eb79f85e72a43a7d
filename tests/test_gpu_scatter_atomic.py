"""The atomic table-gradient scatters (csrc/rn_grid_scatter.hip) against the exact sum, ELEMENT BY ELEMENT.

Reference: the oracle's addends restated in numpy fp32 (tests/scatter_ref.py, held to the CPU oracle by tests/test_scatter_ref.py)
and summed in float64.  For every table element, with n addends of total magnitude mag:
    n == 0   the contents keep their bits;
    n == 1   the value IS the addend (the kernels multiply in the oracle's order, so there is nothing to round differently);
    n >= 2   |got - exact| <= gamma(n - 1) mag, gamma(k) = k u / (1 - k u), u = 2^-24: the bound of an fp32 sum in any order,
             which covers run merges, LDS atomics, memory-side atomics and bucket sums alike.
No other tolerance appears below.  Routes: `lbc` (rn_grid_scatter_lbc: no host offsets, every level line-merged, one chunk), `jobs`
(rn_grid_scatter_jobs with host offsets: direct levels, 8-chunk tables -- the default training route), `binned` (the same with a
workspace: hashed levels through k_grid_bin / k_grid_scatter_buckets), `wrapper` (train_head.grid_scatter), `encode`
(rn_grid_encode_backward, csrc/rn_grid.hip: k_grid_bwd_table_merge, fp32, C = 2, no dy_dx, in both layouts; it has no device count,
so it gets the live rows alone; every addition on its way to memory is an fp32 add -- run sum, ds_add_f32, global atomic -- and a
row with one addend is 0 + w g throughout, so the same three clauses hold).  Grids: the smallest
at which every path exists (scatter_ref.plan).  What each input pattern is for, and that it gets there, is asserted on the CPU in
tests/test_scatter_ref.py; rows past the live count are NaN in the inputs and the gradients, so reading one would show.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import scatter_ref as ref

pytestmark = pytest.mark.gpu

_ENC, _CASES = {}, {}


@pytest.fixture(autouse=True)
def _knobs_unset():
    """RN_SCATTER_DIRECT / _CHUNKS / _BUCKET_SHIFT are read once per process into statics: the plan these tests restate holds only
    with all three unset, and a skip would hide the case."""
    for knob in ("RN_SCATTER_DIRECT", "RN_SCATTER_CHUNKS", "RN_SCATTER_BUCKET_SHIFT"):
        assert knob not in os.environ, knob


def _encoder(name, L=16):
    if (name, L) not in _ENC:
        from gridencoder import GridEncoder
        enc = GridEncoder(num_levels=L, level_dim=2, base_resolution=16, desired_resolution=2048, **ref.GRIDS[name]).cuda()
        assert np.array_equal(enc.offsets.cpu().numpy(), ref.grid(name, L).offsets)       # the CPU preconditions are about this grid
        _ENC[name, L] = enc
    return _ENC[name, L]


def _device(enc, x, g, live, po):
    """One case: device tensors, the exact reference; precondition: the oracle's result on the live rows is finite."""
    assert np.isfinite(ref._oracle(po, enc, x, g, live)).all() if live else True
    return dict(enc=enc, x=x, g=g, live=live, cap=x.shape[0], ref=ref.reference(enc, x, g, live), xd=torch.from_numpy(x).cuda(),
                gd=torch.from_numpy(g).cuda(), cnt=torch.tensor([live], dtype=torch.int32, device="cuda"))


def _case(po, grid, pattern, L=16):
    """Computed once and shared (nobody writes to them)."""
    if (grid, pattern, L) not in _CASES:
        enc = _encoder(grid, L)
        _CASES[grid, pattern, L] = _device(enc, *ref.PATTERNS[pattern](enc), po)
    return _CASES[grid, pattern, L]


def _grid_args(enc, table):
    import radnerf_hip as hip
    from radnerf.fused import _grid_desc
    return _grid_desc(enc, table), hip.host_offsets(enc.offsets)


def _workspace(enc, M):
    """Zeroed bucket workspace of rn_grid_scatter_workspace() bytes for row capacity M."""
    import radnerf_hip as hip
    gd, off = _grid_args(enc, enc.embeddings)
    return torch.zeros(int(hip._lib.rn_grid_scatter_workspace(M, C.byref(gd), off)), dtype=torch.uint8, device="cuda")


def _scatter(route, entries, M, cnt, ws=None):
    """entries = [(grad, inputs, enc, table), ...] through `route` on the current stream."""
    import radnerf_hip as hip
    count = None if cnt is None else cnt.data_ptr()
    if route == "lbc":
        (grad, inputs, enc, table), = entries
        gd, _ = _grid_args(enc, table)
        hip.call("rn_grid_scatter_lbc", grad.data_ptr(), inputs.data_ptr(), M, count, C.byref(gd), table.data_ptr(), hip.stream())
    else:
        assert (route == "binned") == (ws is not None)
        arr, keep = ref._jobs(entries)
        hip.call("rn_grid_scatter_jobs", arr, len(entries), M, count, None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel(), hip.stream())
    torch.cuda.synchronize()


def _encode(case, layout):
    """The table gradient of the case's live rows through rn_grid_encode_backward into a zero table: `lbc` takes the gradient as
    the case holds it, [L, B, 2]; `blc` takes its transpose [B, L * 2]."""
    import radnerf_hip as hip
    enc, live = case["enc"], case["live"]
    L = case["g"].shape[0]
    x, g = case["xd"][:live].contiguous(), case["gd"][:, :live].contiguous()
    if layout == "blc":
        g = g.permute(1, 0, 2).contiguous()
    table = torch.zeros_like(enc.embeddings)
    hip.call("rn_grid_encode_backward", hip.ptr(g), hip.ptr(x), hip.ptr(enc.embeddings.detach()), hip.ptr(enc.offsets, torch.int32), hip.ptr(table),
             live, enc.input_dim, 2, L, float(np.log2(enc.per_level_scale)), ref.BASE, None, None, enc.gridtype_id, 0, 0, hip.RN_F32,
             {"lbc": hip.RN_LAYOUT_LBC, "blc": hip.RN_LAYOUT_BLC}[layout], hip.stream())
    torch.cuda.synchronize()
    return table.cpu().numpy()


def _cursors(ws, enc):
    """The bucket cursors and both spill counters at the start of the workspace."""
    p = ref.plan(enc)
    total = int(p["n_buckets"][p["binned"]].sum())
    assert total > 0
    return ws[:4 * (total + 2)].view(torch.int32).cpu().numpy()


def _run(case, route, ws=None, prior=None, cnt="case"):
    enc = case["enc"]
    table = torch.zeros_like(enc.embeddings) if prior is None else torch.full_like(enc.embeddings, prior)
    if route == "binned" and ws is None:
        ws = _workspace(enc, case["cap"])
    _scatter(route, [(case["gd"], case["xd"], enc, table)], case["cap"], case["cnt"] if cnt == "case" else cnt, ws)
    return table.cpu().numpy()


def _check(label, got, case, prior=None, rows=None):
    """The three clauses of the module docstring for `got` (the rows `rows` of it); prints the largest err / bound and the longest run."""
    r = case["ref"]
    before = None if prior is None else np.full_like(got, prior)
    if rows is not None:
        got, r, before = got[rows], tuple(a[rows] for a in r), None if before is None else before[rows]
    v = ref.verdict(got, r, before)
    print(label, "largest err / bound: %.3f" % v["worst"], "longest run:", v["longest"], "rows with one addend:", int((r[0] == 1).sum()))
    misses = ref.first_failures(got, r, case["enc"], before) if rows is None else None       # (level, row, channel, n, got, wanted, bound)
    assert v["untouched_changed"] == v["single_wrong"] == v["over"] == v["nan"] == 0, (label, v, misses)


def test_the_library_plans_the_levels_as_restated(hiplib):
    import radnerf_hip as hip
    for name in ref.GRIDS:
        enc = _encoder(name)
        gd, off = _grid_args(enc, enc.embeddings)
        p = ref.plan(enc)
        assert int(hip._lib.rn_grid_scatter_binned_levels(C.byref(gd), off)) == p["binned_mask"]
        total = int(p["n_buckets"][p["binned"]].sum())
        for M in (1, 4096, 4608):
            need = int(hip._lib.rn_grid_scatter_workspace(M, C.byref(gd), off))
            if not total:
                assert need == 256
            else:   # cursors + 2 counters | (row, value) per bucket entry and per spill entry (every entry of a launch fits the list)
                spill = (M << enc.input_dim) * int(p["binned"].sum())
                assert need == (-(-(total + 2) * 4 // 256) * 256) + (total * ref.bucket_capacity(M, enc) + spill) * 12 + 256 > 256


PATTERN_CASES = ([(route, grid, pattern) for route in ("lbc", "jobs") for grid in ref.GRIDS for pattern in ("uniform", "ray_runs", "coincident")]
                 + [("jobs", grid, "mixed") for grid in ref.GRIDS] + [("binned", "hash17", pattern) for pattern in ("uniform", "ray_runs", "mixed", "coincident")]
                 + [("encode", grid, pattern) for grid in ref.GRIDS for pattern in ("uniform", "ray_runs", "coincident")])


@pytest.mark.parametrize("route,grid,pattern", PATTERN_CASES)
def test_every_element_within_the_bound_of_its_exact_sum(po, hiplib, route, grid, pattern):
    """uniform: the table is emptied in the middle of the chunk loop (a contribution dropped or added twice there breaks a row with
    one addend); most touched rows of the fine levels have one addend, so equality carries most of the test; the direct path's
    lane-to-float mapping is held the same way.  ray_runs: the segmented scan of sum_runs.  mixed: a chunk is inserted into a
    table that holds close to its slot count, which makes the probe-limit fallback LIKELY; the test cannot see which path a line
    took and does not claim the fallback ran.  coincident: runs of 4 608 (and, binned, ~256 spilled entries per bucket); the derived
    bound is wide there (gamma(4607) ~ 2.7e-4 of the magnitude), so ONE dropped addend can hide inside it -- this case checks the
    long-run machinery to that bound only; the patterns with short runs are the sharp ones.  encode: both layouts of the operator's
    own table gradient, whose workgroups (256 samples of one level) each flush on their own."""
    case = _case(po, grid, pattern)
    if route == "encode":
        for layout in ("lbc", "blc"):
            _check(f"encode {layout} {grid} {pattern}", _encode(case, layout), case)
        return
    _check(f"{route} {grid} {pattern}", _run(case, route), case)


@pytest.mark.parametrize("scatter", [None, "binned"])
def test_the_wrapper_on_both_routes(po, hiplib, monkeypatch, scatter):
    """train_head.grid_scatter with RN_SCATTER unset (the default training route) and =binned (persistent workspace sized for the
    capacity rounded up to 65 536 rows; the second call finds the cursors the first one left)."""
    from radnerf import train_head
    monkeypatch.delenv("RN_TRAIN_DETERMINISTIC", raising=False)
    monkeypatch.delenv("RN_SCATTER", raising=False)
    if scatter:
        monkeypatch.setenv("RN_SCATTER", scatter)
    assert train_head.binning_active() == bool(scatter) and not train_head.deterministic()
    case = _case(po, "hash17", "uniform")
    enc = case["enc"]
    for call in range(2):
        table = torch.zeros_like(enc.embeddings)
        gd, _ = _grid_args(enc, table)
        train_head.grid_scatter([(case["gd"], case["xd"], enc, gd, table)], case["cap"], case["cnt"])
        torch.cuda.synchronize()
        _check(f"wrapper RN_SCATTER={scatter} call {call}", table.cpu().numpy(), case)


def test_an_overfull_bucket_spills_and_the_cursors_return_to_zero(po, hiplib):
    """Bucket 0 of one hashed level gets twice its capacity in runs of at most 9: a lost spilled entry breaks a tight bound or an
    equality.  Three calls on ONE workspace -- overfull, uniform at a smaller live count (no spill), overfull again -- each held to
    its own reference; afterwards the cursors and both spill counters are zero."""
    over = _case(po, "hash17", "overfull_bucket")
    enc = over["enc"]
    x, g, _ = ref.uniform(enc, live=3000, cap=4096)
    if ("hash17", "uniform3000", 16) not in _CASES:
        _CASES["hash17", "uniform3000", 16] = _device(enc, x, g, 3000, po)
    between = _CASES["hash17", "uniform3000", 16]
    assert over["cap"] == between["cap"] == 4096
    ws = _workspace(enc, 4096)
    for label, case in (("overfull 1", over), ("uniform", between), ("overfull 2", over)):
        _check("binned hash17 " + label, _run(case, "binned", ws), case)
    assert not _cursors(ws, enc).any()


EDGES = [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1025]
ENCODE_EDGES = [1, 63, 64, 65, 255, 256, 257, 513]        # rn_grid_encode_backward: a wave is 64 samples, a workgroup 256


@pytest.mark.parametrize("M", EDGES)
@pytest.mark.parametrize("grid", ["hash17", "tiled2"])
def test_live_counts_around_the_chunk_the_bin_block_and_eight_chunks(po, hiplib, grid, M):
    """Every row live, no device count: M around the samples of a workgroup (64 for D = 3, 128 for D = 2), k_grid_bin's 256, and
    eight chunks (512 / 1 024) -- the last partial chunk of a table that has summed others before it.  The operator's own table
    gradient (route `encode`, both layouts) at the counts around its wave and its workgroup."""
    enc = _encoder(grid)
    case = _device(enc, *ref.uniform(enc, seed=100 + M, live=M, cap=M), po)
    for route in ("jobs", "binned") if grid == "hash17" else ("jobs",):
        _check(f"{route} {grid} M={M}", _run(case, route, cnt=None), case)
    if M in ENCODE_EDGES:
        for layout in ("lbc", "blc"):
            _check(f"encode {layout} {grid} M={M}", _encode(case, layout), case)


ROUTES = [("lbc", "hash17"), ("lbc", "tiled2"), ("lbc", "tiled3"), ("jobs", "hash17"), ("jobs", "tiled2"), ("jobs", "tiled3"), ("binned", "hash17")]


@pytest.mark.parametrize("route,grid", ROUTES)
def test_a_device_count_below_the_capacity(po, hiplib, route, grid):
    """Live 700 of 777 (the ordered tests' inputs): the rows past the count are NaN and must not be read."""
    if (grid, "700of777", 16) not in _CASES:
        enc = _encoder(grid)
        _CASES[grid, "700of777", 16] = _device(enc, *ref._inputs(enc.input_dim, 777, 700), 700, po)
    case = _CASES[grid, "700of777", 16]
    _check(f"{route} {grid} 700 of 777", _run(case, route), case)


@pytest.mark.parametrize("route,grid", ROUTES)
def test_a_device_count_of_zero_leaves_the_table_zero(po, hiplib, route, grid):
    case = _case(po, grid, "uniform")
    ws = _workspace(case["enc"], case["cap"]) if route == "binned" else None
    got = _run(case, route, ws, cnt=torch.zeros(1, dtype=torch.int32, device="cuda"))
    assert not ref._bits(got).any()
    if ws is not None:
        assert not _cursors(ws, case["enc"]).any()


@pytest.mark.parametrize("route", ["jobs", "binned"])
@pytest.mark.parametrize("first,second,L2", [("hash17", "tiled2", 16), ("tiled2", "hash17", 16), ("hash17", "tiled3", 8)])
def test_two_jobs_in_one_launch_meet_their_single_job_references(po, hiplib, route, first, second, L2):
    """The workgroups of the two jobs alternate along x; the second job has fewer workgroups along x (D = 2: 128 samples each) or
    fewer levels along y (8) than the launch grid, or more of either than the first.  Only job 0 can be binned."""
    a, b = _case(po, first, "uniform"), _case(po, second, "uniform", L2)
    assert a["cap"] == b["cap"] and a["live"] == b["live"]
    ta, tb = torch.zeros_like(a["enc"].embeddings), torch.zeros_like(b["enc"].embeddings)
    ws = _workspace(a["enc"], a["cap"]) if route == "binned" else None
    _scatter(route, [(a["gd"], a["xd"], a["enc"], ta), (b["gd"], b["xd"], b["enc"], tb)], a["cap"], a["cnt"], ws)
    _check(f"{route} two jobs, job 0 {first}", ta.cpu().numpy(), a)
    _check(f"{route} two jobs, job 1 {second} L={L2}", tb.cpu().numpy(), b)


@pytest.mark.parametrize("grid,seed,live,binned", ref.SUMMED_ONCE)
def test_accumulated_levels_keep_a_prefill_and_binned_levels_overwrite_it(po, hiplib, grid, seed, live, binned):
    """include/radnerf_train.h: rows of line-merged and direct levels are ACCUMULATED into, rows of binned levels are WRITTEN.  The
    table starts at 0.5.  Accumulated: got = 0.5 + sum within bound + u |got| (one more rounding), untouched elements exactly 0.5.
    That bound holds where a row receives its whole sum in one addition to memory, so these inputs fit one workgroup and one chunk
    per level, and on the jobs route no row of a direct level has two addends (scatter_ref.summed_once, asserted on the CPU).
    Binned: the levels of rn_grid_scatter_binned_levels() hold the sum alone, untouched rows 0."""
    import radnerf_hip as hip
    enc = _encoder(grid)
    case = _device(enc, *ref.spread(enc, seed, live), po)
    assert ref.summed_once(enc, case["x"], live, case["ref"], binned) is None
    got = _run(case, "binned" if binned else "jobs", prior=0.5)
    gd, off = _grid_args(enc, enc.embeddings)
    mask = int(hip._lib.rn_grid_scatter_binned_levels(C.byref(gd), off)) if binned else 0
    assert mask == (ref.plan(enc)["binned_mask"] if binned else 0)
    offs = ref._offsets(enc)
    written = np.zeros(got.shape[0], bool)
    for level in range(16):
        written[offs[level]:offs[level + 1]] = (mask >> level) & 1
    if written.any():
        _check(f"prefilled binned {grid}: written levels", got, case, rows=written)
    _check(f"prefilled {'binned' if binned else 'jobs'} {grid}: accumulated levels", got, case, prior=0.5, rows=~written)
