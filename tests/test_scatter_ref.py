"""The scatter tests' reference (tests/scatter_ref.py) against the CPU oracle, and the preconditions of the input patterns that
tests/test_gpu_scatter_atomic.py runs, for the committed seeds: a change of seed or shape cannot quietly turn a path off."""
import numpy as np
import pytest

import scatter_ref as ref

_CACHE = {}


def _case(grid, pattern):
    if (grid, pattern) not in _CACHE:
        enc = ref.grid(grid)
        x, g, live = ref.PATTERNS[pattern](enc)
        _CACHE[grid, pattern] = (enc, x, g, live, ref.reference(enc, x, g, live))
    return _CACHE[grid, pattern]


def test_the_level_plan_of_the_grids():
    """hash17 / tiled2 / tiled3 as the GPU tests need them, and the product's hash-19 table: eleven direct levels, three 8-chunk
    levels, two 1-chunk levels."""
    h = ref.plan(ref.grid("hash17"))
    assert int(h["rows"].sum()) == 1709560 and h["rows"][3] == 85184 and (h["rows"][4:] == 131072).all()
    assert h["chunks"].tolist() == [8, 8, 8] + [1] * 13 and not h["hashed"][:4].any() and h["hashed"][4:].all()
    assert (h["direct"] == h["hashed"]).all() and (h["binned"] == h["hashed"]).all() and (h["n_buckets"][4:] == 32).all()
    assert h["binned_mask"] == 0xfff0 and not ref.plan(ref.grid("hash17"), host_offsets=False)["direct"].any()
    assert ref.bucket_capacity(4096, ref.grid("hash17")) == 4096 and ref.bucket_capacity(4608, ref.grid("hash17")) == 4352
    for name, total in (("tiled2", 555520), ("tiled3", 903480)):          # the published tables (test_oracle_grid.py)
        t = ref.plan(ref.grid(name))
        assert int(t["rows"].sum()) == total and t["rows"].max() == 65536 and (t["chunks"] == 8).all()
        assert not t["hashed"].any() and not t["direct"].any() and t["binned_mask"] == 0 and ref.bucket_capacity(4096, ref.grid(name)) == 0
    assert (ref.plan(ref.grid("tiled3"), host_offsets=False)["chunks"] == 1).all()
    p19 = ref.plan(ref.Grid(3, 19, "hash"))
    assert int(p19["rows"].sum()) == 6119864
    assert int(p19["direct"].sum()) == 11 and int((p19["chunks"] == 8).sum()) == 3 and int((~p19["direct"] & (p19["chunks"] == 1)).sum()) == 2
    assert ref.plan(ref.grid("tiled3", num_levels=8))["rows"].shape == (8,)


def test_the_bound_of_one_fp32_sum():
    n, mag = np.array([0.0, 1.0, 2.0, 4608.0]), np.ones((4, 2))
    b = ref.bound(n, mag)
    assert b[0, 0] == 0.0 and b[1, 0] == 0.0 and b[2, 0] == ref.U / (1 - ref.U) and b[3, 1] == 4607 * ref.U / (1 - 4607 * ref.U)
    # a sequential fp32 sum of 4096 random terms: inexact, and inside the bound
    v = np.random.default_rng(0).standard_normal(4096).astype(np.float32)
    s = np.float32(0)
    for t in v:
        s = np.float32(s + t)
    err = abs(float(s) - float(v.astype(np.float64).sum()))
    assert 0 < err <= float(ref.bound(np.array([4096.0]), np.array([[float(np.abs(v.astype(np.float64)).sum())] * 2]))[0, 0])


GRID_PATTERNS = [(g, p) for g in ref.GRIDS for p in ("uniform", "ray_runs", "mixed", "coincident")] + [("hash17", "overfull_bucket")]


@pytest.mark.parametrize("grid,pattern", GRID_PATTERNS)
def test_the_oracle_lies_within_the_bound_of_the_exact_sum(po, grid, pattern):
    enc, x, g, live, (n, mag, exact) = _case(grid, pattern)
    want = ref._oracle(po, enc, x, g, live)
    assert np.isfinite(want).all() and np.isfinite(mag).all()
    assert not (want[n == 0] != 0).any()                                   # the oracle touches the rows with n > 0 and no other
    assert (want[n > 0] != 0).any(axis=1).mean() > 0.999                   # (a sum may cancel to zero; here next to none does)
    assert (np.abs(want.astype(np.float64) - exact) <= ref.bound(n, mag)).all()
    assert np.array_equal(want[n == 1].astype(np.float64), exact[n == 1])  # one addend: the oracle's bits are the restated addend's
    v = ref.verdict(want, (n, mag, exact))
    print(grid, pattern, "oracle: largest err / bound %.3f" % v["worst"], "longest run", v["longest"], "rows with one addend", int((n == 1).sum()))
    assert v["untouched_changed"] == v["single_wrong"] == v["over"] == v["nan"] == 0


def test_the_eight_level_grid_of_the_two_job_case(po):
    enc = ref.grid("tiled3", num_levels=8)
    x, g, live = ref.uniform(enc)
    n, mag, exact = ref.reference(enc, x, g, live)
    want = ref._oracle(po, enc, x, g, live)
    assert g.shape[0] == 8 and not (want[n == 0] != 0).any() and (np.abs(want.astype(np.float64) - exact) <= ref.bound(n, mag)).all()


@pytest.mark.parametrize("grid", list(ref.GRIDS))
def test_uniform_flushes_mid_loop_and_most_fine_rows_have_one_addend(grid):
    enc, x, g, live, (n, mag, exact) = _case(grid, "uniform")
    assert live == 4096 and x.shape[0] == ref.CAP and np.isnan(x[live:]).all() and np.isnan(g[:, live:]).all()
    xs = x[:live]
    assert (xs[0] == 0).all() and (xs[1] == 1).all() and xs[2, 0] == 0 and xs[3, -1] == 1 and xs[4, 0] > 1 and xs[5, -1] < 0
    p, off = ref.plan(enc), ref._offsets(enc)
    for level in range(16):
        flushes, peaks, per_chunk = ref.simulate_tables(enc, x, live, level, int(p["chunks"][level]))
        heads = ref.wave_heads(enc, x, live, level)
        assert heads.min() > ref.MERGE_HEADS                               # sum_runs's early return: nothing to merge
        if p["chunks"][level] == 8 and not (grid == "tiled2" and level < 4):
            # every workgroup empties its table for the next chunk at least once (tiled2's levels 0-2 have fewer lines in all
            # than the threshold, level 3 flushes in some workgroups only)
            assert flushes.min() >= 1, (grid, level)
        if grid in ("hash17", "tiled3"):
            assert 202 <= per_chunk.min() or level >= 9 and grid == "tiled3"
        if grid == "hash17" and level >= 3:
            nl = n[off[level]:off[level + 1]]
            assert (nl == 1).sum() >= 0.7 * (nl > 0).sum()
        if grid == "tiled3" and level >= 9:                                # z is dropped: two corners fall on one row
            nl = n[off[level]:off[level + 1]]
            assert nl[nl > 0].min() >= 2


@pytest.mark.parametrize("grid", list(ref.GRIDS))
def test_ray_runs_reach_the_segmented_scan(grid):
    """On the coarsest level most waves have at most 40 run heads (the scan runs) and fewer heads than live lanes (it has runs to
    merge); on the finest level some waves have more than 40 (the other branch, in the same launch)."""
    enc, x, g, live, _ = _case(grid, "ray_runs")
    coarse, fine = ref.wave_heads(enc, x, live, 0), ref.wave_heads(enc, x, live, 15)
    print(grid, "level 0 heads per wave", coarse.min(), np.median(coarse), coarse.max(), "scanned share", (coarse <= ref.MERGE_HEADS).mean())
    assert (coarse <= ref.MERGE_HEADS).mean() >= 0.5 and coarse.max() < 64
    assert (fine > ref.MERGE_HEADS).any()


@pytest.mark.parametrize("grid", list(ref.GRIDS))
def test_mixed_fills_a_table_close_to_its_slot_count(grid):
    enc, x, g, live, _ = _case(grid, "mixed")
    p = ref.plan(enc)
    best = 0
    for level in np.flatnonzero(p["chunks"] == 8):
        flushes, peaks, per_chunk = ref.simulate_tables(enc, x, live, int(level), 8)
        assert per_chunk.reshape(-1, 8)[:, :ref.MIXED_CLUSTERED].max() <= 190, (grid, level)
        best = max(best, int(peaks.max()))
    print(grid, "mixed: most lines one table is offered between two flushes", best, "of", ref.SC_SLOTS, "slots")
    assert 448 <= best


def test_the_overfull_bucket_spills_in_short_runs():
    enc, x, g, live, _ = _case("hash17", "overfull_bucket")
    cap = ref.bucket_capacity(live, enc)
    entries, runs = ref.bucket_load(enc, x, live, ref.OVERFULL_LEVEL)
    print("bucket 0 of level", ref.OVERFULL_LEVEL, "entries", int(entries[0]), "capacity", cap, "longest run", int(runs[0]))
    assert x.shape[0] == live == 4096 and cap == 4096 and ref.plan(enc)["binned"][ref.OVERFULL_LEVEL]
    assert entries[0] > cap and runs[0] <= 16
    # the call in between: uniform samples at a smaller live count fill no bucket of any binned level
    enc, x, g, _, _ = _case("hash17", "uniform")
    for level in np.flatnonzero(ref.plan(enc)["binned"]):
        assert ref.bucket_load(enc, x, 3000, int(level))[0].max() < cap


def test_coincident_samples_overflow_their_buckets():
    enc, x, g, live, (n, mag, exact) = _case("hash17", "coincident")
    cap = ref.bucket_capacity(live, enc)
    assert live == ref.CAP == 4608 and cap == 4352 and n.max() >= live
    for level in np.flatnonzero(ref.plan(enc)["binned"]):
        entries, runs = ref.bucket_load(enc, x, live, int(level))
        assert entries.sum() == 8 * live and runs.max() >= live and entries.max() > cap


@pytest.mark.parametrize("grid,seed,live,binned", ref.SUMMED_ONCE)
def test_the_prefilled_cases_add_to_memory_once_per_row(grid, seed, live, binned):
    enc = ref.grid(grid)
    x, g, live = ref.spread(enc, seed, live)
    r = ref.reference(enc, x, g, live)
    assert ref.summed_once(enc, x, live, r, binned) is None
    assert (r[0] > 1).sum() >= 20                                          # rows with several addends exist all the same
