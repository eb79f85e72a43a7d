"""CPU pins of the ray families of tests/walk_cases.py: every family really reaches the branch of Dda::walk (csrc/rn_dda_dev.h) it
is named for -- asserted against the oracle, with floors well below what was measured -- and the oracle's walk keeps its invariants
on cascades and a variable dt.  Each test prints the measured shares (pytest -s shows them; DESIGN.md quotes them).
"""
import numpy as np
import pytest

import walk_cases as wc


def _per_sample_ray(w):
    """Row of `rays` that owns each sample (the oracle hands out slices in ray order)."""
    return np.repeat(np.arange(w["rays"].shape[0]), w["rays"][:, 2])


def _shares(po, case):
    w = wc.oracle_walk(po, case)
    dt = w["deltas"][:, 0]
    lp, ld = wc.levels(case, w["xyzs"], dt)
    counts = w["rays"][:, 2]
    m = case.max_abs_d
    s = dict(N=case.N, samples=w["total"], rays_with_samples=int((counts > 0).sum()), max_count=int(counts.max()),
             generic=int((m <= wc.SEAM).sum()), generic_with_samples=int(((m <= wc.SEAM) & (counts > 0)).sum()),
             near_seam=float(((m > wc.SEAM) & (m <= 0.60)).mean()), max_abs_d=(float(m.min()), float(m.max())),
             interior_dt=float(wc.interior(case, dt).mean()) if w["total"] else 0.0,
             ld_gt_lp=float((ld > lp).mean()) if w["total"] else 0.0,
             levels=np.bincount(np.maximum(lp, ld), minlength=case.C).tolist())
    print(f"\n[{case.name}] " + ", ".join(f"{k}={v:.3f}" if isinstance(v, float) else f"{k}={v}" for k, v in s.items()))
    return s, w


@pytest.mark.parametrize("name", wc.FAMILIES)
def test_family_reaches_its_branch(po, name):
    case = wc.family(name, po)
    s, w = _shares(po, case)
    if name == "plus_y":
        assert s["generic"] == 0
    elif name == "diagonal":
        assert s["generic_with_samples"] >= 40 and s["near_seam"] >= 0.5
    elif name == "short":
        assert s["max_abs_d"][1] <= 0.25 and s["rays_with_samples"] >= 0.75 * case.N
    elif name == "needles":
        assert case.N >= wc.NEEDLE_FLOOR and s["max_abs_d"][1] <= 0.25
    elif name == "vardt_c1":
        assert s["interior_dt"] >= 0.9
    elif name == "casc2":
        assert min(s["levels"]) >= 1000 and s["ld_gt_lp"] >= 0.05
    elif name == "casc3":
        assert min(s["levels"]) >= 1000 and s["interior_dt"] >= 0.5
    elif name == "casc3_rec":
        assert case.max_steps <= 32 and s["interior_dt"] >= 0.25 and s["ld_gt_lp"] >= 0.10
    elif name == "degenerate":
        assert np.array_equal(w["nears"], wc.DEGENERATE_NEARS)
        assert np.array_equal(np.isnan(w["fars"]), np.isnan(wc.DEGENERATE_FARS))
        ok = ~np.isnan(wc.DEGENERATE_FARS)
        assert np.array_equal(w["fars"][ok], wc.DEGENERATE_FARS[ok])
        assert w["rays"][:, 2].tolist() == wc.DEGENERATE_COUNTS
    # constant-dt families: the clamp has no interior, so one_step_skips is decided by the direction alone
    if name in ("plus_y", "diagonal", "short", "needles", "degenerate"):
        assert case.C == 1 and case.dt_min == case.dt_max
    else:
        assert case.dt_min < case.dt_max


def _ulp_shift(x, k):
    """x moved by k units in the last place (x > 0, float32)."""
    return (x.view(np.int32) + np.int32(k)).view(np.float32)


@pytest.mark.parametrize("name", wc.FAMILIES)
def test_oracle_walk_invariants(po, name):
    """test_oracle_raymarching.py::test_march_rays_invariants_and_step_size, on cascades and a variable dt."""
    case = wc.family(name, po)
    w = wc.oracle_walk(po, case)
    xyz, dirs, dl, rays = w["xyzs"], w["dirs"], w["deltas"], w["rays"]
    counts = rays[:, 2]
    assert w["counter"][1] == case.N and w["total"] == counts.sum() and (counts <= case.max_steps).all()
    assert np.array_equal(rays[:, 0], np.arange(case.N)) and np.array_equal(rays[:, 1], np.cumsum(counts) - counts)
    # rays whose box test fails (FLT_MAX ends) or is undefined (a NaN end) emit nothing
    dead = ~(w["nears"] < w["fars"])
    assert not counts[dead].any()
    if w["total"] == 0:
        return
    owner = _per_sample_ray(w)
    assert np.array_equal(dirs, case.d[owner])
    assert (np.abs(xyz) <= case.bound).all()
    dt = dl[:, 0]
    assert (dt >= case.dt_min).all() and (dt <= case.dt_max).all()
    # every sample sits in a set cell of level max(lp, ld)
    lp, ld = wc.levels(case, xyz, dt)
    assert wc.occupied(case, xyz, np.maximum(lp, ld)).all()
    # there is ONE t per sample with xyz = clip(o + t d), dt = clamp(t dt_gamma) and deltas[1] = t + dt: the float32 difference
    # deltas[1] - dt is within two units of it
    o, d = case.o[owner], case.d[owner]
    guess = (dl[:, 1] - dt).astype(np.float32)
    # (rounding can let two neighbouring t pass all three: t_lo / t_hi are the least and the greatest that do)
    t_lo = np.full(w["total"], np.inf, np.float32)
    t_hi = np.full(w["total"], -np.inf, np.float32)
    g32 = np.float32(case.dt_gamma)
    for k in (-2, -1, 0, 1, 2):
        tc = _ulp_shift(guess, k)
        ok = ((tc + dt).astype(np.float32) == dl[:, 1]) & (np.clip((tc * g32).astype(np.float32), case.dt_min, case.dt_max) == dt)
        p = np.clip(o + tc[:, None] * d, np.float32(-case.bound), np.float32(case.bound)).astype(np.float32)
        ok &= (p == xyz).all(1)
        t_lo = np.where(ok, np.minimum(t_lo, tc), t_lo)
        t_hi = np.where(ok, np.maximum(t_hi, tc), t_hi)
    assert np.isfinite(t_hi).all(), int((~np.isfinite(t_hi)).sum())
    # along a ray the next sample is taken at or after the point the previous one ends at, and before the far end
    same = owner[1:] == owner[:-1]
    assert (t_hi[1:][same] >= dl[:-1, 1][same]).all()
    assert (t_lo < w["fars"][owner]).all() and (t_hi >= w["nears"][owner]).all()


@pytest.mark.parametrize("name,n_step", [("diagonal", 5), ("casc3", 8), ("vardt_c1", 7)])
def test_chained_inference_marcher_reproduces_the_training_marcher(po, name, n_step):
    """test_march_rays_train_matches_inference_marcher's logic with the inference loop's chunks: march n_step samples, move rays_t to
    the last sample's end, drop the rays that came back short."""
    case = wc.family(name, po)
    w = wc.oracle_walk(po, case)
    bound, dt_gamma, max_steps, C, H = case.march_args
    rays_t = w["nears"].copy()
    alive = np.arange(case.N, dtype=np.int32)
    got_x = [[] for _ in range(case.N)]
    got_d = [[] for _ in range(case.N)]
    have = np.zeros(case.N, np.int64)
    for _ in range(max_steps // n_step + 2):
        if alive.size == 0:
            break
        x, _, dl = po.march_rays(alive.size, n_step, alive, rays_t, case.o, case.d, bound, dt_gamma, max_steps, C, H, case.bits, w["nears"],
                                 w["fars"], np.zeros(alive.size, np.float32))
        x, dl = x.reshape(alive.size, n_step, 3), dl.reshape(alive.size, n_step, 2)
        k = (dl[:, :, 0] > 0).sum(1)
        for j, r in enumerate(alive):
            got_x[r].append(x[j, :k[j]])
            got_d[r].append(dl[j, :k[j]])
        have[alive] += k
        full = k == n_step
        rays_t[alive[full]] = dl[full, -1, 1]
        alive = alive[full & (have[alive] < max_steps)]
    assert alive.size == 0
    counts, offs = w["rays"][:, 2], w["rays"][:, 1]
    assert (have >= counts).all() and np.array_equal(have[counts < max_steps], counts[counts < max_steps])
    gx = np.concatenate([np.concatenate(g)[:c] for g, c in zip(got_x, counts)])
    gd = np.concatenate([np.concatenate(g)[:c] for g, c in zip(got_d, counts)])
    assert np.array_equal(gx, w["xyzs"]) and np.array_equal(gd, w["deltas"])
    assert offs[-1] + counts[-1] == w["total"]


def test_single_pass_rule_agrees_with_the_oracle_off_the_diagonal(po):
    """The comment in Dda::init as a test: for max|d_i| > 0.58 (one cascade, constant dt) leaving an empty cell by ONE t += dt
    gives the oracle's samples, bit for bit -- on all plus_y rays and on the diagonal rays on the shortcut's side of the seam."""
    n = 0
    for name in ("plus_y", "diagonal"):
        case = wc.family(name)
        fast = case.max_abs_d > wc.SEAM
        differs = wc.single_pass_differs(po, case)
        assert not differs[fast].any(), (name, int(differs[fast].sum()))
        n += int(fast.sum())
        print(f"\n[{name}] single-pass == oracle on {int(fast.sum())} shortcut rays; differs on {int(differs[~fast].sum())} of "
              f"{int((~fast).sum())} generic rays")
    assert n >= 8000


def test_needles_are_rays_the_shortcut_would_get_wrong(po):
    case = wc.family("needles", po)
    print(f"\n[needles] {case.N} of {wc.NEEDLE_SEARCH_RAYS} short rays")
    assert case.N >= wc.NEEDLE_FLOOR
    assert wc.single_pass_differs(po, case).all()
    assert (case.max_abs_d <= wc.SEAM).all()            # the device walks them on the generic path
