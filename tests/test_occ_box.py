"""The occupied box's span on the CPU: numpy float32 restatement (tests/occ_box_cases.py) of Dda::set_span and of cell_of()'s cell.

The property the clipped walk (Dda::walk<true>) rests on: on a ray that uses the span, EVERY lattice point the ray visits with
t < t_lo or t >= t_hi has its cell outside the box -- so not testing it loses no sample.  Checked lattice point by lattice point, on
every ray family of tests/walk_cases.py and on rays built to meet the slab test's weak spots (exact zeros in d, origins on and beside
the faces, rays through edges and corners, origins inside the box), against small, border-touching, full and empty boxes.  No ray and
no lattice point is left out; families the span does not apply to (more than one cascade, variable dt, max|d_i| <= 0.58) must report
`use` false on every ray.
"""
import numpy as np
import pytest

import occ_box_cases as ob
import walk_cases as wc

F = np.float32


def _check(o, d, near, far, lo, hi, H, bound, C, dt_gamma, dt_min, dt_max):
    """Walks every ray's orbit; returns (rays that use the span, lattice points outside the span on those rays, all lattice points)."""
    lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    use, t_lo, t_hi = ob.span(o, d, lo, hi, H, bound, C, dt_min, dt_max)
    if C > 1 or F(dt_min) != F(dt_max):
        assert not use.any()
        return 0, 0, 0
    assert not (use & ~(np.abs(d).max(1) > F(0.58))).any()
    assert np.isfinite(t_lo[use]).all() and np.isfinite(t_hi[use]).all()
    skipped = total = 0
    for idx, t in ob.orbit(near, far, dt_gamma, dt_min, dt_max):
        out = use[idx] & ((t < t_lo[idx]) | (t >= t_hi[idx]))
        c = ob.cells(o[idx], d[idx], t, H, bound)
        in_box = ((c >= lo) & (c <= hi)).all(1)
        wrong = out & in_box
        assert not wrong.any(), (idx[wrong][:5], t[wrong][:5], c[wrong][:5], t_lo[idx][wrong][:5], t_hi[idx][wrong][:5])
        skipped += int(out.sum())
        total += int(use[idx].sum())
    return int(use.sum()), skipped, total


@pytest.mark.parametrize("box", sorted(ob.boxes(128)))
@pytest.mark.parametrize("name", wc.FAMILIES)
def test_no_lattice_point_outside_the_span_is_in_the_box(po, name, box):
    case = wc.family(name, po)
    lo, hi = ob.boxes(case.H)[box]
    near, far = po.near_far_from_aabb(case.o, case.d, case.aabb, wc.MIN_NEAR)
    used, skipped, total = _check(case.o, case.d, near, far, lo, hi, case.H, case.bound, case.C, case.dt_gamma, case.dt_min, case.dt_max)
    if name in ("plus_y", "diagonal"):
        # every ray of plus_y has max|d_i| > 0.58; the diagonal family straddles the seam
        assert used >= (case.N if name == "plus_y" else 30)
        if box == "head" and name == "plus_y":
            # the camera looks along -y through a box 0.84 + 2 cells deep in a 2.0 deep cube: more than half of the points lie outside
            assert skipped > 0.5 * total, (skipped, total)
        if box == "full":
            assert skipped == 0
        if box == "empty":
            assert skipped == total
    if name in ("short", "needles", "vardt_c1", "casc2", "casc3", "casc3_rec"):
        assert used == 0


@pytest.mark.parametrize("H,bound", [(128, 1.0), (64, 1.0), (128, 2.0), (256, 0.5)])
@pytest.mark.parametrize("box", sorted(ob.boxes(128)))
def test_rays_aimed_at_faces_edges_corners_and_zeros(po, box, H, bound):
    lo, hi = ob.boxes(H)[box]
    o, d = ob.special_rays(lo, hi, H, bound, seed=H + len(box))
    aabb = np.array([-bound] * 3 + [bound] * 3, F)
    near, far = po.near_far_from_aabb(o, d, aabb, wc.MIN_NEAR)
    dt = F(F(F(2) * wc.SQRT3) / F(H))
    used, skipped, total = _check(o, d, near, far, lo, hi, H, bound, 1, 1 / 256, dt, dt)
    assert used > o.shape[0] // 2
    # the walk may start anywhere on a ray (rays_t of a later iteration): the same from a third of the way in
    with np.errstate(invalid="ignore", over="ignore"):
        later = (near + (far - near) * F(0.37)).astype(F)
    _check(o, d, later, far, lo, hi, H, bound, 1, 1 / 256, dt, dt)


def test_a_far_origin_and_an_overflowing_span_keep_the_full_walk():
    lo, hi = ob.boxes(128)["head"]
    o = np.array([[5000.0, 0, 0], [0, 0, 3], [0, 0, 3], [4096.0, 0, 0]], F)
    d = np.array([[-1, 0, 0], [1e-38, 0, -1], [0, 0, -1], [-1, 0, 0]], F)
    use, t_lo, t_hi = ob.span(o, d, lo, hi, 128, 1.0)
    assert use.tolist() == [False, True, True, True]


def test_box_of_restates_the_morton_order():
    H = 16
    cells = np.array([[3, 0, 15], [7, 9, 2], [5, 5, 5]])
    lo, hi = ob.box_of(ob.bits_from_cells(cells, H), H)
    assert lo.tolist() == [3, 0, 2] and hi.tolist() == [7, 9, 15]
    lo, hi = ob.box_of(np.zeros(H ** 3 // 8, np.uint8), H)
    assert lo.tolist() == [H] * 3 and hi.tolist() == [-1] * 3
    from radnerf.scene import ellipsoid_bitfield
    lo, hi = ob.box_of(ellipsoid_bitfield(128, 1.0, (0.40, 0.42, 0.40))[0], 128)
    # cell centres (i + 0.5) / 64 - 1 within 0.40 / 0.42 / 0.40 of the centre
    assert lo.tolist() == [38, 37, 38] and hi.tolist() == [89, 90, 89]
