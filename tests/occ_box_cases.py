"""The occupied box's span (csrc/rn_dda_dev.h: Dda::set_span / walk<true>) restated in numpy float32, every operation rounded on its
own, with the boxes and ray sets tests/test_occ_box.py (CPU) and tests/test_gpu_occ_box.py share.

    box_of(bits, H)                    what rn_occ_box computes: (lo[3], hi[3]) of the set cells of cascade 0; lo = H, hi = -1 when empty
    span(o, d, box, ...)               (use, t_lo, t_hi) per ray: `use` is Dda::span, i.e. the lanes on which the walk is clipped
    cells(o, d, t, H, bound)           cell_of()'s cell of the lattice point at t (one cascade)
    orbit(near, far, ...)              the t values a ray visits: t += clamp(t * dt_gamma, dt_min, dt_max) from near while t < far

numpy only; nothing here needs a device.
"""
import numpy as np

import walk_cases as wc

F = np.float32
FLT_MAX = np.finfo(np.float32).max
ORIGIN_LIMIT = 4096.0                  # set_span: |o_i| <= 4096 mb1


def invert(code):
    """morton3D_invert (raymarching.cu:73-81) of an int64 array."""
    x = code.astype(np.uint32) & np.uint32(0x49249249)
    x = (x | (x >> np.uint32(2))) & np.uint32(0xc30c30c3)
    x = (x | (x >> np.uint32(4))) & np.uint32(0x0f00f00f)
    x = (x | (x >> np.uint32(8))) & np.uint32(0xff0000ff)
    x = (x | (x >> np.uint32(16))) & np.uint32(0x0000ffff)
    return x.astype(np.int64)


def box_of(bits, H):
    """(lo, hi) int32 [3] each over the set bits among the first H^3 (cascade 0), morton order."""
    occ = np.nonzero(np.unpackbits(np.asarray(bits[: H ** 3 // 8], np.uint8), bitorder="little"))[0]
    if occ.size == 0:
        return np.full(3, H, np.int32), np.full(3, -1, np.int32)
    c = np.stack([invert(occ), invert(occ >> 1), invert(occ >> 2)], 1)
    return c.min(0).astype(np.int32), c.max(0).astype(np.int32)


def box_words(bits, H):
    """The 8 int32 words rn_occ_box writes."""
    lo, hi = box_of(bits, H)
    return np.concatenate([lo, hi, np.zeros(2, np.int32)]).astype(np.int32)


def bits_from_cells(cells_xyz, H, C=1):
    """A bitfield of C cascades with exactly the given cells of cascade 0 set."""
    occ = np.zeros(C * H ** 3, bool)
    c = np.asarray(cells_xyz, np.int64).reshape(-1, 3)
    if c.size:
        occ[wc.morton(c)] = True
    return np.packbits(occ, bitorder="little")


def blob_bits(H, centre, semi_axes, bound=1.0, C=1):
    """Cells of cascade 0 whose centre lies in the ellipsoid (radnerf.scene.ellipsoid_bitfield with a centre), C cascades long."""
    idx = np.arange(H)
    c = ((idx + 0.5) / H * 2 - 1) * min(1.0, bound)
    X, Y, Z = np.meshgrid(c, c, c, indexing="ij")
    inside = ((X - centre[0]) / semi_axes[0]) ** 2 + ((Y - centre[1]) / semi_axes[1]) ** 2 + ((Z - centre[2]) / semi_axes[2]) ** 2 <= 1.0
    return bits_from_cells(np.argwhere(inside), H, C)


def one_step_skips(d, C, dt_min, dt_max):
    return (C == 1) & (F(dt_min) == F(dt_max)) & (np.abs(d).max(1) > F(0.58))


def span(o, d, lo, hi, H, bound, C=1, dt_min=None, dt_max=None):
    """Dda::set_span per ray, float32.  Returns (use [N] bool, t_lo [N], t_hi [N]); t_lo / t_hi are meaningful where use."""
    o, d = np.asarray(o, F), np.asarray(d, F)
    N = o.shape[0]
    if dt_max is None:
        dt_max = F(F(F(2) * wc.SQRT3 * F(1 << (C - 1))) / F(H))
    if dt_min is None:
        dt_min = dt_max
    mb1 = F(min(1.0, bound))
    rH = F(1) / F(H)
    use = one_step_skips(d, C, dt_min, dt_max) & (H <= 256)
    use &= np.abs(o).max(1) <= F(F(ORIGIN_LIMIT) * mb1)
    a = np.full(N, -FLT_MAX, F)
    b = np.full(N, FLT_MAX, F)
    with np.errstate(all="ignore"):
        rd = (F(1) / d).astype(F)
        for k in range(3):
            l, h = int(lo[k]), int(hi[k])
            open_lo, open_hi = l <= 0, h >= H - 1
            f_lo = F(F(F(F(l - 1) * rH) * F(2) - F(1)) * mb1)
            f_hi = F(F(F(F(h + 2) * rH) * F(2) - F(1)) * mb1)
            ok, dk = o[:, k], d[:, k]
            still = dk == 0
            out = still & (((not open_lo) & (ok < f_lo)) | ((not open_hi) & (ok > f_hi)))
            a[out], b[out] = FLT_MAX, -FLT_MAX
            t_f_lo = ((f_lo - ok).astype(F) * rd[:, k]).astype(F)
            t_f_hi = ((f_hi - ok).astype(F) * rd[:, k]).astype(F)
            pos, neg = dk > 0, dk < 0
            # fmaxf / fminf: a NaN operand is ignored
            if not open_lo:
                a = np.where(pos, np.fmax(a, t_f_lo), a)
                b = np.where(neg, np.fmin(b, t_f_lo), b)
            if not open_hi:
                b = np.where(pos, np.fmin(b, t_f_hi), b)
                a = np.where(neg, np.fmax(a, t_f_hi), a)
        use &= (np.abs(a) <= FLT_MAX) & (np.abs(b) <= FLT_MAX)
    return use, a.astype(F), b.astype(F)


def cells(o, d, t, H, bound):
    """cell_of() with one cascade: [N, 3] int64."""
    mb1 = F(min(1.0, bound))
    rmb1 = F(1) / mb1
    with np.errstate(all="ignore"):
        p = np.clip((o + (t[:, None] * d).astype(F)).astype(F), F(-bound), F(bound)).astype(F)
        v = (((p * rmb1).astype(F) + F(1)).astype(F) * F(0.5 * H)).astype(F)
    return np.clip(v, F(0), F(H - 1)).astype(np.int64)


def orbit(near, far, dt_gamma, dt_min, dt_max, limit=4096):
    """Yields (idx, t): the rays still walking and their t, lattice point by lattice point."""
    with np.errstate(invalid="ignore"):
        idx = np.nonzero(near < far)[0]
        t = near[idx].astype(F)
        far = far[idx]
        for _ in range(limit):
            if not idx.size:
                return
            yield idx, t
            dt = np.clip((t * F(dt_gamma)).astype(F), F(dt_min), F(dt_max)).astype(F)
            t = (t + dt).astype(F)
            keep = t < far
            idx, t, far = idx[keep], t[keep], far[keep]
    raise AssertionError("orbit: a ray did not end")


# ---------------------------------------------------------------------------------------------------------------- boxes and rays

def boxes(H):
    """name -> (lo, hi): small, border-touching, full, empty, single corner cells, the synthetic head's."""
    e = (H * 3) // 10                   # the ellipsoid 0.40 / 0.42 / 0.40 in cells from the centre, roughly
    return {
        "small": ((H // 2 - 3, H // 2 - 2, H // 2), (H // 2, H // 2 - 2, H // 2 + 7)),
        "head": ((H // 2 - e, H // 2 - e - 1, H // 2 - e), (H // 2 + e - 1, H // 2 + e, H // 2 + e - 1)),
        "face_lo": ((0, H // 3, H // 3), (H // 4, H // 2, H // 2)),
        "face_hi": ((H // 3, H // 2, H // 3), (H // 2, H - 1, H // 2)),
        "edge": ((0, 0, H // 3), (H // 5, H // 6, H // 2)),
        "full": ((0, 0, 0), (H - 1, H - 1, H - 1)),
        "empty": ((H, H, H), (-1, -1, -1)),
        "cell_0": ((0, 0, 0), (0, 0, 0)),
        "cell_top": ((H - 1, H - 1, H - 1), (H - 1, H - 1, H - 1)),
        "next_to_border": ((1, 1, 1), (H - 2, H - 2, H - 2)),
    }


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


def special_rays(lo, hi, H, bound, seed, n=1500):
    """Rays aimed at what a slab test gets wrong first: axis-parallel rays (exact zeros in d, on both sides of every face and ON the
    grown faces), rays from inside the box, rays through the edges and corners of the box and of the grown box, random rays."""
    rng = np.random.default_rng(seed)
    mb1 = min(1.0, bound)
    face = lambda c: (np.asarray(c, np.float64) / H * 2 - 1) * mb1
    lo_c, hi_c = np.clip(np.asarray(lo), 0, H - 1), np.clip(np.asarray(hi), -1, H - 1)
    corners_true = np.stack([face(lo_c), face(hi_c + 1)])                 # [2, 3]
    corners_grown = np.stack([face(lo_c - 1), face(hi_c + 2)])
    O, D = [], []

    def add(o, d):
        O.append(np.asarray(o, F).reshape(-1, 3))
        D.append(np.asarray(d, F).reshape(-1, 3))

    # random rays from outside and from inside the cube
    o = rng.uniform(-3 * bound, 3 * bound, (n, 3))
    add(o, _unit(rng.uniform(-bound, bound, (n, 3)) - o))
    o = rng.uniform(-bound, bound, (n, 3))
    add(o, _unit(rng.standard_normal((n, 3))))
    # from inside the box
    o = rng.uniform(0, 1, (n, 3)) * (corners_true[1] - corners_true[0]) + corners_true[0]
    add(o, _unit(rng.standard_normal((n, 3))))
    # through corners and edge points of the box and of the grown box
    for corners in (corners_true, corners_grown):
        pick = rng.integers(0, 2, (n, 3))
        target = corners[pick, np.arange(3)]
        along = rng.integers(0, 3, n)                                      # half of them: a point ON an edge, not the corner
        on_edge = rng.uniform(0, 1, n) < 0.5
        edge_val = corners[0, along] + rng.uniform(0, 1, n) * (corners[1, along] - corners[0, along])
        target[np.arange(n), along] = np.where(on_edge, edge_val, target[np.arange(n), along])
        o = rng.uniform(-3 * bound, 3 * bound, (n, 3))
        add(o, _unit(target - o))
    # axis-parallel: exact zeros on two axes, the origin on a face value or beside it
    vals = np.concatenate([corners_true.reshape(-1), corners_grown.reshape(-1), [0.0, -bound, bound]])
    vals = np.concatenate([vals, np.nextafter(vals.astype(F), F(9)), np.nextafter(vals.astype(F), F(-9))])
    for axis in range(3):
        for sign in (1.0, -1.0):
            m = 200
            o = rng.choice(vals, (m, 3))
            o[:, axis] = -sign * rng.uniform(1.5, 3.0, m) * bound
            d = np.zeros((m, 3))
            d[:, axis] = sign
            d[::2, (axis + 1) % 3] = -0.0
            add(o, d)
    # one exact zero, tiny components
    o = rng.uniform(-3 * bound, 3 * bound, (n, 3))
    d = _unit(rng.uniform(-bound, bound, (n, 3)) - o).astype(np.float64)
    d[np.arange(n), rng.integers(0, 3, n)] = rng.choice([0.0, -0.0, 1e-30, -1e-30, 1e-42, 1e-7], n)
    add(o, d)
    return np.concatenate(O), np.concatenate(D)
