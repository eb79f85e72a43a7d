"""Ray families for the occupancy-grid walk (csrc/rn_dda_dev.h: Dda::walk), one per combination of its data-dependent branches,
with the numpy quantities their preconditions are stated in.  tests/test_walk_cases.py asserts the preconditions against the
CPU oracle; tests/test_gpu_walk.py runs every marcher on the same rays.

The walk's branches ("The walk's four branches"):
  one_cascade      C == 1 and H <= 256: hoisted constants, level 0
  one_step_skips   C == 1, dt_min == dt_max and max|d_i| > 0.58: an empty cell is left by ONE t += dt; otherwise the cell-exit
                   time tt and the do .. while (t < tt) loop
  dt               clamp(t * dt_gamma, dt_min, dt_max): a constant whenever max_steps <= H / 2^(C-1)
  mip level        max(level from the position, level from dt) when C > 1

numpy only: nothing here needs a device or reads a file.  Functions that need the oracle take the `pyoracle` module as an argument.
"""
import numpy as np

MIN_NEAR = 0.05
SEAM = 0.58                                   # Dda::init: one_step_skips needs max|d_i| > 0.58f
CAM_PLUS_Y = (0.05, 3.3, -0.1)                # the camera of tests/test_gpu_ops.py::make_rays
SQRT3 = np.float32(1.7320508075688772)

DEGENERATE_O = [(0, 3, 0), (0, 0, 0), (1, 3, 0), (0.5, 0.5, 3), (0, 3, 0), (1, 0, 0)]
DEGENERATE_D = [(0, -1, 0), (0, 0, 1), (0, -1, 0), (0, 0, -1), (1, 0, 0), (-1, 0, 0)]
FLT_MAX = np.finfo(np.float32).max
DEGENERATE_NEARS = np.array([2, 0.05, 2, 2, FLT_MAX, 0.05], np.float32)
DEGENERATE_FARS = np.array([4, 1, np.nan, 4, FLT_MAX, 2], np.float32)
DEGENERATE_COUNTS = [16, 14, 0, 0, 0, 16]

NEEDLE_SEARCH_RAYS = 500000
NEEDLE_FLOOR = 4

FAMILIES = ("plus_y", "diagonal", "short", "needles", "vardt_c1", "casc2", "casc3", "casc3_rec", "degenerate")


def look(cam, targets):
    """Unit directions (float32) from `cam` to every row of `targets`."""
    d = np.asarray(targets, np.float32) - np.asarray(cam, np.float32)
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def _targets(seed, N, half):
    return np.random.default_rng(seed).uniform(-half, half, (N, 3)).astype(np.float32)


def _from(cam, d):
    return np.tile(np.asarray([cam], np.float32), (d.shape[0], 1)), np.ascontiguousarray(d, dtype=np.float32)


_BITS = {}


def bits_of(kind, C, H):
    """"ellipsoid": the synthetic head (C = 1, H = 128).  ("random", k): k independent uint8 draws ANDed together over
    C * H^3 / 8 bytes -- about 2^-k of the cells set."""
    key = (kind, C, H)
    if key not in _BITS:
        if kind == "ellipsoid":
            assert C == 1 and H == 128
            from radnerf.scene import ellipsoid_bitfield
            _BITS[key] = ellipsoid_bitfield(128, 1.0, (0.40, 0.42, 0.40))[0]
        else:
            rng = np.random.default_rng(1000 + 10 * C + kind[1])
            b = rng.integers(0, 256, C * H ** 3 // 8).astype(np.uint8)
            for _ in range(kind[1] - 1):
                b &= rng.integers(0, 256, C * H ** 3 // 8).astype(np.uint8)
            _BITS[key] = b
    return _BITS[key]


class Case:
    """One family: rays + walk parameters.  The box is the cube [-bound, bound]^3."""

    def __init__(self, name, o, d, bound=1.0, C=1, H=128, max_steps=16, dt_gamma=1 / 256, bits=("ellipsoid",)):
        self.name, self.o, self.d = name, o, d
        self.bound, self.C, self.H, self.max_steps, self.dt_gamma = float(bound), C, H, max_steps, dt_gamma
        self.bits_kind = bits if len(bits) > 1 else bits[0]
        self.N = o.shape[0]
        self.aabb = np.array([-bound] * 3 + [bound] * 3, np.float32)
        # Dda::init / raymarching.cu:386-387, in float32 as written there
        self.dt_max = np.float32(np.float32(np.float32(2) * SQRT3 * np.float32(1 << (C - 1))) / np.float32(H))
        self.dt_min = np.float32(min(self.dt_max, np.float32(np.float32(2) * SQRT3) / np.float32(max_steps)))

    @property
    def bits(self):
        return bits_of(self.bits_kind, self.C, self.H)

    @property
    def max_abs_d(self):
        return np.abs(self.d).max(1)

    @property
    def march_args(self):
        """(bound, dt_gamma, max_steps, C, H) in the order every marcher takes them."""
        return self.bound, self.dt_gamma, self.max_steps, self.C, self.H


def _plus_y(seed, N):
    return _from(CAM_PLUS_Y, look(CAM_PLUS_Y, _targets(seed, N, 0.7)))


def _diagonal(seed, N):
    return _from((1.9, 1.9, 1.9), look((1.9, 1.9, 1.9), _targets(seed, N, 0.12)))


def _short(seed, N):
    return _from(CAM_PLUS_Y, look(CAM_PLUS_Y, _targets(seed, N, 0.9)) * np.float32(0.25))


_CASES = {}
_NEEDLES = {}


def family(name, po=None):
    """The named family.  "needles" is found by search against the oracle and needs `po` the first time."""
    if name in _CASES:
        return _CASES[name]
    rnd2 = dict(bits=("random", 2))
    if name == "plus_y":
        c = Case(name, *_plus_y(11, 4096))
    elif name == "diagonal":
        c = Case(name, *_diagonal(12, 4096))
    elif name == "short":
        c = Case(name, *_short(13, 4096), **rnd2)
    elif name == "needles":
        o, d = find_needles(po)
        c = Case(name, o, d, **rnd2)
    elif name == "vardt_c1":
        (o1, d1), (o2, d2) = _plus_y(14, 1024), _diagonal(15, 1024)
        c = Case(name, np.concatenate([o1, o2]), np.concatenate([d1, d2]), max_steps=1024)
    elif name == "casc2":
        cam = (0.1, 4.5, -0.2)
        c = Case(name, *_from(cam, look(cam, _targets(16, 1024, 1.5))), bound=2.0, C=2, H=128, max_steps=1024, bits=("random", 3))
    elif name == "casc3":
        cam = (4.4, 4.5, 4.6)
        c = Case(name, *_from(cam, look(cam, _targets(17, 1024, 1.0))), bound=4.0, C=3, H=64, max_steps=512, bits=("random", 3))
    elif name == "casc3_rec":
        cam = (3, 6, -5)
        c = Case(name, *_from(cam, look(cam, _targets(18, 1024, 3.0))), bound=4.0, C=3, H=64, max_steps=32, dt_gamma=1 / 64,
                 bits=("random", 3))
    elif name == "degenerate":
        c = Case(name, np.array(DEGENERATE_O, np.float32), np.array(DEGENERATE_D, np.float32))
    else:
        raise KeyError(name)
    _CASES[name] = c
    return c


# ---------------------------------------------------------------------------------------------- the oracle's walk of a family

_WALKS = {}


def oracle_walk(po, case, noises=None):
    """dict(nears, fars, xyzs, dirs, deltas, rays, counter, total) of the oracle's training marcher over the whole family with
    room for every sample; noises None = no jitter (cached: the arrays are shared, do not write to them)."""
    key = case.name if noises is None else None
    if key in _WALKS:
        return _WALKS[key]
    nears, fars = po.near_far_from_aabb(case.o, case.d, case.aabb, MIN_NEAR)
    nz = np.zeros(case.N, np.float32) if noises is None else noises
    M = case.N * case.max_steps
    bound, dt_gamma, max_steps, C, H = case.march_args
    xyzs, dirs, deltas, rays, cnt = po.march_rays_train(case.o, case.d, case.bits, bound, dt_gamma, max_steps, C, H, M, nears, fars, nz)
    total = int(cnt[0])
    w = dict(nears=nears, fars=fars, xyzs=xyzs[:total], dirs=dirs[:total], deltas=deltas[:total], rays=rays, counter=cnt, total=total)
    if key is not None:
        _WALKS[key] = w
    return w


# ---------------------------------------------------------------------------------------------- numpy quantities of the table

def levels(case, xyz, dt):
    """(lp, ld): the mip level from a sample's position and from its dt (raymarching.cu:42-54), recomputed in numpy."""
    top = case.C - 1
    lp = np.clip(np.frexp(np.abs(xyz).max(1))[1], 0, top)
    mx = ((dt.astype(np.float32) * np.float32(case.H)).astype(np.float64) * 0.5).astype(np.float32)
    ld = np.clip(np.frexp(mx)[1], 0, top)
    return lp.astype(np.int64), ld.astype(np.int64)


def interior(case, dt):
    """dt strictly inside the clamp."""
    return (dt > case.dt_min * 1.0001) & (dt < case.dt_max * 0.9999)


def morton(c):
    def part(v):
        v = v.astype(np.uint32)
        v = (v * np.uint32(0x00010001)) & np.uint32(0xFF0000FF)
        v = (v * np.uint32(0x00000101)) & np.uint32(0x0F00F00F)
        v = (v * np.uint32(0x00000011)) & np.uint32(0xC30C30C3)
        v = (v * np.uint32(0x00000005)) & np.uint32(0x49249249)
        return v
    return (part(c[:, 0]) | (part(c[:, 1]) << np.uint32(1)) | (part(c[:, 2]) << np.uint32(2))).astype(np.int64)


def occupied(case, xyz, level):
    """The occupancy bit of every sample's cell at `level`, the cell recomputed in float64 from xyz (raymarching.cu:404-419)."""
    mip_bound = np.minimum(np.exp2(level.astype(np.float64)), case.bound)
    v = (0.5 * (xyz.astype(np.float64) / mip_bound[:, None] + 1) * case.H).astype(np.float32)
    cell = np.clip(v, 0, case.H - 1).astype(np.int64)
    index = level * case.H ** 3 + morton(cell)
    return np.unpackbits(case.bits, bitorder="little")[index].astype(bool)


# ---------------------------------------------------------------------------------------------- the single-pass rule, in numpy

def single_pass_walk(case, nears, fars):
    """The walk with the shortcut taken on EVERY ray (one cascade, constant dt): on each lattice point p = clip(o + t d), the cell
    (int)clip((p + 1) * 0.5 H, 0, H - 1), its morton bit; a hit records the sample and counts a step; t += dt either way; the ray
    ends at t >= far or after max_steps samples.  float32 throughout, every operation rounded on its own.
    Returns (counts [N], xyz [N, max_steps, 3] zero-padded)."""
    assert case.C == 1 and case.bound == 1.0 and case.dt_min == case.dt_max
    N, S, H = case.N, case.max_steps, case.H
    occ = np.unpackbits(case.bits, bitorder="little").astype(bool)
    dt = case.dt_max
    half_h, top = np.float32(0.5 * H), np.float32(H - 1)
    counts = np.zeros(N, np.int64)
    out = np.zeros((N, S, 3), np.float32)
    with np.errstate(invalid="ignore"):
        idx = np.nonzero(nears < fars)[0]            # t < far is false for NaN / equal ends
        t = nears[idx].astype(np.float32)
        o, d, far = case.o[idx], case.d[idx], fars[idx]
        while idx.size:
            p = np.clip(o + t[:, None] * d, np.float32(-1), np.float32(1)).astype(np.float32)
            cell = np.clip((p + np.float32(1)) * half_h, np.float32(0), top).astype(np.int64)
            hit = occ[morton(cell)]
            h = np.nonzero(hit)[0]
            out[idx[h], counts[idx[h]]] = p[h]
            counts[idx[h]] += 1
            t = (t + dt).astype(np.float32)
            keep = (t < far) & (counts[idx] < S)
            idx, t, o, d, far = idx[keep], t[keep], o[keep], d[keep], far[keep]
    return counts, out


def single_pass_differs(po, case):
    """Per ray: does the single-pass walk give another sample count or another sample position than the oracle?"""
    nears, fars = po.near_far_from_aabb(case.o, case.d, case.aabb, MIN_NEAR)
    counts, xyz = single_pass_walk(case, nears, fars)
    bound, dt_gamma, max_steps, C, H = case.march_args
    ex, _, edl = po.march_rays(case.N, max_steps, np.arange(case.N, dtype=np.int32), nears, case.o, case.d, bound, dt_gamma, max_steps, C, H,
                               case.bits, nears, fars, np.zeros(case.N, np.float32))
    ecounts = (edl[:, 0].reshape(case.N, max_steps) > 0).sum(1)
    return (ecounts != counts) | (ex.reshape(case.N, max_steps, 3) != xyz).any((1, 2))


def find_needles(po):
    """Rays on which the shortcut would be WRONG: `short`-style rays (generic path on the device) whose single-pass walk differs
    from the oracle's.  With a constant dt both visit the same lattice of t; they part only where the rounded cell-exit time
    disagrees with cell membership at a cell boundary.  Deterministic; run once per session."""
    if "rays" not in _NEEDLES:
        if po is None:
            raise RuntimeError("the needles family is found against the oracle: pass pyoracle the first time")
        probe = Case("needle_search", *_short(19, NEEDLE_SEARCH_RAYS), bits=("random", 2))
        bad = single_pass_differs(po, probe)
        _NEEDLES["rays"] = (np.ascontiguousarray(probe.o[bad]), np.ascontiguousarray(probe.d[bad]))
    return _NEEDLES["rays"]
