"""Marching tetrahedra on the Kuhn subdivision in numpy: the reference the mesh-export tests hold csrc/rn_mesh_dev.h and the
kernels of csrc/rn_mesh.hip to.  Written from the contract ("mesh export"), not from the kernel: nothing here is
a table -- the triangles of a case come from the geometry of the tetrahedron, oriented by a cross product.

The contract:
  * lattice [X,Y,Z] in C order; a value is inside iff u > threshold (NaN is outside);
  * every cell is cut into six tetrahedra c0 = v000, c1 = c0 + e_a, c2 = c1 + e_b, c3 = v111, one per permutation (a, b, c) of the
    axes, in lexicographic order of the permutation;
  * the edges of all tetrahedra are of seven kinds, owned by their lower lattice point: EDGE_OFFSETS below, in this order; an owned
    edge whose ends differ carries one vertex p_a + t (p_b - p_a), t = (threshold - u_a) / (u_b - u_a), fp32, lattice units;
    world units are v / (R - 1) * (bmax - bmin) + bmin per axis;
  * local edges of a tetrahedron are numbered LOCAL_EDGES; one or three corners inside: one triangle on the three crossed edges,
    starting with the lowest-numbered one; two inside (i < j) and two outside (k < l): the quad is split along the diagonal from
    edge (i, k) to edge (j, l), both triangles start at edge (i, k), the one with the lower-numbered third edge comes first;
  * (v1 - v0) x (v2 - v0) points from inside to outside;
  * vertices are ordered by owning point in C order, then by edge kind; triangles by cell in C order, then tetrahedron, then
    position in the split.
"""
import itertools

import numpy as np

EDGE_OFFSETS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
PERMUTATIONS = tuple(itertools.permutations(range(3)))
LOCAL_EDGES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def tet_corners(perm):
    """Cube-corner offsets [4][3] of the tetrahedron of a permutation."""
    c = np.zeros((4, 3), np.int64)
    c[1, perm[0]] = 1
    c[2] = c[1]
    c[2, perm[1]] = 1
    c[3] = 1
    return c


def case_triangles(corners, mask):
    """The triangles (local edge numbers) of the tetrahedron `corners` [4,3] whose corner i is inside iff bit i of mask."""
    inside = [i for i in range(4) if mask >> i & 1]
    outside = [i for i in range(4) if not mask >> i & 1]
    if not inside or not outside:
        return []
    edge_no = {e: n for n, e in enumerate(LOCAL_EDGES)}
    no = lambda i, j: edge_no[(min(i, j), max(i, j))]
    if len(inside) == 2:
        (i, j), (k, l) = inside, outside
        first, last = no(i, k), no(j, l)
        tris = [[first, last, third] for third in sorted((no(i, l), no(j, k)))]
    else:
        lone = inside[0] if len(inside) == 1 else outside[0]
        tris = [sorted(no(lone, o) for o in range(4) if o != lone)]
    pts = corners.astype(np.float64)
    mid = {n: (pts[a] + pts[b]) / 2 for n, (a, b) in enumerate(LOCAL_EDGES)}
    outward = pts[outside].mean(0) - pts[inside].mean(0)
    out = []
    for t in tris:
        normal = np.cross(mid[t[1]] - mid[t[0]], mid[t[2]] - mid[t[0]])
        s = float(normal @ outward)
        assert abs(s) > 1e-9
        out.append(t if s > 0 else [t[0], t[2], t[1]])
    return out


def marching_tetrahedra(field, threshold, bound_min=None, bound_max=None):
    """(vertices [V,3] float32, triangles [T,3] int32) of the contract above; lattice units without bounds."""
    u = np.ascontiguousarray(field, np.float32)
    X, Y, Z = u.shape
    thr = np.float32(threshold)
    inside = u > thr
    n_pts = X * Y * Z
    lin = np.arange(n_pts, dtype=np.int64).reshape(X, Y, Z)
    cross = np.zeros((n_pts, 7), bool)
    for e, (dx, dy, dz) in enumerate(EDGE_OFFSETS):
        a = inside[:X - dx, :Y - dy, :Z - dz]
        b = inside[dx:, dy:, dz:]
        cross[lin[:X - dx, :Y - dy, :Z - dz].reshape(-1), e] = (a != b).reshape(-1)
    owner, kind = np.nonzero(cross)                                  # C order: by point, then by edge kind
    weld = {(int(p), int(e)): n for n, (p, e) in enumerate(zip(owner, kind))}
    off = np.asarray(EDGE_OFFSETS, np.int64)[kind]
    pa = np.stack(np.unravel_index(owner, (X, Y, Z)), 1)
    pb = pa + off
    ua = u[pa[:, 0], pa[:, 1], pa[:, 2]]
    ub = u[pb[:, 0], pb[:, 1], pb[:, 2]]
    with np.errstate(all="ignore"):
        t = ((thr - ua) / (ub - ua)).astype(np.float32)
        fa, fb = pa.astype(np.float32), pb.astype(np.float32)
        verts = (fa + (t[:, None] * (fb - fa)).astype(np.float32)).astype(np.float32)
        if bound_min is not None:
            lo, hi = np.asarray(bound_min, np.float32), np.asarray(bound_max, np.float32)
            res = np.asarray([X - 1, Y - 1, Z - 1], np.float32)
            verts = (((verts / res).astype(np.float32) * (hi - lo).astype(np.float32)).astype(np.float32) + lo).astype(np.float32)
    cells = lin[:X - 1, :Y - 1, :Z - 1].reshape(-1)                   # origin point of every cell, in C order of the cells
    kind_of = {o: e for e, o in enumerate(EDGE_OFFSETS)}
    stride = np.asarray([Y * Z, Z, 1], np.int64)
    rows, keys = [], []
    for k, perm in enumerate(PERMUTATIONS):
        corners = tet_corners(perm)
        cin = [inside.reshape(-1)[cells + int(c @ stride)] for c in corners]
        mask = sum(ci.astype(np.int64) << i for i, ci in enumerate(cin))
        for m in range(1, 15):
            sel = np.nonzero(mask == m)[0]
            if not len(sel):
                continue
            for pos, tri in enumerate(case_triangles(corners, m)):
                key = np.empty((len(sel), 3, 2), np.int64)
                for c, e in enumerate(tri):
                    i, j = LOCAL_EDGES[e]
                    key[:, c, 0] = cells[sel] + int(corners[i] @ stride)
                    key[:, c, 1] = kind_of[tuple(int(v) for v in corners[j] - corners[i])]
                rows.append(np.stack([sel, np.full(len(sel), k), np.full(len(sel), pos)], 1))
                keys.append(key)
    if not rows:
        return verts, np.zeros((0, 3), np.int32)
    rows, keys = np.concatenate(rows), np.concatenate(keys)
    order = np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))
    keys = keys[order].reshape(-1, 2)
    tris = np.fromiter((weld[(p, e)] for p, e in keys.tolist()), np.int32, len(keys)).reshape(-1, 3)
    return verts, tris


# ---------------------------------------------------------------------------------------------------------- test helpers
def directed_edges(tris):
    t = np.asarray(tris, np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def edge_use(tris):
    """(undirected edges [E,2], uses [E], balance [E]): how often each undirected edge is used, and uses a->b minus uses b->a."""
    d = directed_edges(tris)
    lo, hi = d.min(1), d.max(1)
    sign = np.where(d[:, 0] < d[:, 1], 1, -1)
    und, inv = np.unique(np.stack([lo, hi], 1), axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    return und, np.bincount(inv, minlength=len(und)), np.bincount(inv, weights=sign, minlength=len(und)).astype(np.int64)


def euler_characteristic(verts, tris):
    return len(verts) - len(edge_use(tris)[0]) + len(tris)


def signed_volume(verts, tris):
    v = np.asarray(verts, np.float64)
    a, b, c = v[tris[:, 0]], v[tris[:, 1]], v[tris[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def sphere_field(R, r=0.6):
    ax = np.linspace(-1, 1, R)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    return (10 + 20 * (r - np.sqrt(x * x + y * y + z * z))).astype(np.float32)


def torus_field(R, major=0.55, minor=0.25):
    """Tube radius 0.25 on a lattice step of 2 / (R - 1): 8 cells across at R = 33."""
    ax = np.linspace(-1, 1, R)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    return (10 + 20 * (minor - np.sqrt((np.sqrt(x * x + y * y) - major) ** 2 + z * z))).astype(np.float32)


def sines_field(shape=(9, 13, 20)):
    x, y, z = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    return (10 + 3 * np.sin(0.9 * x + 0.3) + 2 * np.sin(0.7 * y - 0.2 * z) + 2.5 * np.sin(0.45 * z + 0.5 * x) + np.sin(1.3 * y)).astype(np.float32)


def threshold_field(shape=(11, 12, 10), threshold=10.0, seed=3):
    """Uniform values around the threshold, a tenth of them exactly on it."""
    rng = np.random.default_rng(seed)
    u = rng.uniform(threshold - 4, threshold + 4, shape).astype(np.float32)
    u[rng.uniform(size=shape) < 0.1] = np.float32(threshold)
    return u


def plane_field(shape=(10, 9, 12)):
    x, y, z = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    return (10 + 0.8 * (x - 4.3) + 0.45 * (y - 3.1) - 0.3 * (z - 5.2)).astype(np.float32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
