"""Mesh export without a GPU (rad-nerf_amd/radnerf/mesh.py, csrc/rn_mesh.hip, csrc/rn_mesh_dev.h):
  * the numpy reference of tests/mesh_reference.py on analytic solids -- closed, oriented, the right genus, the right volume;
  * csrc/rn_mesh_dev.h built into a stand-alone host program against that reference: the same triangle array, bit-equal vertices;
  * the case table through rn_mesh_tet_case; the argument checks of the entry points; the PLY writer."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import mesh_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rad-nerf_amd", "csrc")
RN_ERR_INVALID_ARG = -1

# argv: X Y Z threshold world(0/1) field.bin vertices.bin triangles.bin; world: the box [-1, 1] x [-0.5, 2] x [0.25, 0.75]
PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "rn_mesh_dev.h"
using namespace rn::mesh;
int main(int argc, char **argv) {
    if (argc != 9) return 2;
    const uint32_t X = atoi(argv[1]), Y = atoi(argv[2]), Z = atoi(argv[3]);
    const float threshold = (float)atof(argv[4]);
    const bool world = atoi(argv[5]) != 0;
    const float lo[3] = {-1.0f, -0.5f, 0.25f}, hi[3] = {1.0f, 2.0f, 0.75f};
    const uint32_t N = X * Y * Z, R[3] = {X, Y, Z};
    std::vector<float> u(N);
    FILE *f = fopen(argv[6], "rb");
    if (!f || fread(u.data(), 4, N, f) != N) return 3;
    fclose(f);
    auto at = [&](uint32_t x, uint32_t y, uint32_t z) { return (x * Y + y) * Z + z; };
    auto corner = [&](uint32_t i, uint32_t q) { return i + (q & 1u) * Y * Z + ((q >> 1) & 1u) * Z + (q >> 2); };
    std::vector<uint32_t> code(N), base(N);
    uint32_t n_vert = 0;
    for (uint32_t x = 0; x < X; x++)
        for (uint32_t y = 0; y < Y; y++)
            for (uint32_t z = 0; z < Z; z++) {
                uint32_t in_bits = 0;
                for (uint32_t q = 0; q < 8; q++) {
                    const uint32_t cx = x + (q & 1u), cy = y + ((q >> 1) & 1u), cz = z + (q >> 2);
                    if (cx < X && cy < Y && cz < Z && inside(u[at(cx, cy, cz)], threshold)) in_bits |= 1u << q;
                }
                const uint32_t i = at(x, y, z);
                code[i] = point_code(in_bits, x + 1 < X, y + 1 < Y, z + 1 < Z);
                base[i] = n_vert;
                n_vert += popcount7(code[i]);
            }
    std::vector<float> verts;
    std::vector<int32_t> tris;
    for (uint32_t x = 0; x < X; x++)
        for (uint32_t y = 0; y < Y; y++)
            for (uint32_t z = 0; z < Z; z++) {
                const uint32_t i = at(x, y, z), p[3] = {x, y, z};
                for (uint32_t e = 0; e < kEdgeKinds; e++) {
                    if (!((code[i] >> e) & 1u)) continue;
                    float v[3];
                    edge_vertex(p, e, u[i], u[corner(i, edge_offset(e))], threshold, v);
                    if (verts.size() != 3 * (size_t)(base[i] + vertex_slot(code[i], e))) return 4;
                    for (int a = 0; a < 3; a++) verts.push_back(world ? to_world(v[a], R[a], lo[a], hi[a]) : v[a]);
                }
                if (!(x + 1 < X && y + 1 < Y && z + 1 < Z)) continue;
                const uint32_t in_bits = cell_inside_bits(code[i]);
                uint32_t n_here = 0;
                for (uint32_t k = 0; k < kTets; k++) {
                    uint32_t tri[2][3];
                    const uint32_t n = tet_case(tet_mask(in_bits, k), tet_is_odd(k), tri);
                    if (n != tet_triangle_count(tet_mask(in_bits, k))) return 5;
                    n_here += n;
                    for (uint32_t t = 0; t < n; t++)
                        for (int a = 0; a < 3; a++) {
                            uint32_t q, kind;
                            tet_edge(k, tri[t][a], q, kind);
                            const uint32_t j = corner(i, q);
                            if (!((code[j] >> kind) & 1u)) return 6;
                            tris.push_back((int32_t)(base[j] + vertex_slot(code[j], kind)));
                        }
                }
                if (n_here != cell_triangle_count(code[i])) return 7;
            }
    if (verts.size() != 3 * (size_t)n_vert) return 8;
    f = fopen(argv[7], "wb");
    fwrite(verts.data(), 4, verts.size(), f);
    fclose(f);
    f = fopen(argv[8], "wb");
    fwrite(tris.data(), 4, tris.size(), f);
    fclose(f);
    return 0;
}
"""
BOX = ([-1.0, -0.5, 0.25], [1.0, 2.0, 0.75])


@pytest.fixture(scope="module")
def sphere():
    """The issue's sphere: u = 10 + 20 (r - |x|), r = 0.6, 33^3 over [-1, 1]^3, threshold 10 -- computed once."""
    return ref.marching_tetrahedra(ref.sphere_field(33), 10.0, [-1, -1, -1], [1, 1, 1])


def test_reference_sphere_is_closed_oriented_and_of_the_right_size(sphere):
    verts, tris = sphere
    _, uses, balance = ref.edge_use(tris)
    assert len(tris) > 1000 and tris.min() == 0 and tris.max() == len(verts) - 1
    assert (uses == 2).all() and (balance == 0).all()          # every edge in exactly two triangles, once in each direction
    assert ref.euler_characteristic(verts, tris) == 2
    # every vertex lies on a tetrahedron edge of length <= h sqrt(3) that crosses the sphere
    r, h = 0.6, 2 / 32
    vol = ref.signed_volume(verts, tris)
    print(f"sphere: V {len(verts)} T {len(tris)} volume {vol:.6f} (ball {4 / 3 * np.pi * r ** 3:.6f})")
    assert 4 / 3 * np.pi * (r - h * np.sqrt(3)) ** 3 < vol < 4 / 3 * np.pi * (r + h * np.sqrt(3)) ** 3
    dist = np.linalg.norm(verts.astype(np.float64), axis=1)
    assert np.abs(dist - r).max() <= h * np.sqrt(3)


def test_reference_torus_has_genus_one():
    """Tube radius 0.25 = 4 lattice steps of 2 / 32: the tube is 8 cells thick, the hole 2 (0.55 - 0.25) = 9.6 cells wide."""
    verts, tris = ref.marching_tetrahedra(ref.torus_field(33), 10.0)
    _, uses, balance = ref.edge_use(tris)
    assert (uses == 2).all() and (balance == 0).all()
    assert ref.euler_characteristic(verts, tris) == 0
    assert ref.signed_volume(verts, tris) > 0


def test_reference_plane_is_open_along_the_lattice_boundary():
    field = ref.plane_field()
    verts, tris = ref.marching_tetrahedra(field, 10.0)
    und, uses, _ = ref.edge_use(tris)
    assert set(np.unique(uses)) == {1, 2}
    on_face = ((verts == 0) | (verts == np.asarray(field.shape, np.float32) - 1)).any(1)
    assert on_face[und[uses == 1]].all()
    assert ref.euler_characteristic(verts, tris) == 1                                     # a disc


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """csrc/rn_mesh_dev.h compiled for the host (RN_MESH_CXXFLAGS adds flags, e.g. a sanitizer's) around the serial loops above."""
    d = tmp_path_factory.mktemp("mesh_host")
    cxx = shutil.which("g++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src, exe = d / "mesh.cpp", d / "mesh"
    src.write_text(PROGRAM)
    flags = os.environ.get("RN_MESH_CXXFLAGS", "").split()
    subprocess.run([cxx, "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-I", CSRC] + flags + ["-o", str(exe), str(src)], check=True)

    def run(field, threshold, world):
        field = np.ascontiguousarray(field, np.float32)
        field.tofile(d / "field.bin")
        r = subprocess.run([str(exe)] + [str(n) for n in field.shape] + [repr(float(threshold)), str(int(world)), str(d / "field.bin"),
                                                                          str(d / "v.bin"), str(d / "t.bin")], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        return np.fromfile(d / "v.bin", np.float32).reshape(-1, 3), np.fromfile(d / "t.bin", np.int32).reshape(-1, 3)
    return run


@pytest.mark.parametrize("name", ["sphere", "sines", "threshold"])
@pytest.mark.parametrize("world", [False, True])
def test_host_program_equals_the_reference(host_program, name, world):
    field = {"sphere": lambda: ref.sphere_field(33), "sines": ref.sines_field, "threshold": ref.threshold_field}[name]()
    if name == "threshold":
        assert 0.05 < (field == np.float32(10.0)).mean() < 0.15
    verts, tris = host_program(field, 10.0, world)
    want_v, want_t = ref.marching_tetrahedra(field, 10.0, *(BOX if world else (None, None)))
    assert len(want_t) > 500
    assert np.array_equal(tris, want_t)
    assert ref.same_bits(verts, want_v)


LINSPACE_PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "rn_mesh_dev.h"
// argv: lo hi R as the bits of two floats and a count; stdout: the bits of the R elements
int main(int argc, char **argv) {
    if (argc != 4) return 2;
    const uint32_t lo_bits = (uint32_t)strtoul(argv[1], 0, 10), hi_bits = (uint32_t)strtoul(argv[2], 0, 10), R = atoi(argv[3]);
    float lo, hi;
    memcpy(&lo, &lo_bits, 4);
    memcpy(&hi, &hi_bits, 4);
    const float step = rn::mesh::linspace_step(lo, hi, R);
    for (uint32_t i = 0; i < R; i++) {
        const float v = rn::mesh::linspace_at(lo, hi, step, i, R);
        uint32_t bits;
        memcpy(&bits, &v, 4);
        printf("%u\n", bits);
    }
    return 0;
}
"""


def test_lattice_axis_is_torch_linspace_bit_for_bit(tmp_path):
    """linspace_at of csrc/rn_mesh_dev.h, built for the host, against torch.linspace on the CPU for odd and even counts."""
    import torch
    cxx = shutil.which("g++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src, exe = tmp_path / "lin.cpp", tmp_path / "lin"
    src.write_text(LINSPACE_PROGRAM)
    flags = os.environ.get("RN_MESH_CXXFLAGS", "").split()
    subprocess.run([cxx, "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-I", CSRC] + flags + ["-o", str(exe), str(src), "-lm"], check=True)
    for lo, hi in ((-1.0, 1.0), (-0.7, 0.9), (-1.0, 0.33), (0.1, 2.3), (-0.5, 0.5)):
        for R in (2, 3, 7, 24, 33, 128, 256, 257):
            want = torch.linspace(lo, hi, R).numpy()
            bits = [str(int(np.float32(v).view(np.uint32))) for v in (lo, hi)]
            r = subprocess.run([str(exe)] + bits + [str(R)], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr[-2000:]
            got = np.array([int(v) for v in r.stdout.split()], np.uint32)
            assert np.array_equal(got, want.view(np.uint32)), (lo, hi, R)


def _case(lib, mask):
    n, edges = C.c_int32(-1), (C.c_int32 * 6)(*([-1] * 6))
    assert lib.rn_mesh_tet_case(mask, C.byref(n), edges) == 0
    return [tuple(edges[3 * t:3 * t + 3]) for t in range(n.value)]


def test_tet_case_table(hiplib):
    lib = hiplib._lib
    assert _case(lib, 0) == [] and _case(lib, 15) == []
    corners = ref.tet_corners((0, 1, 2))
    for mask in range(1, 15):
        tris = _case(lib, mask)
        assert len(tris) == (2 if bin(mask).count("1") == 2 else 1)
        for tri in tris:
            assert len(set(tri)) == 3
            for e in tri:                                          # every edge joins an inside corner to an outside one
                i, j = ref.LOCAL_EDGES[e]
                assert (mask >> i & 1) != (mask >> j & 1), (mask, e)
        # the complement: the same triangles, the winding reversed
        assert [(a, c, b) for a, b, c in tris] == _case(lib, 15 - mask)
        # and the geometry's own answer for the tetrahedron of the identity permutation
        assert tris == [tuple(t) for t in ref.case_triangles(corners, mask)]
    n = C.c_int32(0)
    assert lib.rn_mesh_tet_case(16, C.byref(n), (C.c_int32 * 6)()) == RN_ERR_INVALID_ARG
    assert lib.rn_mesh_tet_case(3, None, None) == RN_ERR_INVALID_ARG and "mesh_tet_case" in hiplib.last_error()


def test_entry_points_refuse_bad_lattices(hiplib):
    """Axes below 2 and lattices whose counts would not fit an int32 come back as an error code before any launch."""
    lib, err = hiplib._lib, hiplib.last_error
    ws = lib.rn_mesh_workspace
    assert ws(1, 8, 8) == 0 and ws(8, 8, 1) == 0 and ws(0, 0, 0) == 0
    assert ws(565, 565, 565) == 0                                   # 12 * 564^3 = 2.15e9 >= 2^31
    assert ws(564, 564, 564) > 0                                    # 12 * 563^3 = 2.14e9
    n = 256 ** 3
    assert n * 5 <= ws(256, 256, 256) <= n * 5 + (1 << 20)          # a code byte and an int32 per point, and the chunk sums
    assert ws(2, 2, 2) >= 8 + 4 * 8
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.rn_mesh_count(p, 1, 4, 4, 10.0, p, p, None) == RN_ERR_INVALID_ARG and "axis" in err()
    assert lib.rn_mesh_count(None, 4, 4, 4, 10.0, p, p, None) == RN_ERR_INVALID_ARG and "null pointer" in err()
    assert lib.rn_mesh_emit(p, 4, 1, 4, 10.0, None, p, 1, 1, p, p, None) == RN_ERR_INVALID_ARG and "axis" in err()
    assert lib.rn_mesh_emit(p, 4, 4, 4, 10.0, None, p, 0, 0, None, None, None) == 0          # an empty surface: nothing to do
    assert lib.rn_mesh_emit(p, 4, 4, 4, 10.0, None, p, 3, 1, None, p, None) == RN_ERR_INVALID_ARG and "null pointer" in err()
    assert lib.rn_mesh_lattice_points(4, 4, 4, p, 60, 5, p, None) == RN_ERR_INVALID_ARG and "range" in err()
    assert lib.rn_mesh_lattice_points(4, 4, 4, p, 64, 0, p, None) == 0                         # an empty range
    assert lib.rn_mesh_lattice_points(4, 4, 4, None, 0, 5, p, None) == RN_ERR_INVALID_ARG and "null pointer" in err()


def test_ply_round_trip(hiplib, tmp_path, sphere):
    from radnerf import mesh
    verts, tris = sphere
    path = tmp_path / "sphere.ply"
    mesh.write_ply(path, verts, tris)
    raw = open(path, "rb").read()
    header = raw[:raw.index(b"end_header\n")].decode("ascii").split("\n")
    assert header[:2] == ["ply", "format binary_little_endian 1.0"]
    assert f"element vertex {len(verts)}" in header and f"element face {len(tris)}" in header
    assert len(raw) == raw.index(b"end_header\n") + 11 + 12 * len(verts) + 13 * len(tris)
    got_v, got_t = mesh.read_ply(path)
    assert ref.same_bits(got_v, verts) and got_t.dtype == np.int32 and np.array_equal(got_t, tris)
    # an empty mesh is a valid file
    empty = tmp_path / "empty.ply"
    mesh.write_ply(empty, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    got_v, got_t = mesh.read_ply(empty)
    assert got_v.shape == (0, 3) and got_t.shape == (0, 3)
    assert b"element vertex 0\n" in open(empty, "rb").read() and b"element face 0\n" in open(empty, "rb").read()
    # a truncated file is refused
    open(tmp_path / "cut.ply", "wb").write(raw[:-5])
    with pytest.raises(ValueError):
        mesh.read_ply(tmp_path / "cut.ply")
