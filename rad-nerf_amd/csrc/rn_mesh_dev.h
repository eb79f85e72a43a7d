// rn_mesh_dev.h -- the case logic and the vertex formula of the mesh export (rn_mesh.hip; DESIGN.md section 3, "mesh export"), plain
// functions for host and device.  No HIP header is needed: a host compiler builds the same text (tests/test_mesh.py does, as
// tests/test_camera_pose_abi.py does with rn_camera_dev.h), the kernels include it as it is.
//
// Marching tetrahedra on the Kuhn subdivision of a C-ordered lattice [X,Y,Z]:
//   * a value is inside iff u > threshold (NaN is outside);
//   * corner q of a cell is the point at offset (q & 1, q >> 1 & 1, q >> 2) from the cell's lowest point;
//   * tetrahedron k = 0..5 of a cell has the corners c0 = v000, c1 = c0 + e_a, c2 = c1 + e_b, c3 = v111 for the k-th permutation
//     (a, b, c) of the axes in lexicographic order: 012 021 102 120 201 210.  k = 1, 2, 5 are odd permutations: mirror images;
//   * every edge of every tetrahedron is one of seven kinds, owned by its lower point: offsets (1,0,0) (0,1,0) (0,0,1) (1,1,0)
//     (1,0,1) (0,1,1) (1,1,1), in this order.  An owned edge whose ends differ carries one vertex;
//   * a point's code byte: bits 0..6 = "edge kind e starts here, lies inside the lattice and its ends differ", bit 7 = the point
//     is inside.  The code of a cell's lowest point therefore holds the inside bits of all eight corners: everything after the
//     first pass works from the codes, the field is read again only to place the vertices;
//   * local edges of a tetrahedron: 0..5 = (c0,c1) (c0,c2) (c0,c3) (c1,c2) (c1,c3) (c2,c3).  One or three corners inside: one
//     triangle on the three crossed edges, starting with the lowest-numbered one.  Two inside (i < j), two outside (k < l): the quad
//     is split along the diagonal from edge (i,k) to edge (j,l); both triangles start at edge (i,k), the one whose third edge has the
//     lower number comes first.  (v1 - v0) x (v2 - v0) points from inside to outside.
// All vertex arithmetic is fp32 and rounds as written (the tree builds with -ffp-contract=off).
#pragma once

#include <stdint.h>

#ifndef RN_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define RN_HD __host__ __device__ inline
#else
#define RN_HD inline
#endif
#endif

namespace rn {
namespace mesh {

constexpr uint32_t kEdgeKinds = 7, kTets = 6;

RN_HD bool inside(float u, float threshold) { return u > threshold; }

// offset of edge kind e as corner bits (x | y << 1 | z << 2): 1 2 4 3 5 6 7 -- and the kind of an offset
RN_HD uint32_t edge_offset(uint32_t e) { return (0x7653421u >> (4u * e)) & 7u; }
RN_HD uint32_t edge_kind(uint32_t offset_bits) { return (0x65423100u >> (4u * offset_bits)) & 7u; }

// corner l = 0..3 of tetrahedron k as corner bits of the cell, and whether k is a mirror image
RN_HD uint32_t tet_corner(uint32_t k, uint32_t l) {
    const uint32_t a = k >> 1, b = (k & 1u) ? (a == 2u ? 1u : 2u) : (a == 0u ? 1u : 0u);
    return l == 0u ? 0u : (l == 1u ? 1u << a : (l == 2u ? (1u << a) | (1u << b) : 7u));
}
RN_HD bool tet_is_odd(uint32_t k) { return (0x26u >> k) & 1u; }

// the two corners of local edge e
RN_HD uint32_t local_edge_lo(uint32_t e) { return (e >= 3u ? 1u : 0u) + (e >= 5u ? 1u : 0u); }
RN_HD uint32_t local_edge_hi(uint32_t e) { return (0xFB9u >> (2u * e)) & 3u; }

// The triangles of a tetrahedron whose corner l is inside iff bit l of mask: local edge numbers into tri[][3], the count returned.
// The eight entries are the cases with c3 outside of a tetrahedron that is not mirrored; the complement of a case has the same
// triangles with the winding reversed, and so has the mirror image: reversing exchanges the last two corners of a triangle.
#define RN_MESH_TRI(a, b, c) ((uint32_t)(a) | ((uint32_t)(b) << 3) | ((uint32_t)(c) << 6))
#define RN_MESH_CASE(n, t0, t1) ((uint32_t)(n) | ((t0) << 2) | ((t1) << 11))
RN_HD uint32_t tet_case(uint32_t mask, bool odd, uint32_t tri[2][3]) {
    const uint32_t cases[8] = {
        RN_MESH_CASE(0, 0u, 0u),
        RN_MESH_CASE(1, RN_MESH_TRI(0, 1, 2), 0u),                        // c0
        RN_MESH_CASE(1, RN_MESH_TRI(0, 4, 3), 0u),                        // c1
        RN_MESH_CASE(2, RN_MESH_TRI(1, 2, 4), RN_MESH_TRI(1, 4, 3)),      // c0 c1
        RN_MESH_CASE(1, RN_MESH_TRI(1, 3, 5), 0u),                        // c2
        RN_MESH_CASE(2, RN_MESH_TRI(0, 5, 2), RN_MESH_TRI(0, 3, 5)),      // c0 c2
        RN_MESH_CASE(2, RN_MESH_TRI(0, 5, 1), RN_MESH_TRI(0, 4, 5)),      // c1 c2
        RN_MESH_CASE(1, RN_MESH_TRI(2, 4, 5), 0u),                        // c0 c1 c2
    };
    mask &= 15u;
    const bool complement = mask > 7u;
    const uint32_t c = cases[complement ? 15u - mask : mask], n = c & 3u;
    const bool flip = complement != odd;
    for (uint32_t t = 0; t < n; t++) {
        const uint32_t bits = (c >> (2u + 9u * t)) & 511u;
        tri[t][0] = bits & 7u;
        tri[t][flip ? 2 : 1] = (bits >> 3) & 7u;
        tri[t][flip ? 1 : 2] = (bits >> 6) & 7u;
    }
    return n;
}
#undef RN_MESH_TRI
#undef RN_MESH_CASE
RN_HD uint32_t tet_triangle_count(uint32_t mask) {
    const uint32_t m = mask & 15u;
    return (m == 0u || m == 15u) ? 0u : ((m == 3u || m == 5u || m == 6u || m == 9u || m == 10u || m == 12u) ? 2u : 1u);
}

// Code byte of a point.  in_bits: bit q = corner q of the cell that starts at the point is inside (bits of corners beyond the
// lattice are ignored); has_x / has_y / has_z: the lattice goes on past the point along that axis.
RN_HD uint32_t point_code(uint32_t in_bits, bool has_x, bool has_y, bool has_z) {
    const uint32_t reach = (has_x ? 1u : 0u) | (has_y ? 2u : 0u) | (has_z ? 4u : 0u);
    uint32_t code = (in_bits & 1u) << 7;
    for (uint32_t e = 0; e < kEdgeKinds; e++) {
        const uint32_t q = edge_offset(e);
        if ((q & ~reach) == 0u && (((in_bits >> q) ^ in_bits) & 1u)) code |= 1u << e;
    }
    return code;
}
// The inside bits of the eight corners of the cell whose lowest point has this code (a cell: all seven edges lie inside the lattice)
RN_HD uint32_t cell_inside_bits(uint32_t code) {
    const uint32_t in0 = (code >> 7) & 1u;
    uint32_t bits = in0;
    for (uint32_t q = 1; q < 8u; q++) bits |= (in0 ^ ((code >> edge_kind(q)) & 1u)) << q;
    return bits;
}
RN_HD uint32_t tet_mask(uint32_t in_bits, uint32_t k) {
    uint32_t m = 0;
    for (uint32_t l = 0; l < 4u; l++) m |= ((in_bits >> tet_corner(k, l)) & 1u) << l;
    return m;
}
RN_HD uint32_t cell_triangle_count(uint32_t code) {
    const uint32_t in_bits = cell_inside_bits(code);
    uint32_t n = 0;
    for (uint32_t k = 0; k < kTets; k++) n += tet_triangle_count(tet_mask(in_bits, k));
    return n;
}
RN_HD uint32_t popcount7(uint32_t code) {
    uint32_t v = code & 127u;
    v = v - ((v >> 1) & 0x55u);
    v = (v & 0x33u) + ((v >> 2) & 0x33u);
    return (v + (v >> 4)) & 15u;
}
// Where the vertex of edge kind e of a point stands among the point's vertices
RN_HD uint32_t vertex_slot(uint32_t code, uint32_t e) { return popcount7(code & ((1u << e) - 1u)); }

// Local edge e of tetrahedron k: the corner of the cell that owns it and its kind
RN_HD void tet_edge(uint32_t k, uint32_t e, uint32_t &owner_corner, uint32_t &kind) {
    const uint32_t lo = tet_corner(k, local_edge_lo(e)), hi = tet_corner(k, local_edge_hi(e));
    owner_corner = lo;
    kind = edge_kind(hi - lo);                 // the corners of a tetrahedron only gain axes: hi - lo has the bits hi adds to lo
}

// The vertex of edge kind e of the point p (lattice coordinates): p_a + t (p_b - p_a), t = (threshold - u_a) / (u_b - u_a)
RN_HD void edge_vertex(const uint32_t p[3], uint32_t e, float ua, float ub, float threshold, float v[3]) {
    const float t = (threshold - ua) / (ub - ua);
    const uint32_t q = edge_offset(e);
    for (uint32_t d = 0; d < 3u; d++) {
        const float pa = (float)p[d], pb = (float)(p[d] + ((q >> d) & 1u));
        v[d] = pa + t * (pb - pa);
    }
}
// lattice units -> world: v / (R - 1) * (bmax - bmin) + bmin (nerf/utils.py:398), one axis
RN_HD float to_world(float v, uint32_t R, float bmin, float bmax) { return v / (float)(R - 1u) * (bmax - bmin) + bmin; }

// Element i of torch.linspace(lo, hi, R) in fp32: step = (hi - lo) / (R - 1), the lower half counted up from lo (lo + step * i), the
// upper half down from hi (hi - step * (R - 1 - i)).  torch's builds contract each of the two into ONE fused multiply-add, on the
// host and on the device alike (measured: every element of 40 axes agrees with the fused form, 998 of them differ from the two-
// rounding form), so the fused form is spelled out here: this tree contracts nothing on its own.
RN_HD float linspace_step(float lo, float hi, uint32_t R) { return (hi - lo) / (float)(R - 1u); }
RN_HD float linspace_at(float lo, float hi, float step, uint32_t i, uint32_t R) {
    return i < R / 2u ? __builtin_fmaf(step, (float)i, lo) : __builtin_fmaf(-step, (float)(R - 1u - i), hi);
}

}  // namespace mesh
}  // namespace rn
