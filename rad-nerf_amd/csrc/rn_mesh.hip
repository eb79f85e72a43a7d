// rn_mesh.hip -- geometry export as gfx950 kernels: the density lattice of Trainer.save_mesh (nerf/utils.py:369-384, 871-891) and
// its isosurface (nerf/utils.py:387-399, where the reference calls mcubes on the CPU).
//
// Lattice points: k_mesh_points writes a contiguous range of the C-ordered [X,Y,Z] lattice, torch.linspace's fp32 formula per axis
// (rn_mesh_dev.h linspace_at), so that the point buffer holds one chunk of the density query and never the whole lattice.
//
// Isosurface: marching tetrahedra on the Kuhn subdivision; every convention is in rn_mesh_dev.h.  Passes:
//   k_mesh_codes      a workgroup stages the inside tests of its (4+1) x (4+1) x (32+1) points in LDS and writes one code byte per
//                     point: which of its seven owned edges cross the surface, and whether it is inside.  The code of a cell's
//                     lowest point holds the inside bits of all eight corners, so no later pass tests the field again.
//   k_mesh_sums       the lattice in C order in chunks of 1024 points: vertices (set edge bits) and triangles (of the cells that
//                     start in the chunk) per chunk.
//   k_mesh_scan       one workgroup: exclusive scan of both sums in chunk order, the totals to device memory.  Three plain launches;
//                     no workgroup waits for another one.
//   -- the host reads the two totals (the export's only synchronisation) and allocates --
//   k_mesh_vertices   per chunk: the scan of the vertex counts again, base[p] = index of the point's first vertex, and the vertices
//                     at base[p] + (number of lower edge kinds that cross).
//   k_mesh_triangles  per chunk: the scan of the triangle counts again; every corner of a triangle is an (owner point, edge kind)
//                     pair, looked up as base[owner] + popcount(code[owner] & ((1 << kind) - 1)).
// Vertices are ordered by point then edge kind, triangles by cell, tetrahedron, position: no atomic decides an index.
#include "rn_common.h"
#include "rn_mesh_dev.h"

#include "../../include/radnerf_fused.h"

namespace rn {
namespace mesh {

constexpr int kTileX = 4, kTileY = 4, kTileZ = 32;                              // points per workgroup of k_mesh_codes
constexpr int kCodeThreads = kTileX * kTileY * kTileZ;                          // 512
constexpr int kStage = (kTileX + 1) * (kTileY + 1) * (kTileZ + 1);              // 825 staged inside tests
constexpr int kChunkThreads = 256, kPerThread = 4, kChunk = kChunkThreads * kPerThread;   // 1024 points in C order
constexpr int kScanThreads = 1024;

struct Dims { uint32_t X, Y, Z, N; };

__device__ __forceinline__ void coords_of(uint32_t i, const Dims d, uint32_t p[3]) {
    const uint32_t yz = d.Y * d.Z;
    p[0] = i / yz;
    const uint32_t r = i - p[0] * yz;
    p[1] = r / d.Z;
    p[2] = r - p[1] * d.Z;
}
__device__ __forceinline__ bool is_cell(const uint32_t p[3], const Dims d) { return p[0] + 1 < d.X && p[1] + 1 < d.Y && p[2] + 1 < d.Z; }
// linear index of corner q of the cell that starts at point i
__device__ __forceinline__ uint32_t corner_index(uint32_t i, uint32_t q, const Dims d) {
    return i + (q & 1u) * d.Y * d.Z + ((q >> 1) & 1u) * d.Z + (q >> 2);
}

__global__ void __launch_bounds__(256)
k_mesh_points(Dims d, const float *__restrict__ box, uint32_t first, uint32_t n, float *__restrict__ points) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n) return;
    uint32_t p[3];
    coords_of(first + t, d, p);
    const uint32_t R[3] = {d.X, d.Y, d.Z};
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float lo = box[a], hi = box[3 + a];
        points[(size_t)t * 3 + a] = linspace_at(lo, hi, linspace_step(lo, hi, R[a]), p[a], R[a]);
    }
}

__global__ void __launch_bounds__(kCodeThreads)
k_mesh_codes(const float *__restrict__ field, Dims d, float threshold, uint8_t *__restrict__ codes) {
    __shared__ uint8_t in_lds[kStage];
    const uint32_t x0 = blockIdx.z * kTileX, y0 = blockIdx.y * kTileY, z0 = blockIdx.x * kTileZ;
    for (uint32_t s = threadIdx.x; s < (uint32_t)kStage; s += kCodeThreads) {
        const uint32_t sz = s % (kTileZ + 1), sy = (s / (kTileZ + 1)) % (kTileY + 1), sx = s / ((kTileZ + 1) * (kTileY + 1));
        const uint32_t x = x0 + sx, y = y0 + sy, z = z0 + sz;
        const bool in_lattice = x < d.X && y < d.Y && z < d.Z;
        in_lds[s] = in_lattice && inside(field[((size_t)x * d.Y + y) * d.Z + z], threshold) ? 1 : 0;
    }
    __syncthreads();
    const uint32_t tz = threadIdx.x % kTileZ, ty = (threadIdx.x / kTileZ) % kTileY, tx = threadIdx.x / (kTileZ * kTileY);
    const uint32_t x = x0 + tx, y = y0 + ty, z = z0 + tz;
    if (x >= d.X || y >= d.Y || z >= d.Z) return;
    uint32_t in_bits = 0;
#pragma unroll
    for (uint32_t q = 0; q < 8; q++) {
        const uint32_t s = ((tx + (q & 1u)) * (kTileY + 1) + ty + ((q >> 1) & 1u)) * (kTileZ + 1) + tz + (q >> 2);
        in_bits |= (uint32_t)in_lds[s] << q;
    }
    codes[((size_t)x * d.Y + y) * d.Z + z] = (uint8_t)point_code(in_bits, x + 1 < d.X, y + 1 < d.Y, z + 1 < d.Z);
}

// What a chunk's thread holds: the codes of its kPerThread consecutive points and their counts
struct ThreadCounts { uint32_t code[kPerThread], tris[kPerThread], n_vert, n_tri; };

// tri_lut[c] = triangles of a cell whose lowest point has code c: built by the workgroup (thread c computes entry c), ends in a barrier
__device__ __forceinline__ void build_tri_lut(uint8_t *tri_lut) {
    tri_lut[threadIdx.x] = (uint8_t)cell_triangle_count(threadIdx.x);
    __syncthreads();
}
__device__ __forceinline__ ThreadCounts chunk_counts(const uint8_t *__restrict__ codes, const Dims d, const uint8_t *tri_lut, uint32_t first) {
    ThreadCounts c;
    c.n_vert = c.n_tri = 0;
#pragma unroll
    for (int k = 0; k < kPerThread; k++) {
        const uint32_t i = first + k;
        c.code[k] = 0;
        c.tris[k] = 0;
        if (i < d.N) {
            uint32_t p[3];
            coords_of(i, d, p);
            c.code[k] = codes[i];
            c.tris[k] = is_cell(p, d) ? tri_lut[c.code[k]] : 0u;
        }
        c.n_vert += popcount7(c.code[k]);
        c.n_tri += c.tris[k];
    }
    return c;
}

__global__ void __launch_bounds__(kChunkThreads)
k_mesh_sums(const uint8_t *__restrict__ codes, Dims d, uint32_t *__restrict__ vert_sums, uint32_t *__restrict__ tri_sums) {
    __shared__ uint8_t tri_lut[256];
    __shared__ uint32_t red_v[kChunkThreads / kWave], red_t[kChunkThreads / kWave];
    build_tri_lut(tri_lut);
    const ThreadCounts c = chunk_counts(codes, d, tri_lut, blockIdx.x * kChunk + threadIdx.x * kPerThread);
    const uint32_t v = block_sum_first<uint32_t, kChunkThreads>(c.n_vert, red_v);
    const uint32_t t = block_sum_first<uint32_t, kChunkThreads>(c.n_tri, red_t);
    if (threadIdx.x == 0) {
        vert_sums[blockIdx.x] = v;
        tri_sums[blockIdx.x] = t;
    }
}

// In place: sums -> exclusive offsets, in chunk order; totals = {V, T}
__global__ void __launch_bounds__(kScanThreads)
k_mesh_scan(uint32_t *__restrict__ vert_sums, uint32_t *__restrict__ tri_sums, uint32_t n_chunks, int32_t *__restrict__ totals) {
    __shared__ uint32_t lds_v[kScanThreads / kWave], lds_t[kScanThreads / kWave];
    uint32_t carry_v = 0, carry_t = 0;
    for (uint32_t b0 = 0; b0 < n_chunks; b0 += kScanThreads) {
        const uint32_t b = b0 + threadIdx.x;
        const uint32_t v = b < n_chunks ? vert_sums[b] : 0u, t = b < n_chunks ? tri_sums[b] : 0u;
        uint32_t all_v, all_t;
        const uint32_t ev = block_exclusive_scan<kScanThreads>(v, lds_v, &all_v);
        const uint32_t et = block_exclusive_scan<kScanThreads>(t, lds_t, &all_t);
        if (b < n_chunks) {
            vert_sums[b] = carry_v + ev;
            tri_sums[b] = carry_t + et;
        }
        carry_v += all_v;
        carry_t += all_t;
        __syncthreads();                        // lds_v / lds_t are read until here
    }
    if (threadIdx.x == 0) {
        totals[0] = (int32_t)carry_v;
        totals[1] = (int32_t)carry_t;
    }
}

__global__ void __launch_bounds__(kChunkThreads)
k_mesh_vertices(const float *__restrict__ field, const uint8_t *__restrict__ codes, Dims d, float threshold, const float *__restrict__ box,
                const uint32_t *__restrict__ vert_offsets, uint32_t n_vertices, int32_t *__restrict__ base, float *__restrict__ vertices) {
    __shared__ uint8_t tri_lut[256];
    __shared__ uint32_t lds[kChunkThreads / kWave];
    build_tri_lut(tri_lut);
    const uint32_t first = blockIdx.x * kChunk + threadIdx.x * kPerThread;
    const ThreadCounts c = chunk_counts(codes, d, tri_lut, first);
    uint32_t at = vert_offsets[blockIdx.x] + block_exclusive_scan<kChunkThreads>(c.n_vert, lds);
    const uint32_t R[3] = {d.X, d.Y, d.Z};
#pragma unroll
    for (int k = 0; k < kPerThread; k++) {
        const uint32_t i = first + k;
        if (i >= d.N) break;
        base[i] = (int32_t)at;
        const uint32_t code = c.code[k];
        if (!(code & 127u)) continue;
        uint32_t p[3];
        coords_of(i, d, p);
        const float ua = field[i];
        for (uint32_t e = 0; e < kEdgeKinds; e++) {
            if (!((code >> e) & 1u)) continue;
            float v[3];
            edge_vertex(p, e, ua, field[corner_index(i, edge_offset(e), d)], threshold, v);
            if (at < n_vertices) {
#pragma unroll
                for (int a = 0; a < 3; a++) vertices[(size_t)at * 3 + a] = box ? to_world(v[a], R[a], box[a], box[3 + a]) : v[a];
            }
            at++;
        }
    }
}

__global__ void __launch_bounds__(kChunkThreads)
k_mesh_triangles(const uint8_t *__restrict__ codes, Dims d, const uint32_t *__restrict__ tri_offsets, const int32_t *__restrict__ base,
                 uint32_t n_triangles, int32_t *__restrict__ triangles) {
    __shared__ uint8_t tri_lut[256];
    __shared__ uint32_t lds[kChunkThreads / kWave];
    build_tri_lut(tri_lut);
    const uint32_t first = blockIdx.x * kChunk + threadIdx.x * kPerThread;
    const ThreadCounts c = chunk_counts(codes, d, tri_lut, first);
    uint32_t at = tri_offsets[blockIdx.x] + block_exclusive_scan<kChunkThreads>(c.n_tri, lds);
#pragma unroll
    for (int k = 0; k < kPerThread; k++) {
        if (!c.tris[k]) continue;                       // also: not a cell, or beyond the lattice
        const uint32_t i = first + k;
        const uint32_t in_bits = cell_inside_bits(c.code[k]);
        // the cell's eight corner points: first vertex and code of each, fetched once (a corner that owns no vertex is never used)
        int32_t corner_base[8];
        uint32_t corner_code[8];
#pragma unroll
        for (uint32_t q = 0; q < 8; q++) {
            const uint32_t j = corner_index(i, q, d);
            corner_base[q] = base[j];
            corner_code[q] = codes[j];
        }
        for (uint32_t tet = 0; tet < kTets; tet++) {
            uint32_t tri[2][3];
            const uint32_t n = tet_case(tet_mask(in_bits, tet), tet_is_odd(tet), tri);
            for (uint32_t t = 0; t < n; t++) {
                if (at < n_triangles) {
                    for (int a = 0; a < 3; a++) {
                        uint32_t q, kind;
                        tet_edge(tet, tri[t][a], q, kind);
                        triangles[(size_t)at * 3 + a] = corner_base[q] + (int32_t)vertex_slot(corner_code[q], kind);
                    }
                }
                at++;
            }
        }
    }
}

static bool lattice_ok(uint32_t X, uint32_t Y, uint32_t Z) {
    if (X < 2 || Y < 2 || Z < 2) return false;
    const unsigned __int128 cells = (unsigned __int128)(X - 1) * (Y - 1) * (Z - 1), points = (unsigned __int128)X * Y * Z;
    return 12 * cells < ((unsigned __int128)1 << 31) && 7 * points < ((unsigned __int128)1 << 31);
}

// codes [N] (padded to 16 bytes) | base int32 [N] | vertex sums uint32 [chunks] | triangle sums uint32 [chunks]
struct Workspace {
    uint8_t *codes;
    int32_t *base;
    uint32_t *vert_sums, *tri_sums;
    uint32_t n_chunks;
    size_t bytes;
};
static Workspace carve(void *ws, uint32_t N) {
    Workspace w;
    const size_t codes_bytes = ((size_t)N + 15u) & ~(size_t)15u;
    w.n_chunks = div_up(N, kChunk);
    w.codes = static_cast<uint8_t *>(ws);
    w.base = reinterpret_cast<int32_t *>(w.codes + codes_bytes);
    w.vert_sums = reinterpret_cast<uint32_t *>(w.base + N);
    w.tri_sums = w.vert_sums + w.n_chunks;
    w.bytes = codes_bytes + (size_t)N * 4u + (size_t)w.n_chunks * 8u;
    return w;
}

}  // namespace mesh
}  // namespace rn

using namespace rn;
using namespace rn::mesh;

extern "C" {

size_t rn_mesh_workspace(uint32_t X, uint32_t Y, uint32_t Z) {
    if (!lattice_ok(X, Y, Z)) return 0;
    return carve(nullptr, X * Y * Z).bytes;
}

int rn_mesh_lattice_points(uint32_t X, uint32_t Y, uint32_t Z, const float *box, uint32_t first, uint32_t n, float *points,
                           rn_stream_t stream) {
    RN_REQUIRE(lattice_ok(X, Y, Z), "mesh_lattice_points: every axis >= 2 and 12 cells < 2^31 (got %u x %u x %u)", X, Y, Z);
    const uint32_t N = X * Y * Z;
    RN_REQUIRE(first <= N && n <= N - first, "mesh_lattice_points: range %u + %u beyond the %u lattice points", first, n, N);
    if (n == 0) return RN_OK;
    RN_REQUIRE(box && points, "mesh_lattice_points: null pointer");
    hipLaunchKernelGGL(k_mesh_points, dim3(div_up(n, 256)), dim3(256), 0, as_stream(stream), Dims{X, Y, Z, N}, box, first, n, points);
    return check_launch("mesh_lattice_points");
}

int rn_mesh_count(const float *field, uint32_t X, uint32_t Y, uint32_t Z, float threshold, void *workspace, int32_t *totals,
                  rn_stream_t stream) {
    RN_REQUIRE(lattice_ok(X, Y, Z), "mesh_count: every axis >= 2 and 12 cells < 2^31 (got %u x %u x %u)", X, Y, Z);
    RN_REQUIRE(field && workspace && totals, "mesh_count: null pointer");
    RN_REQUIRE(((uintptr_t)workspace & 15u) == 0, "mesh_count: workspace must be 16-byte aligned");
    const Dims d{X, Y, Z, X * Y * Z};
    const Workspace w = carve(workspace, d.N);
    const dim3 tiles(div_up(Z, kTileZ), div_up(Y, kTileY), div_up(X, kTileX));
    RN_REQUIRE(tiles.y <= 65535u && tiles.z <= 65535u, "mesh_count: lattice too wide for one launch");
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_mesh_codes, tiles, dim3(kCodeThreads), 0, s, field, d, threshold, w.codes);
    hipLaunchKernelGGL(k_mesh_sums, dim3(w.n_chunks), dim3(kChunkThreads), 0, s, w.codes, d, w.vert_sums, w.tri_sums);
    hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(kScanThreads), 0, s, w.vert_sums, w.tri_sums, w.n_chunks, totals);
    return check_launch("mesh_count");
}

int rn_mesh_emit(const float *field, uint32_t X, uint32_t Y, uint32_t Z, float threshold, const float *box, void *workspace,
                 uint32_t n_vertices, uint32_t n_triangles, float *vertices, int32_t *triangles, rn_stream_t stream) {
    RN_REQUIRE(lattice_ok(X, Y, Z), "mesh_emit: every axis >= 2 and 12 cells < 2^31 (got %u x %u x %u)", X, Y, Z);
    if (n_vertices == 0 && n_triangles == 0) return RN_OK;
    RN_REQUIRE(field && workspace && vertices && triangles, "mesh_emit: null pointer");
    RN_REQUIRE(n_vertices > 0 && n_triangles > 0, "mesh_emit: a surface has both vertices and triangles");
    RN_REQUIRE(((uintptr_t)workspace & 15u) == 0, "mesh_emit: workspace must be 16-byte aligned");
    const Dims d{X, Y, Z, X * Y * Z};
    const Workspace w = carve(workspace, d.N);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_mesh_vertices, dim3(w.n_chunks), dim3(kChunkThreads), 0, s, field, w.codes, d, threshold, box, w.vert_sums,
                       n_vertices, w.base, vertices);
    hipLaunchKernelGGL(k_mesh_triangles, dim3(w.n_chunks), dim3(kChunkThreads), 0, s, w.codes, d, w.tri_sums, w.base, n_triangles,
                       triangles);
    return check_launch("mesh_emit");
}

int rn_mesh_tet_case(uint32_t mask, int32_t *n_triangles, int32_t *edges) {
    RN_REQUIRE(mask < 16u && n_triangles && edges, "mesh_tet_case: mask is 4 bits, the outputs are not null");
    uint32_t tri[2][3];
    const uint32_t n = tet_case(mask, false, tri);
    *n_triangles = (int32_t)n;
    for (uint32_t t = 0; t < n; t++)
        for (int a = 0; a < 3; a++) edges[3 * t + a] = (int32_t)tri[t][a];
    return RN_OK;
}

}  // extern "C"
