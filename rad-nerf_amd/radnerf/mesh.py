"""Geometry export on the device: what Trainer.save_mesh, extract_fields and extract_geometry do in the reference
(nerf/utils.py:369-399, 871-891), without mcubes or trimesh and without a read-back per block.

    extract_fields    the density lattice [R,R,R]: rn_mesh_lattice_points writes one range of lattice points at a time (the point
                      buffer holds `chunk` points, never the lattice), the density query is the fused kernel's sigma branch
                      (fused.density_forward; `model.density` through the PyTorch layers when the network is not of the fused
                      shape).  Raw sigma, as the reference thresholds it.  Nothing is read back.
    isosurface        marching tetrahedra on the Kuhn subdivision (csrc/rn_mesh_dev.h states the conventions; DESIGN.md section 3
                      why not the 256-case cube table): rn_mesh_count, ONE read-back of the two totals, rn_mesh_emit.  Vertex and
                      triangle order are specified, two runs give the same bytes.
    extract_geometry  both over model.aabb_infer.
    write_ply         binary little-endian PLY with numpy alone; read_ply reads such a file back.

The head's geometry depends on the audio window and the eye value, so the export takes them (the reference's save_mesh calls
self.model.density(pts), which this network's density(x, enc_a, e) never accepted).
"""
import numpy as np
import torch

import radnerf_hip as hip

_lib = hip._lib


def _resolution(resolution):
    r = (int(resolution),) * 3 if np.ndim(resolution) == 0 else tuple(int(v) for v in resolution)
    if len(r) != 3 or int(_lib.rn_mesh_workspace(*r)) == 0:
        raise ValueError(f"mesh: a lattice needs three axes >= 2 and 12 cells < 2^31, got {resolution}")
    return r


def _box(bound_min, bound_max, device):
    """{min x, y, z, max x, y, z} on the device, built without reading anything back."""
    parts = [torch.as_tensor(b, dtype=torch.float32).to(device).reshape(-1) for b in (bound_min, bound_max)]
    if parts[0].numel() != 3 or parts[1].numel() != 3:
        raise ValueError("mesh: bound_min and bound_max have three components")
    return torch.cat(parts).contiguous()


def lattice_points(bound_min, bound_max, resolution, first, n, out=None, device="cuda"):
    """Points first .. first + n - 1 (C order) of the lattice torch.linspace(min, max, R) per axis spans through
    meshgrid(indexing='ij'): [n, 3] fp32 (the first n rows of `out` when given).  bound_max = None: bound_min is the box
    {min x, y, z, max x, y, z} already on the device."""
    r = _resolution(resolution)
    box = bound_min if bound_max is None else _box(bound_min, bound_max, out.device if out is not None else device)
    if out is None:
        out = torch.empty(n, 3, dtype=torch.float32, device=box.device)
    if out.dtype != torch.float32 or out.numel() < 3 * n:
        raise ValueError("mesh: the point buffer must hold n x 3 fp32")
    hip.call("rn_mesh_lattice_points", *r, hip.ptr(box), int(first), int(n), hip.ptr(out), hip.stream())
    return out[:n]


@torch.no_grad()
def extract_fields(model, bound_min, bound_max, resolution, enc_a, eye=None, chunk=1 << 21):
    """sigma on the lattice: a device tensor [R,R,R] fp32 (nerf/utils.py:369-384 with the network's audio code and eye value)."""
    from . import fused
    r = _resolution(resolution)
    dev = next(model.parameters()).device
    n_all = r[0] * r[1] * r[2]
    chunk = min((max(int(chunk), 1) + 63) // 64 * 64, n_all)          # whole waves: every range's slice of the field stays 256-byte aligned
    box = _box(bound_min, bound_max, dev)
    pts = torch.empty(chunk, 3, dtype=torch.float32, device=dev)
    field = torch.empty(n_all, dtype=torch.float32, device=dev)
    use_fused = fused.supported(model)
    for first in range(0, n_all, chunk):
        n = min(chunk, n_all - first)
        p = lattice_points(box, None, r, first, n, out=pts)
        if use_fused:
            fused.density_forward(model, p, enc_a, eye, out=field[first:first + n])
        else:
            field[first:first + n] = model.density(p, enc_a, eye)["sigma"].reshape(-1).float()
    return field.view(*r)


def isosurface(field, threshold, bound_min=None, bound_max=None):
    """(vertices [V,3] fp32, triangles [T,3] int32) on the device for a contiguous fp32 [X,Y,Z] device tensor: the surface
    u = threshold, inside where u > threshold, wound so that (v1 - v0) x (v2 - v0) points outwards.  Without bounds the vertices
    are in lattice units, with them v / (R - 1) * (max - min) + min per axis.  One synchronisation: the two totals."""
    if field.dim() != 3 or field.dtype != torch.float32 or not field.is_cuda or not field.is_contiguous():
        raise ValueError("isosurface: a contiguous fp32 [X,Y,Z] device tensor")
    if (bound_min is None) != (bound_max is None):
        raise ValueError("isosurface: both bounds or none")
    r = _resolution(field.shape)
    dev = field.device
    box = None if bound_min is None else _box(bound_min, bound_max, dev)
    ws = torch.empty(int(_lib.rn_mesh_workspace(*r)), dtype=torch.uint8, device=dev)
    totals = torch.empty(2, dtype=torch.int32, device=dev)
    s = hip.stream()
    hip.call("rn_mesh_count", hip.ptr(field), *r, float(threshold), hip.ptr(ws), hip.ptr(totals), s)
    n_v, n_t = totals.tolist()                                        # the export's only read-back
    vertices = torch.empty(n_v, 3, dtype=torch.float32, device=dev)
    triangles = torch.empty(n_t, 3, dtype=torch.int32, device=dev)
    if n_v and n_t:
        hip.call("rn_mesh_emit", hip.ptr(field), *r, float(threshold), hip.ptr(box), hip.ptr(ws), n_v, n_t, hip.ptr(vertices),
                 hip.ptr(triangles), s)
    return vertices, triangles


def extract_geometry(model, resolution, threshold, enc_a, eye=None, chunk=1 << 21):
    """The surface sigma = threshold inside model.aabb_infer, in world coordinates (nerf/utils.py:387-399, 886)."""
    lo, hi = model.aabb_infer[:3], model.aabb_infer[3:]
    field = extract_fields(model, lo, hi, resolution, enc_a, eye, chunk)
    return isosurface(field, threshold, lo, hi)


_PLY_HEADER = ("ply\nformat binary_little_endian 1.0\nelement vertex {}\nproperty float x\nproperty float y\nproperty float z\n"
               "element face {}\nproperty list uchar int vertex_indices\nend_header\n")
_PLY_FACE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


def _host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def write_ply(path, vertices, triangles):
    """Binary little-endian PLY: float x y z per vertex, a uchar count and three int indices per face."""
    v = np.ascontiguousarray(_host(vertices), "<f4").reshape(-1, 3)
    t = _host(triangles).reshape(-1, 3)
    faces = np.empty(len(t), _PLY_FACE)
    faces["n"] = 3
    faces["v"] = t
    with open(path, "wb") as f:
        f.write(_PLY_HEADER.format(len(v), len(t)).encode("ascii"))
        f.write(v.tobytes())
        f.write(faces.tobytes())


def read_ply(path):
    """(vertices [V,3] float32, triangles [T,3] int32) of a file write_ply wrote."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError(f"{path}: not a binary little-endian PLY")
    counts = {ln.split()[1]: int(ln.split()[2]) for ln in lines if ln.startswith("element ")}
    n_v, n_t = counts["vertex"], counts["face"]
    if len(data) != end + 12 * n_v + _PLY_FACE.itemsize * n_t:
        raise ValueError(f"{path}: {len(data) - end} bytes of data do not hold {n_v} vertices and {n_t} triangles")
    v = np.frombuffer(data, "<f4", 3 * n_v, end).reshape(n_v, 3).astype(np.float32)
    faces = np.frombuffer(data, _PLY_FACE, n_t, end + 12 * n_v)
    if n_t and not (faces["n"] == 3).all():
        raise ValueError(f"{path}: faces must be triangles")
    return v, faces["v"].astype(np.int32).reshape(n_t, 3)
