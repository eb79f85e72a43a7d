"""Mesh export on the device (rad-nerf_amd/radnerf/mesh.py over csrc/rn_mesh.hip) against the numpy reference of
tests/mesh_reference.py on the read-back field, the lattice and the density query against torch, Trainer.save_mesh end to end.

Bars: triangle arrays equal; vertices equal bit for bit (ALLOWED_SPACINGS = 0: the device divides as IEEE-754 says; the issue
would allow up to 4 spacings -- three roundings in the vertex formula, two in the world transform -- none is needed); the density
lattice within rel 2e-4 of model.density through the PyTorch layers, the bar tests/test_occupancy.py holds the fused query to."""
import numpy as np
import pytest
import torch

import mesh_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALLOWED_SPACINGS = 0
BOX = ([-1.0, -0.5, 0.25], [1.0, 2.0, 0.75])


def _ellipsoid_field(shape):
    x, y, z = np.meshgrid(*[np.linspace(-1, 1, n) for n in shape], indexing="ij")
    return (10 + 20 * (0.7 - np.sqrt(x * x + 1.3 * y * y + 0.8 * z * z))).astype(np.float32)


def _slab_field(shape):
    x, y, z = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    return (10 + 2 * np.sin(0.31 * x + 0.2) + 1.5 * np.sin(0.8 * y + 0.27 * z) + 2 * np.sin(0.23 * z - 0.11 * x)).astype(np.float32)


# name -> field.  The code pass works on tiles of 4 x 4 x 32 points, the later passes on chunks of 1024 points in C order and one
# workgroup scans 1024 chunk sums at a time: tile_plus_1 / tile_plus_2 end one point / one cell past a multiple of the tile on every
# axis, `chunks` has 1068 chunks (the scan's second round), the others are the issue's.
FIELDS = {
    "sphere17": lambda: ref.sphere_field(17),
    "sines": ref.sines_field,
    "threshold": ref.threshold_field,
    "plane": ref.plane_field,
    "slab": lambda: _slab_field((65, 5, 66)),
    "tile_plus_1": lambda: _slab_field((9, 5, 33)),
    "tile_plus_2": lambda: _slab_field((10, 6, 34)),
    "chunks": lambda: _ellipsoid_field((102, 103, 104)),
}
_CACHE = {}


def _case(name):
    """(field, reference vertices in lattice units, reference triangles), computed once per session and never written to."""
    if name not in _CACHE:
        field = FIELDS[name]()
        verts, tris = ref.marching_tetrahedra(field, 10.0)
        for a in (field, verts, tris):
            a.setflags(write=False)
        _CACHE[name] = (field, verts, tris)
    return _CACHE[name]


def _dev(field):
    return torch.from_numpy(np.array(field)).to(DEV)          # a copy: the cached arrays are read-only


def _worst_spacings(got, want):
    if got.shape != want.shape:
        return float("inf")
    if ref.same_bits(got, want):
        return 0.0
    with np.errstate(all="ignore"):
        d = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
    d[np.isnan(got) & np.isnan(want)] = 0
    return float(np.nan_to_num(d, nan=np.inf).max())


@pytest.mark.parametrize("name", list(FIELDS))
def test_isosurface_equals_the_reference(hiplib, name):
    from radnerf import mesh
    field, want_v, want_t = _case(name)
    assert len(want_t) > 100
    v, t = mesh.isosurface(_dev(field), 10.0)
    assert v.dtype == torch.float32 and t.dtype == torch.int32 and v.is_cuda and t.is_cuda
    got_v, got_t = v.cpu().numpy(), t.cpu().numpy()
    worst = _worst_spacings(got_v, want_v)
    print(f"{name} {field.shape}: V {len(got_v)} T {len(got_t)} worst vertex difference {worst} spacings")
    assert np.array_equal(got_t, want_t)
    assert worst <= ALLOWED_SPACINGS


def test_isosurface_in_world_coordinates(hiplib):
    from radnerf import mesh
    field, _, want_t = _case("sines")
    want_v, _ = ref.marching_tetrahedra(field, 10.0, *BOX)
    v, t = mesh.isosurface(_dev(field), 10.0, *BOX)
    worst = _worst_spacings(v.cpu().numpy(), want_v)
    print(f"world coordinates: worst vertex difference {worst} spacings")
    assert np.array_equal(t.cpu().numpy(), want_t) and worst <= ALLOWED_SPACINGS
    lo, hi = np.asarray(BOX[0], np.float32), np.asarray(BOX[1], np.float32)
    assert (v.cpu().numpy() >= lo).all() and (v.cpu().numpy() <= hi).all()


@pytest.mark.parametrize("value", [0.0, 20.0, float("nan")])
def test_no_surface_gives_empty_tensors(hiplib, value):
    """All outside, all inside, all NaN (outside): V = T = 0, empty tensors, no launch error."""
    from radnerf import mesh
    v, t = mesh.isosurface(torch.full((9, 6, 37), value, device=DEV), 10.0)
    torch.cuda.synchronize()
    assert tuple(v.shape) == (0, 3) and tuple(t.shape) == (0, 3) and v.dtype == torch.float32 and t.dtype == torch.int32


def test_plane_gives_an_open_surface_along_the_lattice_boundary(hiplib):
    from radnerf import mesh
    field, _, _ = _case("plane")
    v, t = mesh.isosurface(_dev(field), 10.0)
    verts, tris = v.cpu().numpy(), t.cpu().numpy()
    und, uses, balance = ref.edge_use(tris)
    assert set(np.unique(uses)) == {1, 2} and (balance[uses == 2] == 0).all()
    on_face = ((verts == 0) | (verts == np.asarray(field.shape, np.float32) - 1)).any(1)
    assert on_face[und[uses == 1]].all()                       # boundary edges are used once and lie on the lattice boundary
    # and the surface points up the field's gradient reversed: from inside (u > threshold) to outside
    n = np.cross(verts[tris[:, 1]] - verts[tris[:, 0]], verts[tris[:, 2]] - verts[tris[:, 0]]).sum(0)
    assert n @ np.array([0.8, 0.45, -0.3]) < 0


def test_two_calls_return_the_same_bytes(hiplib):
    from radnerf import mesh
    field = _dev(_case("slab")[0])
    a, b = mesh.isosurface(field, 10.0), mesh.isosurface(field, 10.0)
    assert a[0].data_ptr() != b[0].data_ptr()
    assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))


def test_isosurface_refuses_what_it_cannot_take(hiplib):
    from radnerf import mesh
    with pytest.raises(ValueError):
        mesh.isosurface(torch.zeros(4, 4, 1, device=DEV), 10.0)
    with pytest.raises(ValueError):
        mesh.isosurface(torch.zeros(4, 4, 4, device=DEV).transpose(0, 2), 10.0)
    with pytest.raises(ValueError):
        mesh.isosurface(torch.zeros(4, 4, 4, device=DEV, dtype=torch.float64), 10.0)


# ------------------------------------------------------------------------------------------------ the density lattice
@pytest.fixture(scope="module")
def scene():
    """The small synthetic model of tests/test_occupancy.py, an audio window, its code and the eye value."""
    from radnerf.rays import get_audio_features
    from radnerf.scene import SyntheticScene, default_opt
    sc = SyntheticScene(H=32, W=32, n_frames=8, device=DEV, opt=default_opt(engine="fused", torso=False))
    auds = get_audio_features(sc.aud_features, sc.opt.att, 3)
    with torch.no_grad():
        enc_a = sc.model.encode_audio(auds)
    return sc, auds, enc_a, torch.tensor([[0.25]], device=DEV)


def test_lattice_points_are_torch_linspace_through_meshgrid(hiplib):
    from radnerf import mesh
    for lo, hi, R in (([-1.0, -0.5, -1.0], [1.0, 0.5, 1.0], 24), ([-0.7, 0.1, -1.0], [0.9, 2.3, 0.33], (13, 24, 7))):
        shape = (R,) * 3 if isinstance(R, int) else R
        axes = [torch.linspace(lo[a], hi[a], shape[a], device=DEV) for a in range(3)]
        xx, yy, zz = torch.meshgrid(*axes, indexing="ij")
        want = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1), zz.reshape(-1, 1)], dim=-1)          # nerf/utils.py:380-381
        on_host = torch.stack(torch.meshgrid(*[torch.linspace(lo[a], hi[a], shape[a]) for a in range(3)], indexing="ij"), -1)
        assert torch.equal(on_host.reshape(-1, 3), want.cpu())                                       # the reference builds them on the host
        n_all, chunk = want.shape[0], 1000                                                         # 1000 divides neither lattice
        assert n_all % chunk
        got = torch.cat([mesh.lattice_points(lo, hi, R, first, min(chunk, n_all - first)).clone() for first in range(0, n_all, chunk)])
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    with pytest.raises(RuntimeError):
        mesh.lattice_points(lo, hi, 24, 24 ** 3 - 5, 6)


def test_extract_fields_is_model_density_on_the_lattice(hiplib, scene):
    from radnerf import fused, mesh
    sc, _, enc_a, eye = scene
    m = sc.model
    assert fused.supported(m)
    lo, hi = m.aabb_infer[:3], m.aabb_infer[3:]
    field = mesh.extract_fields(m, lo, hi, 24, enc_a, eye, chunk=5000)            # 5000 does not divide 24^3 = 13824
    assert tuple(field.shape) == (24, 24, 24) and field.dtype == torch.float32 and field.is_cuda
    pts = mesh.lattice_points(lo, hi, 24, 0, 24 ** 3)
    with torch.no_grad():
        want = m.density(pts, enc_a, eye)["sigma"].reshape(24, 24, 24).float()
    err = ((field - want).abs() / want.abs().clamp(min=1e-30)).max().item()
    print(f"extract_fields against model.density: worst relative difference {err:.3e}")
    np.testing.assert_allclose(field.cpu().numpy(), want.cpu().numpy(), rtol=2e-4, atol=1e-6)
    other = mesh.extract_fields(m, lo, hi, 24, enc_a, eye, chunk=1 << 21)
    assert torch.equal(field.view(torch.int32), other.view(torch.int32))         # the chunking changes no bit


# ----------------------------------------------------------------------------------------------------- Trainer.save_mesh
def test_save_mesh_writes_the_isosurface_of_the_field(hiplib, scene, tmp_path):
    from radnerf import mesh
    from radnerf.train import Trainer
    sc, auds, enc_a, eye = scene
    m = sc.model
    tr = Trainer(m, sc.opt, update_extra_interval=0, ema_decay=0.95, ema_update_interval=4)
    g = torch.Generator(device=DEV).manual_seed(10)
    with torch.no_grad():
        for p, s in tr.ema.pairs():
            s.add_(0.02 * torch.randn(s.shape, device=DEV, generator=g) * s.abs().mean())
    live = [p.detach().clone() for p in m.parameters()]
    m.train()
    lo, hi = m.aabb_infer[:3], m.aabb_infer[3:]
    with torch.no_grad(), tr.ema_scope():                                        # what the export sees: the averaged weights
        field = mesh.extract_fields(m, lo, hi, 32, m.encode_audio(auds), eye)
    threshold = float(field.median())                                             # a random network: put the surface where it has one
    want_v, want_t = mesh.isosurface(field, threshold, lo, hi)
    assert want_t.shape[0] > 100
    path = tmp_path / "meshes" / "head.ply"
    tr.save_mesh(str(path), resolution=32, threshold=threshold, auds=auds, eye=eye)
    got_v, got_t = mesh.read_ply(path)                                            # the file parses
    assert np.array_equal(got_t, want_t.cpu().numpy()) and ref.same_bits(got_v, want_v.cpu().numpy())
    box = m.aabb_infer.cpu().numpy()
    assert (got_v >= box[:3]).all() and (got_v <= box[3:]).all()
    assert got_t.min() == 0 and got_t.max() == len(got_v) - 1
    assert m.training                                                             # the mode comes back
    for p, q in zip(m.parameters(), live):                                        # ... and so do the live weights
        assert torch.equal(p, q)
    # the code instead of the window: the same file
    tr.save_mesh(str(tmp_path / "code.ply"), resolution=32, threshold=threshold, enc_a=enc_a.clone(), eye=eye)
    with torch.no_grad(), tr.ema_scope():
        code_v, code_t = mesh.extract_geometry(m, 32, threshold, enc_a, eye)
    again_v, again_t = mesh.read_ply(tmp_path / "code.ply")
    assert np.array_equal(again_t, code_t.cpu().numpy()) and ref.same_bits(again_v, code_v.cpu().numpy())
    with pytest.raises(ValueError):
        tr.save_mesh(str(tmp_path / "x.ply"), resolution=32, auds=auds, enc_a=enc_a, eye=eye)
    with pytest.raises(ValueError):
        tr.save_mesh(str(tmp_path / "x.ply"), resolution=32, eye=eye)
    with pytest.raises(ValueError):
        tr.save_mesh(str(tmp_path / "x.ply"), resolution=32, auds=auds)           # exp_eye without an eye value
    assert not (tmp_path / "x.ply").exists()
