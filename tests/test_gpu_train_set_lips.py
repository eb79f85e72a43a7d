"""rn_train_set_batch_rect / rn_train_set_batch_patch (csrc/rn_train_batch.hip) through DeviceTrainSet on the GPU: against the
reference loader's recorded lip fine-tuning batches (tests/golden/reference_batch_lips.npz) and, at the edges, against the class's
torch path.  Shapes are the fixture's 20 x 28 image (non-square: a swapped row / column shows) and 8 frames.  Bars: everything
bit-equal except rays_d (<= 2e-7) and poses (<= 1e-6), as tests/test_gpu_train_set.py has them for the same formulas."""
import numpy as np
import pytest
import torch

import lips_cases as lc
import train_set_cases as tc

pytestmark = pytest.mark.gpu

H, W = 20, 28


def _copy(d):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in d.items()}


def _same_batch(a, a_set, b, b_set, what):
    tc.compare_batches(a, b, what)
    tc.same_bits(a_set.inds, b_set.inds, f"{what} inds")
    assert a["_packed"].numel() == b["_packed"].numel() == 15 * a_set.inds.numel()


@pytest.mark.parametrize("tag,torso_mode,att,index", lc.rect_cases())
def test_rect_kernel_equals_the_reference_collate(hiplib, tag, torso_mode, att, index):
    ds = lc.make_set("cuda", torso_mode, att)
    assert ds.kernel == "hip"
    out = ds.batch_rect([index])
    lc.compare_with_golden(out, ds, tag, torso_mode)
    assert out["rect"] == tuple(lc.golden()["lips_rect"][index].tolist())
    oracle = ds.clone(kernel="torch")
    _same_batch(out, ds, oracle.batch_rect([index]), oracle, tag)


@pytest.mark.parametrize("tag,torso_mode,att,index", lc.patch_cases())
def test_patch_kernel_equals_the_reference_collate(hiplib, tag, torso_mode, att, index):
    g = lc.golden()
    corners = lc.corners_of(g[f"{tag}_inds"], 4, W)
    ds = lc.make_set("cuda", torso_mode, att)
    out = ds.batch_patch([index], 4, corners=corners)
    lc.compare_with_golden(out, ds, tag, torso_mode)
    oracle = ds.clone(kernel="torch")
    _same_batch(out, ds, oracle.batch_patch([index], 4, corners=corners), oracle, tag)
    ds.check()


# the image's border on every side; 1 x 1, 1 x w and h x 1; n = 255 and 256 at the edge of the 256-thread workgroup
RECTS = [(0, H, 0, W), (0, H, 20, W), (12, H, 0, 9), (19, 20, 27, 28), (0, 1, 0, 1), (7, 8, 3, 25), (2, 19, 11, 12),
         (1, 16, 4, 21), (2, 18, 5, 21), (0, 1, 0, 28), (0, H, 0, 1)]


@pytest.mark.parametrize("rect", RECTS)
@pytest.mark.parametrize("torso_mode", [False, True])
def test_rect_kernel_equals_the_torch_path_at_the_edges(hiplib, rect, torso_mode):
    n = (rect[1] - rect[0]) * (rect[3] - rect[2])
    assert {(r[1] - r[0]) * (r[3] - r[2]) for r in RECTS} >= {1, 255, 256, H * W}
    ds = lc.make_set("cuda", torso_mode, 2)
    oracle = ds.clone(kernel="torch")
    out = ds.batch_rect([6], rect=rect)
    _same_batch(out, ds, oracle.batch_rect([6], rect=rect), oracle, f"rect {rect}")
    rows, cols = np.meshgrid(np.arange(rect[0], rect[1]), np.arange(rect[2], rect[3]), indexing="ij")
    inds = (rows * W + cols).reshape(-1)
    tc.same_bits(ds.inds, inds, "ascending pixels, x along the rows")
    assert ds.inds.numel() == n and out["rect"] == rect
    # ... and the same pixels handed to the kernel's first instantiation as explicit inds
    plain = lc.make_set("cuda", torso_mode, 2)
    assert torch.equal(plain.batch([6], inds=inds)["_packed"], out["_packed"])


@pytest.mark.parametrize("n", [255, 256, 257])
def test_rect_kernel_at_the_workgroup_edge(hiplib, n):
    """257 is prime: a rect of 257 pixels is one row (or column) of an image at least that long, so this set is 5 x 300."""
    from types import SimpleNamespace
    from radnerf.dataset import DeviceTrainSet
    g, rng = lc.golden(), np.random.default_rng(31)
    h, w = 5, 300
    images, torso, bg = (rng.integers(0, 256, s, dtype=np.uint8) for s in ((8, h, w, 3), (8, h, w, 4), (h, w, 3)))
    ds = DeviceTrainSet(images, torso, bg, g["poses"], [310.0, 305.0, 150.0, 2.5], g["auds"], [[1, 5, 20, 270]] * 8, eye_area=g["eye_area"],
                        opt=SimpleNamespace(att=2, torso=False, exp_eye=True), device="cuda")
    oracle = ds.clone(kernel="torch")
    for rect in ((2, 3, 30, 30 + n), (4, 5, w - n, w)):
        out = ds.batch_rect([1], rect=rect)
        _same_batch(out, ds, oracle.batch_rect([1], rect=rect), oracle, f"n = {n}")
        tc.same_bits(ds.inds, np.arange(rect[0] * w + rect[2], rect[0] * w + rect[3]), "pixels")
        assert 0 < float(out["face_mask"].sum()) and out["face_mask"].shape == (1, n)
    if n == 257:                                                # ... and as a column: W = 5, H = 300
        tall = DeviceTrainSet(images.reshape(8, w, h, 3), torso.reshape(8, w, h, 4), bg.reshape(w, h, 3), g["poses"], [305.0, 310.0, 2.5, 150.0],
                              g["auds"], [[20, 270, 1, 5]] * 8, eye_area=g["eye_area"], opt=SimpleNamespace(att=2, torso=True, exp_eye=True),
                              device="cuda")
        oracle = tall.clone(kernel="torch")
        out = tall.batch_rect([1], rect=(43, 300, 4, 5))
        _same_batch(out, tall, oracle.batch_rect([1], rect=(43, 300, 4, 5)), oracle, "257 x 1")
        tc.same_bits(tall.inds, np.arange(43, 300) * h + 4, "pixels")


PATCHES = [(2, [[0, 0]]), (2, [[17, 25]]), (16, [[0, 0], [3, 11], [2, 5]]), (4, [[15, 23], [0, 23], [15, 0], [7, 9]]),
           (19, [[0, 8]]), (3, [[16, 24]] * 29)]        # the largest legal corners of every size; 29 * 9 = 261 rays: two workgroups


@pytest.mark.parametrize("ps,corners", PATCHES)
def test_patch_kernel_equals_the_torch_path_at_the_edges(hiplib, ps, corners):
    for torso_mode in (False, True):
        ds = lc.make_set("cuda", torso_mode, 1)
        oracle = ds.clone(kernel="torch")
        out = ds.batch_patch([3], ps, corners=corners)
        _same_batch(out, ds, oracle.batch_patch([3], ps, corners=corners), oracle, f"ps {ps}")
        o = np.arange(ps * ps)
        c = np.asarray(corners)
        want = ((c[:, :1] + o // ps) * W + c[:, 1:] + o % ps).reshape(-1)
        tc.same_bits(ds.inds, want, "patch pixels in 'ij' order")
        assert out["patch_size"] == ps and ds._draw == 0
        ds.check()


def test_out_of_range_corners_are_clamped_and_reported(hiplib):
    ds = lc.make_set("cuda", True, 2)
    clean = _copy(ds.batch_patch([4], 4, corners=[[0, 0], [15, 23], [15, 0], [7, 9], [0, 23]]))
    ds.check()
    out = ds.batch_patch([4], 4, corners=[[-1, -7], [16, 24], [2 ** 31 - 1, 0], [7, 9], [-2 ** 31, 2 ** 31 - 1]])
    assert torch.equal(out["_packed"], clean["_packed"])
    with pytest.raises(IndexError, match="4 pixel indices"):     # one count per corner, not per ray and not per coordinate
        ds.check()
    ds.check()
    oracle = ds.clone(kernel="torch")
    assert torch.equal(oracle.batch_patch([4], 4, corners=[[-1, -7], [16, 24], [99, 0], [7, 9], [-5, 99]])["_packed"][6 * 80:], clean["_packed"][6 * 80:])
    with pytest.raises(IndexError, match="4 pixel indices"):
        oracle.check()


@pytest.mark.parametrize("ps,num_rays", [(4, 64), (16, 768), (2, 1028)])
def test_drawn_corners(hiplib, ps, num_rays):
    """corners == NULL: the kernel's draw equals dataset.drawn_corners, and the draw counter advances once per call."""
    from radnerf.dataset import drawn_corners
    seed, P = 23, num_rays // (ps * ps)
    ds = lc.make_set("cuda", False, 2, num_rays=num_rays, seed=seed)
    oracle = ds.clone(kernel="torch")
    for draw in range(3):
        assert ds._draw == draw
        out = ds.batch_patch([draw], ps)
        want = drawn_corners(seed, draw, P, H, W, ps, "cuda")
        assert int(want[:, 0].max()) < H - ps and int(want[:, 1].max()) < W - ps
        tc.same_bits(ds.inds[::ps * ps], want[:, 0] * W + want[:, 1], f"draw {draw}")
        _same_batch(out, ds, oracle.batch_patch([draw], ps), oracle, f"self-drawn, draw {draw}")
    assert ds._draw == oracle._draw == 3
    again = lc.make_set("cuda", False, 2, num_rays=num_rays, seed=seed)
    again._draw = 2
    assert torch.equal(again.batch_patch([2], ps)["_packed"], out["_packed"])
    ds.check()


@pytest.mark.parametrize("att", [0, 1, 2])
def test_per_call_outputs_equal_those_of_batch(hiplib, att):
    ds, plain = lc.make_set("cuda", False, att), lc.make_set("cuda", False, att)
    for index in (0, 3, 7):                                     # the audio window pads on the left at 0 and 3, on the right at 7
        want = _copy(plain.batch([index]))
        for out in (ds.batch_rect([index]), ds.batch_patch([index], 4)):
            for k in ("poses", "poses_matrix", "eye", "auds"):
                tc.same_bits(out[k], want[k], f"att {att} index {index} {k}")
            assert out["index"] == want["index"]


def test_batch_and_frame_are_unchanged(hiplib):
    """The regression guard: the two earlier instantiations of the kernel against reference_batch.npz, after rect and patch calls
    on the same set."""
    g = tc.golden()
    for tag, torso_mode, att, index in tc.cases()[:4]:
        ds = tc.make_set("cuda", torso_mode, att)
        ds.batch_rect([index], rect=(1, 30, 2, 40))
        ds.batch_patch([index], 4, corners=[[0, 0]])
        tc.compare_with_golden(ds.batch([index], inds=g[f"{tag}_inds"]), tag, torso_mode)
    torso_mode, att, index = (int(v) for v in g["frame_case"])
    tc.compare_with_golden(tc.make_set("cuda", bool(torso_mode), att).frame(index), "frame", bool(torso_mode), training=False)
