"""Lip fine-tuning without a GPU: DeviceTrainSet.batch_rect / batch_patch on the torch path against the reference loader's
recorded batches (tests/golden/reference_batch_lips.npz), lips_rect_from_landmarks, the corner draw, the argument checks of
rn_train_set_batch_rect / rn_train_set_batch_patch through ctypes, and the patch term of train_step on the per-operator route."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import lips_cases as lc
import train_set_cases as tc


@pytest.fixture(scope="module")
def _pkg(hiplib):
    import radnerf.dataset as dataset
    return dataset


@pytest.mark.parametrize("tag,torso_mode,att,index", lc.rect_cases())
def test_rect_batch_equals_the_reference_collate(_pkg, tag, torso_mode, att, index):
    """collate with finetune_lips=True: every section, the per-call outputs and the pixel order, bit for bit."""
    g = lc.golden()
    ds = lc.make_set("cpu", torso_mode, att)
    out = ds.batch_rect([index])
    lc.compare_with_golden(out, ds, tag, torso_mode, exact=True)
    assert out["rect"] == tuple(g[f"{tag}_rect"].tolist()) == tuple(g["lips_rect"][index].tolist())
    n = int(g[f"{tag}_inds"].size)
    assert out["rays_o"].shape == (1, n, 3) and out["face_mask"].shape == (1, n) and out["_packed"].numel() == 15 * n
    assert "patch_size" not in out


@pytest.mark.parametrize("tag,torso_mode,att,index", lc.patch_cases())
def test_patch_batch_equals_the_reference_collate(_pkg, tag, torso_mode, att, index):
    """collate with patch_size=4, num_rays=64, the corners recovered from the recorded inds (every 16th entry)."""
    g = lc.golden()
    ps, W = int(g["shape"][5]), int(g["shape"][2])
    ds = lc.make_set("cpu", torso_mode, att)
    out = ds.batch_patch([index], ps, corners=lc.corners_of(g[f"{tag}_inds"], ps, W))
    lc.compare_with_golden(out, ds, tag, torso_mode, exact=True)
    assert out["patch_size"] == ps and "rect" not in out and out["rays_o"].shape == (1, 64, 3)
    ds.check()                                                  # the reference's corners are in range


def test_lips_rect_from_landmarks_equals_the_reference(_pkg):
    g = lc.golden()
    F, H, W = (int(v) for v in g["shape"][:3])
    assert _pkg.lips_rect_from_landmarks(g["lms"], H, W) == g["lips_rect"].tolist()
    assert _pkg.lips_rect_from_landmarks(g["lms"][2], H, W) == g["lips_rect"][2].tolist()
    lips = g["lips_rect"]
    assert (lips[:, 0] == 0).any() and (lips[:, 1] == H).any() and (lips[:, 2] == 0).any() and (lips[:, 3] == W).any()    # every clip


def test_drawn_corners(_pkg):
    """In randint's ranges [0, H - ps) x [0, W - ps), a function of (seed, draw, q) alone, and pinned by literals computed once
    from this Python mirror (the GPU suite holds the kernel to the mirror)."""
    H, W = 20, 28
    for ps in (4, 16):
        c = _pkg.drawn_corners(11, 2, 4096, H, W, ps, "cpu")
        assert c.shape == (4096, 2) and c.dtype == torch.int64
        assert int(c[:, 0].min()) == 0 and int(c[:, 0].max()) == H - ps - 1      # the last start position is never drawn
        assert int(c[:, 1].min()) == 0 and int(c[:, 1].max()) == W - ps - 1
        assert torch.equal(_pkg.drawn_corners(11, 2, 100, H, W, ps, "cpu"), c[:100])        # q alone picks the element
        assert not torch.equal(_pkg.drawn_corners(11, 3, 4096, H, W, ps, "cpu"), c)
        assert not torch.equal(_pkg.drawn_corners(12, 2, 4096, H, W, ps, "cpu"), c)
    assert _pkg.drawn_corners(7, 3, 5, H, W, 4, "cpu").tolist() == [[6, 17], [3, 7], [6, 20], [14, 4], [14, 8]]
    assert _pkg.drawn_corners(7, 3, 3, H, W, 16, "cpu").tolist() == [[1, 8], [0, 3], [1, 10]]
    assert _pkg.drawn_corners(0, 0, 4, H, W, 4, "cpu").tolist() == [[0, 3], [5, 16], [15, 7], [9, 17]]
    # x0 is element 2q, y0 element 2q + 1 of the pixel draw's hash, multiply-high onto the range
    h = lambda k: int(_pkg._mix32(_pkg._mix32(_pkg._mix32(torch.tensor(k)) ^ 3) ^ 7))
    assert [[(h(2 * q) * 16) >> 32, (h(2 * q + 1) * 24) >> 32] for q in range(5)] == _pkg.drawn_corners(7, 3, 5, H, W, 4, "cpu").tolist()


def test_self_drawn_patches_on_the_torch_path(_pkg):
    ds = lc.make_set("cpu", False, 2, seed=7)
    ds._draw = 3
    out = ds.batch_patch([1], 4)
    first, picked = out["_packed"].clone(), ds.inds.clone()
    assert ds._draw == 4                                        # advanced once
    corners = _pkg.drawn_corners(7, 3, 4, 20, 28, 4, "cpu")
    assert torch.equal(picked[::16], corners[:, 0] * 28 + corners[:, 1])
    assert torch.equal(ds.batch_patch([1], 4, corners=corners)["_packed"], first) and ds._draw == 4     # explicit corners draw nothing
    assert not torch.equal(ds.batch_patch([1], 4)["_packed"], first)


@pytest.mark.parametrize("rect", [(3, 9, 5, 12), (0, 20, 0, 28), (19, 20, 27, 28), (4, 5, 2, 20), (2, 17, 6, 7)])
def test_rect_batch_equals_the_same_pixels_as_explicit_inds(_pkg, rect):
    ds, other = lc.make_set("cpu", True, 1), lc.make_set("cpu", True, 1)
    xmin, xmax, ymin, ymax = rect
    out = ds.batch_rect([4], rect=rect)
    inds = (np.arange(xmin, xmax)[:, None] * 28 + np.arange(ymin, ymax)[None, :]).reshape(-1)
    want = other.batch([4], inds=inds)
    assert torch.equal(out["_packed"], want["_packed"]) and torch.equal(ds.inds, other.inds)
    tc.compare_batches(out, want, f"rect {rect}")
    assert out["rect"] == rect


def test_rect_sizes_share_one_buffer(_pkg):
    """Rect sizes differ per frame: the views of every call lie in ONE buffer allocated at the largest lips rect of the set."""
    g = lc.golden()
    ds = lc.make_set("cpu", False, 2)
    largest = int(max((r[1] - r[0]) * (r[3] - r[2]) for r in g["lips_rect"]))
    ptrs = set()
    for f in range(8):
        out = ds.batch_rect([f])
        ptrs.add(out["_packed"].data_ptr())
        assert ds._rect_buf[1].numel() == largest and ds.inds.numel() == out["_packed"].numel() // 15
    assert len(ptrs) == 1 and not ds._bufs
    big = ds.batch_rect([0], rect=(0, 20, 0, 28))               # larger than any lips rect: replaced once
    assert big["_packed"].numel() == 15 * 560 and ds._rect_buf[1].numel() == 560
    assert ds.clone().lips_rect == g["lips_rect"].tolist()      # clone carries the rects


def test_python_side_refusals(_pkg):
    ds = lc.make_set("cpu", False, 2)
    for rect in ((5, 5, 2, 9), (6, 5, 2, 9), (2, 9, 7, 7), (-1, 4, 0, 4), (0, 21, 0, 4), (0, 4, 0, 29), (0, 4, -2, 4)):
        with pytest.raises(ValueError, match="empty or outside"):
            ds.batch_rect([0], rect=rect)
    with pytest.raises(ValueError, match="no lips_rect"):
        lc.make_set("cpu", False, 2, lips=False).batch_rect([0])
    with pytest.raises(ValueError, match="multiple of patch_size"):
        lc.make_set("cpu", False, 2, num_rays=65).batch_patch([0], 4)           # main.py:125
    with pytest.raises(ValueError, match="multiple of patch_size"):
        lc.make_set("cpu", False, 2, num_rays=64).batch_patch([0], 3)
    for ps in (1, 20, 28):
        with pytest.raises(ValueError, match="patch_size < min"):
            ds.batch_patch([0], ps)
    with pytest.raises(ValueError, match="empty or outside"):         # a lips rect that leaves the image is refused at once
        _pkg.DeviceTrainSet(*(lc.golden()[k] for k in ("images", "torso", "bg", "poses", "intrinsics", "auds", "face_rect")),
                            eye_area=lc.golden()["eye_area"], opt=types.SimpleNamespace(att=0, torso=False, exp_eye=True), device="cpu",
                            lips_rect=[[0, 30, 0, 4]] * 8)


def test_out_of_range_corners_are_clamped_and_reported(_pkg):
    ds = lc.make_set("cpu", False, 0)
    clean = ds.batch_patch([2], 4, corners=[[0, 0], [15, 23], [15, 0], [7, 9]])["_packed"].clone()      # 15 / 23: the largest legal
    ds.check()
    out = ds.batch_patch([2], 4, corners=[[-3, -1], [16, 24], [99, 0], [7, 9]])
    assert torch.equal(out["_packed"], clean)
    with pytest.raises(IndexError, match="3 pixel indices"):
        ds.check()
    ds.check()


def test_entry_points_refuse_bad_arguments(hiplib):
    """As tests/test_train_set_host.py does for rn_train_set_batch: refused on the host with RN_ERR_INVALID_ARG and a message,
    before anything touches a GPU.  Host memory stands in for the device buffers: every call below is one the library refuses."""
    from radnerf_hip import abi
    lib, err = hiplib._lib, hiplib.last_error
    buf = (C.c_float * 64)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)
    odd = C.c_void_p(p.value + 4)

    def desc(**kw):
        d = abi.TrainSetT(images=p, torso=p, bg=p, poses=p, face_rect=p, eye=p, auds=p, fx=30.0, fy=30.0, cx=14.0, cy=10.0, H=20, W=28,
                          F=8, Fa=8, C=5, att=2, torso_mode=0)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def rect(r=(2, 6, 3, 9), d=desc(), frame=0, aud=0, **null):
        a = dict(packed=p, poses6=p, pose_matrix=p, auds_out=p)
        a.update(null)
        return lib.rn_train_set_batch_rect(C.byref(d) if d is not None else None, frame, aud, *r, a["packed"], None, a["poses6"],
                                           a["pose_matrix"], None, a["auds_out"], None)

    def patch(P=4, ps=4, d=desc(), frame=0, aud=0, **null):
        a = dict(packed=p, poses6=p, pose_matrix=p, auds_out=p, bad=p)
        a.update(null)
        return lib.rn_train_set_batch_patch(C.byref(d) if d is not None else None, frame, aud, None, P, ps, 0, 0, a["packed"], None,
                                            a["poses6"], a["pose_matrix"], None, a["auds_out"], a["bad"], None)

    for r in ((5, 5, 2, 9), (6, 5, 2, 9), (2, 9, 7, 7), (2, 9, 8, 7), (-1, 4, 0, 4), (0, 4, -1, 4)):        # empty / negative
        assert rect(r) == -1 and "empty or outside" in err(), r
    assert rect((0, 21, 0, 4)) == -1 and "empty or outside the 20 x 28 image" in err()                     # past H
    assert rect((0, 4, 0, 29)) == -1 and "empty or outside" in err()                                       # past W
    assert patch(ps=20) == -1 and "patch < H" in err()                                                      # patch >= H
    assert patch(ps=21) == -1 and patch(ps=1) == -1 and "2 <= patch" in err()
    assert patch(ps=28, d=desc(H=40)) == -1 and patch(ps=30, d=desc(H=40)) == -1 and "patch < W" in err()   # patch >= W
    assert patch(P=0) == -1 and "P >= 1" in err()
    assert patch(P=1 << 27, ps=4) == -1 and "2^31" in err()
    for call in (rect, patch):
        assert call(d=None) == -1 and "null descriptor" in err()
        assert call(d=desc(images=None)) == -1 and "null pointer" in err()
        assert call(frame=8) == -1 and "frame 8 is outside the 8 frames" in err()
        assert call(aud=8) == -1 and "audio frame 8" in err()
        for name in ("packed", "poses6", "pose_matrix", "auds_out"):
            assert call(**{name: None}) == -1 and "null pointer" in err(), name
        assert call(packed=odd) == -1 and "8-byte aligned" in err()
    assert patch(bad=None) == -1 and "null pointer" in err()
    assert lib.rn_train_head_loss_chain(None, None, None, 3, None, 0, None, None, None, None, None) == -1 and "N must be" in err()
    assert lib.rn_train_head_loss_chain(None, None, None, 3, None, 35, None, None, None, None, None) == -1 and "null pointer" in err()


# ------------------------------------------------------------------------------------------------------------- the step
class _Stub(torch.nn.Module):
    """A stand-in model: render() hands back fixed outputs scaled by one parameter (tests/test_train_host.py's)."""

    def __init__(self, out):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(1))
        self.out, self.kwargs = out, None

    def render(self, *a, **kw):
        self.kwargs = kw
        return {k: v * self.w for k, v in self.out.items()}

    def get_params(self, lr, lr_net, wd=0):
        return [{"params": [self.w], "lr": lr_net}]


def _criterion(pred, target):
    """A stand-in perceptual function with LPIPS's output shape [P,1,1,1]; it weighs rows, columns and channels differently, so a
    wrong view of the rays shows."""
    P, _, h, w = pred.shape
    ramp = (1 + torch.arange(h).view(1, 1, h, 1)) * (1 + 0.5 * torch.arange(w).view(1, 1, 1, w)) * torch.tensor([1.0, 2.0, 3.0]).view(1, 3, 1, 1)
    return ((pred - target).abs() * ramp).mean(dim=(1, 2, 3), keepdim=True)


def _step_inputs(N, seed):
    g = torch.Generator().manual_seed(seed)
    out = dict(image=torch.rand(1, N, 3, generator=g), weights_sum=torch.rand(N, generator=g), ambient=torch.rand(N, generator=g))
    data = dict(rays_o=None, rays_d=None, auds=None, bg_coords=None, poses=None, eye=None, index=[0], bg_color=None,
                images=torch.rand(1, N, 3, generator=g), face_mask=torch.rand(1, N, generator=g) > 0.5)
    return out, data


def _plain_loss(out, data, w_amb):
    from radnerf.train import entropy_of
    mse = ((out["image"] - data["images"]) ** 2).mean(-1).mean()
    return mse + 1e-4 * entropy_of(out["weights_sum"]).mean() + w_amb * (out["ambient"] * (~data["face_mask"].view(-1))).mean()


@pytest.mark.parametrize("kind", ["rect", "patch"])
def test_train_step_adds_the_patch_term(_pkg, kind):
    """loss = (the plain loss) + w * criterion(views).mean(): w = 0.01 on ONE [1,3,h,w] view of a rect batch, 0.001 on [P,3,ps,ps]
    views of a patch batch, which also marches all rays (nerf/utils.py:741, 757-783)."""
    from radnerf import train as tr
    opt = types.SimpleNamespace(torso=False, dt_gamma=1 / 256, max_steps=16)
    if kind == "rect":
        N, extra, weight, shape = 35, dict(rect=(3, 8, 2, 9)), 0.01, (1, 5, 7)
    else:
        N, extra, weight, shape = 48, dict(patch_size=4), 0.001, (3, 4, 4)
    out, data = _step_inputs(N, 3)
    data.update(extra)
    m = _Stub(out)
    pred, rgb, loss = tr.train_step(m, data, opt, global_step=50000, patch_criterion=_criterion)
    assert m.kwargs["force_all_rays"] is (kind == "patch")
    nchw = lambda t: t.reshape(*shape, 3).permute(0, 3, 1, 2)
    term = _criterion(nchw(out["image"]), nchw(data["images"]))
    assert term.shape == (shape[0], 1, 1, 1)
    plain = _plain_loss(out, data, 0.025)
    assert abs(float(loss.detach()) - float(plain + weight * term.mean())) < 1e-6 and float(weight * term.mean()) > 1e-4
    # the reference's own expression: the [P,1,1,1] term broadcast onto the [B,N] squared errors, then the mean
    mse = ((out["image"] - data["images"]) ** 2).mean(-1)
    assert (mse + weight * term).shape == (shape[0], 1, 1, N)
    assert abs(float((mse + weight * term).mean()) - float(mse.mean() + weight * term.mean())) < 1e-6
    loss.backward()
    assert m.w.grad is not None and torch.isfinite(m.w.grad).all()
    # no criterion: trained as a plain batch -- a patch batch still marches all rays
    m2 = _Stub(out)
    _, _, loss2 = tr.train_step(m2, data, opt, global_step=50000)
    assert abs(float(loss2.detach()) - float(plain)) < 1e-6 and m2.kwargs["force_all_rays"] is (kind == "patch")


def test_train_step_refuses_views_that_do_not_fit(_pkg):
    from radnerf import train as tr
    opt = types.SimpleNamespace(torso=False, dt_gamma=1 / 256, max_steps=16)
    out, data = _step_inputs(35, 3)
    with pytest.raises(ValueError, match="does not hold"):
        tr.train_step(_Stub(out), dict(data, rect=(3, 8, 2, 8)), opt, patch_criterion=_criterion)
    with pytest.raises(ValueError, match="no multiple"):
        tr.train_step(_Stub(out), dict(data, patch_size=4), opt, patch_criterion=_criterion)
    with pytest.raises(ValueError, match="not both"):
        tr.train_step(_Stub(out), dict(data, rect=(3, 8, 2, 9), patch_size=4), opt)


def test_lips_schedule_alternates(_pkg):
    """nerf/utils.py:769-770: the rect on even steps, random pixels on odd ones."""
    from radnerf.train import lips_schedule
    ds = lc.make_set("cpu", False, 2)
    for step in range(4):
        b = lips_schedule(ds, [step], step)
        assert ("rect" in b) == (step % 2 == 0)
        assert b["rays_o"].shape[1] == ((lambda r: (r[1] - r[0]) * (r[3] - r[2]))(ds.lips_rect[step]) if step % 2 == 0 else 64)


def test_graphed_trainer_refuses_a_lips_batch(_pkg):
    from radnerf.train import GraphedTrainer, Trainer
    out, data = _step_inputs(35, 3)
    opt = types.SimpleNamespace(torso=False, dt_gamma=1 / 256, max_steps=16)
    t = GraphedTrainer(_Stub(out), opt, prefer_rocblas=False)
    for extra in (dict(rect=(3, 8, 2, 9)), dict(patch_size=4)):
        with pytest.raises(ValueError, match="lip fine-tuning batch"):
            t.step(dict(data, **extra))
    assert t.global_step == 0
    assert Trainer(_Stub(out), opt, prefer_rocblas=False, patch_criterion=_criterion).patch_criterion is _criterion
    # a trainer assembled without __init__ around another one's state (the benchmark's eager probe) has no criterion
    assert Trainer.__new__(Trainer).patch_criterion is None and GraphedTrainer.__new__(GraphedTrainer).patch_criterion is None
