"""The file loaders in front of the device routes: a DeviceTrainSet built from a dataset directory hands out bit-identical batches
through the same kernel as one built from the same arrays, and ClipScene feeds model.render exactly what a hand-assembled frame
from the reference loader's recorded clip fields (tests/golden/reference_dataset.npz) does.  The directory is tests/dataset_dir.py's
20 x 16 one, decoded through its .npy hook; nothing here adds a kernel -- these are the existing launches behind new host code."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dataset_dir as dd  # noqa: E402


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "reference_dataset.npz"))


@pytest.fixture(scope="module")
def root(tmp_path_factory, gold):
    path = str(tmp_path_factory.mktemp("dataset"))
    dd.write_dataset(path, int(gold["seed"]))
    return path


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def test_from_directory_batches_equal_the_set_built_from_the_arrays(hiplib, root):
    """batch (explicit and drawn pixels), batch_rect, batch_patch and frame at frames 0, 13 and the mirrored index 26 (the audio
    file has 30 rows, the set 24 frames: 26 -> frame 21, audio row 26)."""
    from radnerf import datafiles
    from radnerf.dataset import DeviceTrainSet
    opt = dd.dataset_opt(root, finetune_lips=True, aud=os.path.join(root, "clip_aud.npy"))
    ds = DeviceTrainSet.from_directory(root, opt, "train", num_rays=256, seed=5, device="cuda", decode=dd.npy_decode, kernel="hip")
    d = datafiles.load_split(root, opt, "train", decode=dd.npy_decode)
    hand = DeviceTrainSet(d.images, d.torso, d.bg, d.poses, d.intrinsics, d.auds, d.face_rect, eye_area=d.eye_area, opt=opt, num_rays=256,
                          seed=5, device="cuda", kernel="hip", lips_rect=d.lips_rect)
    assert ds.kernel == "hip" and ds.F == dd.N_TRAIN and ds.auds.shape[0] == dd.N_AUD and ds.mirror_index(26) == 21
    inds = torch.tensor([0, dd.W - 1, dd.W, 137, 137, dd.H * dd.W - 1], device="cuda")
    small = ("poses", "poses_matrix", "eye", "auds")
    for i in (0, 13, 26):
        for call in (lambda s: s.batch([i], inds=inds), lambda s: s.batch([i]), lambda s: s.batch_rect([i]),
                     lambda s: s.batch_patch([i], 4)):
            a, b = call(ds), call(hand)
            assert a["index"] == b["index"] == [ds.mirror_index(i)]
            assert _bits_equal(a["_packed"], b["_packed"]) and torch.equal(ds.inds, hand.inds)
            assert all(_bits_equal(a[k], b[k]) for k in small)
            assert a.get("rect") == b.get("rect")
        a, b = ds.frame(i), hand.frame(i)
        for k in ("rays_o", "rays_d", "bg_coords", "bg_color", "images") + small:
            assert _bits_equal(a[k], b[k]), (i, k)
        assert a["index"] == b["index"]
    ds.check()
    hand.check()
    # and the frame's target really is the file's pixels
    want = torch.from_numpy(d.images[21].astype(np.float32) / np.float32(255)).cuda()
    assert torch.equal(ds.frame(26)["images"][0], want)


@pytest.fixture(scope="module")
def clip_setup(root, gold):
    """A synthetic-state model on the fused engine, the ClipScene over the directory's pose and audio files, and the golden clip
    fields on the device."""
    from radnerf import fused
    from radnerf.clip import ClipScene
    from radnerf.scene import SyntheticScene
    opt = dd.dataset_opt(root, engine="fused", pose=os.path.join(root, "clip.json"), aud=os.path.join(root, "clip_aud.npy"),
                         bg_img=os.path.join(root, "bc.jpg"), smooth_path=True, smooth_eye=True)
    model = SyntheticScene(H=dd.H, W=dd.W, n_frames=8, device="cuda", opt=opt).model
    scene = ClipScene.from_files(model, opt, "cuda", decode=dd.npy_decode)
    g = {k: torch.from_numpy(gold[f"clip_{k}"]).cuda() for k in ("poses", "auds", "eye_area")}
    g["poses6"] = fused.convert_poses(g["poses"])
    g["bg_coords"] = fused.get_bg_coords(dd.H, dd.W, torch.device("cuda"))
    g["bg_color"] = torch.from_numpy((gold["clip_bg"].astype(np.float32) / np.float32(255)).reshape(1, dd.H * dd.W, 3)).cuda()
    g["intrinsics"] = gold["clip_intrinsics"].astype(np.float32)
    return scene, g


def _by_hand(scene, g, i, eye=None):
    """model.render on frame i of the clip assembled from the golden fields: the audio window around i itself, pose and eye at the
    mirrored index, individual code 0, the file's background."""
    from radnerf.dataset import mirror_index
    from radnerf.rays import get_audio_features
    n_poses = g["poses"].shape[0]
    p = mirror_index(i, n_poses)
    rays_o, rays_d = (torch.empty(1, dd.H * dd.W, 3, device="cuda") for _ in range(2))
    return scene.model.render(rays_o, rays_d, get_audio_features(g["auds"], scene.opt.att, i), g["bg_coords"], g["poses6"][p:p + 1],
                              eye=g["eye_area"][p:p + 1] if eye is None else eye, index=0, bg_color=g["bg_color"], want_u8=True,
                              ray_source=(g["poses"][p], g["intrinsics"], dd.W), **scene.render_kwargs())


@pytest.mark.parametrize("i", [0, dd.N_AUD - 1, 15])
def test_clip_scene_renders_the_hand_assembled_frame(hiplib, clip_setup, i):
    """Frame 0 and the last frame (the audio window pads at either end), and 15 >= n_poses = 11 (mirrored to pose 6)."""
    scene, g = clip_setup
    assert scene.n_frames == dd.N_AUD and scene.n_poses == dd.N_CLIP_POSES and (scene.H, scene.W) == (dd.H, dd.W)
    with torch.no_grad():
        scene.model.enc_a = None
        got = scene.render(i, want_u8=True)
        got = {k: got[k].clone() for k in ("image", "image_u8", "depth")}
        scene.model.enc_a = None
        want = _by_hand(scene, g, i)
    f = scene.frame(i, lazy_rays=True)
    assert "ray_source" in f and f["index"] == 0 and f["bg_color"].shape == (1, dd.H * dd.W, 3) and f["bg_color"].dtype == torch.float32
    for k in ("image", "image_u8", "depth"):
        assert _bits_equal(got[k], want[k]), k
    assert got["image_u8"].dtype == torch.uint8 and int(got["image_u8"].max()) > 0


def test_clip_scene_fix_eye_and_no_eye(hiplib, clip_setup, root):
    import copy
    from radnerf.clip import ClipScene
    from radnerf.datafiles import load_clip
    scene, g = clip_setup
    opt = copy.copy(scene.opt)
    opt.fix_eye = 0.17
    fixed = ClipScene(scene.model, load_clip(opt, decode=dd.npy_decode), opt, "cuda")
    eye = torch.full((1, 1), 0.17, device="cuda")
    with torch.no_grad():
        scene.model.enc_a = None
        got = fixed.render(4, want_u8=True)["image"].clone()
        scene.model.enc_a = None
        want = _by_hand(scene, g, 4, eye=eye)["image"]
        scene.model.enc_a = None
        per_frame = scene.render(4, want_u8=True)["image"]
    assert _bits_equal(got, want) and not torch.equal(got, per_frame)
    assert torch.equal(fixed.eye, eye) and torch.equal(fixed.frame(3)["eye"], eye)
    with pytest.raises(AttributeError, match="per-frame eye"):
        scene.eye
    opt2 = copy.copy(scene.opt)
    opt2.exp_eye = False
    assert ClipScene(scene.model, load_clip(opt2, decode=dd.npy_decode), opt2, "cuda").frame(0)["eye"] is None


def test_frame_parallel_renderer_over_a_clip_equals_sequential_renders(hiplib, clip_setup):
    from radnerf.parallel import FrameParallelRenderer
    scene, _ = clip_setup
    m = scene.model
    assert m.smooth_lips
    with torch.no_grad():
        m.enc_a = None
        want = [scene.render(i, want_u8=True)["image_u8"].reshape(dd.H, dd.W, 3).clone() for i in range(10)]
        m.enc_a = None
        r = FrameParallelRenderer(scene, rank=0, world=1)
        got = [r.step(s).clone() for s in range(10)]
        r.finish()
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert any(not torch.equal(want[0], w) for w in want[1:])
