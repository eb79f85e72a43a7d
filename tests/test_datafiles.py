"""radnerf/datafiles.py (load_split, load_clip) and DeviceTrainSet.from_directory against the reference's own loader: every field
that tests/golden/reference_dataset.npz records (tests/golden/make_golden_dataset.py ran NeRFDataset / NeRFDataset_Test on the
directory tests/dataset_dir.py writes) must come back exactly -- integers, uint8 and float32 bit for bit, the float64 intrinsics
to the last bit.  Host only; needs an image decoder (PIL or cv2) and nothing else."""
import os
import sys

import numpy as np
import pytest
import torch

try:
    import cv2  # noqa: F401
except ImportError:
    pytest.importorskip("PIL")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dataset_dir as dd  # noqa: E402

from radnerf import datafiles  # noqa: E402
from radnerf.dataset import DeviceTrainSet, lips_rect_from_landmarks  # noqa: E402

SPLITS = {"train": ("train", {}), "part": ("train", dict(part=True)), "range": ("train", dict(data_range=[2, 17])),
          "val": ("val", {}), "trainval": ("trainval", {}), "smooth": ("train", dict(smooth_eye=True))}


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "reference_dataset.npz"))


@pytest.fixture(scope="module")
def root(tmp_path_factory, gold):
    path = str(tmp_path_factory.mktemp("dataset"))
    dd.write_dataset(path, int(gold["seed"]))
    return path


@pytest.fixture(scope="module")
def loaded(root):
    """Every split loaded once (the default decoder), shared and left unchanged."""
    return {tag: datafiles.load_split(root, dd.dataset_opt(root, finetune_lips=True, **kw), split) for tag, (split, kw) in SPLITS.items()}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("tag", list(SPLITS))
def test_split_equals_the_reference_loader(gold, loaded, tag):
    d = loaded[tag]
    H, W, F = (int(v) for v in gold[f"{tag}_shape"])
    assert (d.H, d.W, d.F) == (H, W, F) and (H, W) == (dd.H, dd.W)
    assert d.poses.dtype == np.float32 and same_bits(d.poses, gold[f"{tag}_poses"])
    if tag != "smooth":
        assert d.auds.dtype == np.float32 and same_bits(d.auds, gold[f"{tag}_auds"])
    assert same_bits(d.face_rect, gold[f"{tag}_face_rect"]) and same_bits(d.lips_rect, gold[f"{tag}_lips_rect"])
    assert d.eye_area.dtype == np.float32 and same_bits(d.eye_area, gold[f"{tag}_eye_area"])
    assert d.intrinsics.dtype == np.float64 and same_bits(d.intrinsics, gold[f"{tag}_intrinsics"])
    assert d.radius == float(gold[f"{tag}_radius"])
    assert d.bg.dtype == np.uint8 and same_bits(d.bg, gold[f"{tag}_bg"])
    assert d.images.dtype == np.uint8 and d.images.shape == (F, H, W, 3) and d.torso.shape == (F, H, W, 4)
    for f in (0, 13):
        if f"{tag}_image{f}" in gold.files:
            assert same_bits(d.images[f], gold[f"{tag}_image{f}"]) and same_bits(d.torso[f], gold[f"{tag}_torso{f}"])
    assert d.has_gt


def test_what_the_splits_exercise(gold, loaded, root):
    """The skip, --part's stride, the slice, val's cap, the audio clamp, and the raw eye areas under the smoothed ones."""
    train = loaded["train"]
    ids = [100 + f for f in range(dd.N_TRAIN_LISTED) if f != dd.MISSING]
    assert train.frame_ids == ids and train.F == dd.N_TRAIN
    assert loaded["part"].frame_ids == [100, 110, 120]
    assert loaded["range"].frame_ids == [100 + f for f in range(2, 17) if f != dd.MISSING]
    assert loaded["val"].frame_ids == [100 + dd.N_TRAIN_LISTED + f for f in range(dd.N_VAL)]
    assert loaded["trainval"].frame_ids == ids + loaded["val"].frame_ids
    aud = np.load(os.path.join(root, "aud_eo.npy")).transpose(0, 2, 1)
    assert same_bits(loaded["val"].auds[-1], aud[dd.N_AUD - 1]) and dd.N_TRAIN_LISTED + dd.N_VAL - 1 > dd.N_AUD - 1     # the clamp
    assert same_bits(loaded["smooth"].eye_area_raw, loaded["train"].eye_area)
    assert not same_bits(loaded["smooth"].eye_area, loaded["train"].eye_area)
    assert same_bits(datafiles.smooth_eye(loaded["train"].eye_area[:, 0]), loaded["smooth"].eye_area[:, 0])
    assert dd.H != dd.W


def test_lips_rect_from_landmarks_agrees_with_the_loader(loaded):
    d = loaded["train"]
    assert d.landmarks.shape == (d.F, 68, 2)
    assert np.array_equal(np.array(lips_rect_from_landmarks(d.landmarks, d.H, d.W), dtype=np.int32), d.lips_rect)
    assert (d.lips_rect[:, 0] == 0).any() and (d.lips_rect[:, 1] == d.H).any() and (d.lips_rect[:, 2] == 0).any() and \
        (d.lips_rect[:, 3] == d.W).any()


@pytest.mark.parametrize("tag,kw", [("clip", dict(smooth_path=True, smooth_eye=True)), ("clipraw", {})])
def test_clip_equals_the_reference_loader(gold, root, tag, kw):
    opt = dd.dataset_opt(root, pose=os.path.join(root, "clip.json"), aud=os.path.join(root, "clip_aud.npy"),
                         bg_img=os.path.join(root, "bc.jpg"), **kw)
    c = datafiles.load_clip(opt)
    H, W, N = (int(v) for v in gold[f"{tag}_shape"])
    assert (c.H, c.W, c.poses.shape[0]) == (H, W, N) and N == dd.N_CLIP_POSES
    assert c.poses.dtype == np.float32
    print(f"{tag}: max |poses - reference| = {np.abs(c.poses - gold[f'{tag}_poses']).max():.3e}")
    assert same_bits(c.poses, gold[f"{tag}_poses"])
    if tag == "clip":
        assert same_bits(c.auds, gold["clip_auds"]) and c.auds.shape == (dd.N_AUD, dd.AUD_K, 16)
    assert c.eye_area.dtype == np.float32 and same_bits(c.eye_area, gold[f"{tag}_eye_area"])
    assert same_bits(c.bg, gold[f"{tag}_bg"])
    assert c.intrinsics.dtype == np.float64 and same_bits(c.intrinsics, gold[f"{tag}_intrinsics"])


def test_clip_without_aud_uses_the_frames_aud_ids(root):
    opt = dd.dataset_opt(root, pose=os.path.join(root, "clip.json"), bg_img="white")
    c = datafiles.load_clip(opt)
    aud = np.load(os.path.join(root, "aud_eo.npy")).transpose(0, 2, 1)
    assert same_bits(c.auds, aud[:dd.N_CLIP_POSES]) and (c.bg == 255).all()
    assert c.eye_area[2, 0] == np.float32(0.25)                       # a frame without eye_ratio


def test_background_choices(root, loaded):
    white = datafiles.load_split(root, dd.dataset_opt(root, bg_img="white"), "val")
    black = datafiles.load_split(root, dd.dataset_opt(root, bg_img="black"), "val")
    named = datafiles.load_split(root, dd.dataset_opt(root, bg_img=os.path.join(root, "bc.jpg")), "val")
    assert (white.bg == 255).all() and (black.bg == 0).all() and same_bits(named.bg, loaded["val"].bg)
    big = dd.npy_decode(os.path.join(root, "bc.jpg"))
    assert big.shape == (2 * dd.H, 2 * dd.W, 3)
    want = big.astype(np.int32).reshape(dd.H, 2, dd.W, 2, 3).sum(axis=(1, 3))
    assert (want % 4 == 0).all() and np.array_equal(named.bg, want // 4)          # the area mean, exact


def test_a_real_jpeg_decodes_in_rgb_order(tmp_path):
    from PIL import Image
    red = np.zeros((12, 9, 3), dtype=np.uint8)
    red[..., 0] = 250
    path = str(tmp_path / "red.jpg")
    Image.fromarray(red).save(path, format="JPEG", quality=95)
    img = datafiles.default_decoder()(path)
    assert img.dtype == np.uint8 and img.shape == (12, 9, 3)
    assert img[..., 0].min() > 230 and img[..., 1].max() < 25 and img[..., 2].max() < 25
    rgba = np.zeros((5, 7, 4), dtype=np.uint8)
    rgba[..., 2], rgba[..., 3] = 200, 77
    path = str(tmp_path / "blue.png")
    Image.fromarray(rgba).save(path)
    assert np.array_equal(datafiles.default_decoder()(path), rgba)


def _rewrite_head(root, tmp_path, head):
    import json
    import shutil
    new = str(tmp_path / "d")
    shutil.copytree(root, new)
    for name in ("transforms_train.json", "transforms_val.json"):
        with open(os.path.join(new, name)) as fh:
            t = json.load(fh)
        with open(os.path.join(new, name), "w") as fh:
            json.dump(dict(head, frames=t["frames"]), fh)
    return new


def test_the_three_intrinsics_branches(root, tmp_path, loaded):
    assert np.array_equal(loaded["val"].intrinsics, np.array([loaded["val"].intrinsics[0]] * 2 + [dd.CX, dd.CY]))      # focal_len
    new = _rewrite_head(root, tmp_path, dict(fl_y=61.0, h=2 * dd.H, w=2 * dd.W, cx=17.0, cy=21.0))
    d = datafiles.load_split(new, dd.dataset_opt(new), "val", downscale=2)
    assert (d.H, d.W) == (dd.H, dd.W) and np.array_equal(d.intrinsics, np.array([30.5, 30.5, 8.5, 10.5]))
    new2 = _rewrite_head(root, tmp_path / "x", dict(fl_x=40.0, fl_y=44.0, h=dd.H, w=dd.W))
    d = datafiles.load_split(new2, dd.dataset_opt(new2), "val")
    assert np.array_equal(d.intrinsics, np.array([40.0, 44.0, dd.W / 2, dd.H / 2]))
    new3 = _rewrite_head(root, tmp_path / "y", dict(camera_angle_x=0.7, h=dd.H, w=dd.W))
    d = datafiles.load_split(new3, dd.dataset_opt(new3), "val")
    f = dd.W / (2 * np.tan(0.7 / 2))
    assert np.array_equal(d.intrinsics, np.array([f, f, dd.W / 2, dd.H / 2]))
    new4 = _rewrite_head(root, tmp_path / "z", dict(h=dd.H, w=dd.W))
    with pytest.raises(RuntimeError, match="focal"):
        datafiles.load_split(new4, dd.dataset_opt(new4), "val")


def test_a_missing_image_is_one_warning_line(root, capsys):
    datafiles.load_split(root, dd.dataset_opt(root), "train")
    lines = [ln for ln in capsys.readouterr().out.splitlines() if "NOT FOUND" in ln]
    assert len(lines) == 1 and f"{100 + dd.MISSING}.jpg" in lines[0] and lines[0].startswith("[WARN]")


def test_emb_and_label_arrays_are_refused(root, tmp_path):
    with pytest.raises(NotImplementedError, match="--emb"):
        datafiles.load_split(root, dd.dataset_opt(root, emb=True), "val")
    labels = str(tmp_path / "labels.npy")
    np.save(labels, np.zeros((30, 16), dtype=np.int64))
    with pytest.raises(NotImplementedError, match="--emb"):
        datafiles.load_split(root, dd.dataset_opt(root, aud=labels), "val")
    with pytest.raises(NotImplementedError, match="--emb"):
        datafiles.load_clip(dd.dataset_opt(root, pose=os.path.join(root, "clip.json"), aud=labels, bg_img="white"))


def test_the_other_audio_files_follow_asr_model(root, tmp_path):
    import shutil
    new = str(tmp_path / "d")
    shutil.copytree(root, new)
    aud = np.load(os.path.join(new, "aud_eo.npy"))
    os.remove(os.path.join(new, "aud_eo.npy"))
    np.save(os.path.join(new, "aud_ds.npy"), aud + 1)
    np.save(os.path.join(new, "aud.npy"), aud + 2)
    ds = datafiles.load_split(new, dd.dataset_opt(new, asr_model="deepspeech"), "val")
    other = datafiles.load_split(new, dd.dataset_opt(new, asr_model="facebook/wav2vec2-large-960h-lv60-self"), "val")
    assert ds.auds[0, 0, 0] == aud[dd.N_TRAIN_LISTED, 0, 0] + 1 and other.auds[0, 0, 0] == aud[dd.N_TRAIN_LISTED, 0, 0] + 2
    whole = datafiles.load_split(new, dd.dataset_opt(new, aud=os.path.join(root, "clip_aud.npy")), "val")
    assert whole.auds.shape == (dd.N_AUD, dd.AUD_K, 16) and not whole.has_gt                  # opt.aud: the whole array is kept


def test_the_decode_pool_is_sized_by_the_affinity_mask():
    assert datafiles.decode_workers() == min(16, len(os.sched_getaffinity(0)))


def test_no_decoder_names_both_libraries(monkeypatch):
    monkeypatch.setattr(datafiles, "_cv2", lambda: None)
    monkeypatch.setattr(datafiles, "_pil", lambda: None)
    with pytest.raises(ImportError, match="cv2.*PIL"):
        datafiles.default_decoder()


def test_a_non_uint8_decoder_is_refused_by_the_set(root):
    opt = dd.dataset_opt(root)
    with pytest.raises(TypeError, match="must be uint8"):
        DeviceTrainSet.from_directory(root, opt, "val", device="cpu", kernel="torch", decode=lambda p: dd.npy_decode(p).astype(np.float32) / 255)


@pytest.mark.parametrize("lips", [False, True])
def test_from_directory_equals_the_set_built_by_hand(root, loaded, lips):
    opt = dd.dataset_opt(root, finetune_lips=lips)
    ds = DeviceTrainSet.from_directory(root, opt, "train", num_rays=64, seed=3, device="cpu", kernel="torch", decode=dd.npy_decode)
    d = loaded["train"]
    hand = DeviceTrainSet(d.images, d.torso, d.bg, d.poses, d.intrinsics, d.auds, d.face_rect, eye_area=d.eye_area, opt=opt,
                          num_rays=64, seed=3, device="cpu", kernel="torch", lips_rect=d.lips_rect if lips else None)
    assert (ds.lips_rect is None) == (not lips) and ds.F == dd.N_TRAIN and (ds.H, ds.W) == (dd.H, dd.W)
    inds = torch.tensor([0, 5, dd.W, dd.H * dd.W - 1, 137, 137])
    for i in (0, 13, dd.N_TRAIN - 1):
        a, b = ds.batch([i], inds=inds), hand.batch([i], inds=inds)
        assert torch.equal(a["_packed"], b["_packed"]) and a["index"] == b["index"]
        for k in ("poses", "poses_matrix", "eye", "auds"):
            assert torch.equal(a[k], b[k]), k
    if lips:
        a, b = ds.batch_rect([2]), hand.batch_rect([2])
        assert a["rect"] == b["rect"] == tuple(d.lips_rect[2].tolist()) and torch.equal(a["_packed"], b["_packed"])
    assert ds.loaded.frame_ids == d.frame_ids and ds.loaded.radius == d.radius


def test_split_all_reads_every_json_of_the_root(root, loaded, capsys):
    """clip.json lies in the root too: its 11 frames have no images and are skipped, one warning each, next to the train split's one."""
    d = datafiles.load_split(root, dd.dataset_opt(root), "all")
    assert d.frame_ids == loaded["trainval"].frame_ids and same_bits(d.poses, loaded["trainval"].poses)
    assert sum("NOT FOUND" in ln for ln in capsys.readouterr().out.splitlines()) == dd.N_CLIP_POSES + 1
    test = datafiles.load_split(root, dd.dataset_opt(root), "test")
    assert test.frame_ids == loaded["val"].frame_ids and test.split == "test"
    with pytest.raises(ValueError, match="unknown split"):
        datafiles.load_split(root, dd.dataset_opt(root), "dev")
