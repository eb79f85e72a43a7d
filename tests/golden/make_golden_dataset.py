"""Generates tests/golden/reference_dataset.npz -- run ONLY in the build container (needs the reference checkout).

    python tests/golden/make_golden_dataset.py

What runs is the reference's OWN loader, imported unmodified at run time through make_golden.install_reference():
NeRFDataset.__init__ (nerf/provider.py:311-612, `--preload 1`) and NeRFDataset_Test.__init__ (:80-239), on the directory that
tests/dataset_dir.py writes.  cv2 is not installed here, so the stub module gets the four things the loader uses, backed by PIL:
imread (channels handed over in cv2's BGR(A) order), cvtColor (the two swaps), resize (INTER_AREA -> PIL's BOX; the helper's
background makes the area mean exact) and the constants.  trimesh stays an empty module.

Recorded per split: what the loader object holds afterwards -- poses, auds, face and lips rects, eye area (raw and smoothed),
intrinsics, H, W, radius, the background and two frames' images as round(x * 255) uint8.  For the clip: poses (raw and after
smooth_path), auds, eye (raw and smoothed), bg.  Only data is committed, nothing of the reference's text.
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden  # noqa: E402  (paths, stub modules, the reference on sys.path)
import dataset_dir  # noqa: E402

OUT = os.path.join(HERE, "reference_dataset.npz")
SEED = 0
# tag -> (split, option overrides)
SPLITS = {"train": ("train", {}), "part": ("train", dict(part=True)), "range": ("train", dict(data_range=[2, 17])),
          "val": ("val", {}), "trainval": ("trainval", {}), "smooth": ("train", dict(smooth_eye=True))}
IMAGE_FRAMES = (0, 13)             # kept-frame indices whose images are recorded (13: the first after the missing image)


def install_cv2_stub():
    from PIL import Image
    cv2 = sys.modules["cv2"]
    cv2.IMREAD_UNCHANGED, cv2.COLOR_BGR2RGB, cv2.COLOR_BGRA2RGBA, cv2.INTER_AREA = -1, 4, 5, 3

    def imread(path, flag):
        a = np.asarray(Image.open(path))
        return np.ascontiguousarray(a[..., [2, 1, 0] + ([3] if a.shape[-1] == 4 else [])])

    def cvtColor(img, code):
        assert code in (cv2.COLOR_BGR2RGB, cv2.COLOR_BGRA2RGBA) and img.shape[-1] == (3 if code == cv2.COLOR_BGR2RGB else 4)
        return np.ascontiguousarray(img[..., [2, 1, 0] + ([3] if img.shape[-1] == 4 else [])])

    def resize(img, size, interpolation):
        assert interpolation == cv2.INTER_AREA
        return np.asarray(Image.fromarray(img).resize(size, Image.BOX))

    cv2.imread, cv2.cvtColor, cv2.resize = imread, cvtColor, resize


def u8(x):
    return np.round(make_golden.t2n(x.float()) * 255).astype(np.uint8)


def main():
    make_golden.install_reference()
    install_cv2_stub()
    import nerf.provider as ref
    assert ref.__file__.startswith(make_golden.REF)
    out = {}
    with tempfile.TemporaryDirectory() as root:
        dataset_dir.write_dataset(root, SEED)
        for tag, (split, kw) in SPLITS.items():
            opt = dataset_dir.dataset_opt(root, preload=1, finetune_lips=True, **kw)
            d = ref.NeRFDataset(opt, "cpu", type=split)
            out[f"{tag}_poses"] = make_golden.t2n(d.poses)
            if tag != "smooth":
                out[f"{tag}_auds"] = make_golden.t2n(d.auds)
            out[f"{tag}_face_rect"] = np.array(d.face_rect, dtype=np.int32)
            out[f"{tag}_lips_rect"] = np.array(d.lips_rect, dtype=np.int32)
            out[f"{tag}_eye_area"] = make_golden.t2n(d.eye_area)
            out[f"{tag}_intrinsics"] = np.asarray(d.intrinsics)
            assert out[f"{tag}_intrinsics"].dtype == np.float64
            out[f"{tag}_shape"] = np.array([d.H, d.W, d.poses.shape[0]])
            out[f"{tag}_radius"] = np.array(d.radius, dtype=np.float64)
            out[f"{tag}_bg"] = u8(d.bg_img)
            for f in IMAGE_FRAMES:
                if f < d.poses.shape[0] and tag in ("train", "val"):
                    out[f"{tag}_image{f}"], out[f"{tag}_torso{f}"] = u8(d.images[f]), u8(d.torso_img[f])
        lips = out["train_lips_rect"]
        print("lips rects:", lips.tolist())
        assert (lips[:, 0] == 0).any() and (lips[:, 1] == dataset_dir.H).any() and (lips[:, 2] == 0).any() and \
            (lips[:, 3] == dataset_dir.W).any()                                    # every clip of provider.py:497-500 is taken
        assert out["train_shape"][2] == dataset_dir.N_TRAIN and out["part_shape"][2] == 3

        for tag, kw in (("clip", dict(smooth_path=True, smooth_eye=True)), ("clipraw", {})):
            opt = dataset_dir.dataset_opt(root, pose=os.path.join(root, "clip.json"), aud=os.path.join(root, "clip_aud.npy"),
                                          bg_img=os.path.join(root, "bc.jpg"), **kw)
            c = ref.NeRFDataset_Test(opt, "cpu")
            out[f"{tag}_poses"] = make_golden.t2n(c.poses)
            if tag == "clip":
                out[f"{tag}_auds"] = make_golden.t2n(c.auds)
            out[f"{tag}_eye_area"] = make_golden.t2n(c.eye_area)
            out[f"{tag}_bg"] = u8(c.bg_img)
            out[f"{tag}_intrinsics"] = np.asarray(c.intrinsics)
            out[f"{tag}_shape"] = np.array([c.H, c.W, c.poses.shape[0]])
    out["seed"] = np.array(SEED)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(out)} arrays")
    assert os.path.getsize(OUT) < 96 * 1024


if __name__ == "__main__":
    main()
