"""A synthetic RAD-NeRF dataset directory for the file-loader tests, deterministic from a seed (shared helper, no test).

Layout written under `root` (what radnerf/datafiles.py reads; INTEGRATION.md "From a dataset directory"):

    transforms_train.json  transforms_val.json     focal_len, cx, cy and per frame img_id, aud_id, transform_matrix
    aud_eo.npy                                     [30,16,44] float32 logits
    bc.jpg                                         background at TWICE the frame size (the area resize is taken)
    gt_imgs/<id>.jpg  torso_imgs/<id>.png  ori_imgs/<id>.lms
    clip.json  clip_aud.npy                        a pose file (eye_ratio on some frames) and a driving audio file

H = 20, W = 16 (non-square: a row/column swap shows).  25 train frames are listed and the colour image of one is missing, so 24
are kept; 9 val frames.  The audio has 30 rows and the val frames' aud_ids run past its end (the clamp).  Every image file is a
PNG stream under the name the layout prescribes -- cv2 and PIL both decode by content -- so no pixel comparison depends on a JPEG
decoder's rounding; each is also written as `<name>.npy` for the GPU tests' `decode=` hook (npy_decode).  The 2 x 2 blocks of bc
are (t+3, t+1 / t-1, t-3): every pair sum is even and every block sum is 4t, so an area resize gives t in either library and in
either pass order.
"""
import json
import os
from types import SimpleNamespace

import numpy as np

H, W = 20, 16
N_TRAIN_LISTED, N_TRAIN, N_VAL, N_AUD, AUD_K = 25, 24, 9, 30, 44
MISSING = 13                       # the listed train frame whose colour image is not written
N_CLIP_POSES = 11                  # fewer poses than audio rows: the clip mirrors
CX, CY = 8.25, 10.5                # int(cx) * 2 = W, int(cy) * 2 = H

# lips boxes (row0, row1, col0, col1): wider than tall, taller than wide, one against each border
_LIPS = [(7.2, 12.9, 5.5, 11.4), (0.3, 5.7, 1.1, 9.8), (12.3, 19.6, 3.2, 15.9), (5.5, 14.5, 12.0, 15.8),
         (9.0, 12.0, 0.2, 6.2), (2.4, 9.7, 8.3, 15.6), (10.1, 18.8, 0.4, 5.1), (8.8, 13.1, 6.7, 10.2)]


def dataset_opt(root, **overrides):
    """default_opt() plus the loader's fields at the reference CLI's defaults."""
    import sys
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rad-nerf_amd")
    if pkg not in sys.path:
        sys.path.insert(0, pkg)
    from radnerf.scene import default_opt
    opt = default_opt(path=root, data_range=[0, -1], part=False, part2=False, asr=False, aud="", preload=0, scale=4, offset=[0, 0, 0],
                      finetune_lips=False, smooth_eye=False, smooth_path=False, smooth_path_window=7, bg_img="", num_rays=256,
                      patch_size=1, pose="", fix_eye=-1)
    for k, v in overrides.items():
        setattr(opt, k, v)
    return opt


def npy_decode(path):
    """decode= hook: the .npy twin of an image file."""
    return np.load(os.path.splitext(path)[0] + ".npy")


def _raw_pose(ngp):
    """The dataset-convention matrix that nerf_matrix_to_ngp(scale=4, offset=0) maps onto `ngp` (exactly: /4 and *4 are exact)."""
    raw = np.zeros((4, 4), dtype=np.float32)
    for new, old in ((0, 1), (1, 2), (2, 0)):
        raw[old] = [ngp[new, 0], -ngp[new, 1], -ngp[new, 2], ngp[new, 3] / np.float32(4)]
    raw[3, 3] = 1
    return raw


def _audio(a, b, c):
    """[N_AUD,16,AUD_K] logits as a pattern of (row, tap, channel): the loaders only pick rows and swap the last two axes, so every
    row and both axes are told apart, and the recorded copies compress to almost nothing."""
    n, t, k = np.meshgrid(np.arange(N_AUD), np.arange(16), np.arange(AUD_K), indexing="ij")
    return (((a * n + b * t + c * k + (n * k) // 5) % 17 - 8) / 4).astype(np.float32)


def _write_png(path, arr):
    from PIL import Image
    with open(path, "wb") as fh:
        Image.fromarray(arr).save(fh, format="PNG")
    np.save(os.path.splitext(path)[0] + ".npy", arr)


def write_dataset(root, seed=0, scale=1):
    """Writes the directory; returns a SimpleNamespace of what was written (frames per split, arrays).  scale = s: the same
    directory at s H x s W with every landmark coordinate multiplied by s (a lips rect must be 31 pixels wide before the perceptual
    term takes it); the fixture and every other test use scale = 1."""
    H, W = scale * globals()["H"], scale * globals()["W"]
    import sys
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rad-nerf_amd")
    if pkg not in sys.path:
        sys.path.insert(0, pkg)
    from radnerf.rays import intrinsics_from_fovy, orbit_pose
    from radnerf.scene import default_opt
    o = default_opt()
    rng = np.random.default_rng(20250301 + seed)
    for sub in ("gt_imgs", "torso_imgs", "ori_imgs"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    focal = float(intrinsics_from_fovy(H, W, o.fovy)[0])
    n_all = N_TRAIN_LISTED + N_VAL
    images = rng.integers(0, 256, (n_all, H, W, 3), dtype=np.uint8)
    torso = rng.integers(0, 256, (n_all, H, W, 4), dtype=np.uint8)
    kind = rng.integers(0, 4, (n_all, H, W))
    torso[..., 3][kind == 0] = 0
    torso[..., 3][kind == 1] = 255
    lms = np.round(rng.random((n_all, 68, 2)) * np.array([W - 1, H - 1]), 1)
    frames = []
    for f in range(n_all):
        r0, r1, c0, c1 = (scale * v for v in _LIPS[f % len(_LIPS)])
        lms[f, 48:60, 0] = np.round(c0 + (c1 - c0) * rng.random(12), 1)
        lms[f, 48:60, 1] = np.round(r0 + (r1 - r0) * rng.random(12), 1)
        lms[f, 48], lms[f, 54] = (c0, round(0.5 * (r0 + r1), 1)), (c1, round(0.5 * (r0 + r1), 1))
        lms[f, 51], lms[f, 57] = (round(0.5 * (c0 + c1), 1), r0), (round(0.5 * (c0 + c1), 1), r1)
        lms[f, 31:36, 1] = np.round(scale * (1.0 + 5.0 * rng.random(5)), 1)             # the nose row that opens the face rect
        lms[f, 0, 1] = scale * 18.4                                                   # ... and a chin row that closes it
        t = f / 25.0
        pose = orbit_pose(o.radius, 8.0 * np.sin(2 * np.pi * t / 0.9), 4.0 * np.cos(2 * np.pi * t / 0.7))
        img_id = 100 + f
        aud_id = f                                                            # the last val frames lie past the 30 audio rows
        frames.append(dict(img_id=img_id, aud_id=aud_id, transform_matrix=[[float(v) for v in row] for row in _raw_pose(pose)]))
        if f != MISSING:
            _write_png(os.path.join(root, "gt_imgs", f"{img_id}.jpg"), images[f])
            _write_png(os.path.join(root, "torso_imgs", f"{img_id}.png"), torso[f])
            np.savetxt(os.path.join(root, "ori_imgs", f"{img_id}.lms"), lms[f], fmt="%.1f")
    head = dict(focal_len=focal, cx=W / 2 + 0.25, cy=H / 2 + 0.5)
    with open(os.path.join(root, "transforms_train.json"), "w") as fh:
        json.dump(dict(head, frames=frames[:N_TRAIN_LISTED]), fh)
    with open(os.path.join(root, "transforms_val.json"), "w") as fh:
        json.dump(dict(head, frames=frames[N_TRAIN_LISTED:]), fh)

    aud = _audio(7, 3, 1)
    np.save(os.path.join(root, "aud_eo.npy"), aud)

    t_bg = rng.integers(3, 253, (H, W, 3)).astype(np.int32)
    big = np.zeros((2 * H, 2 * W, 3), dtype=np.int32)
    big[0::2, 0::2], big[0::2, 1::2], big[1::2, 0::2], big[1::2, 1::2] = t_bg + 3, t_bg + 1, t_bg - 1, t_bg - 3
    _write_png(os.path.join(root, "bc.jpg"), big.astype(np.uint8))

    # the inference side: a pose file with its own (shorter) pose stream and a driving audio file
    clip_frames = []
    for f in range(N_CLIP_POSES):
        pose = orbit_pose(o.radius, 6.0 * np.sin(0.7 * f), 3.0 * np.cos(1.1 * f))
        fr = dict(img_id=f, aud_id=f, transform_matrix=[[float(v) for v in row] for row in _raw_pose(pose)])
        if f % 3 != 2:
            fr["eye_ratio"] = float(np.round(0.1 + 0.3 * rng.random(), 3))
        clip_frames.append(fr)
    with open(os.path.join(root, "clip.json"), "w") as fh:
        json.dump(dict(head, frames=clip_frames), fh)
    clip_aud = _audio(5, 1, 3)
    np.save(os.path.join(root, "clip_aud.npy"), clip_aud)
    return SimpleNamespace(root=root, images=images, torso=torso, lms=lms, bg=t_bg.astype(np.uint8), aud=aud, clip_aud=clip_aud,
                           focal=focal, frames=frames, clip_frames=clip_frames)
