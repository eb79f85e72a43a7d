"""The files of a RAD-NeRF dataset directory, decoded ONCE to host arrays: what DeviceTrainSet (training) and ClipScene
(inference) take.  Nothing here touches a GPU and nothing here runs per step or per frame.

Reference: NeRFDataset.__init__ (nerf/provider.py:311-612) -> load_split, NeRFDataset_Test.__init__ (:80-239) -> load_clip.

    <root>/transforms_train.json  transforms_val.json      focal_len | fl_x, fl_y | camera_angle_x, _y; cx, cy; h, w (optional);
                                                           frames: [{img_id, aud_id, transform_matrix [4][4]}, ...]
    <root>/aud_eo.npy | aud_ds.npy | aud.npy                [N,16,K] logits (chosen by opt.asr_model; opt.aud overrides, and so
                                                           does opt.aud_features: [N,K,16] values already in memory, --aud_wav)
    <root>/bc.jpg                                           the background (opt.bg_img = '')
    <root>/gt_imgs/<img_id>.jpg                             the frame, RGB
    <root>/torso_imgs/<img_id>.png                          the torso layer, RGBA
    <root>/ori_imgs/<img_id>.lms                            68 face landmarks, text, (column, row) per line

Images stay uint8 end to end: that is DeviceTrainSet's contract, and `uint8 / 255` in float32 on the picked pixels is the
arithmetic of the reference's `--preload 0` and `--preload 1`.  `--preload` itself is accepted and ignored -- the set is always
device-resident uint8; `--preload 2`'s fp16 copies are not reproduced.  Label arrays ([N,16]) and `--emb` are not built: the
device routes take logits only.

Decoding: `decode(path) -> uint8 [H,W,3|4]` in RGB(A) order.  The default tries cv2 (with the BGR swap), then PIL.  A background
of another size is area-resized, with cv2.INTER_AREA when cv2 imports and PIL's BOX filter otherwise; the two can differ by one
count where the mean of a block falls on a rounding tie and are not pinned against each other.
"""
import glob
import json
import os
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from .rays import nerf_matrix_to_ngp, smooth_camera_path


def _o(opt, name, default):
    return getattr(opt, name, default)


def decode_workers():
    """The decode pool's size: the CPUs this process may run on, 16 at the most -- never the machine's CPU count."""
    return max(1, min(16, len(os.sched_getaffinity(0))))


def _cv2():
    try:
        import cv2
        return cv2
    except ImportError:
        return None


def _pil():
    try:
        from PIL import Image
        return Image
    except ImportError:
        return None


def default_decoder():
    """decode(path) with cv2 when it imports, else PIL; ImportError naming both when neither does."""
    cv2 = _cv2()
    if cv2 is not None:
        def decode(path):
            img = cv2.imread(path, cv2.IMREAD_UNCHANGED)
            if img is None:
                raise FileNotFoundError(f"datafiles: cannot decode {path}")
            if img.ndim == 2:
                img = np.repeat(img[..., None], 3, axis=-1)
            return np.ascontiguousarray(img[..., [2, 1, 0] + ([3] if img.shape[-1] == 4 else [])])
        return decode
    Image = _pil()
    if Image is not None:
        def decode(path):
            with Image.open(path) as im:
                if im.mode not in ("RGB", "RGBA"):
                    im = im.convert("RGBA" if "A" in im.mode or "transparency" in im.info else "RGB")
                return np.asarray(im, dtype=np.uint8).copy()
        return decode
    raise ImportError("datafiles: decoding image files needs cv2 (opencv-python) or PIL (pillow); neither imports.  "
                      "Pass decode=<callable path -> uint8 [H,W,3|4]> to use another decoder.")


def area_resize(img, H, W):
    """uint8 [h,w,C] -> [H,W,C] by area averaging: cv2.INTER_AREA when cv2 imports, else PIL's BOX."""
    cv2 = _cv2()
    if cv2 is not None:
        return cv2.resize(img, (W, H), interpolation=cv2.INTER_AREA)
    Image = _pil()
    if Image is None:
        raise ImportError("datafiles: resizing the background needs cv2 (opencv-python) or PIL (pillow); neither imports")
    return np.asarray(Image.fromarray(img).resize((W, H), Image.BOX), dtype=np.uint8).copy()


def _checked(img, name, path, channels=None):
    """The shape is checked here, where the file name is known; a wrong dtype is left to DeviceTrainSet's own message."""
    img = np.asarray(img)
    if img.ndim != 3 or img.shape[2] != channels:
        raise ValueError(f"datafiles: {name} {path} decoded to {img.shape}, expected [H,W,{channels}]")
    return img


def polygon_area(x, y):
    """Shoelace area of a closed polygon about its centroid (provider.py:47-52)."""
    x_, y_ = x - x.mean(), y - y.mean()
    correction = x_[-1] * y_[0] - y_[-1] * x_[0]
    main_area = np.dot(x_[:-1], y_[1:]) - np.dot(y_[:-1], x_[1:])
    return 0.5 * np.abs(main_area + correction)


def smooth_eye(eye):
    """The three-tap mean of provider.py:554-561 (float32 [N]); a new array."""
    eye = np.asarray(eye, dtype=np.float32)
    out = eye.copy()
    for i in range(eye.shape[0]):
        out[i] = eye[max(0, i - 1):min(eye.shape[0], i + 2)].mean()
    return out


def _audio_features(path, opt):
    """[N,16,K] logits -> float32 [N,K,16] (provider.py:402-414)."""
    aud = np.load(path)
    if _o(opt, "emb", False) or aud.ndim != 3:
        raise NotImplementedError(f"datafiles: {path} holds {'labels' if aud.ndim != 3 else 'logits'} and --emb "
                                  f"{'is' if _o(opt, 'emb', False) else 'would be'} needed: the --emb route (audio class + embedding) is "
                                  "not built here, the device routes take [N,16,K] logits only")
    return np.ascontiguousarray(aud.astype(np.float32).transpose(0, 2, 1))


def _given_features(opt):
    """opt.aud_features: the clip's audio as [N,K,16] float32 values already in memory (an array, or a tensor on any device) --
    what radnerf.cli leaves there for --aud_wav; None without one.  It stands where opt.aud's file would."""
    feats = _o(opt, "aud_features", None)
    if feats is None:
        return None
    if feats.ndim != 3 or feats.shape[2] != 16:
        raise ValueError(f"datafiles: opt.aud_features must be [N,K,16], got {tuple(feats.shape)}")
    return feats


def _default_audio_file(root, opt):
    model = _o(opt, "asr_model", "")
    name = "aud_eo.npy" if "esperanto" in model else "aud_ds.npy" if "deepspeech" in model else "aud.npy"
    return os.path.join(root, name)


def _background(opt, root, H, W, decode):
    bg = _o(opt, "bg_img", "")
    if bg == "white":
        return np.full((H, W, 3), 255, dtype=np.uint8)
    if bg == "black":
        return np.zeros((H, W, 3), dtype=np.uint8)
    if bg == "":
        if root is None:
            raise ValueError("datafiles: opt.bg_img = '' means <root>/bc.jpg, and there is no dataset root (opt.path); give "
                             "'white', 'black' or a file")
        bg = os.path.join(root, "bc.jpg")
    img = np.asarray(decode(bg))
    if img.ndim == 3 and img.shape[2] == 4:
        img = img[..., :3]
    # a decoder that hands out something else than uint8 is DeviceTrainSet's to refuse (its message names the fault); nothing is
    # resized for it
    if (img.shape[0] != H or img.shape[1] != W) and img.dtype == np.uint8:
        img = area_resize(np.ascontiguousarray(img), H, W)
    return np.ascontiguousarray(img)


def _intrinsics(transform, H, W, downscale):
    """float64 (fx, fy, cx, cy), the three branches of provider.py:592-609."""
    if "focal_len" in transform:
        fl_x = fl_y = transform["focal_len"]
    elif "fl_x" in transform or "fl_y" in transform:
        fl_x = (transform["fl_x"] if "fl_x" in transform else transform["fl_y"]) / downscale
        fl_y = (transform["fl_y"] if "fl_y" in transform else transform["fl_x"]) / downscale
    elif "camera_angle_x" in transform or "camera_angle_y" in transform:
        fl_x = W / (2 * np.tan(transform["camera_angle_x"] / 2)) if "camera_angle_x" in transform else None
        fl_y = H / (2 * np.tan(transform["camera_angle_y"] / 2)) if "camera_angle_y" in transform else None
        fl_x = fl_y if fl_x is None else fl_x
        fl_y = fl_x if fl_y is None else fl_y
    else:
        raise RuntimeError("datafiles: no focal length (focal_len, fl_x / fl_y or camera_angle_x / _y) in the transforms file")
    cx = (transform["cx"] / downscale) if "cx" in transform else (W / 2)
    cy = (transform["cy"] / downscale) if "cy" in transform else (H / 2)
    return np.array([fl_x, fl_y, cx, cy], dtype=np.float64)


def _sliced(frames, opt):
    start, end = _o(opt, "data_range", [0, -1])
    return frames[start:len(frames) if end == -1 else end]


def _poses(frames, opt):
    scale, offset = _o(opt, "scale", 4), _o(opt, "offset", [0, 0, 0])
    raw = np.array([f["transform_matrix"] for f in frames], dtype=np.float32).reshape(len(frames), 4, 4)
    return nerf_matrix_to_ngp(raw, scale=scale, offset=offset)


@dataclass
class LoadedSplit:
    """One split on the host.  images [F,H,W,3], torso [F,H,W,4], bg [H,W,3]: uint8.  poses [F,4,4] float32 (after smooth_path when
    set), intrinsics float64 (fx, fy, cx, cy), auds [Fa,K,16] float32 (Fa = F unless opt.aud was given), face_rect / lips_rect [F,4]
    int32 = (xmin, xmax, ymin, ymax) with x along the ROWS, eye_area [F,1] float32 (smoothed with opt.smooth_eye; eye_area_raw is
    what the landmarks gave), landmarks [F,68,2], frame_ids: the img_id of every kept frame, radius: mean camera distance,
    has_gt: the audio is the set's own (provider.py:733)."""
    H: int
    W: int
    images: np.ndarray
    torso: np.ndarray
    bg: np.ndarray
    poses: np.ndarray
    intrinsics: np.ndarray
    auds: np.ndarray
    face_rect: np.ndarray
    lips_rect: np.ndarray
    eye_area: np.ndarray
    eye_area_raw: np.ndarray
    landmarks: np.ndarray
    frame_ids: list
    radius: float
    has_gt: bool
    split: str = "train"

    @property
    def F(self):
        return int(self.poses.shape[0])


@dataclass
class LoadedClip:
    """A pose file and an audio-feature file on the host: poses [N,4,4] float32, auds [Fa,K,16] float32, eye_area [N,1] float32,
    bg [H,W,3] uint8, intrinsics float64."""
    H: int
    W: int
    poses: np.ndarray
    intrinsics: np.ndarray
    auds: np.ndarray
    eye_area: np.ndarray
    bg: np.ndarray
    root: Optional[str] = None


def _read_transforms(root, split):
    def read(path):
        with open(path, "r") as fh:
            return json.load(fh)
    if split == "all":
        paths = sorted(glob.glob(os.path.join(root, "*.json")))      # sorted: the reference takes glob's order, which is the file system's
        if not paths:
            raise FileNotFoundError(f"datafiles: no *.json in {root}")
        transform = read(paths[0])
        for p in paths[1:]:
            transform["frames"].extend(read(p)["frames"])
        return transform
    if split == "trainval":
        transform = read(os.path.join(root, "transforms_train.json"))
        transform["frames"].extend(read(os.path.join(root, "transforms_val.json"))["frames"])
        return transform
    if split not in ("train", "val", "test"):
        raise ValueError(f"datafiles: unknown split {split!r} (train, val, test, trainval, all)")
    return read(os.path.join(root, f"transforms_{'val' if split == 'test' else split}.json"))


def load_split(root, opt, split="train", downscale=1, decode=None):
    """The files of one split -> LoadedSplit (NeRFDataset.__init__, provider.py:311-612)."""
    if _o(opt, "asr", False):
        raise NotImplementedError("datafiles: live ASR (--asr) is not built here")
    transform = _read_transforms(root, split)
    if "h" in transform and "w" in transform:
        H, W = int(transform["h"]) // downscale, int(transform["w"]) // downscale
    else:
        H, W = int(transform["cy"]) * 2 // downscale, int(transform["cx"]) * 2 // downscale
    frames = _sliced(transform["frames"], opt)
    if split == "train":
        if _o(opt, "part", False):
            frames = frames[::10]
        elif _o(opt, "part2", False):
            frames = frames[:375]
    elif split == "val":
        frames = frames[:100]

    given = _given_features(opt)
    own_audio = _o(opt, "aud", "") == "" and given is None
    aud_features = given if given is not None else _audio_features(_default_audio_file(root, opt) if own_audio else opt.aud, opt)

    kept = []
    for f in frames:
        path = os.path.join(root, "gt_imgs", str(f["img_id"]) + ".jpg")
        if not os.path.exists(path):
            print("[WARN]", path, "NOT FOUND!")
            continue
        kept.append(f)
    if not kept:
        raise FileNotFoundError(f"datafiles: no frame of split {split!r} has its image under {os.path.join(root, 'gt_imgs')}")
    decode = default_decoder() if decode is None else decode
    ids = [str(f["img_id"]) for f in kept]
    with ThreadPoolExecutor(max_workers=decode_workers()) as pool:
        images = list(pool.map(lambda i: _checked(decode(os.path.join(root, "gt_imgs", i + ".jpg")), "image", i, 3), ids))
        torso = list(pool.map(lambda i: _checked(decode(os.path.join(root, "torso_imgs", i + ".png")), "torso image", i, 4), ids))
    for name, arrs in (("image", images), ("torso image", torso)):
        for i, a in zip(ids, arrs):
            if a.shape[:2] != (H, W):
                raise ValueError(f"datafiles: {name} {i} is {a.shape[0]} x {a.shape[1]}, the transforms file says {H} x {W}")

    from .dataset import lips_rect_from_landmarks
    lms = np.stack([np.loadtxt(os.path.join(root, "ori_imgs", i + ".lms")) for i in ids]).reshape(len(ids), 68, 2)
    face = np.array([[int(l[31:36, 1].min()), int(l[:, 1].max()), int(l[:, 0].min()), int(l[:, 0].max())] for l in lms], dtype=np.int32)
    lips = np.array(lips_rect_from_landmarks(lms, H, W), dtype=np.int32)
    eye_raw = np.array([(polygon_area(l[36:42, 0], l[36:42, 1]) + polygon_area(l[42:48, 0], l[42:48, 1])) / (H * W) * 100 for l in lms],
                       dtype=np.float32)
    eye = smooth_eye(eye_raw) if _o(opt, "smooth_eye", False) else eye_raw.copy()

    if own_audio:
        auds = np.stack([aud_features[min(f["aud_id"], aud_features.shape[0] - 1)] for f in kept])
    else:
        auds = aud_features
    poses = _poses(kept, opt)
    if _o(opt, "smooth_path", False):
        poses = smooth_camera_path(poses, _o(opt, "smooth_path_window", 7))
    radius = torch.from_numpy(poses)[:, :3, 3].norm(dim=-1).mean(0).item()
    return LoadedSplit(H=H, W=W, images=np.stack(images), torso=np.stack(torso), bg=_background(opt, root, H, W, decode), poses=poses,
                       intrinsics=_intrinsics(transform, H, W, downscale), auds=auds, face_rect=face, lips_rect=lips,
                       eye_area=eye.reshape(-1, 1), eye_area_raw=eye_raw.reshape(-1, 1), landmarks=lms,
                       frame_ids=[f["img_id"] for f in kept], radius=radius, has_gt=own_audio, split=split)


def load_clip(opt, decode=None, downscale=1):
    """opt.pose (a transforms file) and opt.aud (an audio-feature file) -> LoadedClip (NeRFDataset_Test.__init__,
    provider.py:80-239).  Without opt.aud the frames' own aud_ids pick rows of the default audio file next to the data
    (opt.path, else the pose file's directory)."""
    if _o(opt, "asr", False):
        raise NotImplementedError("datafiles: live ASR (--asr) is not built here")
    if not _o(opt, "pose", ""):
        raise ValueError("datafiles.load_clip: opt.pose (a transforms file) is required")
    with open(opt.pose, "r") as fh:
        transform = json.load(fh)
    H, W = int(transform["cy"]) * 2 // downscale, int(transform["cx"]) * 2 // downscale
    frames = _sliced(transform["frames"], opt)
    root = _o(opt, "path", "") or None
    if _given_features(opt) is not None:
        auds = _given_features(opt)
    elif _o(opt, "aud", "") != "":
        auds = _audio_features(opt.aud, opt)
    else:
        if any("aud_id" not in f for f in frames):
            raise ValueError("datafiles.load_clip: opt.aud is required (the pose file's frames carry no aud_id)")
        feats = _audio_features(_default_audio_file(root or os.path.dirname(os.path.abspath(opt.pose)), opt), opt)
        auds = np.stack([feats[min(f["aud_id"], feats.shape[0] - 1)] for f in frames])
    eye = np.array([f.get("eye_ratio", 0.25) for f in frames], dtype=np.float32)
    if _o(opt, "smooth_eye", False):
        eye = smooth_eye(eye)
    poses = _poses(frames, opt)
    if _o(opt, "smooth_path", False):
        poses = smooth_camera_path(poses, _o(opt, "smooth_path_window", 7))
    decode_bg = decode if decode is not None else (default_decoder() if _o(opt, "bg_img", "") not in ("white", "black") else None)
    intr = np.array([transform["focal_len"], transform["focal_len"], transform["cx"] / downscale, transform["cy"] / downscale],
                    dtype=np.float64)
    return LoadedClip(H=H, W=W, poses=poses, intrinsics=intr, auds=auds, eye_area=eye.reshape(-1, 1),
                      bg=_background(opt, root, H, W, decode_bg), root=root)
