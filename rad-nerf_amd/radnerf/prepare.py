"""A dataset directory's image files and transforms from the video's frames: tasks 5, 6 and 9 of the reference's
data_utils/process.py, the first two on the device (csrc/rn_prep.hip; csrc/rn_prep_dev.h states every convention).

    python -m radnerf.prepare DIR --task -1         # 5, 6, then 9 when DIR/track_params.pt exists

    DIR/ori_imgs/<id>.jpg      the frames                         } given: tasks 3 and 4 of process.py (ffmpeg, face parsing)
    DIR/parsing/<id>.png       their face-parsing label images    }
    DIR/track_params.pt        the face tracker's result          } given: task 8
    DIR/bc.jpg                 task 5: the background plate
    DIR/gt_imgs/<id>.jpg       task 6: the frame over the plate
    DIR/torso_imgs/<id>.png    task 6: the torso layer, RGBA
    DIR/transforms_{train,val}.json   task 9

    labels_from_parsing(rgb)            host: a parsing image's colours -> the label byte of every pixel
    background_plate(frames, labels)    device: uint8 [F,H,W,3] and [F,H,W] -> the plate [H,W,3]; PlateBuilder takes the frames in batches
    layers(frames, labels, plate)       device: -> (gt [F,H,W,3], torso [F,H,W,4])

Everything on the device is integer or table-driven, so the files are a function of the inputs alone: the batch size changes nothing.
Frame ids are sorted numerically (the reference takes glob's order, which is the file system's).  The plate is written and the gt
images are written with radnerf.video.JpegEncoder; task 6 reads bc.jpg back from disk, so the gt background is the plate that training
loads.  Files are read with `decode(path) -> uint8 [H,W,3|4]` (datafiles.default_decoder) and PNGs are written with
`write(path, uint8 [H,W,4])` (PIL); both are hooks.
"""
import glob
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .datafiles import decode_workers, default_decoder

OTHER, HEAD, NECK, TORSO, BACKGROUND = 0, 1, 2, 3, 4
LABEL_COLOURS = {HEAD: (0, 0, 255), NECK: (0, 255, 0), TORSO: (255, 0, 0), BACKGROUND: (255, 255, 255)}      # RGB
SURE_D2 = 25                      # a plate pixel is sure when some frame has it MORE than 5 pixels from the foreground
DARKEN_ROWS = 53
# what writes the outputs of the tasks that are not built here
ELSEWHERE = {1: "ffmpeg (aud.wav out of the video)", 2: "python -m radnerf.asr (aud_eo.npy out of aud.wav)",
             3: "ffmpeg (ori_imgs/<id>.jpg out of the video)", 4: "a face-parsing network (parsing/<id>.png; plain PyTorch, no kernel of this tree)",
             7: "a landmark detector (ori_imgs/<id>.lms; plain PyTorch)", 8: "the reference's 3DMM face tracker (track_params.pt; plain PyTorch)"}


def labels_from_parsing(rgb):
    """uint8 [...,3] (RGB; an alpha channel is ignored) -> uint8 [...]: HEAD, NECK, TORSO, BACKGROUND by exact colour, OTHER else."""
    rgb = np.asarray(rgb)
    if rgb.dtype != np.uint8 or rgb.ndim < 1 or rgb.shape[-1] not in (3, 4):
        raise ValueError(f"prepare: a parsing image is uint8 [...,3], got {rgb.dtype} {rgb.shape}")
    out = np.zeros(rgb.shape[:-1], dtype=np.uint8)
    for label, (r, g, b) in LABEL_COLOURS.items():
        out[(rgb[..., 0] == r) & (rgb[..., 1] == g) & (rgb[..., 2] == b)] = label
    return out


def darken_table():
    """float64 [53]: numpy's 0.98 ** k, the bits the reference multiplies with."""
    return 0.98 ** np.arange(DARKEN_ROWS)


def _checked(frames, labels):
    if frames.dim() == 3:
        frames, labels = frames[None], labels[None]
    if (frames.dtype != torch.uint8 or labels.dtype != torch.uint8 or not frames.is_cuda or not labels.is_cuda or frames.dim() != 4
            or frames.shape[3] != 3 or tuple(labels.shape) != tuple(frames.shape[:3]) or frames.shape[0] < 1):
        raise ValueError(f"prepare: frames are uint8 [F,H,W,3] and labels uint8 [F,H,W] on the device, got {frames.dtype} "
                         f"{tuple(frames.shape)} and {labels.dtype} {tuple(labels.shape)}")
    return frames.contiguous(), labels.contiguous()


def _workspace(hip, F, H, W, device):
    n = int(hip._lib.rn_prep_workspace(F, H, W))
    if n == 0:
        raise ValueError(f"prepare: {F} frames of {H} x {W} are not a batch the kernels take (sides <= 16384, F H W < 2^31)")
    return torch.empty(n, dtype=torch.uint8, device=device)


class PlateBuilder:
    """The background plate of frames that arrive in batches, in frame order: add(frames, labels) ..., then finish()."""

    def __init__(self, H, W, device="cuda"):
        import radnerf_hip as hip
        self._hip, self.H, self.W, self.device = hip, int(H), int(W), torch.device(device)
        self.best_d2 = torch.full((self.H, self.W), -1, dtype=torch.int32, device=self.device)
        self.best_id = torch.zeros((self.H, self.W), dtype=torch.int32, device=self.device)
        self.plate = torch.zeros((self.H, self.W, 3), dtype=torch.uint8, device=self.device)
        self.frames = 0

    def add(self, frames, labels):
        hip = self._hip
        frames, labels = _checked(frames, labels)
        F = int(frames.shape[0])
        if tuple(frames.shape[1:3]) != (self.H, self.W):
            raise ValueError(f"prepare: the plate is {self.H} x {self.W}, the frames are {frames.shape[1]} x {frames.shape[2]}")
        ws = _workspace(hip, F, self.H, self.W, self.device)
        hip.call("rn_prep_plate_accumulate", hip.ptr(frames), hip.ptr(labels), F, self.H, self.W, self.frames, hip.ptr(self.best_d2),
                 hip.ptr(self.best_id), hip.ptr(self.plate), hip.ptr(ws), hip.stream())
        self.frames += F

    def finish(self, thresh_d2=SURE_D2):
        """The filled plate [H,W,3] (a new tensor; the builder's arrays stay as accumulated).  ValueError when no pixel is sure."""
        hip = self._hip
        plate = self.plate.clone()
        n_sure = torch.zeros(1, dtype=torch.int32, device=self.device)
        ws = _workspace(hip, 1, self.H, self.W, self.device)
        hip.call("rn_prep_plate_fill", hip.ptr(self.best_d2), hip.ptr(plate), self.H, self.W, int(thresh_d2), hip.ptr(n_sure), hip.ptr(ws),
                 hip.stream())
        self.n_sure = int(n_sure.item())
        if self.n_sure == 0:
            raise ValueError(f"prepare: no pixel of the {self.frames} frames is ever more than sqrt({int(thresh_d2)}) pixels from the "
                             "foreground: there is no background to take a plate from")
        return plate


def background_plate(frames, labels, batch=None, thresh_d2=SURE_D2):
    """The plate [H,W,3] of frames [F,H,W,3] with labels [F,H,W] (uint8, on the device); `batch` frames per launch (default: all)."""
    frames, labels = _checked(frames, labels)
    F = int(frames.shape[0])
    batch = F if batch is None else int(batch)
    if batch < 1:
        raise ValueError(f"prepare: batch must be at least 1, got {batch}")
    builder = PlateBuilder(frames.shape[1], frames.shape[2], frames.device)
    for at in range(0, F, batch):
        builder.add(frames[at:at + batch], labels[at:at + batch])
    return builder.finish(thresh_d2)


def layers(frames, labels, plate):
    """(gt [F,H,W,3], torso [F,H,W,4]) of frames [F,H,W,3], labels [F,H,W] and the plate [H,W,3]: uint8, on the device."""
    import radnerf_hip as hip
    frames, labels = _checked(frames, labels)
    F, H, W = (int(v) for v in frames.shape[:3])
    if plate.dtype != torch.uint8 or not plate.is_cuda or tuple(plate.shape) != (H, W, 3):
        raise ValueError(f"prepare: the plate is uint8 [{H},{W},3] on the device, got {plate.dtype} {tuple(plate.shape)}")
    plate = plate.contiguous()
    darken = torch.from_numpy(darken_table()).to(frames.device)
    gt = torch.empty((F, H, W, 3), dtype=torch.uint8, device=frames.device)
    torso = torch.empty((F, H, W, 4), dtype=torch.uint8, device=frames.device)
    ws = _workspace(hip, F, H, W, frames.device)
    hip.call("rn_prep_layers", hip.ptr(frames), hip.ptr(labels), hip.ptr(plate), hip.ptr(darken), F, H, W, hip.ptr(gt), hip.ptr(torso),
             hip.ptr(ws), hip.stream())
    return gt, torso


# ------------------------------------------------------------------------------------------------------------------- files
def frame_ids(root):
    """The ids of ori_imgs/*.jpg, sorted by number (then by name for ids that are no numbers)."""
    names = [os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(root, "ori_imgs", "*.jpg"))]
    if not names:
        raise FileNotFoundError(f"prepare: no *.jpg under {os.path.join(root, 'ori_imgs')}")
    return sorted(names, key=lambda n: (0, int(n), n) if n.isdigit() else (1, 0, n))


def default_png_writer():
    """write(path, uint8 [H,W,4]) through PIL; a clear ImportError without it."""
    try:
        from PIL import Image
    except ImportError:
        raise ImportError("prepare: writing torso_imgs/<id>.png needs PIL (pillow), which does not import.  Pass "
                          "write=<callable (path, uint8 [H,W,4])> to write them another way.") from None

    def write(path, rgba):
        with open(path, "wb") as fh:
            Image.fromarray(rgba).save(fh, format="PNG")
    return write


def _rgb(img, path):
    img = np.asarray(img)
    if img.ndim == 3 and img.shape[2] == 4:
        img = img[..., :3]
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError(f"prepare: {path} decoded to {img.dtype} {img.shape}, expected uint8 [H,W,3]")
    return img


class _Reader:
    """Frames and labels of a list of ids, a batch at a time, decoded on the pool; the next batch decodes while this one is used."""

    def __init__(self, root, ids, batch, decode, pool):
        self.root, self.ids, self.batch, self.decode, self.pool = root, ids, int(batch), decode, pool

    def _one(self, i):
        frame = _rgb(self.decode(os.path.join(self.root, "ori_imgs", i + ".jpg")), i + ".jpg")
        path = os.path.join(self.root, "parsing", i + ".png")
        label = labels_from_parsing(_rgb(self.decode(path), path))
        if label.shape != frame.shape[:2]:
            raise ValueError(f"prepare: parsing/{i}.png is {label.shape[0]} x {label.shape[1]}, ori_imgs/{i}.jpg is {frame.shape[0]} x {frame.shape[1]}")
        return frame, label

    def _submit(self, at):
        return [self.pool.submit(self._one, i) for i in self.ids[at:at + self.batch]]

    def __iter__(self):
        """(ids, frames uint8 [F,H,W,3], labels uint8 [F,H,W]) on the host."""
        pending = self._submit(0)
        for at in range(0, len(self.ids), self.batch):
            done = [f.result() for f in pending]
            pending = self._submit(at + self.batch)
            shapes = {d[0].shape for d in done}
            if len(shapes) != 1:
                raise ValueError(f"prepare: the frames of one video have one size, got {sorted(shapes)}")
            yield self.ids[at:at + self.batch], np.stack([d[0] for d in done]), np.stack([d[1] for d in done])


def _check_batch(batch):
    if int(batch) < 1:
        raise ValueError(f"prepare: --batch must be at least 1, got {batch}")
    return int(batch)


def extract_background(root, bg_stride=20, batch=64, jpeg_quality=95, jpeg_subsampling="420", device="cuda", decode=None, log=print):
    """Task 5: DIR/bc.jpg from every bg_stride-th frame.  Returns the plate (uint8 [H,W,3], on the device) before it was encoded."""
    from .video import JpegEncoder
    if int(bg_stride) < 1:
        raise ValueError(f"prepare: --bg_stride must be at least 1, got {bg_stride}")
    ids = frame_ids(root)[::int(bg_stride)]
    decode = default_decoder() if decode is None else decode
    builder = None
    with ThreadPoolExecutor(max_workers=decode_workers()) as pool:
        for _, frames, labels in _Reader(root, ids, _check_batch(batch), decode, pool):
            if builder is None:
                builder = PlateBuilder(frames.shape[1], frames.shape[2], device)
            builder.add(torch.from_numpy(frames).to(device), torch.from_numpy(labels).to(device))
    plate = builder.finish()
    data = JpegEncoder(builder.H, builder.W, jpeg_quality, jpeg_subsampling).files(plate[None])[0]
    with open(os.path.join(root, "bc.jpg"), "wb") as fh:
        fh.write(data)
    log(f"prepare: bc.jpg from {len(ids)} frames, {builder.n_sure} of {builder.H * builder.W} pixels seen as background")
    return plate


def extract_torso_and_gt(root, batch=64, jpeg_quality=95, jpeg_subsampling="420", device="cuda", decode=None, write=None, log=print):
    """Task 6: DIR/gt_imgs/<id>.jpg and DIR/torso_imgs/<id>.png of every frame, `batch` frames at a time.  Returns the frame count."""
    from .video import JpegEncoder
    ids = frame_ids(root)
    decode = default_decoder() if decode is None else decode
    write = default_png_writer() if write is None else write
    bc = os.path.join(root, "bc.jpg")
    if not os.path.exists(bc):
        raise FileNotFoundError(f"prepare: {bc} is missing; task 5 writes it")
    plate_host = _rgb(decode(bc), bc)
    plate = torch.from_numpy(np.ascontiguousarray(plate_host)).to(device)
    for sub in ("gt_imgs", "torso_imgs"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    encoder, writes = None, []
    with ThreadPoolExecutor(max_workers=decode_workers()) as pool:
        for batch_ids, frames, labels in _Reader(root, ids, _check_batch(batch), decode, pool):
            if frames.shape[1:3] != plate_host.shape[:2]:
                raise ValueError(f"prepare: bc.jpg is {plate_host.shape[0]} x {plate_host.shape[1]}, the frames are {frames.shape[1]} x {frames.shape[2]}")
            if encoder is None:
                encoder = JpegEncoder(frames.shape[1], frames.shape[2], jpeg_quality, jpeg_subsampling)
            gt, torso = layers(torch.from_numpy(frames).to(device), torch.from_numpy(labels).to(device), plate)
            files = encoder.files(gt)
            torso_host = torso.cpu().numpy()
            for f in writes:                    # the last batch's PNGs: at most two batches are in flight
                f.result()
            writes = [pool.submit(write, os.path.join(root, "torso_imgs", i + ".png"), torso_host[k]) for k, i in enumerate(batch_ids)]
            for i, data in zip(batch_ids, files):
                with open(os.path.join(root, "gt_imgs", i + ".jpg"), "wb") as fh:
                    fh.write(data)
        for f in writes:
            f.result()
    log(f"prepare: gt_imgs and torso_imgs of {len(ids)} frames")
    return len(ids)


def _matmul3(a, b):
    """[N,3,3] x [N,3,3] with every product and sum rounded in float32, k ascending: ((a0 b0 + a1 b1) + a2 b2)."""
    rows = []
    for i in range(3):
        rows.append(torch.stack([(a[:, i, 0] * b[:, 0, j] + a[:, i, 1] * b[:, 1, j]) + a[:, i, 2] * b[:, 2, j] for j in range(3)], dim=1))
    return torch.stack(rows, dim=1)


def euler2rot(euler):
    """[N,3] float32 -> [N,3,3]: rot_x (rot_y rot_z) with the reference's matrices (process.py:276-298)."""
    theta, phi, psi = euler[:, 0], euler[:, 1], euler[:, 2]
    one, zero = torch.ones_like(theta), torch.zeros_like(theta)

    def mat(*rows):
        return torch.stack([torch.stack(r, dim=1) for r in rows], dim=1)
    rot_x = mat((one, zero, zero), (zero, theta.cos(), -theta.sin()), (zero, theta.sin(), theta.cos()))
    rot_y = mat((phi.cos(), zero, phi.sin()), (zero, one, zero), (-phi.sin(), zero, phi.cos()))
    rot_z = mat((psi.cos(), psi.sin(), zero), (-psi.sin(), psi.cos(), zero), (zero, zero, one))
    return _matmul3(rot_x, _matmul3(rot_y, rot_z))


def transforms_from_track(params, h, w):
    """{'train': dict, 'val': dict} of a track_params dict (focal [1], euler [N,3], trans [N,3]): float32 torch on the host."""
    focal = params["focal"]
    euler = torch.as_tensor(params["euler"]).detach().to("cpu", torch.float32)
    trans = torch.as_tensor(params["trans"]).detach().to("cpu", torch.float32) / 10.0
    n = int(euler.shape[0])
    rot_inv = euler2rot(euler).permute(0, 2, 1)
    trans_inv = -((rot_inv[:, :, 0] * trans[:, 0:1] + rot_inv[:, :, 1] * trans[:, 1:2]) + rot_inv[:, :, 2] * trans[:, 2:3])
    split = int(n * 10 / 11)
    out = {}
    for name, ids in (("train", range(0, split)), ("val", range(split, n))):
        frames = []
        for i in ids:
            pose = torch.eye(4, dtype=torch.float32)
            pose[:3, :3] = rot_inv[i]
            pose[:3, 3] = trans_inv[i]
            frames.append(dict(img_id=i, aud_id=i, transform_matrix=pose.numpy().tolist()))
        out[name] = dict(focal_len=float(torch.as_tensor(focal).reshape(-1)[0]), cx=float(w / 2.0), cy=float(h / 2.0), frames=frames)
    return out


def save_transforms(root, decode=None, log=print):
    """Task 9: DIR/transforms_train.json and transforms_val.json from DIR/track_params.pt (process.py:259-342)."""
    track = os.path.join(root, "track_params.pt")
    if not os.path.exists(track):
        raise FileNotFoundError(f"prepare: {track} is missing; the face tracker (task 8) writes it")
    decode = default_decoder() if decode is None else decode
    first = frame_ids(root)[0]
    h, w = np.asarray(decode(os.path.join(root, "ori_imgs", first + ".jpg"))).shape[:2]
    out = transforms_from_track(torch.load(track, map_location="cpu"), h, w)
    for name, transform in out.items():
        with open(os.path.join(root, f"transforms_{name}.json"), "w") as fp:
            json.dump(transform, fp, indent=2, separators=(",", ": "))
    log(f"prepare: transforms of {len(out['train']['frames'])} train and {len(out['val']['frames'])} val frames")
    return out


def build_parser():
    import argparse
    p = argparse.ArgumentParser(prog="python -m radnerf.prepare",
                                description="bc.jpg, gt_imgs/, torso_imgs/ and the transforms files of a dataset directory")
    p.add_argument("path", type=str, help="the dataset directory: ori_imgs/, parsing/ and, for task 9, track_params.pt")
    p.add_argument("--task", type=int, default=-1, help="5 background, 6 torso and gt images, 9 transforms; -1: all three")
    p.add_argument("--bg_stride", type=int, default=20, help="task 5 takes every bg_stride-th frame")
    p.add_argument("--batch", type=int, default=64, help="frames on the device at a time")
    p.add_argument("--jpeg_quality", type=int, default=95)
    p.add_argument("--jpeg_subsampling", type=str, default="420", choices=("420", "444"))
    p.add_argument("--device", type=str, default="cuda")
    return p


def main(argv=None, log=print, decode=None, write=None):
    """python -m radnerf.prepare DIR [--task N].  Returns the list of tasks that ran."""
    p = build_parser()
    a = p.parse_args(argv)
    if a.task in ELSEWHERE:
        p.error(f"task {a.task} is not built here: its output comes from {ELSEWHERE[a.task]}.  Tasks 5, 6 and 9 (or -1) are.")
    if a.task not in (-1, 5, 6, 9):
        p.error(f"--task is one of -1, 5, 6, 9, got {a.task}")
    if a.bg_stride < 1 or a.batch < 1 or not 1 <= a.jpeg_quality <= 100:
        p.error("--bg_stride and --batch are at least 1, --jpeg_quality is 1 .. 100")
    if not os.path.isdir(os.path.join(a.path, "ori_imgs")):
        p.error(f"{a.path} has no ori_imgs/ directory")
    ran = []
    if a.task in (-1, 5):
        extract_background(a.path, a.bg_stride, a.batch, a.jpeg_quality, a.jpeg_subsampling, a.device, decode, log)
        ran.append(5)
    if a.task in (-1, 6):
        extract_torso_and_gt(a.path, a.batch, a.jpeg_quality, a.jpeg_subsampling, a.device, decode, write, log)
        ran.append(6)
    if a.task == 9 or (a.task == -1 and os.path.exists(os.path.join(a.path, "track_params.pt"))):
        save_transforms(a.path, decode, log)
        ran.append(9)
    elif a.task == -1:
        log("prepare: no track_params.pt, task 9 skipped")
    return ran


if __name__ == "__main__":
    import sys
    main(sys.argv[1:])
