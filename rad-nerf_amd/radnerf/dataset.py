"""The training step's input stage for a data set that already lives in device memory: the loader's batch of one frame, built
by ONE kernel launch over the N picked pixels (C ABI rn_train_set_batch / _batch_rect / _batch_patch / rn_train_set_frame,
csrc/rn_train_batch.hip).

Reference: NeRFDataset.collate (nerf/provider.py:625-714) with mirror_index (:615-622), get_rays (nerf/utils.py:249-333),
get_audio_features (:42-72), convert_poses (:231-237) and the dataloader's shuffle (provider.py:729).  With the data preloaded
the reference blends the FULL frame's torso over the background, builds a full-frame meshgrid and gathers five times per
step; here the decoded arrays stay uint8 (7 bytes per pixel and frame) and only the picked pixels are touched.

Values are the reference's float32 loader arithmetic (`--preload 0` / `1`: `astype(np.float32) / 255`, float32 blend).  Its
`--preload 2` keeps fp16 copies of the images; that rounding is NOT reproduced.  Decoding files (cv2, json, the audio
features' .npy) is not part of this module: a loader hands over arrays -- radnerf/datafiles.py is that loader, and
DeviceTrainSet.from_directory() builds the set from a dataset directory through it.

The two samplings of lip fine-tuning (nerf/utils.py:277-303) are further instantiations of the same kernel: batch_rect() takes
every pixel of a rect -- by default the frame's lips rect (provider.py:488-502, lips_rect_from_landmarks) -- and batch_patch()
`num_rays // patch_size^2` square patches whose corners the kernel draws.  Their ray count follows the rect, so such a batch
feeds the eager trainer (radnerf/train.py: train_step's patch_criterion, lips_schedule) or, opt-in, a GraphedTrainer that keeps
one captured graph per rect shape (lips_graphs; lips_shapes() counts the shapes).

On CPU tensors, or with RN_TRAIN_SET=torch (or kernel="torch"), the same class runs a plain-torch path that restates collate on
the N picked pixels: the oracle of the kernel's tests, itself pinned to the reference by tests/golden/reference_batch.npz.
"""
import ctypes

import numpy as np
import torch

from . import switches
from .rays import convert_poses, get_audio_features

_MASK32 = 0xFFFFFFFF


def mirror_index(index, size):
    """provider.py:615-622: frames replay forwards, then backwards, then forwards ..."""
    turn, res = divmod(int(index), int(size))
    return res if turn % 2 == 0 else size - res - 1


def _mix32(x):
    """rn_common.h's mix32 on int64 tensors that hold uint32 values (an int64 product wraps, its low 32 bits are exact)."""
    x = x ^ (x >> 16)
    x = (x * 0x7feb352d) & _MASK32
    x = x ^ (x >> 15)
    x = (x * 0x846ca68b) & _MASK32
    return x ^ (x >> 16)


def drawn_pixels(seed, draw, n, n_px, device):
    """The kernel's own draw (csrc/rn_train_batch.hip drawn_pixel): pixel k of draw `draw` of stream `seed`."""
    k = torch.arange(n, dtype=torch.int64, device=device)
    h = _mix32(_mix32(_mix32(k) ^ (int(draw) & _MASK32)) ^ (int(seed) & _MASK32))
    return (h * int(n_px)) >> 32


def drawn_corners(seed, draw, P, H, W, patch, device):
    """The kernel's own draw of P patch corners (csrc/rn_train_batch.hip patch_corner): int64 [P,2] = (x0, y0), x0 from element
    2q of draw `draw` of stream `seed` onto [0, H - patch), y0 from element 2q + 1 onto [0, W - patch) -- randint's exclusive
    upper end (nerf/utils.py:282-283)."""
    e = torch.arange(2 * int(P), dtype=torch.int64, device=device)
    h = _mix32(_mix32(_mix32(e) ^ (int(draw) & _MASK32)) ^ (int(seed) & _MASK32))
    return torch.stack(((h[0::2] * (int(H) - int(patch))) >> 32, (h[1::2] * (int(W) - int(patch))) >> 32), dim=-1)


def lips_rect_from_landmarks(lms, H, W):
    """provider.py:488-502: the lips rect (xmin, xmax, ymin, ymax; x along the ROWS) of one frame's 68 face landmarks [68,2] =
    (column, row) -- the bounding box of landmarks 48..59, padded to a square around its centre and clipped to the image.
    [F,68,2] gives a list of F rects."""
    lms = np.asarray(lms)
    if lms.ndim == 3:
        return [lips_rect_from_landmarks(one, H, W) for one in lms]
    lips = lms[48:60]
    xmin, xmax = int(lips[:, 1].min()), int(lips[:, 1].max())
    ymin, ymax = int(lips[:, 0].min()), int(lips[:, 0].max())
    cx, cy = (xmin + xmax) // 2, (ymin + ymax) // 2
    half = max(xmax - xmin, ymax - ymin) // 2
    return [max(0, cx - half), min(int(H), cx + half), max(0, cy - half), min(int(W), cy + half)]


class DeviceTrainSet:
    """images [F,H,W,3], torso [F,H,W,4] (RGBA), bg [H,W,3]: uint8 (numpy or torch), kept uint8 on the device.  poses [F,4,4]
    cam2world, intrinsics (fx, fy, cx, cy), auds [Fa,C,16], face_rect [F,4] = (xmin, xmax, ymin, ymax) with x along the ROWS
    (provider.py:657-658), eye_area [F] or [F,1] (needed with opt.exp_eye).  `opt` supplies att, torso and exp_eye.  lips_rect
    [F,4] (optional, same convention): what batch_rect() samples by default (provider.py:488-502)."""

    _WIDTHS = (3, 3, 2, 3, 3, 1)          # rays_o | rays_d | bg_coords | bg_color | target | face: SyntheticTrainStream's sections
    _FRAME_WIDTHS = (3, 3, 2, 3, 3)       # the evaluation form has no face section

    def __init__(self, images, torso, bg, poses, intrinsics, auds, face_rect, eye_area=None, opt=None, num_rays=4096, seed=0,
                 device="cuda", kernel=None, lips_rect=None):
        dev = self.device = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = self.device = torch.device("cuda", torch.cuda.current_device())

        def u8(x, name):
            x = torch.as_tensor(x)
            if x.dtype != torch.uint8:
                raise TypeError(f"DeviceTrainSet: {name} must be uint8 (the decoded image bytes), got {x.dtype}")
            return x.to(dev).contiguous()

        self.images, self.torso_img, self.bg_img = u8(images, "images"), u8(torso, "torso"), u8(bg, "bg")
        F, H, W = self.images.shape[:3]
        if self.images.shape != (F, H, W, 3) or self.torso_img.shape != (F, H, W, 4) or self.bg_img.shape != (H, W, 3):
            raise ValueError("DeviceTrainSet: expected images [F,H,W,3], torso [F,H,W,4] and bg [H,W,3]")
        if H < 2 or W < 2 or H * W >= 2 ** 31:
            raise ValueError("DeviceTrainSet: H, W >= 2 and H * W < 2^31 are required")
        self.F, self.H, self.W = int(F), int(H), int(W)
        self.poses = torch.as_tensor(poses).to(dev, torch.float32).contiguous()
        self.auds = torch.as_tensor(auds).to(dev, torch.float32).contiguous()
        rect = torch.as_tensor(face_rect).to(torch.int32).cpu()
        if self.poses.shape != (F, 4, 4) or rect.shape != (F, 4) or self.auds.dim() != 3 or self.auds.shape[2] != 16:
            raise ValueError("DeviceTrainSet: expected poses [F,4,4], face_rect [F,4] and auds [Fa,C,16]")
        if self.auds.shape[0] < 8:
            raise ValueError("DeviceTrainSet: at least 8 audio frames are required (the window's padding below that is not restated)")
        self._rect_host = rect.tolist()
        self.face_rect = rect.to(dev).contiguous()
        self._lips_host = None
        if lips_rect is not None:
            lips = torch.as_tensor(lips_rect).to(torch.int32).cpu()
            if lips.shape != (F, 4):
                raise ValueError("DeviceTrainSet: expected lips_rect [F,4]")
            self._lips_host = lips.tolist()
            for r in self._lips_host:
                self._checked_rect(r)
        self.intrinsics = np.asarray(intrinsics, dtype=np.float32).reshape(4)
        self.opt = opt
        self.att, self.torso, self.exp_eye = int(opt.att), bool(opt.torso), bool(opt.exp_eye)
        if self.att not in (0, 1, 2):
            raise NotImplementedError(f"wrong att_mode: {self.att}")
        self.eye_area = None
        if eye_area is not None:
            self.eye_area = torch.as_tensor(eye_area).to(dev, torch.float32).reshape(F, 1).contiguous()
        if self.exp_eye and self.eye_area is None:
            raise ValueError("DeviceTrainSet: opt.exp_eye needs eye_area")
        self.num_rays, self.seed, self._draw = int(num_rays), int(seed), 0
        if kernel is None:
            kernel = switches.get("RN_TRAIN_SET") if dev.type == "cuda" else "torch"
        if kernel not in ("hip", "torch") or (kernel == "hip" and dev.type != "cuda"):
            raise ValueError(f"DeviceTrainSet: kernel={kernel!r} on {dev}: the kernel needs a GPU, the other path is 'torch'")
        self.kernel = kernel

        rows, C = (1 if self.att == 0 else 8), int(self.auds.shape[1])
        self._poses6 = torch.zeros(1, 6, device=dev)
        self._pose_matrix = torch.zeros(1, 4, 4, device=dev)
        self._eye = torch.zeros(1, 1, device=dev) if self.exp_eye else None
        self._auds = torch.zeros(rows, C, 16, device=dev)
        self._bad = torch.zeros(1, dtype=torch.int32, device=dev)
        self._bufs, self._frame_buf, self._index, self._last = {}, None, [0], None
        self._rect_buf = None             # batch_rect's outputs: ONE buffer at the largest lips rect, whatever the frame's size
        self._frame_ids = torch.arange(self.F, dtype=torch.int64, device=dev)     # `index` as a device tensor: a view of this, no upload
        if kernel == "hip":
            import radnerf_hip as hip
            self._hip = hip
            fx, fy, cx, cy = (float(v) for v in self.intrinsics)
            self._desc = hip.abi.TrainSetT(
                images=hip.ptr(self.images), torso=hip.ptr(self.torso_img), bg=hip.ptr(self.bg_img), poses=hip.ptr(self.poses),
                face_rect=hip.ptr(self.face_rect), eye=hip.ptr(self.eye_area) if self.exp_eye else None, auds=hip.ptr(self.auds),
                fx=fx, fy=fy, cx=cx, cy=cy, H=self.H, W=self.W, F=self.F, Fa=int(self.auds.shape[0]), C=C, att=self.att,
                torso_mode=int(self.torso))
        else:
            # what the torch path divides by lives on the device: torch turns a division by a HOST scalar into a multiplication by
            # its reciprocal on the GPU, which is not the reference's (CPU) arithmetic
            t = lambda v: torch.tensor(float(v), dtype=torch.float32, device=dev)
            self._fx, self._fy, self._cx, self._cy = (t(v) for v in self.intrinsics)
            self._lut = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255)).to(dev)   # provider.py:671, 694
            self._X = torch.arange(H, device=dev).float() / t(H - 1) * 2 - 1                          # nerf/utils.py:241-242
            self._Y = torch.arange(W, device=dev).float() / t(W - 1) * 2 - 1

    # ------------------------------------------------------------------------------------------------------- interface
    def mirror_index(self, index):
        return mirror_index(index, self.F)

    def order(self, epoch):
        """The frames of one epoch in the loader's shuffled order (DataLoader(shuffle=True), provider.py:729): a permutation of
        range(F) from a CPU generator seeded by (seed, epoch).  The frame index is a host integer; nothing here needs the device."""
        g = torch.Generator().manual_seed((self.seed * 1000003 + int(epoch)) & 0x7FFFFFFFFFFFFFFF)
        return torch.randperm(self.F, generator=g).tolist()

    def install(self, model):
        """What update_extra_state samples from (main.py:183-186 hands the loader's arrays to the model)."""
        model.aud_features, model.poses = self.auds, self.poses
        model.eye_area = self.eye_area
        return model

    @property
    def inds(self):
        """The pixels of the last batch() (device int64 [n]; out-of-range entries of an explicit `inds` clamped)."""
        return self._last

    def clone(self, kernel=None, num_rays=None, seed=None):
        """A second set over the SAME device arrays (nothing is copied) with its own output buffers and draw counter, e.g. the
        torch path next to the kernel."""
        return type(self)(self.images, self.torso_img, self.bg_img, self.poses, self.intrinsics, self.auds, self.face_rect,
                          eye_area=self.eye_area, opt=self.opt, num_rays=self.num_rays if num_rays is None else num_rays,
                          seed=self.seed if seed is None else seed, device=self.device, kernel=kernel, lips_rect=self._lips_host)

    @property
    def lips_rect(self):
        """[F][4] host integers (xmin, xmax, ymin, ymax), or None."""
        return self._lips_host

    def lips_shapes(self):
        """{(h, w): number of frames} of the set's lips rects, h along the rows -- what batch_rect() will hand out.  A captured
        lips step needs one graph per shape and row capacity (radnerf/train.py: GraphedTrainer's lips_graphs is sized from this).
        Host only."""
        if self._lips_host is None:
            raise ValueError("DeviceTrainSet.batch_rect: the set has no lips_rect; pass rect=(xmin, xmax, ymin, ymax)")
        shapes = {}
        for xmin, xmax, ymin, ymax in self._lips_host:
            shapes[(xmax - xmin, ymax - ymin)] = shapes.get((xmax - xmin, ymax - ymin), 0) + 1
        return shapes

    def check(self):
        """Raises when an explicit `inds` held pixels outside the image -- or explicit patch corners start positions outside
        the range the draw covers -- since the last check (they were clamped, never read out of bounds).  Reads one device word back: call it where the host waits for the device anyway."""
        bad = int(self._bad.item())
        if bad:
            self._bad.zero_()
            raise IndexError(f"DeviceTrainSet: {bad} pixel indices were outside [0, {self.H * self.W}), or patch corners outside "
                             "[0, H - patch) x [0, W - patch), and were clamped")

    def batch(self, index, inds=None):
        """The loader's training batch of frame index[0] (a Python list, as the reference's collate takes it): the dict
        SyntheticTrainStream.unpack returns -- per-ray entries are views of one `_packed` buffer that is rewritten in place by
        every call -- plus poses_matrix, H, W.  inds: explicit pixel indices (int64); None: `num_rays` pixels drawn on the device
        from (seed, draw counter), the counter advanced on the host.  One launch, nothing read back."""
        aud_frame, frame = self._frames(index)
        if inds is not None:
            inds = torch.as_tensor(inds).to(self.device, torch.int64).reshape(-1).contiguous()
        n = self.num_rays if inds is None else int(inds.numel())
        packed, picked = self._buf(n)
        if self.kernel == "hip":
            hip = self._hip
            hip.call("rn_train_set_batch", ctypes.byref(self._desc), frame, aud_frame, hip.ptr(inds), n, self.seed & _MASK32,
                     self._draw & _MASK32, hip.ptr(packed), hip.ptr(picked), hip.ptr(self._poses6), hip.ptr(self._pose_matrix),
                     hip.ptr(self._eye), hip.ptr(self._auds), hip.ptr(self._bad), hip.stream())
        else:
            n_px = self.H * self.W
            if inds is None:
                pix = drawn_pixels(self.seed, self._draw, n, n_px, self.device)
            else:
                self._bad += ((inds < 0) | (inds >= n_px)).sum().to(torch.int32)
                pix = inds.clamp(0, n_px - 1)
            picked.copy_(pix)
            self._torch_fill(frame, aud_frame, pix, packed, training=True)
        if inds is None:
            self._draw += 1
        self._index, self._last = [frame], picked
        return self.unpack(packed)

    def batch_rect(self, index, rect=None):
        """The batch of lip fine-tuning (provider.py:642-645, get_rays with `rect`, nerf/utils.py:297-303): EVERY pixel of `rect` =
        (xmin, xmax, ymin, ymax), x along the rows, in ascending order -- the frame's lips rect unless given.  The dict of batch()
        plus `rect`; the ray count is the rect's, so the views are laid out for this call inside one buffer sized for the
        largest lips rect of the set (a larger explicit rect replaces it once).  An empty rect, or one that leaves the image, is
        an error (the reference's slice would clamp silently).  One launch, nothing read back."""
        aud_frame, frame = self._frames(index)
        if rect is None:
            if self._lips_host is None:
                raise ValueError("DeviceTrainSet.batch_rect: the set has no lips_rect; pass rect=(xmin, xmax, ymin, ymax)")
            rect = self._lips_host[frame]
        xmin, xmax, ymin, ymax = rect = self._checked_rect(rect)
        w = ymax - ymin
        n = (xmax - xmin) * w
        packed, picked = self._rect_views(n)
        if self.kernel == "hip":
            hip = self._hip
            hip.call("rn_train_set_batch_rect", ctypes.byref(self._desc), frame, aud_frame, xmin, xmax, ymin, ymax, hip.ptr(packed),
                     hip.ptr(picked), hip.ptr(self._poses6), hip.ptr(self._pose_matrix), hip.ptr(self._eye), hip.ptr(self._auds),
                     hip.stream())
        else:
            k = torch.arange(n, dtype=torch.int64, device=self.device)
            i = torch.div(k, w, rounding_mode="floor")
            pix = (xmin + i) * self.W + ymin + (k - i * w)
            picked.copy_(pix)
            self._torch_fill(frame, aud_frame, pix, packed, training=True)
        self._index, self._last = [frame], picked
        out = self.unpack(packed)
        out["rect"] = rect
        return out

    def batch_patch(self, index, patch_size, corners=None):
        """The patch batch (`--patch_size`, get_rays nerf/utils.py:277-294): P = num_rays // patch_size^2 square patches, each in
        meshgrid 'ij' order.  corners: explicit top-left corners, int [P,2] = (x0, y0) with x along the rows (P is then theirs);
        one outside [0, H - patch_size) x [0, W - patch_size) is clamped and reported by check().  None: drawn on the device from
        (seed, draw counter) over exactly those ranges (drawn_corners).  The dict of batch() plus `patch_size`."""
        aud_frame, frame = self._frames(index)
        ps = int(patch_size)
        if not (2 <= ps < self.H and ps < self.W):
            raise ValueError(f"DeviceTrainSet.batch_patch: 2 <= patch_size < min(H, W) is required, got {ps} on {self.H} x {self.W}")
        if corners is None:
            if self.num_rays % (ps * ps) != 0 or self.num_rays < ps * ps:      # main.py:125
                raise ValueError(f"DeviceTrainSet.batch_patch: num_rays = {self.num_rays} is not a positive multiple of patch_size^2 = {ps * ps}")
            P = self.num_rays // (ps * ps)
        else:
            corners = torch.as_tensor(corners).to(self.device, torch.int32).reshape(-1, 2).contiguous()
            P = int(corners.shape[0])
            if P < 1:
                raise ValueError("DeviceTrainSet.batch_patch: at least one corner is required")
        n = P * ps * ps
        packed, picked = self._buf(n)
        if self.kernel == "hip":
            hip = self._hip
            hip.call("rn_train_set_batch_patch", ctypes.byref(self._desc), frame, aud_frame, hip.ptr(corners), P, ps, self.seed & _MASK32,
                     self._draw & _MASK32, hip.ptr(packed), hip.ptr(picked), hip.ptr(self._poses6), hip.ptr(self._pose_matrix),
                     hip.ptr(self._eye), hip.ptr(self._auds), hip.ptr(self._bad), hip.stream())
        else:
            nx, ny = self.H - ps, self.W - ps
            if corners is None:
                c = drawn_corners(self.seed, self._draw, P, self.H, self.W, ps, self.device)
            else:
                c = corners.to(torch.int64)
                self._bad += ((c[:, 0] < 0) | (c[:, 0] >= nx) | (c[:, 1] < 0) | (c[:, 1] >= ny)).sum().to(torch.int32)
                c = torch.stack((c[:, 0].clamp(0, nx - 1), c[:, 1].clamp(0, ny - 1)), dim=-1)
            o = torch.arange(ps * ps, dtype=torch.int64, device=self.device)
            i = torch.div(o, ps, rounding_mode="floor")
            pix = ((c[:, 0:1] + i) * self.W + c[:, 1:2] + (o - i * ps)).reshape(-1)       # nerf/utils.py:287-292
            picked.copy_(pix)
            self._torch_fill(frame, aud_frame, pix, packed, training=True)
        if corners is None:
            self._draw += 1
        self._index, self._last = [frame], picked
        out = self.unpack(packed)
        out["patch_size"] = ps
        return out

    def frame(self, index, aud_index=None):
        """The loader's evaluation form (training = False) of frame `index`: every pixel in order, no face mask.  The index is
        mirrored for the pose and the images (provider.py:637-640); the audio index -- `index` itself unless given -- is not."""
        aud_frame = int(index if aud_index is None else aud_index)
        frame = self.mirror_index(int(index))
        if not 0 <= aud_frame < self.auds.shape[0]:
            raise IndexError(f"DeviceTrainSet: audio frame {aud_frame} is outside the {self.auds.shape[0]} audio frames")
        n = self.H * self.W
        if self._frame_buf is None:
            self._frame_buf = torch.zeros(n * sum(self._FRAME_WIDTHS), device=self.device)
        flat = self._frame_buf
        if self.kernel == "hip":
            hip = self._hip
            hip.call("rn_train_set_frame", ctypes.byref(self._desc), frame, aud_frame, hip.ptr(flat), hip.ptr(self._poses6),
                     hip.ptr(self._pose_matrix), hip.ptr(self._eye), hip.ptr(self._auds), hip.stream())
        else:
            self._torch_fill(frame, aud_frame, torch.arange(n, device=self.device), flat, training=False)
        sec = self._sections(flat, n, self._FRAME_WIDTHS)
        return dict(rays_o=sec[0], rays_d=sec[1], bg_coords=sec[2], bg_color=sec[3], images=sec[4].view(1, self.H, self.W, 3),
                    poses=self._poses6, poses_matrix=self._pose_matrix, eye=self._eye, auds=self._auds, index=[frame], H=self.H,
                    W=self.W)

    def unpack(self, flat):
        """Batch dict over the sections of `flat` (see SyntheticTrainStream.unpack); the per-call entries are this set's own
        buffers, which the next batch() rewrites in place as well."""
        n = flat.numel() // sum(self._WIDTHS)
        sec = self._sections(flat, n, self._WIDTHS)
        return dict(rays_o=sec[0], rays_d=sec[1], bg_coords=sec[2], poses=self._poses6, face_mask=sec[5].view(1, n),
                    eye=self._eye, auds=self._auds, index=list(self._index), bg_color=sec[3], images=sec[4], bg_torso_color=sec[4],
                    poses_matrix=self._pose_matrix, H=self.H, W=self.W, _packed=flat, _unpack=self.unpack,
                    _index_dev=self._frame_ids[self._index[0]:self._index[0] + 1])

    # -------------------------------------------------------------------------------------------------------- internals
    @staticmethod
    def _sections(flat, n, widths):
        sec, at = [], 0
        for w in widths:
            sec.append(flat[at:at + n * w].view(1, n, w))
            at += n * w
        return sec

    def _frames(self, index):
        """(audio frame, mirrored frame) of a loader index list: the audio uses the original index (provider.py:632-640)."""
        aud_frame = int(index[0])
        if not 0 <= aud_frame < self.auds.shape[0]:
            raise IndexError(f"DeviceTrainSet: audio frame {aud_frame} is outside the {self.auds.shape[0]} audio frames")
        return aud_frame, self.mirror_index(aud_frame)

    def _checked_rect(self, rect):
        xmin, xmax, ymin, ymax = (int(v) for v in rect)
        if not (0 <= xmin < xmax <= self.H and 0 <= ymin < ymax <= self.W):
            raise ValueError(f"DeviceTrainSet: rect {(xmin, xmax, ymin, ymax)} is empty or outside the {self.H} x {self.W} image "
                             "(0 <= xmin < xmax <= H and 0 <= ymin < ymax <= W are required)")
        return xmin, xmax, ymin, ymax

    def _rect_views(self, n):
        """(packed [15 n], picked [n]) for a rect of n pixels: the head of ONE flat buffer allocated at the largest lips rect of
        the set -- rect sizes differ per frame, and a buffer per size would grow with every new one."""
        if self._rect_buf is None or self._rect_buf[1].numel() < n:
            cap = max([n] + [(r[1] - r[0]) * (r[3] - r[2]) for r in (self._lips_host or [])])
            self._rect_buf = (torch.zeros(cap * sum(self._WIDTHS), device=self.device),
                              torch.zeros(cap, dtype=torch.int64, device=self.device))
        flat, picked = self._rect_buf
        return flat[:n * sum(self._WIDTHS)], picked[:n]

    def _buf(self, n):
        if n not in self._bufs:       # allocated once per batch size, rewritten in place afterwards
            self._bufs[n] = (torch.zeros(n * sum(self._WIDTHS), device=self.device),
                             torch.zeros(n, dtype=torch.int64, device=self.device))
        return self._bufs[n]

    def _torch_fill(self, frame, aud_frame, pix, flat, training):
        """collate on the pixels `pix` (int64 [n], in range) with torch's elementwise kernels, written into `flat`."""
        n, H, W = int(pix.numel()), self.H, self.W
        r = torch.div(pix, W, rounding_mode="floor")
        c = pix - r * W
        i = c.to(torch.float32).view(1, n) + 0.5                              # nerf/utils.py:268-270 after the gather (:309-310)
        j = r.to(torch.float32).view(1, n) + 0.5
        zs = torch.ones_like(i)
        xs = (i - self._cx) / self._fx * zs                                   # :320-327
        ys = (j - self._cy) / self._fy * zs
        directions = torch.stack((xs, ys, zs), dim=-1)
        directions = directions / torch.norm(directions, dim=-1, keepdim=True)
        pose = self.poses[frame:frame + 1]
        rays_d = directions @ pose[:, :3, :3].transpose(-1, -2)
        rays_o = pose[..., :3, 3][..., None, :].expand_as(rays_d)
        bg_coords = torch.stack((self._X[r], self._Y[c]), dim=-1)            # provider.py:705

        t = self._lut[self.torso_img[frame].view(-1, 4)[pix].long()]         # provider.py:667-673 on the picked pixels
        bg = self._lut[self.bg_img.view(-1, 3)[pix].long()]
        blend = t[..., :3] * t[..., 3:] + bg * (1 - t[..., 3:])
        if training and self.torso:
            target = blend                                                    # bg_torso_color (:686-688)
        else:
            target = self._lut[self.images[frame].view(-1, 3)[pix].long()]    # :690-702
        bg_color = bg if self.torso else blend                                # :676-684

        widths = self._WIDTHS if training else self._FRAME_WIDTHS
        sec = self._sections(flat, n, widths)
        for dst, src in zip(sec, (rays_o, rays_d, bg_coords, bg_color, target)):
            dst.copy_(src.reshape(dst.shape))
        if training:
            xmin, xmax, ymin, ymax = self._rect_host[frame]                   # :657-658
            sec[5].copy_(((j >= xmin) & (j < xmax) & (i >= ymin) & (i < ymax)).to(torch.float32).view(1, n, 1))
        self._poses6.copy_(convert_poses(pose))
        self._pose_matrix.copy_(pose)
        if self._eye is not None:
            self._eye.copy_(self.eye_area[frame:frame + 1])
        self._auds.copy_(get_audio_features(self.auds, self.att, aud_frame))

    # ------------------------------------------------------------------------------------------------------ from files
    @classmethod
    def from_directory(cls, root, opt, split="train", num_rays=4096, seed=0, device="cuda", downscale=1, decode=None, kernel=None):
        """The set of one split of a dataset directory (radnerf/datafiles.py load_split: decoded once, on the host, uploaded as
        uint8).  The lips rects go in with opt.finetune_lips, the eye areas with opt.exp_eye, as the reference's loader keeps them
        (provider.py:475, 487).  `loaded` on the result is the LoadedSplit without its images (radius, frame ids, landmarks, has_gt)."""
        from .datafiles import load_split
        d = load_split(root, opt, split, downscale=downscale, decode=decode)
        ds = cls(d.images, d.torso, d.bg, d.poses, d.intrinsics, d.auds, d.face_rect,
                 eye_area=d.eye_area if getattr(opt, "exp_eye", False) else None, opt=opt, num_rays=num_rays, seed=seed, device=device,
                 kernel=kernel, lips_rect=d.lips_rect if getattr(opt, "finetune_lips", False) else None)
        d.images = d.torso = None          # the set holds them on the device; no second copy stays on the host
        ds.loaded = d
        return ds

    # --------------------------------------------------------------------------------------------------------- stand-in
    @classmethod
    def from_scene(cls, scene, n_frames, num_rays=4096, seed=0, kernel=None):
        """A stand-in data set for tests and tools: a synthetic torso RGBA (opaque lower-centre block with a soft edge) over a
        gradient background, and as ground truth `n_frames` frames of a SyntheticScene rendered once OVER THAT BLEND and quantised
        to uint8 -- the scene's own frozen render as target, as SyntheticTrainStream has it, so a head step sees a target its
        model can already produce.  The face rect is the bounding box of the pixels the head layer changed; poses and audio
        features are the scene's, the eye value is constant.  The lips rect of every frame: the square of half the face rect's
        shorter side, centred in the face rect and clipped as provider.py:492-500 clips."""
        if not 8 <= n_frames <= scene.n_frames:
            raise ValueError("from_scene: 8 <= n_frames <= scene.n_frames is required")
        H, W, m = scene.H, scene.W, scene.model
        rr = np.arange(H, dtype=np.float32)[:, None] / (H - 1)
        cc = np.arange(W, dtype=np.float32)[None, :] / (W - 1)
        alpha = np.clip((rr - 0.6) * 16, 0, 1) * np.clip((cc - 0.1) * 16, 0, 1) * np.clip((0.9 - cc) * 16, 0, 1)
        torso = np.zeros((n_frames, H, W, 4), dtype=np.uint8)
        torso[..., 0] = np.round(255 * (0.3 + 0.4 * cc * np.ones_like(rr)))
        torso[..., 1] = np.round(255 * (0.2 + 0.3 * rr * np.ones_like(cc)))
        torso[..., 2] = 96
        torso[..., 3] = np.round(255 * alpha)
        bg = np.zeros((H, W, 3), dtype=np.uint8)
        bg[..., 0] = np.round(255 * (0.9 - 0.2 * rr * np.ones_like(cc)))
        bg[..., 1] = np.round(255 * (0.8 + 0.1 * cc * np.ones_like(rr)))
        bg[..., 2] = 230
        t, b = torso[0].astype(np.float32) / np.float32(255), bg.astype(np.float32) / np.float32(255)
        blend = torch.from_numpy(t[..., :3] * t[..., 3:] + b * (1 - t[..., 3:])).to(scene.device)      # what batch() hands out as bg_color
        was_training, white = m.training, scene.bg_color
        m.eval()
        images, rects = [], []
        scene.bg_color = blend.reshape(1, H * W, 3)
        try:
            with torch.no_grad():
                for f in range(n_frames):
                    img = scene.render(f)["image"].reshape(H, W, 3).clamp(0, 1)
                    changed = ((img - blend).abs().sum(-1) > 1e-3).cpu()
                    rows, cols = torch.where(changed.any(1))[0], torch.where(changed.any(0))[0]
                    if rows.numel():
                        rects.append([int(rows[0]), int(rows[-1]) + 1, int(cols[0]), int(cols[-1]) + 1])
                    else:
                        rects.append([H // 4, 3 * H // 4, W // 4, 3 * W // 4])
                    images.append((img * 255).round().to(torch.uint8).cpu())
        finally:
            scene.bg_color = white
            m.train(was_training)
        lips = []
        for xmin, xmax, ymin, ymax in rects:
            cx, cy, half = (xmin + xmax) // 2, (ymin + ymax) // 2, max(min(xmax - xmin, ymax - ymin) // 4, 1)
            lips.append([max(0, cx - half), min(H, cx + half), max(0, cy - half), min(W, cy + half)])
        eye = np.full((n_frames,), 0.25, dtype=np.float32)
        return cls(torch.stack(images), torso, bg, scene.poses[:n_frames], scene.intrinsics, scene.aud_features[:n_frames], rects,
                   eye_area=eye, opt=scene.opt, num_rays=num_rays, seed=seed, device=scene.device, kernel=kernel,
                   lips_rect=lips)
