"""ClipScene: a trained model driven by a pose file and an audio-feature file -- the inference-side counterpart of the
reference's NeRFDataset_Test (nerf/provider.py:84-308), with the interface SyntheticScene exposes to FrameParallelRenderer and
TileParallelRenderer.

Per frame i (collate, :250-290, over dataloader's range(len(auds)), :292-308): the audio window is cut around the ORIGINAL index,
the pose and the eye value come from mirror_index(i, n_poses) -- the pose stream replays forwards, backwards, forwards ... under
a longer audio --, the individual code is 0, and the file's background is one [1, H*W, 3] float32 array (uint8 / 255, built
once).  Everything is uploaded once in the constructor; frame() hands out device tensors and, on the fused engine, a
`ray_source` for the frame prologue kernel, exactly as SyntheticScene.frame does.
"""
import numpy as np
import torch

from .dataset import mirror_index
from .rays import convert_poses, get_audio_features, get_bg_coords, get_rays
from .scene import SyntheticScene


class ClipScene(SyntheticScene):
    def __init__(self, model, clip, opt, device="cuda"):
        self.H, self.W = int(clip.H), int(clip.W)
        self.device = torch.device(device)
        self.opt = opt
        self.model = model.to(self.device).eval()
        self.model.ray_order_width = self.W
        self.intrinsics = np.asarray(clip.intrinsics, dtype=np.float32).reshape(4)
        self.poses = torch.as_tensor(clip.poses).to(self.device, torch.float32).contiguous()
        self.n_poses = int(self.poses.shape[0])
        self.aud_features = torch.as_tensor(clip.auds).to(self.device, torch.float32).contiguous()
        self.n_frames = int(self.aud_features.shape[0])                    # dataloader(): the clip is as long as its audio
        if self.n_poses < 1 or self.n_frames < 1:
            raise ValueError("ClipScene: the clip needs at least one pose and one audio frame")
        on_device = self._on_device()
        if on_device:
            from . import fused as _fused
            self.poses6 = _fused.convert_poses(self.poses)
            self.bg_coords = _fused.get_bg_coords(self.H, self.W, self.device)
        else:
            self.poses6 = convert_poses(self.poses)
            self.bg_coords = get_bg_coords(self.H, self.W, self.device)
        bg = np.asarray(clip.bg)
        if bg.dtype != np.uint8 or bg.shape != (self.H, self.W, 3):
            raise ValueError(f"ClipScene: the background must be uint8 [{self.H},{self.W},3], got {bg.dtype} {bg.shape}")
        lut = np.arange(256, dtype=np.float32) / np.float32(255)           # provider.py:178
        self.bg_color = torch.from_numpy(lut[bg].reshape(1, self.H * self.W, 3)).to(self.device)
        fix_eye = float(getattr(opt, "fix_eye", -1))
        self._eyes = None
        if getattr(opt, "exp_eye", False):
            eyes = torch.as_tensor(clip.eye_area).to(self.device, torch.float32).reshape(self.n_poses, 1)
            if fix_eye >= 0:
                eyes = torch.full_like(eyes, fix_eye)
            self._eyes = eyes.contiguous()
        self._constant_eye = self._eyes is None or fix_eye >= 0 or bool((self._eyes == self._eyes[0]).all())
        self._rays = {}

    @classmethod
    def from_files(cls, model, opt, device="cuda", decode=None):
        """opt.pose, opt.aud (and opt.bg_img) through datafiles.load_clip."""
        from .datafiles import load_clip
        return cls(model, load_clip(opt, decode=decode), opt, device)

    def _on_device(self):
        return (self.device.type == "cuda" and getattr(self.opt, "engine", "ops") == "fused"
                and getattr(self.opt, "ray_engine", "fused") == "fused")

    @property
    def eye(self):
        """The clip's one eye value ([1,1]; None without exp_eye): what a renderer that prepares several frames' bias blocks at
        once (audio_batch > 0) bakes into them.  A clip with per-frame values has no such thing."""
        if not self._constant_eye:
            raise AttributeError("ClipScene: this clip has per-frame eye values; a batched audio pass (audio_batch > 0) bakes ONE "
                                 "value into its bias blocks -- render with audio_batch=0, or set opt.fix_eye")
        return None if self._eyes is None else self._eyes[0:1]

    def _auds(self, i):
        """Frame i's audio window; a scene whose audio comes from elsewhere (radnerf/live.py) overrides this."""
        return get_audio_features(self.aud_features, self.opt.att, i)

    def render(self, i, want_u8=False, audio_code=None):
        """SyntheticScene.render; the frame's whole output dict stays at `last_out` (a caller that drives the scene through a
        renderer gets only the uint8 frame back, and the depth map is wanted next to it)."""
        self.last_out = super().render(i, want_u8=want_u8, audio_code=audio_code)
        return self.last_out

    def frame(self, i, lazy_rays=False):
        """Inputs of model.render for frame i of the clip (everything resident on the device)."""
        i = int(i) % self.n_frames
        p = mirror_index(i, self.n_poses)
        base = dict(auds=self._auds(i), bg_coords=self.bg_coords, poses=self.poses6[p:p + 1],
                    eye=None if self._eyes is None else self._eyes[p:p + 1], index=0, bg_color=self.bg_color,
                    poses_matrix=self.poses[p:p + 1])
        if lazy_rays and self._lazy_rays():
            bufs = self.__dict__.setdefault("_ray_bufs", {})
            key = torch.cuda.current_stream().cuda_stream
            if key not in bufs:
                bufs[key] = (torch.empty(1, self.H * self.W, 3, device=self.device), torch.empty(1, self.H * self.W, 3, device=self.device))
            return dict(base, rays_o=bufs[key][0], rays_d=bufs[key][1], ray_source=(self.poses[p], self.intrinsics, self.W))
        if p not in self._rays:
            if self._on_device():
                from . import fused
                r = fused.get_rays(self.poses[p], self.intrinsics, self.H, self.W)
            else:
                r = get_rays(self.poses[p:p + 1], self.intrinsics, self.H, self.W, -1)
            self._rays[p] = (r["rays_o"].contiguous(), r["rays_d"].contiguous())
        rays_o, rays_d = self._rays[p]
        return dict(base, rays_o=rays_o, rays_d=rays_d)
