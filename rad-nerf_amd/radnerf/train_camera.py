"""The pose code of --train_camera as one forward and one backward call into the library (csrc/rn_train_camera.hip, C ABI
include/radnerf_train.h: rn_camera_rays_forward / rn_camera_rays_backward).  Opt-in: RN_TRAIN_CAMERA=fused.

Reference: NeRFRenderer.run_cuda (nerf/renderer.py:170-174) -- `rays_o + camera_dT[index]`, `rays_d @ euler_angles_to_matrix(
camera_dR[index] / 180 * pi + 1e-8)` -- differentiated by torch.autograd: ~30 small launches forward, more backward, two of them
index_put passes that build the dense gradients of the two tables.  Here the forward is one launch and the backward two (partial
sums per 256 rays, then one workgroup that adds them in a fixed order and writes both gradient tables whole, zeros included).
The frame's row is an int64 scalar on the device, so nothing depends on the host knowing it: a captured step replays the same
launches for whatever frame the feed wrote there.  Nothing persistent is allocated here; the backward's workspace (12 floats per
256 rays) is a temporary of the caching allocator like every other buffer of the step.
"""
import torch

import radnerf_hip as hip

from . import switches
from .route import training_call

_lib = hip._lib


def enabled():
    return switches.get("RN_TRAIN_CAMERA") == "fused"


def usable(model, rays_o, rays_d, index):
    """RN_TRAIN_CAMERA=fused, CUDA fp32 rays and tables, grad on, autocast off, rays that carry no gradient themselves (the
    backward returns none for them), one frame index."""
    dT, dR = model.camera_dT, model.camera_dR
    if not enabled() or not training_call(rays_o, rays_d, dT, dR):
        return False
    if rays_o.requires_grad or rays_d.requires_grad or dT.shape != dR.shape or dT.dim() != 2 or dT.shape[1] != 3:
        return False
    if torch.is_tensor(index):
        return index.is_cuda and index.dtype == torch.int64 and index.numel() == 1
    return isinstance(index, (list, tuple)) and len(index) == 1


def index_tensor(model, index, dev):
    """The frame's row as an int64 device tensor.  A device tensor is used as it is (the kernels wrap a negative value and ignore
    a row outside the tables).  A Python list is checked here, on the host, before anything is launched -- IndexError as
    `camera_dT[index]` raises it, a negative index wrapped as torch wraps it -- and uploaded once per distinct value through the
    model's cache (renderer._index_tensor: never inside a capture once the value has been seen)."""
    if torch.is_tensor(index):
        return index.reshape(-1)
    rows = int(model.camera_dT.shape[0])
    i = int(index[0])
    if not -rows <= i < rows:
        raise IndexError(f"index {i} is out of bounds for dimension 0 with size {rows}")
    return model._index_tensor([i + rows if i < 0 else i], dev).reshape(-1)


class _CameraRays(torch.autograd.Function):
    """(rays_o + camera_dT[index], rays_d @ R(camera_dR[index])) for rays [N,3]; index: int64 device tensor with one element."""

    @staticmethod
    def forward(ctx, rays_o, rays_d, camera_dT, camera_dR, index_dev):
        N, rows = rays_o.shape[0], camera_dT.shape[0]
        rays_o, rays_d = rays_o.contiguous(), rays_d.contiguous()
        dT, dR = camera_dT.detach().contiguous(), camera_dR.detach().contiguous()
        out = torch.empty(2, N, 3, dtype=torch.float32, device=rays_o.device)
        hip.call("rn_camera_rays_forward", hip.ptr(rays_o), hip.ptr(rays_d), hip.ptr(dT), hip.ptr(dR), hip.ptr(index_dev), rows, N,
                 out[0].data_ptr(), out[1].data_ptr(), hip.stream())
        ctx.save_for_backward(rays_d, dR, index_dev)
        ctx.shape = (N, rows)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_o, g_d):
        rays_d, dR, index_dev = ctx.saved_tensors
        N, rows = ctx.shape
        dev = rays_d.device
        g_o = g_o.contiguous() if g_o.dtype == torch.float32 else g_o.float().contiguous()
        g_d = g_d.contiguous() if g_d.dtype == torch.float32 else g_d.float().contiguous()
        grads = torch.empty(2, rows, 3, dtype=torch.float32, device=dev)          # written whole by the launch, zeros included
        work = torch.empty(int(_lib.rn_camera_rays_workspace(N)) // 4, dtype=torch.float32, device=dev)
        hip.call("rn_camera_rays_backward", hip.ptr(g_o), hip.ptr(g_d), hip.ptr(rays_d), hip.ptr(dR), hip.ptr(index_dev), rows, N,
                 grads[0].data_ptr(), grads[1].data_ptr(), hip.ptr(work), hip.stream())
        return None, None, grads[0], grads[1], None


def camera_rays(model, rays_o, rays_d, index):
    """rays [N,3] -> the rays of the frame's trained camera pose; call when usable()."""
    idx = index_tensor(model, index, rays_o.device)
    return _CameraRays.apply(rays_o, rays_d, model.camera_dT, model.camera_dR, idx)
