"""Loads libradnerf_hip.so and declares its C ABI (include/*.h) on it, once, from the table in radnerf_hip/abi.py.

PyTorch is only plumbing here: it owns device memory and the current HIP stream; every kernel
of the render hot path lives in the shared object.  There is NO CPU or eager fallback: if the
library is missing this import fails, and calling an op with tensors that cannot be moved to a
GPU fails inside torch, exactly like the reference's `.cuda()` calls do
(raymarching/raymarching.py:34-35).
"""
import ctypes as C
import os

import torch

from . import abi
from .abi import RN_F16, RN_F32, RN_LAYOUT_BLC, RN_LAYOUT_BLC_LEVELMAJOR, RN_LAYOUT_LBC  # noqa: F401

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(_ROOT, "lib", "libradnerf_hip.so")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} not found: the HIP extension is not built. Run `python rad-nerf_amd/build.py` "
        "(or __graft_entry__.build()). There is no fallback path.")

_lib = C.CDLL(LIB_PATH)
abi.bind(_lib)


def exported_symbols():
    """Every function include/*.h declares (abi.FUNCTIONS has one entry for each; tests/test_abi.py checks it)."""
    return sorted(abi.FUNCTIONS)


def prof_enable(on=True):
    _lib.rn_prof_enable(1 if on else 0)


def prof_pause(paused=True):
    """Suspend / resume the kernel timing without dropping what was recorded."""
    _lib.rn_prof_pause(1 if paused else 0)


def prof_collect():
    """(launches, total_ms) of the fused per-sample kernel since prof_enable(True)."""
    n, ms = C.c_uint32(0), C.c_float(0.0)
    rc = _lib.rn_prof_collect(C.byref(n), C.byref(ms))
    if rc != 0:
        raise RuntimeError(f"rn_prof_collect failed ({rc}): {last_error()}")
    return int(n.value), float(ms.value)


def last_error():
    return _lib.rn_last_error().decode()


def version():
    return _lib.rn_version()


def device_count():
    return _lib.rn_device_count()


def stream():
    """Raw hipStream_t of torch's current stream (kernels are enqueued on it, never on the null stream)."""
    return torch.cuda.current_stream().cuda_stream


class KernelTimer:
    """Optional HIP-event timing of selected C-ABI calls, on the stream they launch on (torch's current
    stream).  `select(name, args)` returns a key (or None to skip); durations are read after a sync."""

    def __init__(self, select):
        self.select = select
        self.events = {}

    def results(self):
        torch.cuda.synchronize()
        out = {}
        for key, evs in self.events.items():
            ms = [a.elapsed_time(b) for a, b in evs]
            out[key] = dict(launches=len(ms), total_ms=float(sum(ms)), avg_ms=float(sum(ms) / max(len(ms), 1)))
        return out


_timer = None


def set_timer(timer):
    global _timer
    _timer = timer


def call(name, *args):
    if _timer is not None:
        key = _timer.select(name, args)
        if key is not None:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            rc = getattr(_lib, name)(*args)
            b.record()
            _timer.events.setdefault(key, []).append((a, b))
            if rc != 0:
                raise RuntimeError(f"{name} failed ({rc}): {last_error()}")
            return
    rc = getattr(_lib, name)(*args)
    if rc != 0:
        raise RuntimeError(f"{name} failed ({rc}): {last_error()}")


def prof_durations(capacity=1 << 16):
    """Per-launch durations (ms) of the fused per-sample kernel since prof_enable(True)."""
    buf = (C.c_float * capacity)()
    n = _lib.rn_prof_durations(buf, capacity)
    if n < 0:
        raise RuntimeError(f"rn_prof_durations failed ({n}): {last_error()}")
    return [float(buf[i]) for i in range(n)]


def workspace_bytes(name, n):
    return int(getattr(_lib, name)(n))


_HOST_OFFSETS = {}


def host_offsets(offsets):
    """Host copy (ctypes int32 array) of a grid's `offsets` buffer, made once per buffer (one synchronising copy, then
    cached on its address + version): the planned grid forward sizes its LDS staging from the level sizes."""
    # cached ON the tensor object (with its version): an address-keyed cache would hand a new buffer that happens to reuse a freed
    # one's address the OLD grid's level sizes
    hit = getattr(offsets, "_rn_host_offsets", None)
    if hit is not None and hit[0] == offsets._version:
        return hit[1]
    vals = offsets.detach().to("cpu", torch.int32).tolist()
    arr = (C.c_int32 * len(vals))(*vals)
    try:
        offsets._rn_host_offsets = (offsets._version, arr)
    except AttributeError:
        pass
    return arr


def workspace_bytes_grid(B, L, Cc, dtype_id):
    return int(_lib.rn_grid_encode_forward_workspace(int(B), int(L), int(Cc), int(dtype_id)))


def grid_forward_workspace(B, L, Cc, dtype_id, device):
    """Scratch for rn_grid_encode_forward_ws ([B, L*C] layout): one chunk of level-major features."""
    return workspace(int(_lib.rn_grid_encode_forward_workspace(int(B), int(L), int(Cc), int(dtype_id))), device)


def dev(t):
    """Reference wrappers move stray CPU tensors to the GPU (raymarching/raymarching.py:34-35)."""
    return t if t.is_cuda else t.cuda()


def ptr(t, dtype=None):
    """Device pointer of a contiguous CUDA tensor (None -> NULL).

    The caller must keep `t` referenced until the C-ABI call has been made: a temporary such as
    ptr(x.contiguous()) is freed as soon as ptr() returns and its block can be handed out again
    before the kernel is even enqueued."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("radnerf_hip: expected a CUDA (ROCm) tensor; the HIP path has no CPU fallback")
    if not t.is_contiguous():
        raise RuntimeError("radnerf_hip: tensor must be contiguous")
    if dtype is not None and t.dtype != dtype:
        raise RuntimeError(f"radnerf_hip: expected dtype {dtype}, got {t.dtype}")
    return t.data_ptr()


def mark_written(tensors):
    """Tell PyTorch that kernels wrote these tensors through raw pointers (the one-kernel Adam update, a replayed hipGraph):
    bump their version counters, which is what caches of derived data key on (FusedState's packed weight images,
    GridEncoder.half_table) -- otherwise they would keep serving the values of the first pack."""
    ts = [t for t in tensors if t is not None]
    if ts:
        torch._C._autograd._unsafe_set_version_counter(ts, [t._version + 1 for t in ts])


def aligned(t, nbytes=16):
    """Contiguous tensor whose base address is `nbytes`-aligned (vector loads in the kernels)."""
    t = t.contiguous()
    if t.data_ptr() % nbytes:
        t = t.clone(memory_format=torch.contiguous_format)
    return t


_WS = {}


def persistent_buffer(key, nbytes, device, zero=False, keep_replaced=False):
    """uint8 buffer of at least `nbytes` that belongs to `key` on `device`: created on the first request (zero-filled if asked)
    and kept at its address from then on -- only a larger request replaces it.  A captured step replays that address, so the
    buffer must exist, at its final size, before the capture.  keep_replaced: a buffer that a larger one replaces is never
    freed -- for a buffer whose address graphs captured EARLIER keep replaying after it has grown (GraphedTrainer caches its
    graphs per capacity): they go on using the old one, which only has to exist, not to hold anything between launches."""
    key = (device.index if device.index is not None else torch.cuda.current_device(), key)
    buf = _PERSISTENT.get(key)
    if buf is None or buf.numel() < nbytes:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"radnerf_hip: the buffer {key[1]!r} ({nbytes} bytes) must exist before a step is captured "
                               "(take one eager step, or call the route's prepare(), first)")
        if buf is not None and keep_replaced:
            _REPLACED.append(buf)
        buf = _PERSISTENT[key] = (torch.zeros if zero else torch.empty)(int(nbytes), dtype=torch.uint8, device=device)
    return buf


_PERSISTENT = {}
_REPLACED = []      # superseded keep_replaced buffers: alive for as long as the process, a captured graph may hold their address


def workspace(nbytes, device):
    """Small per-device scratch buffer, grown on demand, reused across calls on one stream."""
    key = (device.index if device.index is not None else torch.cuda.current_device())
    buf = _WS.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 1 << 16), dtype=torch.uint8, device=device)
        _WS[key] = buf
    return buf
