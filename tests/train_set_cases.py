"""Shared by tests/test_train_set_host.py and tests/test_gpu_train_set.py: the reference loader's recorded batches
(tests/golden/reference_batch.npz, written by tests/golden/make_golden_batch.py from the reference's own collate) and the
comparison of a DeviceTrainSet batch with one of them at the bars the issue sets."""
import os
from types import SimpleNamespace

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_batch.npz")
RAYS_D_TOL, POSES_TOL = 2e-7, 1e-6      # tests/test_gpu_render.py's bars for get_rays / convert_poses; everything else is bit-equal
_cache = {}


def golden():
    if "g" not in _cache:
        with np.load(GOLDEN) as z:
            _cache["g"] = {k: z[k] for k in z.files}
    return _cache["g"]


def cases():
    """[(tag, torso_mode, att, index), ...] of the recorded training batches."""
    return [(f"c{k}", bool(t), int(a), int(i)) for k, (t, a, i) in enumerate(golden()["cases"])]


def make_set(device, torso_mode, att, kernel=None, num_rays=None, seed=0, g=None, **replace):
    from radnerf.dataset import DeviceTrainSet
    g = dict(golden() if g is None else g, **replace)
    opt = SimpleNamespace(att=att, torso=torso_mode, exp_eye=True)
    return DeviceTrainSet(g["images"], g["torso"], g["bg"], g["poses"], g["intrinsics"], g["auds"], g["face_rect"],
                          eye_area=g["eye_area"], opt=opt, num_rays=int(g["shape"][3]) if num_rays is None else num_rays, seed=seed,
                          device=device, kernel=kernel)


def n(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def same_bits(a, b, what):
    a, b = n(a), n(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b), \
        f"{what}: {int((a != b).sum())} of {a.size} values differ, max |d| = {np.abs(a.astype(np.float64) - b).max():.3e}"


def close(a, b, tol, what):
    a, b = n(a), n(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    err = float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())
    print(f"{what}: max |d| = {err:.3e} (bar {tol:.0e})")
    assert err <= tol, f"{what}: max |d| = {err:.3e} > {tol:.0e}"


def compare_with_golden(out, tag, torso_mode, training=True, exact=False):
    """A batch() / frame() dict against the reference's recorded collate output `tag`.  exact: rays_d and poses bit-equal too
    (the torch path on the CPU runs the torch ops the reference ran)."""
    g = golden()
    if exact:
        same_bits(out["rays_d"], g[f"{tag}_rays_d"], f"{tag} rays_d")
        same_bits(out["poses"], g[f"{tag}_poses"], f"{tag} poses")
    for k in ("rays_o", "bg_coords", "bg_color", "eye", "auds", "poses_matrix"):
        same_bits(out[k], g[f"{tag}_{k}"], f"{tag} {k}")
    close(out["rays_d"], g[f"{tag}_rays_d"], RAYS_D_TOL, f"{tag} rays_d")
    close(out["poses"], g[f"{tag}_poses"], POSES_TOL, f"{tag} poses")
    assert list(out["index"]) == g[f"{tag}_index"].tolist() and out["H"] == g["shape"][1] and out["W"] == g["shape"][2]
    if not training:
        same_bits(out["images"], g[f"{tag}_images"], f"{tag} images")
        return
    same_bits(out["face_mask"], g[f"{tag}_face_mask"].astype(np.float32), f"{tag} face_mask")
    if torso_mode:
        same_bits(out["bg_torso_color"], g[f"{tag}_bg_torso_color"], f"{tag} bg_torso_color")
    else:
        same_bits(out["images"], g[f"{tag}_images"], f"{tag} images")


def compare_batches(a, b, what, training=True, index=True):
    """Two DeviceTrainSet dicts (kernel against torch path) at the same bars."""
    keys = ["rays_o", "bg_coords", "bg_color", "images", "eye", "auds", "poses_matrix"] + (["face_mask", "bg_torso_color"] if training else [])
    for k in keys:
        same_bits(a[k], b[k], f"{what} {k}")
    close(a["rays_d"], b["rays_d"], RAYS_D_TOL, f"{what} rays_d")
    close(a["poses"], b["poses"], POSES_TOL, f"{what} poses")
    assert not index or list(a["index"]) == list(b["index"])
