"""Shared by tests/test_train_set_lips_host.py and tests/test_gpu_train_set_lips.py: the reference loader's recorded lip
fine-tuning batches (tests/golden/reference_batch_lips.npz, written by tests/golden/make_golden_batch_lips.py from the reference's
own collate with `finetune_lips` and with `patch_size=4`) and the comparison of a DeviceTrainSet batch with one of them.  The bars
are train_set_cases.py's: everything bit-equal except rays_d and poses on the kernel."""
import os
from types import SimpleNamespace

import numpy as np

import train_set_cases as tc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_batch_lips.npz")
_cache = {}


def golden():
    if "g" not in _cache:
        with np.load(GOLDEN) as z:
            _cache["g"] = {k: z[k] for k in z.files}
    return _cache["g"]


def rect_cases():
    """[(tag, torso_mode, att, index), ...] of the recorded `finetune_lips` batches."""
    return [(f"r{k}", bool(t), int(a), int(i)) for k, (t, a, i) in enumerate(golden()["rect_cases"])]


def patch_cases():
    return [(f"p{k}", bool(t), int(a), int(i)) for k, (t, a, i) in enumerate(golden()["patch_cases"])]


def make_set(device, torso_mode, att, kernel=None, num_rays=None, seed=0, lips=True):
    from radnerf.dataset import DeviceTrainSet
    g = golden()
    opt = SimpleNamespace(att=att, torso=torso_mode, exp_eye=True)
    return DeviceTrainSet(g["images"], g["torso"], g["bg"], g["poses"], g["intrinsics"], g["auds"], g["face_rect"],
                          eye_area=g["eye_area"], opt=opt, num_rays=int(g["shape"][3]) if num_rays is None else num_rays, seed=seed,
                          device=device, kernel=kernel, lips_rect=g["lips_rect"] if lips else None)


def corners_of(inds, patch, W):
    """The patches' top-left corners [P,2] = (x0, y0) from recorded pixel indices: every patch^2-th entry is a patch's first pixel."""
    first = np.asarray(inds)[::patch * patch]
    return np.stack((first // W, first % W), axis=-1)


def compare_with_golden(out, ds, tag, torso_mode, exact=False):
    """A batch_rect() / batch_patch() dict and the set's `inds` against the reference's recorded collate output `tag`."""
    g = golden()
    if exact:
        tc.same_bits(out["rays_d"], g[f"{tag}_rays_d"], f"{tag} rays_d")
        tc.same_bits(out["poses"], g[f"{tag}_poses"], f"{tag} poses")
    for k in ("rays_o", "bg_coords", "bg_color", "eye", "auds", "poses_matrix"):
        tc.same_bits(out[k], g[f"{tag}_{k}"], f"{tag} {k}")
    tc.close(out["rays_d"], g[f"{tag}_rays_d"], tc.RAYS_D_TOL, f"{tag} rays_d")
    tc.close(out["poses"], g[f"{tag}_poses"], tc.POSES_TOL, f"{tag} poses")
    assert list(out["index"]) == g[f"{tag}_index"].tolist() and out["H"] == g["shape"][1] and out["W"] == g["shape"][2]
    tc.same_bits(out["face_mask"], g[f"{tag}_face_mask"].astype(np.float32), f"{tag} face_mask")
    tc.same_bits(out["bg_torso_color" if torso_mode else "images"], g[f"{tag}_{'bg_torso_color' if torso_mode else 'images'}"], f"{tag} target")
    tc.same_bits(ds.inds, g[f"{tag}_inds"], f"{tag} inds")
