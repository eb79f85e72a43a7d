"""Generates tests/golden/reference_batch.npz -- run ONLY in the build container (needs the reference checkout).

    python tests/golden/make_golden_batch.py

What runs is the reference's OWN loader code, imported unmodified at run time through make_golden.install_reference() (the
same stub modules): NeRFDataset.collate (nerf/provider.py:625-714) with mirror_index, and under it get_rays, get_audio_features
and convert_poses of nerf/utils.py.  collate is called on a stand-in object that carries exactly the attributes it reads (a
SimpleNamespace with mirror_index bound as a method), in the `--preload 1` state: float32 images = uint8 / 255 as
provider.py:444, 457, 518 decodes them, everything on the CPU.

collate draws its pixels with torch.randint from the global generator (nerf/utils.py:306); seeding that generator just before
the call and drawing once more after the same seed reproduces them, which is how `inds` gets recorded (checked below: the
reference's bg_color equals an index with these inds, bit for bit).

Only data is committed: the uint8 inputs, the draws and the reference's outputs -- no reference source text.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402  (paths, stub modules, the reference on sys.path)

F, H, W, N, C = 9, 37, 53, 257, 29
INDICES = (0, 3, F - 1)           # the audio window pads on the left at 0 and 3, on the right at F - 1
FRAME_INDEX = 5
OUT = os.path.join(HERE, "reference_batch.npz")


def inputs():
    rng = np.random.default_rng(20240611)
    from radnerf.rays import orbit_pose
    images = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    torso = rng.integers(0, 256, (F, H, W, 4), dtype=np.uint8)
    kind = rng.integers(0, 4, (F, H, W))
    torso[..., 3][kind == 0] = 0              # fully transparent and fully opaque pixels next to the random alphas
    torso[..., 3][kind == 1] = 255
    for f in range(F):                        # frames no case reads are shifted copies of their neighbour: they compress away
        if f not in INDICES + (FRAME_INDEX,):
            images[f], torso[f] = np.roll(images[f - 1], 1, axis=1), np.roll(torso[f - 1], 1, axis=1)
    bg = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    poses = np.stack([orbit_pose(3.35 + 0.05 * f, 9.0 * np.sin(0.9 * f), 5.0 * np.cos(1.7 * f)) for f in range(F)]).astype(np.float32)
    intrinsics = np.array([60.5, 58.25, 26.5, 18.5])                     # (fx, fy, cx, cy): float64, as provider.py:609 builds it
    auds = (rng.integers(-2000, 2001, (F, C, 16)) / 64).astype(np.float32)     # the window is a copy: short mantissas keep the file small
    eye = rng.random((F, 1)).astype(np.float32)
    rect = np.stack([np.array([rng.integers(2, 12), rng.integers(20, H - 2), rng.integers(3, 20), rng.integers(30, W - 3)])
                     for _ in range(F)]).astype(np.int32)
    rect[0] = (0, 21, 11, W)                  # touches the top and the right border of the image
    rect[F - 1] = (5, H, 0, 40)               # ... the bottom and the left border
    return dict(images=images, torso=torso, bg=bg, poses=poses, intrinsics=intrinsics, auds=auds, eye_area=eye, face_rect=rect)


def stand_in(ref_provider, ref_utils, d, torso_mode, att, training):
    f32 = lambda a: torch.from_numpy(a.astype(np.float32) / 255)          # provider.py:444, 457, 518 (`--preload 1`)
    opt = types.SimpleNamespace(att=att, torso=torso_mode, exp_eye=True, finetune_lips=False, patch_size=1)
    s = types.SimpleNamespace(
        opt=opt, device="cpu", training=training, preload=1, num_rays=N if training else -1, H=H, W=W, auds=torch.from_numpy(d["auds"]),
        poses=torch.from_numpy(d["poses"]), intrinsics=d["intrinsics"], face_rect=d["face_rect"].tolist(),
        eye_area=torch.from_numpy(d["eye_area"]), torso_img=f32(d["torso"]), images=f32(d["images"]), bg_img=f32(d["bg"]),
        bg_coords=ref_utils.get_bg_coords(H, W, "cpu"))
    s.mirror_index = types.MethodType(ref_provider.NeRFDataset.mirror_index, s)
    return s


def main():
    env = make_golden.install_reference()
    ref_utils = env[-1]
    import nerf.provider as ref_provider
    assert ref_provider.__file__.startswith(make_golden.REF)
    d = inputs()
    out = {k: v for k, v in d.items()}
    out["shape"] = np.array([F, H, W, N, C])

    def put(tag, res, training):
        for k in ("rays_o", "rays_d", "bg_coords", "bg_color", "images", "eye", "auds", "poses", "poses_matrix"):
            out[f"{tag}_{k}"] = make_golden.t2n(res[k]).copy()
        out[f"{tag}_index"] = np.array(res["index"])
        if training:
            out[f"{tag}_face_mask"] = make_golden.t2n(res["face_mask"]).copy()
        if "bg_torso_color" in res:
            out[f"{tag}_bg_torso_color"] = make_golden.t2n(res["bg_torso_color"]).copy()

    cases = []
    for a in (0, 1, 2):
        for p, index in enumerate(INDICES):
            torso_mode = bool((a + p) % 2)            # every index in both modes, every att at every index
            s = stand_in(ref_provider, ref_utils, d, torso_mode, a, True)
            seed = 1000 + 10 * a + p
            torch.manual_seed(seed)
            res = ref_provider.NeRFDataset.collate(s, [index])
            torch.manual_seed(seed)
            inds = torch.randint(0, H * W, size=[N])
            full = s.bg_img.view(-1, 3) if torso_mode else (
                s.torso_img[index][..., :3] * s.torso_img[index][..., 3:] + s.bg_img * (1 - s.torso_img[index][..., 3:])).view(-1, 3)
            assert torch.equal(res["bg_color"][0], full[inds]) and torch.equal(res["images"][0], s.images[index].view(-1, 3)[inds])
            tag = f"c{len(cases)}"
            cases.append((int(torso_mode), a, index))
            out[f"{tag}_inds"] = inds.numpy()
            put(tag, res, True)
    out["cases"] = np.array(cases)                    # (torso_mode, att, index) of c0, c1, ...

    s = stand_in(ref_provider, ref_utils, d, False, 2, False)
    put("frame", ref_provider.NeRFDataset.collate(s, [FRAME_INDEX]), False)
    out["frame_case"] = np.array([0, 2, FRAME_INDEX])
    probe = np.array([0, 3, F - 1, F, F + 2, 2 * F - 1, 2 * F, 2 * F + 4, 3 * F])
    out["mirror_in"] = probe
    out["mirror_out"] = np.array([s.mirror_index(int(i)) for i in probe])

    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(cases)} training cases + 1 frame")
    assert os.path.getsize(OUT) < 300 * 1024


if __name__ == "__main__":
    main()
