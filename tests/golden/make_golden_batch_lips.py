"""Generates tests/golden/reference_batch_lips.npz -- run ONLY in the build container (needs the reference checkout).

    python tests/golden/make_golden_batch_lips.py

The lip fine-tuning side of make_golden_batch.py (which see for how the reference's loader is run): the reference's OWN
NeRFDataset.collate (nerf/provider.py:625-714), imported unmodified at run time, on a NON-SQUARE stand-in set (H = 20, W = 28,
F = 8) in its two other sampling modes --

  * `finetune_lips=True`: get_rays with the frame's lips rect (nerf/utils.py:297-303), every pixel of the rect in ascending order;
  * `patch_size=4, num_rays=64`: four 4 x 4 patches whose corners come from two torch.randint calls (:281-292).  Seeding the
    global generator before the call and drawing the same two calls after the same seed reproduces the corners, which is how
    `inds` gets recorded (checked below against the reference's own gathers).

The lips rects are computed from a recorded landmark array by the reference's own lines (provider.py:487-502): those lines sit
in the middle of the loader's constructor, so they are read from the reference's file at run time and executed on a stand-in
`self` -- nothing of them is kept here.  Only data is committed: the uint8 inputs, the landmarks, the draws and the reference's
outputs -- no reference source text.
"""
import os
import sys
import textwrap
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402  (paths, stub modules, the reference on sys.path)

F, H, W, C = 8, 20, 28, 5              # 5 audio channels: the window is a copy, its width tests nothing here
PATCH, NUM_RAYS = 4, 64
RECT_CASES = ((False, 2, 0), (True, 1, 3), (False, 0, 5), (True, 2, F - 1))      # (torso_mode, att, index)
PATCH_CASES = ((False, 1, 3), (True, 0, 5), (False, 2, F - 1))                   # the same frames in the other mode
OUT = os.path.join(HERE, "reference_batch_lips.npz")


def inputs():
    rng = np.random.default_rng(20240917)
    from radnerf.rays import orbit_pose
    images = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    torso = rng.integers(0, 256, (F, H, W, 4), dtype=np.uint8)
    kind = rng.integers(0, 4, (F, H, W))
    torso[..., 3][kind == 0] = 0
    torso[..., 3][kind == 1] = 255
    used = {i for _, _, i in RECT_CASES + PATCH_CASES}
    for f in range(F):                        # frames no case reads are shifted copies of their neighbour: they compress away
        if f not in used:
            images[f], torso[f] = np.roll(images[f - 1], 1, axis=1), np.roll(torso[f - 1], 1, axis=1)
    bg = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    poses = np.stack([orbit_pose(3.3 + 0.06 * f, 8.0 * np.sin(1.1 * f), 4.0 * np.cos(1.3 * f)) for f in range(F)]).astype(np.float32)
    intrinsics = np.array([33.5, 31.25, 14.0, 10.0])                      # (fx, fy, cx, cy): float64, as provider.py:609 builds it
    auds = (rng.integers(-2000, 2001, (F, C, 16)) / 64).astype(np.float32)
    eye = rng.random((F, 1)).astype(np.float32)
    rect = np.stack([np.array([rng.integers(1, 6), rng.integers(12, H - 1), rng.integers(2, 9), rng.integers(16, W - 2)])
                     for _ in range(F)]).astype(np.int32)
    # 68 landmarks per frame as the loader reads them (np.loadtxt: float, (column, row)); the lips (48..59) of every frame in a
    # box of its own size and place: wider than tall, taller than wide, against each border (the clip of provider.py:497-500)
    boxes = [(7.2, 12.9, 9.5, 19.4), (2.0, 5.7, 1.1, 9.8), (15.3, 19.6, 18.2, 26.9), (5.5, 14.5, 12.0, 15.9),
             (9.0, 12.0, 3.4, 8.2), (0.4, 13.7, 22.3, 27.6), (10.1, 18.8, 0.2, 5.1), (8.8, 11.1, 11.7, 14.2)]   # (row0, row1, col0, col1)
    lms = np.round(rng.random((F, 68, 2)) * np.array([W - 1, H - 1]), 1)
    for f, (r0, r1, c0, c1) in enumerate(boxes):
        lms[f, 48:60, 0] = c0 + (c1 - c0) * rng.random(12)
        lms[f, 48:60, 1] = r0 + (r1 - r0) * rng.random(12)
        lms[f, 48], lms[f, 54] = (c0, 0.5 * (r0 + r1)), (c1, 0.5 * (r0 + r1))        # the box is reached on every side
        lms[f, 51], lms[f, 57] = (0.5 * (c0 + c1), r0), (0.5 * (c0 + c1), r1)
    return dict(images=images, torso=torso, bg=bg, poses=poses, intrinsics=intrinsics, auds=auds, eye_area=eye, face_rect=rect,
                lms=lms)


def reference_lips_rects(lms):
    """provider.py:487-502 run on the recorded landmarks: the block `if self.opt.finetune_lips: ... self.lips_rect.append(...)` is
    cut out of the reference's file and executed once per frame with `lms` and a stand-in `self`."""
    path = os.path.join(make_golden.REF, "nerf", "provider.py")
    lines = open(path).read().split("\n")
    first = next(i for i, ln in enumerate(lines) if ln.strip() == "if self.opt.finetune_lips:")
    last = next(i for i in range(first, len(lines)) if lines[i].strip().startswith("self.lips_rect.append("))
    assert 5 < last - first < 25
    code = compile(textwrap.dedent("\n".join(lines[first:last + 1])), path, "exec")
    me = types.SimpleNamespace(opt=types.SimpleNamespace(finetune_lips=True), H=H, W=W, lips_rect=[])
    for f in range(F):
        exec(code, {"self": me, "lms": lms[f]})
    return np.array(me.lips_rect, dtype=np.int32)


def stand_in(ref_provider, ref_utils, d, lips_rect, torso_mode, att, finetune_lips, patch_size):
    f32 = lambda a: torch.from_numpy(a.astype(np.float32) / 255)          # provider.py:444, 457, 518 (`--preload 1`)
    opt = types.SimpleNamespace(att=att, torso=torso_mode, exp_eye=True, finetune_lips=finetune_lips, patch_size=patch_size)
    s = types.SimpleNamespace(
        opt=opt, device="cpu", training=True, preload=1, num_rays=NUM_RAYS, H=H, W=W, auds=torch.from_numpy(d["auds"]),
        poses=torch.from_numpy(d["poses"]), intrinsics=d["intrinsics"], face_rect=d["face_rect"].tolist(), lips_rect=lips_rect.tolist(),
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
    lips = reference_lips_rects(d["lms"])
    assert lips.shape == (F, 4) and len({tuple(r) for r in lips.tolist()}) == F
    assert (lips[:, 0] == 0).any() and (lips[:, 1] == H).any() and (lips[:, 2] == 0).any() and (lips[:, 3] == W).any()   # every clip is taken
    out = {k: v for k, v in d.items()}
    out["lips_rect"] = lips
    out["shape"] = np.array([F, H, W, NUM_RAYS, C, PATCH])

    def put(tag, res, s, index, inds):
        full = s.bg_img.view(-1, 3) if s.opt.torso else (
            s.torso_img[index][..., :3] * s.torso_img[index][..., 3:] + s.bg_img * (1 - s.torso_img[index][..., 3:])).view(-1, 3)
        assert torch.equal(res["bg_color"][0], full[inds]) and torch.equal(res["images"][0], s.images[index].view(-1, 3)[inds])
        assert torch.equal(res["bg_coords"][0], s.bg_coords[0][inds])
        for k in ("rays_o", "rays_d", "bg_coords", "bg_color", "images", "eye", "auds", "poses", "poses_matrix", "face_mask"):
            out[f"{tag}_{k}"] = make_golden.t2n(res[k]).copy()
        out[f"{tag}_index"] = np.array(res["index"])
        out[f"{tag}_inds"] = inds.numpy()
        if "bg_torso_color" in res:
            out[f"{tag}_bg_torso_color"] = make_golden.t2n(res["bg_torso_color"]).copy()

    rect_cases, patch_cases = [], []
    for torso_mode, att, index in RECT_CASES:
        s = stand_in(ref_provider, ref_utils, d, lips, torso_mode, att, True, 1)
        res = ref_provider.NeRFDataset.collate(s, [index])
        xmin, xmax, ymin, ymax = res["rect"]
        assert [xmin, xmax, ymin, ymax] == lips[index].tolist()
        rows, cols = torch.meshgrid(torch.arange(xmin, xmax), torch.arange(ymin, ymax), indexing="ij")
        inds = (rows * W + cols).reshape(-1)                      # ascending, x along the rows: what torch.where(mask) lists
        assert res["rays_o"].shape == (1, inds.numel(), 3)
        tag = f"r{len(rect_cases)}"
        rect_cases.append((int(torso_mode), att, index))
        out[f"{tag}_rect"] = np.array(res["rect"], dtype=np.int32)
        put(tag, res, s, index, inds)
    for p, (torso_mode, att, index) in enumerate(PATCH_CASES):
        s = stand_in(ref_provider, ref_utils, d, lips, torso_mode, att, False, PATCH)
        seed = 2000 + p
        torch.manual_seed(seed)
        res = ref_provider.NeRFDataset.collate(s, [index])
        torch.manual_seed(seed)
        n_patch = NUM_RAYS // PATCH ** 2
        x0 = torch.randint(0, H - PATCH, size=[n_patch])
        y0 = torch.randint(0, W - PATCH, size=[n_patch])
        o = torch.arange(PATCH ** 2)
        inds = ((x0[:, None] + o // PATCH) * W + y0[:, None] + o % PATCH).reshape(-1)
        assert res["rays_o"].shape == (1, NUM_RAYS, 3)
        tag = f"p{len(patch_cases)}"
        patch_cases.append((int(torso_mode), att, index))
        put(tag, res, s, index, inds)
    out["rect_cases"] = np.array(rect_cases)                  # (torso_mode, att, index) of r0, r1, ...
    out["patch_cases"] = np.array(patch_cases)                # ... of p0, p1, ...

    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(rect_cases)} rect + {len(patch_cases)} patch cases; lips rects {lips.tolist()}")
    assert os.path.getsize(OUT) < 72 * 1024


if __name__ == "__main__":
    main()
