"""rn_train_set_batch / rn_train_set_frame (csrc/rn_train_batch.hip) through DeviceTrainSet on the GPU: against the reference
loader's recorded batches (tests/golden/reference_batch.npz), against the class's torch path, and feeding both trainers.
Shapes are the fixture's: W = 53 is a multiple of nothing, N = 257 is one full 256-thread workgroup plus one thread, 9 frames.
Bars: everything bit-equal except rays_d (<= 2e-7) and poses (<= 1e-6), tests/test_gpu_render.py's bars for the same formulas."""
import numpy as np
import pytest
import torch

import train_set_cases as tc

pytestmark = pytest.mark.gpu


def _copy(d):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in d.items()}


@pytest.mark.parametrize("tag,torso_mode,att,index", tc.cases())
def test_kernel_equals_the_reference_collate_and_the_torch_path(hiplib, tag, torso_mode, att, index):
    g = tc.golden()
    ds = tc.make_set("cuda", torso_mode, att)
    assert ds.kernel == "hip"
    out = ds.batch([index], inds=g[f"{tag}_inds"])
    tc.compare_with_golden(out, tag, torso_mode)
    oracle = ds.clone(kernel="torch").batch([index], inds=g[f"{tag}_inds"])
    tc.compare_with_golden(oracle, tag, torso_mode)             # the oracle on the device is the oracle the CPU fixture pins
    tc.compare_batches(out, oracle, tag)
    ds.check()


@pytest.mark.parametrize("torso_mode", [False, True])
@pytest.mark.parametrize("att", [0, 1, 2])
def test_explicit_pixels_at_the_image_corners_and_the_rect_edges(hiplib, torso_mode, att):
    """Pixel 0, pixel H*W - 1, a duplicated pixel and the pixels on both sides of each face-rect edge; frames whose rect touches
    the image border included."""
    g = tc.golden()
    F, H, W, N, _ = (int(v) for v in g["shape"])
    ds = tc.make_set("cuda", torso_mode, att)
    oracle = ds.clone(kernel="torch")
    rng = np.random.default_rng(5)
    for frame in (0, 4, F - 1):
        xmin, xmax, ymin, ymax = (int(v) for v in g["face_rect"][frame])
        rmid, cmid = (xmin + xmax) // 2, (ymin + ymax) // 2
        px = [(0, 0), (H - 1, W - 1), (rmid, cmid), (rmid, cmid)]
        px += [(r, cmid) for r in (xmin - 1, xmin, xmax - 1, xmax)] + [(rmid, c) for c in (ymin - 1, ymin, ymax - 1, ymax)]
        px += [(r, c) for r in (xmin - 1, xmin, xmax - 1, xmax) for c in (ymin - 1, ymin, ymax - 1, ymax)]
        px = [(r, c) for r, c in px if 0 <= r < H and 0 <= c < W]
        inds = np.array([r * W + c for r, c in px] + rng.integers(0, H * W, N - len(px)).tolist(), dtype=np.int64)
        assert inds.size == N and inds[0] == 0 and inds[1] == H * W - 1 and inds[2] == inds[3]
        out = ds.batch([frame], inds=inds)
        tc.compare_batches(out, oracle.batch([frame], inds=inds), f"frame {frame}")
        r, c = inds // W, inds % W
        face = ((r >= xmin) & (r < xmax) & (c >= ymin) & (c < ymax)).astype(np.float32)
        assert 0 < face.sum() < N
        tc.same_bits(out["face_mask"], face[None], f"frame {frame} face_mask")
        tc.same_bits(ds.inds, inds, "inds_out")
    ds.check()


def test_frame_equals_the_reference_collate_and_the_torch_path(hiplib):
    g = tc.golden()
    F = int(g["shape"][0])
    torso_mode, att, index = (int(v) for v in g["frame_case"])
    ds = tc.make_set("cuda", bool(torso_mode), att)
    oracle = ds.clone(kernel="torch")
    tc.compare_with_golden(ds.frame(index), "frame", bool(torso_mode), training=False)
    for mode in (False, True):                                  # both modes, a mirrored index with its own audio index
        a, b = tc.make_set("cuda", mode, 1), tc.make_set("cuda", mode, 1, kernel="torch")
        out = a.frame(F + 2, aud_index=3)
        assert out["index"] == [F - 3] and out["images"].shape == (1, int(g["shape"][1]), int(g["shape"][2]), 3)
        tc.compare_batches(out, b.frame(F + 2, aud_index=3), f"frame() torso={mode}", training=False)
    tc.compare_batches(ds.frame(index), oracle.frame(index), "frame()", training=False)


def test_decode_and_blend_are_the_loaders_float32_arithmetic(hiplib):
    """uint8 data that holds all 256 values in every channel and in alpha, every pixel of the frame picked: a reciprocal multiply
    in place of the divide, or a blend contracted into an FMA, differs from numpy's float32 arithmetic in many of these."""
    g = tc.golden()
    F, H, W, _, _ = (int(v) for v in g["shape"])
    rng = np.random.default_rng(77)
    images, torso, bg = (rng.integers(0, 256, s, dtype=np.uint8) for s in ((F, H, W, 3), (F, H, W, 4), (H, W, 3)))
    for ch in range(4):                                         # all 256 values in every channel, against every alpha and background
        torso.reshape(F, -1, 4)[:, :256, ch] = rng.permutation(256)
        torso.reshape(F, -1, 4)[:, 256:512, ch] = rng.permutation(256)
    for ch in range(3):
        images.reshape(F, -1, 3)[:, :256, ch] = rng.permutation(256)
        bg.reshape(-1, 3)[:256, ch] = rng.permutation(256)
        bg.reshape(-1, 3)[256:512, ch] = rng.permutation(256)
    torso.reshape(F, -1, 4)[:, 512:768, 3] = np.repeat([0, 255], 128)
    inds = np.arange(H * W, dtype=np.int64)
    f32 = lambda a: a.astype(np.float32) / np.float32(255)
    for torso_mode in (False, True):
        ds = tc.make_set("cuda", torso_mode, 0, images=images, torso=torso, bg=bg)
        out = ds.batch([2], inds=inds)
        t, b = f32(torso[2].reshape(-1, 4)), f32(bg.reshape(-1, 3))
        blend = t[:, :3] * t[:, 3:] + b * (np.float32(1) - t[:, 3:])
        assert blend.dtype == np.float32
        if torso_mode:
            tc.same_bits(out["bg_color"][0], b, "bg_color (torso mode)")
            tc.same_bits(out["bg_torso_color"][0], blend, "bg_torso_color")
        else:
            tc.same_bits(out["bg_color"][0], blend, "bg_color (head mode)")
            tc.same_bits(out["images"][0], f32(images[2].reshape(-1, 3)), "images")
        tc.compare_batches(out, ds.clone(kernel="torch").batch([2], inds=inds), f"all values, torso={torso_mode}")


def test_self_drawn_pixels(hiplib):
    """inds == NULL: N = 4096 draws over the 37 x 53 pixels.  In range, reproduced by (seed, draw), different for the next draw and
    the next seed, and evenly spread: 16 equal pixel ranges each hold 256 +- 25 % (a fixed outcome of the fixed seed; the
    expected count has a standard deviation of 15.5, so the bar is four of them)."""
    g = tc.golden()
    H, W = int(g["shape"][1]), int(g["shape"][2])
    N, seed = 4096, 20
    ds = tc.make_set("cuda", False, 2, num_rays=N, seed=seed)
    first = _copy(ds.batch([3]))
    picked = ds.inds.clone()
    assert picked.shape == (N,) and int(picked.min()) >= 0 and int(picked.max()) < H * W
    oracle = ds.clone(kernel="torch")
    tc.compare_batches(first, oracle.batch([3], inds=picked), "self-drawn")       # inds_out reproduces the packed sections
    counts = np.histogram(picked.cpu().numpy(), bins=16, range=(0, H * W))[0]
    print("counts over 16 pixel ranges:", counts.tolist())
    assert counts.sum() == N and np.all(np.abs(counts - N / 16) <= 0.25 * N / 16), counts
    second = _copy(ds.batch([3]))                               # draw + 1
    assert not torch.equal(ds.inds, picked) and not torch.equal(second["_packed"], first["_packed"])
    again = tc.make_set("cuda", False, 2, num_rays=N, seed=seed)
    assert torch.equal(again.batch([3])["_packed"], first["_packed"]) and torch.equal(again.inds, picked)
    assert torch.equal(again.batch([3])["_packed"], second["_packed"])
    other = tc.make_set("cuda", False, 2, num_rays=N, seed=seed + 1)
    assert not torch.equal(other.batch([3])["_packed"], first["_packed"]) and not torch.equal(other.inds, picked)
    from radnerf.dataset import drawn_pixels                    # the torch path restates the same draw
    assert torch.equal(drawn_pixels(seed, 0, N, H * W, "cuda"), picked)
    assert torch.equal(oracle.batch([3])["_packed"][6 * N:], first["_packed"][6 * N:])    # the oracle's own draw 0: same pixels
    ds.check()


def test_out_of_range_pixels_are_clamped_and_reported(hiplib):
    g = tc.golden()
    H, W, N = int(g["shape"][1]), int(g["shape"][2]), int(g["shape"][3])
    ds = tc.make_set("cuda", True, 2)
    rng = np.random.default_rng(9)
    inds = rng.integers(0, H * W, N)
    clamped = inds.copy()
    inds[[0, 5, 256]] = (-1, H * W, H * W + 12345678901)
    clamped[[0, 5, 256]] = (0, H * W - 1, H * W - 1)
    clean = _copy(ds.batch([4], inds=clamped))
    ds.check()                                                  # a clean call does not raise
    out = ds.batch([4], inds=inds)
    assert torch.equal(out["_packed"], clean["_packed"]) and torch.equal(ds.inds.cpu(), torch.from_numpy(clamped))
    with pytest.raises(IndexError, match="3 pixel indices"):
        ds.check()
    ds.check()


def _scene(**kw):
    from radnerf.scene import SyntheticScene, default_opt
    return SyntheticScene(H=64, W=64, n_frames=8, device="cuda", opt=default_opt(engine="ops", smooth_lips=False, **kw))


def _moved(model, before):
    return sum(int(not torch.equal(p.detach(), b)) for p, b in zip(model.parameters(), before))


@pytest.mark.parametrize("torso", [False, True])
def test_trainer_takes_the_batches(hiplib, torso):
    from radnerf.dataset import DeviceTrainSet
    from radnerf.train import Trainer
    scene = _scene(torso=torso)
    ds = DeviceTrainSet.from_scene(scene, 8, num_rays=1024)
    assert ds.kernel == "hip" and ds.images.dtype == torch.uint8 and ds.images.shape == (8, 64, 64, 3)
    m = ds.install(scene.model)
    assert m.aud_features is ds.auds and m.poses is ds.poses and m.eye_area.shape == (8, 1)
    before = [p.detach().clone() for p in m.parameters()]
    trainer = Trainer(m, scene.opt, update_extra_interval=4)
    order = ds.order(0)
    losses = [float(trainer.step(ds.batch([i]))) for i in order[:3]]
    assert all(np.isfinite(losses)), losses
    assert _moved(m, before) > 0
    ds.check()


@pytest.mark.parametrize("torso", [False, True])
def test_graphed_trainer_follows_the_data(hiplib, torso):
    """Twelve steps cycling through the frames.  Head mode: the first window runs eagerly, the refresh before step 5 gives the
    marcher its budget and the rest replays; after every step the trainer's static inputs are the batch of THAT frame.  Torso mode
    on the default route cannot be captured (it asks the host for the covered pixels): GraphedTrainer serves it on its eager path,
    which it keeps while no refresh has given the marcher a budget (update_extra_interval = 0)."""
    from radnerf.dataset import DeviceTrainSet
    from radnerf.train import GraphedTrainer
    scene = _scene(torso=torso)
    ds = DeviceTrainSet.from_scene(scene, 8, num_rays=1024, seed=2)
    oracle = ds.clone(kernel="torch")
    m = ds.install(scene.model)
    before = [p.detach().clone() for p in m.parameters()]
    trainer = GraphedTrainer(m, scene.opt, update_extra_interval=0 if torso else 4)
    order, losses = ds.order(0), []
    for step in range(12):
        i = order[step % len(order)]
        data = ds.batch([i])
        losses.append(float(trainer.step(data)))
        if trainer.replays:
            want = oracle.batch([i], inds=ds.inds)
            st = trainer._plain.newest()[2].static
            tc.compare_batches(st, want, f"static inputs after step {step} (frame {i})", index=False)
            assert st["index"].tolist() == [i] and st["_packed"] is not data["_packed"]
            assert torch.equal(st["_packed"], data["_packed"])
    assert all(np.isfinite(losses)), losses
    assert _moved(m, before) > 0
    assert (trainer.replays == 0) if torso else (trainer.replays >= 1 and trainer.captures >= 1)
    ds.check()
