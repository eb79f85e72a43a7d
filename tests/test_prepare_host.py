"""The host side of radnerf/prepare.py, and the reference the GPU tests compare with (tests/prepref.py).

  * prepref's brute-force distances against sklearn's k-d tree -- what the reference's extract_background asks -- on every plate
    input of tests/test_gpu_prepare.py: distances and the argmax over the frames, not the tied source choice (which the k-d tree
    leaves open).  A frame without foreground is left out for sklearn, whose fit raises on an empty set.
  * labels_from_parsing, the command line's refusals and defaults, the numeric order of the frame ids.
  * task 9: the JSON files load through datafiles.load_split and equal a float32 numpy restatement EXACTLY.  The restatement is
    numpy in every sum, product, transpose, sign and split; the sines and cosines alone are taken from torch, because torch's and
    numpy's float32 sin / cos differ in the last bit on this very kind of input (asserted below to stay within one float32 ulp of
    numpy's): no numpy expression gives torch's bits.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

import dataset_dir as dd
import prepref as R

from radnerf import datafiles, prepare
from radnerf_hip import abi


# ----------------------------------------------------------------------------------------------------------------- prepref
@pytest.mark.parametrize("name", list(R.plate_cases()))
def test_prepref_distances_equal_the_kd_tree(name):
    neighbors = pytest.importorskip("sklearn.neighbors")
    frames, labels = R.plate_cases()[name]
    F, h, w = labels.shape
    all_xys = np.mgrid[0:h, 0:w].reshape(2, -1).transpose()
    tree_d2, kept = [], []
    for f in range(F):
        fg_xys = np.stack(np.nonzero(labels[f] != R.BACKGROUND)).transpose(1, 0)
        if fg_xys.shape[0] == 0:
            assert (R.squared_distances(labels[f]) == R.FAR).all()
            continue
        dists, _ = neighbors.NearestNeighbors(n_neighbors=1, algorithm="kd_tree").fit(fg_xys).kneighbors(all_xys)
        d2 = R.squared_distances(labels[f])
        assert np.array_equal(np.rint(dists[:, 0] ** 2).astype(np.int64).reshape(h, w), d2)
        assert np.abs(dists[:, 0].reshape(h, w) - np.sqrt(d2)).max() < 1e-9
        tree_d2.append(dists[:, 0])
        kept.append(f)
    if len(kept) == F:                                      # the reference's own max / argmax over the frames
        want_d2, want_id, _ = R.plate_accumulate(frames, labels)
        distss = np.stack(tree_d2)
        assert np.array_equal(np.argmax(distss, 0).reshape(h, w), want_id)
        assert np.array_equal(np.max(distss, 0).reshape(h, w) > 5, want_d2 > 25)


def test_prepref_fill_picks_the_smallest_row_then_column():
    best_d2 = np.zeros((9, 11), dtype=np.int64)
    best_d2[2, 2] = best_d2[2, 8] = best_d2[6, 2] = best_d2[6, 8] = 26
    plate = np.zeros((9, 11, 3), dtype=np.uint8)
    _, source, n = R.plate_fill(best_d2, plate)
    assert n == 4 and tuple(source[4, 5]) == (2, 2) and tuple(source[6, 5]) == (6, 2) and tuple(source[4, 8]) == (2, 8)


def test_prepref_blur_is_within_one_level_of_the_float_gaussian():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (33, 29, 3), dtype=np.uint8)
    k = np.exp(-np.arange(-2, 3) ** 2 / (2 * 4.0 ** 2))
    k /= k.sum()
    assert int(R.BLUR.sum()) == 256 and np.array_equal(np.rint(k * 256).astype(np.int64), R.BLUR)
    pad = np.pad(img.astype(np.float64), ((2, 2), (2, 2), (0, 0)), mode="reflect")
    exact = sum(k[i] * k[j] * pad[i:i + 33, j:j + 29] for i in range(5) for j in range(5))
    assert np.abs(R.integer_blur(img).astype(np.float64) - exact).max() <= 1.0


# ------------------------------------------------------------------------------------------------------------------ labels
def test_labels_from_parsing():
    rgb = np.array([[(0, 0, 255), (0, 255, 0), (255, 0, 0), (255, 255, 255)],
                    [(0, 0, 254), (1, 255, 0), (255, 0, 1), (255, 255, 254)],
                    [(0, 0, 0), (255, 255, 0), (0, 255, 255), (128, 128, 128)]], dtype=np.uint8)
    want = np.array([[1, 2, 3, 4], [0, 0, 0, 0], [0, 0, 0, 0]], dtype=np.uint8)
    got = prepare.labels_from_parsing(rgb)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    rgba = np.concatenate([rgb, np.full((3, 4, 1), 9, np.uint8)], axis=-1)
    assert np.array_equal(prepare.labels_from_parsing(rgba), want)
    assert np.array_equal(prepare.labels_from_parsing(R.parsing_from_labels(want)), want)
    assert (prepare.OTHER, prepare.HEAD, prepare.NECK, prepare.TORSO, prepare.BACKGROUND) == (0, 1, 2, 3, 4)
    with pytest.raises(ValueError, match="uint8"):
        prepare.labels_from_parsing(rgb.astype(np.float32))
    with pytest.raises(ValueError, match="uint8"):
        prepare.labels_from_parsing(rgb[..., :2])


def test_darken_table_is_numpys():
    t = prepare.darken_table()
    assert t.dtype == np.float64 and t.shape == (53,) and np.array_equal(t, 0.98 ** np.arange(53)) and t[0] == 1.0


# --------------------------------------------------------------------------------------------------------------------- CLI
def test_cli_defaults():
    a = prepare.build_parser().parse_args(["some/dir"])
    assert (a.path, a.task, a.bg_stride, a.batch, a.jpeg_quality, a.jpeg_subsampling) == ("some/dir", -1, 20, 64, 95, "420")


@pytest.mark.parametrize("task,names", [(1, "ffmpeg"), (2, "python -m radnerf.asr"), (3, "ffmpeg"), (4, "face-parsing"), (7, "landmark"),
                                        (8, "tracker")])
def test_cli_names_what_writes_the_tasks_it_does_not_run(tmp_path, capsys, task, names):
    os.makedirs(tmp_path / "ori_imgs")
    with pytest.raises(SystemExit) as e:
        prepare.main([str(tmp_path), "--task", str(task)])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert names in err and f"task {task}" in err


def test_cli_refusals(tmp_path, capsys):
    os.makedirs(tmp_path / "with" / "ori_imgs")
    for argv, word in (([str(tmp_path / "with"), "--task", "10"], "--task"), ([str(tmp_path / "with"), "--task", "0"], "--task"),
                       ([str(tmp_path / "without")], "ori_imgs"), ([str(tmp_path / "with"), "--batch", "0"], "--batch"),
                       ([str(tmp_path / "with"), "--bg_stride", "0"], "--bg_stride"),
                       ([str(tmp_path / "with"), "--jpeg_quality", "101"], "--jpeg_quality"),
                       ([str(tmp_path / "with"), "--jpeg_subsampling", "422"], "--jpeg_subsampling")):
        with pytest.raises(SystemExit) as e:
            prepare.main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err
    with pytest.raises(FileNotFoundError, match="track_params.pt"):
        prepare.main([str(tmp_path / "with"), "--task", "9"])
    with pytest.raises(FileNotFoundError, match="no \\*.jpg"):
        prepare.frame_ids(str(tmp_path / "with"))


def test_frame_ids_are_sorted_by_number(tmp_path):
    os.makedirs(tmp_path / "ori_imgs")
    for n in ("10", "9", "100", "0", "2", "x1"):
        (tmp_path / "ori_imgs" / (n + ".jpg")).write_bytes(b"")
    (tmp_path / "ori_imgs" / "3.lms").write_bytes(b"")
    assert prepare.frame_ids(str(tmp_path)) == ["0", "2", "9", "10", "100", "x1"]


def test_png_writer_without_pil(monkeypatch):
    monkeypatch.setitem(sys.modules, "PIL", None)
    with pytest.raises(ImportError, match="PIL"):
        prepare.default_png_writer()


def test_the_four_symbols_are_in_the_abi_table():
    for name in ("rn_prep_workspace", "rn_prep_plate_accumulate", "rn_prep_plate_fill", "rn_prep_layers"):
        assert name in abi.FUNCTIONS
    assert abi.FUNCTIONS["rn_prep_workspace"][0] is abi._sz
    assert len(abi.FUNCTIONS["rn_prep_plate_accumulate"][1]) == 11 and len(abi.FUNCTIONS["rn_prep_layers"][1]) == 11
    assert len(abi.FUNCTIONS["rn_prep_plate_fill"][1]) == 8


# ------------------------------------------------------------------------------------------------------------------ task 9
N9, H9, W9 = 23, 20, 16


def _track(rng):
    return dict(focal=torch.tensor([1234.5, 7.0]), euler=torch.from_numpy((rng.random((N9, 3)) * 1.2 - 0.6).astype(np.float32)),
                trans=torch.from_numpy((rng.random((N9, 3)) * np.array([2, 2, 5]) + np.array([-1, -1, -40])).astype(np.float32)))


def _restated_poses(track):
    """float32 numpy: rot = Rx (Ry Rz) with every product and sum rounded, k ascending; its transpose; -(rot^T (trans / 10))."""
    e = track["euler"]
    f32 = np.float32
    sin, cos = torch.sin(e).numpy(), torch.cos(e).numpy()                   # torch's bits; see the module docstring
    assert np.abs(sin - np.sin(e.numpy())).max() <= 2.0 ** -23 and np.abs(cos - np.cos(e.numpy())).max() <= 2.0 ** -23
    trans = track["trans"].numpy() / f32(10.0)
    poses = []
    for i in range(e.shape[0]):
        (sx, sy, sz), (cx, cy, cz) = sin[i], cos[i]
        rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]], dtype=f32)
        ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], dtype=f32)
        rz = np.array([[cz, sz, 0], [-sz, cz, 0], [0, 0, 1]], dtype=f32)

        def mul(a, b):
            out = np.zeros((3, 3), dtype=f32)
            for r in range(3):
                for c in range(3):
                    out[r, c] = f32(f32(f32(a[r, 0] * b[0, c]) + f32(a[r, 1] * b[1, c])) + f32(a[r, 2] * b[2, c]))
            return out
        inv = mul(rx, mul(ry, rz)).T
        pose = np.eye(4, dtype=f32)
        pose[:3, :3] = inv
        for r in range(3):
            pose[r, 3] = -f32(f32(f32(inv[r, 0] * trans[i, 0]) + f32(inv[r, 1] * trans[i, 1])) + f32(inv[r, 2] * trans[i, 2]))
        poses.append(pose)
    return np.stack(poses)


def test_euler_matrices_are_the_references():
    """One angle at a time: the reference builds each matrix column by column (torch.cat along dim 1, then dim 2)."""
    a = np.float32(0.3)
    s, c = float(torch.sin(torch.tensor(a))), float(torch.cos(torch.tensor(a)))
    for axis, want in ((0, [[1, 0, 0], [0, c, -s], [0, s, c]]), (1, [[c, 0, s], [0, 1, 0], [-s, 0, c]]), (2, [[c, s, 0], [-s, c, 0], [0, 0, 1]])):
        e = torch.zeros(1, 3)
        e[0, axis] = float(a)
        assert np.array_equal(prepare.euler2rot(e)[0].numpy(), np.array(want, dtype=np.float32))


def test_task_9_files_load_and_equal_the_restatement(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(99)
    root = str(tmp_path)
    for sub in ("ori_imgs", "gt_imgs", "torso_imgs"):
        os.makedirs(os.path.join(root, sub))
    track = _track(rng)
    torch.save(track, os.path.join(root, "track_params.pt"))
    for i in range(N9):
        for sub, ext, ch in (("ori_imgs", ".jpg", 3), ("gt_imgs", ".jpg", 3), ("torso_imgs", ".png", 4)):
            with open(os.path.join(root, sub, f"{i}{ext}"), "wb") as fh:
                Image.fromarray(rng.integers(0, 256, (H9, W9, ch), dtype=np.uint8)).save(fh, format="PNG")
        np.savetxt(os.path.join(root, "ori_imgs", f"{i}.lms"), np.round(rng.random((68, 2)) * np.array([W9 - 1, H9 - 1]), 1), fmt="%.1f")
    np.save(os.path.join(root, "aud_eo.npy"), rng.standard_normal((N9, 16, 44)).astype(np.float32))
    log = []
    assert prepare.main([root, "--task", "9"], log=log.append) == [9]

    want = _restated_poses(track)
    split = int(N9 * 10 / 11)
    assert split == 20
    for name, ids in (("train", range(0, split)), ("val", range(split, N9))):
        with open(os.path.join(root, f"transforms_{name}.json")) as fh:
            text = fh.read()
        t = json.loads(text)
        assert text.startswith('{\n  "focal_len": 1234.5,\n  "cx": 8.0,\n  "cy": 10.0,\n  "frames": [\n    {\n      "img_id": ')     # indent=2, (',', ': ')
        assert (t["focal_len"], t["cx"], t["cy"]) == (1234.5, W9 / 2, H9 / 2) and list(t) == ["focal_len", "cx", "cy", "frames"]
        assert [f["img_id"] for f in t["frames"]] == list(ids) and [f["aud_id"] for f in t["frames"]] == list(ids)
        got = np.array([f["transform_matrix"] for f in t["frames"]], dtype=np.float64)
        assert np.array_equal(got, want[list(ids)].astype(np.float64))                  # float32 values, printed in full
        loaded = datafiles.load_split(root, dd.dataset_opt(root, bg_img="white"), name)     # no bc.jpg: that is task 5's
        assert (loaded.H, loaded.W, loaded.F) == (H9, W9, len(ids))
        assert np.array_equal(loaded.intrinsics, np.array([1234.5, 1234.5, W9 / 2, H9 / 2]))
        from radnerf.rays import nerf_matrix_to_ngp
        assert np.array_equal(loaded.poses, nerf_matrix_to_ngp(want[list(ids)], scale=4, offset=[0, 0, 0]))
        assert loaded.frame_ids == list(ids)
    # a rotation: orthonormal to float32 accuracy
    r = want[:, :3, :3].astype(np.float64)
    assert np.abs(r @ r.transpose(0, 2, 1) - np.eye(3)).max() < 1e-6
