"""radnerf/prepare.py on the device against tests/prepref.py, the numpy restatement of the reference's data flow: the background
plate (accumulate and fill), the gt and torso layers, and `python -m radnerf.prepare DIR --task -1` end to end into
DeviceTrainSet.from_directory.  Every array comparison is exact: the kernels are integer and table-driven.

Shapes: the plate at 40 x 56, at W = 1, 63, 64, 65 around the wave width with H = 7, at H = 1, and at W = 300 so that one row takes
two workgroups; the layers at 128 x 72 (the neck in-paint is 53 rows tall).  The dilated neck of a column with a head above it has
at least 4 rows (7 clipped by the bottom edge), so min(n - 1, 4) is pinned with n = 4, 5, 6 and 7 from a single raw neck pixel; a
count of 1 does not exist.

The one comparison that is no equality is the gt JPEG: its mean absolute error against the exact gt must stay within 1.1 x the
error of PIL's own quality-95 4:2:0 file of the same array (same IJG tables; only the rounding differs).
"""
import io
import json
import os

import numpy as np
import pytest
import torch

import dataset_dir as dd
import prepref as R

pytestmark = pytest.mark.gpu

FAR = 1 << 30


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _accumulated(frames, labels, batch):
    from radnerf.prepare import PlateBuilder
    b = PlateBuilder(frames.shape[1], frames.shape[2])
    for at in range(0, frames.shape[0], batch):
        b.add(_dev(frames[at:at + batch]), _dev(labels[at:at + batch]))
    torch.cuda.synchronize()
    return b


def _check_plate(frames, labels, batch=None):
    want_d2, want_id, want_plate = R.plate_accumulate(frames, labels)
    b = _accumulated(frames, labels, frames.shape[0] if batch is None else batch)
    assert np.array_equal(b.best_d2.cpu().numpy(), want_d2)
    assert np.array_equal(b.best_id.cpu().numpy(), want_id)
    assert np.array_equal(b.plate.cpu().numpy(), want_plate)
    return b, want_d2, want_plate


@pytest.fixture(scope="module")
def plate_case():
    return R.plate_cases()["40x56"]


def test_plate_accumulate_and_fill_40x56(hiplib, plate_case):
    frames, labels = plate_case
    b, want_d2, want_plate = _check_plate(frames, labels)
    sure = (want_d2 > 25).mean()
    assert 0.05 < sure < 0.95                       # both kinds of pixel are there
    want, _, n_sure = R.plate_fill(want_d2, want_plate)
    got = b.finish()
    assert b.n_sure == n_sure
    assert np.array_equal(got.cpu().numpy(), want)
    from radnerf.prepare import background_plate
    assert torch.equal(background_plate(_dev(frames), _dev(labels), batch=2), got)


@pytest.mark.parametrize("batch", [1, 2, 5])
def test_plate_does_not_depend_on_the_batching(hiplib, plate_case, batch):
    frames, labels = plate_case
    _check_plate(frames, labels, batch)


@pytest.mark.parametrize("H,W", R.EDGE_SHAPES)
def test_plate_at_the_wave_and_workgroup_edges(hiplib, H, W):
    frames, labels = R.plate_cases()[f"{H}x{W}"]
    b, want_d2, want_plate = _check_plate(frames, labels)
    if (want_d2 > 2).any():                           # a threshold these few pixels can pass
        got = b.finish(thresh_d2=2)
        assert np.array_equal(got.cpu().numpy(), R.plate_fill(want_d2, want_plate, 2)[0])


def test_plate_frame_without_foreground_and_corner_pixel(hiplib):
    frames, labels = R.plate_cases()["empty_and_corner"]      # frame 0: one pixel in a corner; frame 1: no foreground
    H, W = labels.shape[1:]
    b, want_d2, _ = _check_plate(frames, labels)
    assert (want_d2 == FAR).all() and (b.best_id.cpu().numpy() == 1).all()
    only = _accumulated(frames[:1], labels[:1], 1)
    yy, xx = np.mgrid[0:H, 0:W]
    assert np.array_equal(only.best_d2.cpu().numpy(), (yy - (H - 1)) ** 2 + (xx - (W - 1)) ** 2)


def test_plate_first_of_two_identical_frames_wins(hiplib):
    b, _, _ = _check_plate(*R.plate_cases()["identical_frames"])      # frames 0 and 1: the same labels, other colours
    assert not (b.best_id.cpu().numpy() == 1).any()


def _fill(hiplib, best_d2, plate, thresh):
    hip = hiplib
    H, W = best_d2.shape
    d, p = _dev(best_d2.astype(np.int32)), _dev(plate)
    n = torch.full((1,), 12345, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(hip._lib.rn_prep_workspace(1, H, W)), dtype=torch.uint8, device="cuda")
    hip.call("rn_prep_plate_fill", hip.ptr(d), hip.ptr(p), H, W, thresh, hip.ptr(n), hip.ptr(ws), hip.stream())
    return p.cpu().numpy(), int(n.item())


def test_fill_ties_go_to_the_smallest_row_then_column(hiplib):
    H, W = 41, 45
    yy, xx = np.mgrid[0:H, 0:W]
    r2 = (yy - 20) ** 2 + (xx - 22) ** 2
    best_d2 = np.where((r2 >= 144) & (r2 < 196), 100, 0)            # a ring of sure pixels, symmetric in both axes
    best_d2[20, 22 - 5] = best_d2[20, 22 + 5] = best_d2[20 - 5, 22] = best_d2[20 + 5, 22] = 100       # four more: ties at the centre
    plate = np.stack([yy, xx, np.full_like(yy, 7)], axis=-1).astype(np.uint8)                         # a colour names its pixel
    got, n_sure = _fill(hiplib, best_d2, plate, 25)
    want, source, want_sure = R.plate_fill(best_d2, plate, 25)
    assert n_sure == want_sure
    assert np.array_equal(got, want)
    assert np.array_equal(got[..., :2], source)                     # the sources, not only their colours
    assert tuple(got[20, 22, :2]) == (15, 22)                       # four at distance 5: the smallest row
    sy, sx = got[..., 0].astype(np.int64), got[..., 1].astype(np.int64)
    sure_lab = np.where(best_d2 > 25, R.OTHER, R.BACKGROUND).astype(np.uint8)
    assert np.array_equal((yy - sy) ** 2 + (xx - sx) ** 2, R.squared_distances(sure_lab))             # each at the brute-force minimum
    # four corners of a rectangle: (4, 5) ties four ways, (2, 5) between two columns of one row, (4, 2) between two rows of one column
    best_d2 = np.zeros((9, 11), dtype=np.int32)
    best_d2[2, 2] = best_d2[2, 8] = best_d2[6, 2] = best_d2[6, 8] = 26
    yy, xx = np.mgrid[0:9, 0:11]
    plate = np.stack([yy, xx, np.full_like(yy, 7)], axis=-1).astype(np.uint8)
    got, n_sure = _fill(hiplib, best_d2, plate, 25)
    assert n_sure == 4 and np.array_equal(got, R.plate_fill(best_d2, plate, 25)[0])
    assert tuple(got[4, 5, :2]) == (2, 2) and tuple(got[2, 5, :2]) == (2, 2) and tuple(got[4, 2, :2]) == (2, 2)
    assert tuple(got[6, 5, :2]) == (6, 2) and tuple(got[4, 8, :2]) == (2, 8) and tuple(got[5, 5, :2]) == (6, 2)


def test_fill_without_a_sure_pixel(hiplib):
    from radnerf.prepare import background_plate
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, (2, 6, 10, 3), dtype=np.uint8)
    labels = rng.integers(0, 4, (2, 6, 10)).astype(np.uint8)        # all foreground
    with pytest.raises(ValueError, match="no background"):
        background_plate(_dev(frames), _dev(labels))
    plate = rng.integers(0, 256, (6, 10, 3), dtype=np.uint8)
    got, n_sure = _fill(hiplib, np.zeros((6, 10), np.int32), plate, 25)
    assert n_sure == 0 and np.array_equal(got, plate)


# ------------------------------------------------------------------------------------------------------------------ layers
LH, LW = 128, 72


def _layer_maps():
    rng = np.random.default_rng(606)
    maps = [R.portrait_labels(LH, LW, rng) for _ in range(4)]
    maps.append(R.portrait_labels(LH, LW, rng, neck=False))
    maps.append(R.portrait_labels(LH, LW, rng, jag=9, holes=0.05))
    return maps


def _edge_maps():
    rng = np.random.default_rng(707)
    out = {}
    m = R.portrait_labels(LH, LW, rng, neck_top=5, jag=0, holes=0)          # raw neck top at row 5: the dilated top at row 2
    m[0:5, LW // 2 - 4:LW // 2 + 4] = R.HEAD
    out["neck_top_row_2"] = m
    m = R.portrait_labels(LH, LW, rng, neck_top=3, jag=2, holes=0)          # dilated tops at rows 0 .. 2, in-paints leave the image
    for x in np.nonzero((m == R.NECK).any(0))[0]:
        m[:np.argmax(m[:, x] == R.NECK), x] = R.HEAD                        # a head above every neck column ...
    m[LH - 1] = R.HEAD                                                      # ... and where a wrapped row -1 would look
    out["neck_top_row_0_to_2"] = m
    m = np.full((LH, LW), R.BACKGROUND, dtype=np.uint8)                     # torso from row 0 (no head above), row 1 .. 9 under a head
    for x in range(LW):
        top = x % 11
        m[:top, x] = R.HEAD
        m[top:, x] = R.TORSO
    m[LH - 1, ::2] = R.HEAD
    out["torso_top_row_0"] = m
    m = np.full((LH, LW), R.BACKGROUND, dtype=np.uint8)                     # one raw neck pixel near the bottom: n = 4, 5, 6, 7
    for k, x in enumerate(range(4, 60, 4)):
        r = LH - 1 - (k % 5)
        m[:r - 3, x] = R.HEAD
        m[r, x] = R.NECK
    m[10:60, 64] = R.HEAD                                                   # two neck runs: n is the column's count, not the top run's
    m[60, 64] = m[75, 64] = m[76, 64] = R.NECK
    out["neck_counts"] = m
    m = R.portrait_labels(LH, LW, rng, holes=0)                             # a torso patch ABOVE the neck: both in-paints in one column
    cols = slice(LW // 2 - 6, LW // 2 + 6)
    m[30:34, cols] = R.TORSO
    out["overlap"] = m
    return out


@pytest.fixture(scope="module")
def layer_inputs():
    rng = np.random.default_rng(808)
    plate = rng.integers(0, 256, (LH, LW, 3), dtype=np.uint8)
    return plate, lambda n: rng.integers(0, 256, (n, LH, LW, 3), dtype=np.uint8)


def _check_layers(frames, labels, plate):
    from radnerf.prepare import layers
    want_gt, want_torso = R.layers_batch(frames, labels, plate)
    gt, torso = layers(_dev(frames), _dev(labels), _dev(plate))
    gt, torso = gt.cpu().numpy(), torso.cpu().numpy()
    assert np.array_equal(gt, want_gt)
    bad = np.argwhere((torso != want_torso).any(-1))
    assert bad.shape[0] == 0, f"{bad.shape[0]} torso pixels differ, first (frame, row, column) {bad[:5].tolist()}"
    return want_torso


def test_layers_on_portrait_maps(hiplib, layer_inputs):
    plate, make = layer_inputs
    labels = np.stack(_layer_maps())
    want = _check_layers(make(len(labels)), labels, plate)
    assert (want[..., 3] == 255).any() and (want[..., 3] == 0).any()
    assert (want[4][..., 3] == 255).any()                                   # the map without a neck still has its torso


@pytest.mark.parametrize("name", ["neck_top_row_2", "neck_top_row_0_to_2", "torso_top_row_0", "neck_counts", "overlap"])
def test_layers_at_the_edges(hiplib, layer_inputs, name):
    plate, make = layer_inputs
    label = _edge_maps()[name]
    frames = make(1)
    want = _check_layers(frames, label[None], plate)
    if name == "neck_top_row_2":
        assert want[0, 0, LW // 2, 3] == 255                                # the in-paint reaches row 0 and stops there
        assert want[0, LH - 1, 0, 3] == 0
    if name == "neck_counts":
        assert want[0, LH - 60, 4, 3] == 0 and want[0, LH - 30, 4, 3] == 255


def test_layers_batch_equals_single_frames(hiplib, layer_inputs):
    from radnerf.prepare import layers
    plate, make = layer_inputs
    labels = np.stack(_layer_maps()[:3])
    frames = make(3)
    gt, torso = layers(_dev(frames), _dev(labels), _dev(plate))
    for f in range(3):
        g1, t1 = layers(_dev(frames[f:f + 1]), _dev(labels[f:f + 1]), _dev(plate))
        assert torch.equal(g1[0], gt[f]) and torch.equal(t1[0], torso[f])


def test_argument_checks(hiplib):
    hip = hiplib
    assert hip._lib.rn_prep_workspace(0, 4, 4) == 0 and hip._lib.rn_prep_workspace(1, 0, 4) == 0
    assert hip._lib.rn_prep_workspace(1, 16385, 4) == 0 and hip._lib.rn_prep_workspace(1 << 20, 64, 64) == 0
    assert hip._lib.rn_prep_workspace(2, 8, 8) >= 2 * 8 * 8 * 4
    t = torch.zeros(64, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="null pointer"):
        hip.call("rn_prep_layers", hip.ptr(t), None, hip.ptr(t), hip.ptr(t), 1, 2, 2, hip.ptr(t), hip.ptr(t), hip.ptr(t), hip.stream())
    with pytest.raises(RuntimeError, match="F, H, W"):
        hip.call("rn_prep_plate_accumulate", hip.ptr(t), hip.ptr(t), 1, 0, 2, 0, hip.ptr(t), hip.ptr(t), hip.ptr(t), hip.ptr(t), hip.stream())


# -------------------------------------------------------------------------------------------------------------- end to end
def test_task_6_through_the_decode_and_write_hooks(hiplib, tmp_path):
    """.npy twins in, arrays out: no image library on either side.  Three frames in batches of two."""
    from radnerf import prepare
    rng = np.random.default_rng(11)
    root, H, W = str(tmp_path), 70, 40
    for sub in ("ori_imgs", "parsing"):
        os.makedirs(os.path.join(root, sub))
    frames = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    labels = np.stack([R.portrait_labels(H, W, rng) for _ in range(3)])
    plate = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    np.save(os.path.join(root, "bc.npy"), plate)
    open(os.path.join(root, "bc.jpg"), "wb").close()
    for i, name in enumerate(("7", "10", "9")):                             # taken as 7, 9, 10
        open(os.path.join(root, "ori_imgs", name + ".jpg"), "wb").close()
        np.save(os.path.join(root, "ori_imgs", name + ".npy"), frames[i])
        np.save(os.path.join(root, "parsing", name + ".npy"), R.parsing_from_labels(labels[i]))
    written = {}
    assert prepare.main([root, "--task", "6", "--batch", "2"], log=lambda *a: None, decode=dd.npy_decode,
                        write=lambda path, rgba: written.__setitem__(os.path.basename(path), rgba.copy())) == [6]
    want_gt, want_torso = R.layers_batch(frames, labels, plate)
    assert sorted(written) == ["10.png", "7.png", "9.png"]
    for i, name in enumerate(("7", "10", "9")):
        assert np.array_equal(written[name + ".png"], want_torso[i])
        assert os.path.getsize(os.path.join(root, "gt_imgs", name + ".jpg")) > 600
    assert not os.listdir(os.path.join(root, "torso_imgs"))                 # the hook took them


EH, EW, EF = 64, 48, 41


def _write_source_directory(root):
    """ori_imgs/<id>.jpg (PNG streams under the layout's names, so the frames are known exactly), parsing/<id>.png, the landmark
    files and the audio file the loader reads, and track_params.pt."""
    from PIL import Image
    rng = np.random.default_rng(909)
    for sub in ("ori_imgs", "parsing"):
        os.makedirs(os.path.join(root, sub))
    yy, xx = np.mgrid[0:EH, 0:EW]
    frames, labels = [], []
    for i in range(EF):
        shift = int(round(3 * np.sin(i / 4)))
        label = np.roll(R.portrait_labels(EH, EW, np.random.default_rng(i // 8), holes=0.01), shift, axis=1)
        frame = np.stack([(2 * yy + 3 * i) % 256, (3 * xx + 40 * (label == R.HEAD)) % 256, (yy + xx + 90 * (label == R.TORSO)) % 256], -1)
        frame = (frame + rng.integers(0, 4, frame.shape)).clip(0, 255).astype(np.uint8)
        for arr, path in ((frame, os.path.join(root, "ori_imgs", f"{i}.jpg")), (R.parsing_from_labels(label), os.path.join(root, "parsing", f"{i}.png"))):
            with open(path, "wb") as fh:
                Image.fromarray(arr).save(fh, format="PNG")
        lms = np.round(rng.random((68, 2)) * np.array([EW - 1, EH - 1]), 1)
        lms[48:60] = np.round(np.array([EW / 2 - 8, EH / 2]) + rng.random((12, 2)) * 16, 1)
        np.savetxt(os.path.join(root, "ori_imgs", f"{i}.lms"), lms, fmt="%.1f")
        frames.append(frame)
        labels.append(label)
    np.save(os.path.join(root, "aud_eo.npy"), rng.standard_normal((EF, 16, 44)).astype(np.float32))
    torch.save(dict(focal=torch.tensor([1200.0]), euler=torch.from_numpy((rng.random((EF, 3)) * 0.4 - 0.2).astype(np.float32)),
                    trans=torch.from_numpy((rng.random((EF, 3)) * np.array([1, 1, 0]) + np.array([0, 0, -30])).astype(np.float32))),
               os.path.join(root, "track_params.pt"))
    return np.stack(frames), np.stack(labels)


def _pil_decode(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGBA" if im.mode == "RGBA" else "RGB"), dtype=np.uint8).copy()


def _pil_error(arr):
    """Mean absolute error of PIL's own quality-95 4:2:0 JPEG of `arr`, decoded by PIL."""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="JPEG", quality=95, subsampling="4:2:0")
    buf.seek(0)
    return float(np.abs(np.asarray(Image.open(buf).convert("RGB"), dtype=np.int32) - arr).mean())


def test_task_minus_1_end_to_end(hiplib, tmp_path):
    from radnerf import prepare
    from radnerf.dataset import DeviceTrainSet
    root = str(tmp_path)
    frames, labels = _write_source_directory(root)
    log = []
    assert prepare.main([root, "--batch", "16"], log=log.append) == [5, 6, 9]
    bc = _pil_decode(os.path.join(root, "bc.jpg"))
    assert bc.shape == (EH, EW, 3)
    exact_plate = R.background_plate(frames[::20], labels[::20])
    bc_err, bc_pil = np.abs(bc.astype(np.int32) - exact_plate).mean(), _pil_error(exact_plate)
    print(f"bc.jpg mean absolute error: device encoder {bc_err:.4f}, PIL q95 4:2:0 {bc_pil:.4f}")
    assert bc_err <= 1.1 * bc_pil                                           # the file is the plate, through one JPEG round trip
    want_gt, want_torso = R.layers_batch(frames, labels, bc)                # from the DECODED bc.jpg, as task 6 reads it
    ours, pils = [], []
    for i in range(EF):
        torso = _pil_decode(os.path.join(root, "torso_imgs", f"{i}.png"))
        assert torso.shape == (EH, EW, 4) and np.array_equal(torso, want_torso[i])
        gt = _pil_decode(os.path.join(root, "gt_imgs", f"{i}.jpg"))
        assert gt.shape == (EH, EW, 3)
        ours.append(np.abs(gt.astype(np.int32) - want_gt[i]).mean())
        pils.append(_pil_error(want_gt[i]))
    ours, pils = float(np.mean(ours)), float(np.mean(pils))
    print(f"gt JPEG mean absolute error: device encoder {ours:.4f}, PIL q95 4:2:0 {pils:.4f}, ratio {ours / pils:.4f}")
    assert ours <= 1.1 * pils
    with open(os.path.join(root, "transforms_train.json")) as fh:
        assert len(json.load(fh)["frames"]) == int(EF * 10 / 11)
    ds = DeviceTrainSet.from_directory(root, dd.dataset_opt(root), "train", num_rays=64, seed=1, device="cuda", kernel="hip")
    assert ds.loaded.F == int(EF * 10 / 11) and (ds.loaded.H, ds.loaded.W) == (EH, EW)
