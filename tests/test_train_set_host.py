"""DeviceTrainSet (radnerf/dataset.py) without a GPU: its torch path against the reference loader's recorded batches
(tests/golden/reference_batch.npz), the host-side pieces (mirror_index, order, the draw), and the argument checks of
rn_train_set_batch / rn_train_set_frame through ctypes."""
import ctypes as C

import numpy as np
import pytest
import torch

import train_set_cases as tc


@pytest.fixture(scope="module")
def _pkg(hiplib):
    import radnerf.dataset as dataset
    return dataset


@pytest.mark.parametrize("tag,torso_mode,att,index", tc.cases())
def test_torch_path_equals_the_reference_collate(_pkg, tag, torso_mode, att, index):
    """Every recorded case, every output bit for bit: on the CPU the torch path runs the torch ops the reference ran, so rays_d
    and poses are asserted equal as well (their bars of 2e-7 / 1e-6 are for the kernel)."""
    g = tc.golden()
    ds = tc.make_set("cpu", torso_mode, att)
    out = ds.batch([index], inds=g[f"{tag}_inds"])
    tc.compare_with_golden(out, tag, torso_mode, exact=True)
    nrays = int(g["shape"][3])
    assert out["rays_o"].shape == (1, nrays, 3) and out["bg_coords"].shape == (1, nrays, 2) and out["face_mask"].shape == (1, nrays)
    assert out["auds"].shape == ((1 if att == 0 else 8), int(g["shape"][4]), 16) and out["poses"].shape == (1, 6)
    assert out["poses_matrix"].shape == (1, 4, 4) and out["eye"].shape == (1, 1)
    ds.check()                                                  # nothing was out of range


def test_batch_is_views_of_one_buffer_rewritten_in_place(_pkg):
    from radnerf.train import SyntheticTrainStream
    g = tc.golden()
    ds = tc.make_set("cpu", False, 2)
    a = ds.batch([0], inds=g["c0_inds"])
    assert ds._WIDTHS == SyntheticTrainStream._WIDTHS
    assert set(a) == {"rays_o", "rays_d", "bg_coords", "poses", "face_mask", "eye", "auds", "index", "bg_color", "images",
                      "bg_torso_color", "_packed", "_unpack", "poses_matrix", "H", "W", "_index_dev"}
    assert a["_index_dev"].tolist() == a["index"] == [0]
    flat, nrays = a["_packed"], int(g["shape"][3])
    assert flat.numel() == 15 * nrays and a["rays_o"].data_ptr() == flat.data_ptr()
    assert a["face_mask"].data_ptr() == flat.data_ptr() + 14 * nrays * 4 and a["images"].data_ptr() == a["bg_torso_color"].data_ptr()
    before = flat.clone()
    b = ds.batch([3], inds=g["c1_inds"])
    assert b["_packed"] is flat and b["poses"] is a["poses"] and b["auds"] is a["auds"] and not torch.equal(before, flat)
    again = a["_unpack"](before)                                # what GraphedTrainer does with its static copy
    assert again["_packed"] is before and torch.equal(again["rays_d"], before[3 * nrays:6 * nrays].view(1, nrays, 3))
    assert isinstance(b["index"], list) and b["index"] == [3]


def test_frame_equals_the_reference_collate(_pkg):
    g = tc.golden()
    torso_mode, att, index = (int(v) for v in g["frame_case"])
    ds = tc.make_set("cpu", bool(torso_mode), att)
    out = ds.frame(index)
    tc.compare_with_golden(out, "frame", bool(torso_mode), training=False, exact=True)
    H, W = int(g["shape"][1]), int(g["shape"][2])
    assert out["images"].shape == (1, H, W, 3) and out["bg_color"].shape == (1, H * W, 3) and "face_mask" not in out
    # the index is mirrored for the pose and the images, the audio index is not (provider.py:632-640)
    F = int(g["shape"][0])
    m = ds.frame(F + 2, aud_index=3)
    assert m["index"] == [F - 3]
    images, pose = m["images"].clone(), m["poses_matrix"].clone()
    auds = m["auds"].clone()
    plain = ds.frame(F - 3, aud_index=3)
    assert torch.equal(images, plain["images"]) and torch.equal(pose, plain["poses_matrix"]) and torch.equal(auds, plain["auds"])
    from radnerf.rays import get_audio_features
    assert torch.equal(auds, get_audio_features(torch.from_numpy(g["auds"]), att, 3))
    with pytest.raises(IndexError):
        ds.frame(F + 2)                                         # its own audio index F + 2 does not exist in F audio frames


def test_mirror_index(_pkg):
    g = tc.golden()
    F = int(g["shape"][0])
    ds = tc.make_set("cpu", False, 0)
    assert {F - 1, F, 2 * F - 1, 2 * F} <= set(g["mirror_in"].tolist())
    assert [ds.mirror_index(int(i)) for i in g["mirror_in"]] == g["mirror_out"].tolist()       # the reference's own answers
    assert [ds.mirror_index(i) for i in (F - 1, F, 2 * F - 1, 2 * F)] == [F - 1, F - 1, 0, 0]


def test_order_is_a_seeded_permutation(_pkg):
    F = int(tc.golden()["shape"][0])
    a, b = tc.make_set("cpu", False, 0, seed=5), tc.make_set("cpu", False, 0, seed=5)
    assert sorted(a.order(0)) == list(range(F)) and all(isinstance(i, int) for i in a.order(0))
    assert a.order(0) == b.order(0) == a.order(0) and a.order(7) == b.order(7)
    assert a.order(0) != a.order(1) and a.order(1) != a.order(2)
    assert tc.make_set("cpu", False, 0, seed=6).order(0) != a.order(0)


def test_out_of_range_pixels_are_clamped_and_reported(_pkg):
    g = tc.golden()
    H, W = int(g["shape"][1]), int(g["shape"][2])
    ds = tc.make_set("cpu", False, 2)
    a = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in ds.batch([3], inds=[0, H * W - 1, 7]).items()}
    ds.check()
    b = ds.batch([3], inds=[-1, H * W, 7])
    assert torch.equal(a["_packed"], b["_packed"])
    with pytest.raises(IndexError, match="2 pixel indices"):
        ds.check()
    ds.check()                                                  # reported once


def test_self_drawn_pixels_on_the_torch_path(_pkg):
    """The torch path restates the kernel's counter-based draw: in range, a function of (seed, draw) alone."""
    g = tc.golden()
    H, W = int(g["shape"][1]), int(g["shape"][2])
    ds = tc.make_set("cpu", False, 2, num_rays=4096, seed=11)
    first = ds.batch([0])["_packed"].clone()
    picked = ds.inds.clone()
    assert int(picked.min()) >= 0 and int(picked.max()) < H * W and picked.unique().numel() > 1500
    second = ds.batch([0])["_packed"].clone()
    assert not torch.equal(first, second)                       # the draw counter advanced
    again = tc.make_set("cpu", False, 2, num_rays=4096, seed=11)
    assert torch.equal(again.batch([0])["_packed"], first) and torch.equal(again.batch([0])["_packed"], second)
    assert torch.equal(_pkg.drawn_pixels(11, 0, 4096, H * W, "cpu"), picked)
    assert not torch.equal(_pkg.drawn_pixels(12, 0, 4096, H * W, "cpu"), picked)
    assert torch.equal(ds.batch([0], inds=picked)["_packed"], first)


def test_constructor_refuses_what_it_cannot_serve(_pkg):
    g = tc.golden()
    with pytest.raises(TypeError, match="uint8"):
        tc.make_set("cpu", False, 2, images=g["images"].astype(np.float32))
    with pytest.raises(ValueError, match="8 audio frames"):
        tc.make_set("cpu", False, 2, auds=g["auds"][:7])
    with pytest.raises(ValueError, match="needs a GPU"):
        tc.make_set("cpu", False, 2, kernel="hip")
    with pytest.raises(NotImplementedError):
        tc.make_set("cpu", False, 3)


def test_entry_points_refuse_bad_arguments(hiplib):
    """As tests/test_abi.py does for the neighbours: refused on the host with RN_ERR_INVALID_ARG and a message, before anything
    touches a GPU.  Host memory stands in for the device buffers: every call below is one the library refuses."""
    from radnerf_hip import abi
    lib, err = hiplib._lib, hiplib.last_error
    buf = (C.c_float * 64)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)
    odd = C.c_void_p(p.value + 4)

    def desc(**kw):
        d = abi.TrainSetT(images=p, torso=p, bg=p, poses=p, face_rect=p, eye=p, auds=p, fx=60.0, fy=60.0, cx=26.0, cy=18.0, H=37, W=53,
                          F=9, Fa=9, C=29, att=2, torso_mode=0)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def batch(d=desc(), frame=0, aud=0, n=257, **null):
        a = dict(packed=p, poses6=p, pose_matrix=p, auds_out=p, bad=p)
        a.update(null)
        return lib.rn_train_set_batch(C.byref(d) if d is not None else None, frame, aud, None, n, 0, 0, a["packed"], None, a["poses6"],
                                      a["pose_matrix"], None, a["auds_out"], a["bad"], None)

    def frame(d=desc(), frame=0, aud=0, **null):
        a = dict(packed=p, poses6=p, pose_matrix=p, auds_out=p)
        a.update(null)
        return lib.rn_train_set_frame(C.byref(d) if d is not None else None, frame, aud, a["packed"], a["poses6"], a["pose_matrix"], None,
                                      a["auds_out"], None)

    assert batch(d=None, n=0) == 0                                                # nothing to do
    for call in (batch, frame):
        assert call(d=None) == abi_err() and "null descriptor" in err()
        for name in ("images", "torso", "bg", "poses", "face_rect", "auds"):
            assert call(d=desc(**{name: None})) == abi_err() and "null pointer" in err(), name
        assert call(frame=9) == abi_err() and "frame 9 is outside the 9 frames" in err()
        assert call(aud=9) == abi_err() and "audio frame 9" in err()
        assert call(d=desc(Fa=7)) == abi_err() and "at least 8" in err()
        assert call(d=desc(H=1)) == abi_err() and "H, W >= 2" in err()
        assert call(d=desc(W=1)) == abi_err() and "H, W >= 2" in err()
        assert call(d=desc(H=65536, W=32768)) == abi_err() and "2^31" in err()
        assert call(d=desc(att=3)) == abi_err() and "att" in err()
        assert call(d=desc(torso=C.c_void_p(p.value + 1))) == abi_err() and "4-byte aligned" in err()
        for name in ("packed", "poses6", "pose_matrix", "auds_out"):
            assert call(**{name: None}) == abi_err() and "null pointer" in err(), name
        assert call(packed=odd) == abi_err() and "8-byte aligned" in err()
    assert batch(bad=None) == abi_err() and "null pointer" in err()


def abi_err():
    return -1                                                   # RN_ERR_INVALID_ARG (include/radnerf_hip.h; tests/test_abi.py pins it)
