"""The JPEG kernels and the video write-out on the device against tests/jpegref64.py (numpy alone: no PIL, no reference tree):
coefficients under the tie rule, scans byte for byte, complete files through the reference decoder, reproducibility, batching;
VideoSink and `radnerf.cli --test --video` end to end."""
import functools
import os
import sys
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dataset_dir as dd  # noqa: E402
import jpegref64 as R  # noqa: E402

SIZES = [(17, 19), (40, 24), (48, 64), (90, 90)]
SUBS = ["420", "444"]
QUALITIES = [50, 90, 100]


@functools.lru_cache(maxsize=None)
def _frame(hw, seed):
    """A seed of R.scene, ("turned", seed) for that scene turned by 180 degrees, or ("checker", cell, inverted) for R.block_checker."""
    if isinstance(seed, tuple) and seed[0] == "turned":
        f = R.scene(*hw, seed[1], turned=True)
    elif isinstance(seed, tuple):
        _, cell, inverted = seed
        f = 255 - R.block_checker(*hw, cell) if inverted else R.block_checker(*hw, cell)
    else:
        f = R.scene(*hw, seed)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _reference(hw, seed, q, sub):
    """(flags [blocks, 64], the reference file's own decode) of one frame, computed once."""
    frame = _frame(hw, seed)
    flags = R.flagged(R.quotients(frame, q, sub)[0])
    return flags, R.decode(R.encode(frame, q, sub))


def _unflagged_pixels(flags, hw, sub):
    """[H, W] bool: pixels of MCUs none of whose coefficients is flagged."""
    mh, mw, per, _ = R.block_layout(*hw, sub)
    m = R.mcu_side(sub)
    clean = ~flags.reshape(mh, mw, per * 64).any(-1)
    return np.repeat(np.repeat(clean, m, 0), m, 1)[:hw[0], :hw[1]]


def _against_the_reference(hw, sub, q, seeds):
    """The whole write-out of the frames `seeds` name (_frame) against the reference, as one batch.  -> the device's coefficients and
    the flags, [frames, blocks, 64] each."""
    from radnerf.video import JpegEncoder
    n_frames = len(seeds)                                          # different frames: the predictor reset and the offsets matter
    frames = torch.from_numpy(np.stack([_frame(hw, s) for s in seeds])).cuda()
    enc = JpegEncoder(*hw, quality=q, subsampling=sub)
    coefs = enc.coefficients(frames)
    data, sizes = enc.encode(frames)
    coefs = coefs.cpu().numpy()
    assert coefs.shape == (n_frames, enc.blocks, 64) and len(sizes) == n_frames and len(data) == sizes.sum()
    files = enc.wrap(data, sizes)
    at, all_flags = 0, []
    for i, seed in enumerate(seeds):
        # coefficients: the float64 reference's except at flagged ties (within 1 there, at most 2 % flagged)
        flags = R.compare_coefficients(coefs[i], _frame(hw, seed), q, sub)
        # the scan: the reference entropy coder on the device's OWN coefficients, byte for byte
        want = R.entropy(coefs[i], sub)
        assert sizes[i] == len(want)
        assert data[at:at + len(want)] == want
        at += len(want)
        # the complete file through the reference decoder: the reference file's own decode +-1 wherever no coefficient was flagged
        ref_flags, ref_rgb = _reference(hw, seed, q, sub)
        assert np.array_equal(flags, ref_flags)
        all_flags.append(flags)
        got = R.decode(files[i]).astype(np.int64)
        keep = _unflagged_pixels(flags, hw, sub)
        assert got.shape == ref_rgb.shape and (not keep.any() or np.abs(got - ref_rgb.astype(np.int64))[keep].max() <= 1)
    # two runs: the same bytes
    again, sizes2 = enc.encode(frames)
    assert again == data and np.array_equal(sizes2, sizes)
    # a batch of three is three batches of one
    if n_frames > 1:
        singles = [enc.encode(frames[i:i + 1]) for i in range(n_frames)]
        assert b"".join(s[0] for s in singles) == data and [int(s[1][0]) for s in singles] == [int(v) for v in sizes]
    return coefs, np.stack(all_flags)


@pytest.mark.parametrize("n_frames", [1, 3])
@pytest.mark.parametrize("q", QUALITIES)
@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("hw", SIZES)
def test_kernels_against_the_reference(hiplib, hw, sub, q, n_frames):
    _against_the_reference(hw, sub, q, (1, 2, 3)[:n_frames])


@pytest.mark.parametrize("n_frames", [1, 3])
@pytest.mark.parametrize("q", [50, 100])
@pytest.mark.parametrize("hw,sub,blocks", R.ROUND_SHAPES, ids=[f"{b}-blocks-{s}" for _, s, b in R.ROUND_SHAPES])
def test_kernels_past_one_scan_round(hiplib, hw, sub, blocks, q, n_frames):
    """k_jpeg_scan takes 1024 entries a round and carries their sum into the next: frames just below 1024 blocks, just above (one
    carry) and above 2048 (two); with three frames every one of the three scan workgroups carries.  Turned scenes: their last blocks
    hold bits to misplace (tests/test_video.py)."""
    coefs, _ = _against_the_reference(hw, sub, q, (("turned", 1), ("turned", 2), ("turned", 3))[:n_frames])
    assert coefs.shape[1] == blocks


@pytest.mark.parametrize("n_frames", [1, 3])
@pytest.mark.parametrize("q", R.LOW_QUALITIES)
@pytest.mark.parametrize("hw,sub", R.LOW_SHAPES, ids=[f"{h}x{w}-{s}" for (h, w), s in R.LOW_SHAPES])
def test_kernels_below_quality_50(hiplib, hw, sub, q, n_frames):
    """The 5000 / q branch of quant_step; at quality 1 every step is clamped to 255."""
    _against_the_reference(hw, sub, q, (1, 2, 3)[:n_frames])


@pytest.mark.parametrize("q", [50, 100])
@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("hw", list(R.TINY_SEEDS), ids=[f"{h}x{w}" for h, w in R.TINY_SEEDS])
def test_kernels_at_degenerate_sizes(hiplib, hw, sub, q):
    """Sides of 1, sides below one block (every sample of a block replicated from one row or column), a side of exactly one MCU:
    the three seeds of the shape (tests/test_video.py holds them to the tie rule's cap) as a batch, and the first one alone."""
    _against_the_reference(hw, sub, q, R.TINY_SEEDS[hw])
    _against_the_reference(hw, sub, q, R.TINY_SEEDS[hw][:1])


@pytest.mark.parametrize("hw,sub,cell", R.CHECKERS)
def test_kernels_on_block_checkers(hiplib, hw, sub, cell):
    """Black next to white at quality 100: the coefficient pass itself produces DC differences of 2040 (category 11), and since no
    quotient is near a tie its coefficients are the reference's own."""
    seeds = (("checker", cell, False), ("checker", cell, True))
    coefs, flags = _against_the_reference(hw, sub, 100, seeds)
    assert not flags.any()
    for i, seed in enumerate(seeds):
        quot, comp = R.quotients(_frame(hw, seed), 100, sub)
        want = R.round_half_away(quot)
        assert np.array_equal(coefs[i], want) and np.abs(np.diff(want[comp == 0, 0])).max() == 2040


SENTINEL = 0xA5


def _entropy(enc, coefs):
    """rn_jpeg_entropy as JpegEncoder.entropy calls it, into a buffer that holds SENTINEL in every byte: the bytes of every frame, and
    nothing written behind the last one.  coefs: int16 [F, blocks, 64] numpy."""
    hip, F = enc._hip, len(coefs)
    dev = torch.from_numpy(np.array(coefs)).cuda()
    head = enc._head(F)
    buf = torch.full((head + F * enc.capacity,), SENTINEL, dtype=torch.uint8, device="cuda")
    ws = torch.empty(int(hip._lib.rn_jpeg_workspace(F, enc.H, enc.W, enc._sub)), dtype=torch.uint8, device="cuda")
    hip.call("rn_jpeg_entropy", hip.ptr(dev), F, enc.H, enc.W, enc._sub, hip.ptr(ws), hip.ptr(buf[head:]), F * enc.capacity, hip.ptr(buf),
             hip.stream())
    host = buf.cpu().numpy()
    sizes = host[:4 * F].view(np.uint32).astype(np.int64)
    used = int(sizes.sum())
    assert used <= F * enc.capacity and (host[4 * F:head] == SENTINEL).all() and (host[head + used:] == SENTINEL).all()
    # the encoder's own call gives the same bytes
    own = enc.entropy(dev)[:head + used].cpu().numpy()
    assert np.array_equal(own[:4 * F], host[:4 * F]) and np.array_equal(own[head:], host[head:head + used])
    ends = np.cumsum(sizes)
    return [host[head + e - n:head + e].tobytes() for e, n in zip(ends, sizes)]


def test_dense_0xff_across_chunks_vectors_and_frames(hiplib):
    """R.dense_batch: two frames of about 220 KB, a fifth of it 0xFF, over more than 40 chunks each, and a short frame behind them
    (tests/test_video.py holds the scans to having a 0xFF on both sides of chunk and thread seams).  Every stuffed byte's place is
    a sum of the 0xFF counts of the chunks before it (ff_offsets), of the threads before it (`before`) and of the frames before it
    (frame_base)."""
    from radnerf.video import JpegEncoder
    batch = R.dense_batch()
    want = [R.entropy(c, "444") for c in batch]
    enc = JpegEncoder(*R.DENSE_HW, quality=100, subsampling="444")
    assert enc.blocks == batch.shape[1]
    got = _entropy(enc, batch)
    assert [len(g) for g in got] == [len(w) for w in want]
    for g, w in zip(got, want):
        assert g == w
    for i in range(len(batch)):                                    # one frame at a time
        assert _entropy(enc, batch[i:i + 1]) == [want[i]]
    assert _entropy(enc, batch) == got


def test_padded_last_byte_becomes_0xff(hiplib):
    """A frame whose stream ends one bit into a byte: the padding makes that byte 0xFF, which takes a 0x00 behind it and moves the
    frame after it by one more byte."""
    from radnerf.video import JpegEncoder
    enc = JpegEncoder(8, 8, quality=100, subsampling="444")
    padded = R.dense_coefficients(3, R.PADDED_FF_SEED)
    batch = np.stack([padded, R.dense_coefficients(3, R.PADDED_FF_SEED + 1), padded])
    want = [R.entropy(c, "444") for c in batch]
    assert want[0][-2:] == b"\xff\x00"
    assert _entropy(enc, batch) == want and _entropy(enc, batch[:1]) == want[:1]


BIG_HW = (800, 800)


@functools.lru_cache(maxsize=None)
def _big_reference():
    coefs = R.dense_coefficients(R.block_layout(*BIG_HW, "444")[0] ** 2 * 3, 7)
    coefs.setflags(write=False)
    return coefs, R.entropy(coefs, "444")


def test_chunk_scan_past_one_round(hiplib):
    """The scan's second use, over the 0xFF counts of the chunks: one dense frame of 30 000 blocks, whose unstuffed stream passes
    1024 chunks of 4096 bytes."""
    from radnerf.video import JpegEncoder
    coefs, want = _big_reference()
    assert len(want) - want.count(b"\xff\x00") > 1024 * 4096
    enc = JpegEncoder(*BIG_HW, quality=100, subsampling="444")
    assert enc.blocks == len(coefs) == 30000
    got, = _entropy(enc, coefs[None])
    assert len(got) == len(want) and got == want


def test_entropy_pass_clamps_coefficients_beyond_the_invariants(hiplib):
    """int16 extremes in every position: no length passes the worst case the buffers are sized by -- the scan is as long as that of
    the coefficients clamped to |DC difference| <= 2047, |AC| <= 1023."""
    from radnerf.video import JpegEncoder
    enc = JpegEncoder(16, 24, quality=100, subsampling="420")
    rng = np.random.default_rng(5)
    coefs = rng.choice(np.array([-32768, -1024, -1023, 1023, 1024, 32767], np.int16), (2, enc.blocks, 64))
    buf = enc.entropy(torch.from_numpy(coefs).cuda()).cpu().numpy()
    sizes = buf[:8].view(np.uint32)
    clamped = np.clip(coefs.astype(np.int64), -1023, 1023)
    at = enc._head(2)
    for i in range(2):
        c = clamped[i].copy()
        # the DC differences as the device clamps them, turned back into DC values for the reference coder
        per, comps = 6, [0, 0, 0, 0, 1, 2]
        pred_true, pred_ref = [0, 0, 0], [0, 0, 0]
        for b in range(enc.blocks):
            k = comps[b % per]
            diff = int(np.clip(int(coefs[i, b, 0]) - pred_true[k], -2047, 2047))
            pred_true[k] = int(coefs[i, b, 0])
            c[b, 0] = pred_ref[k] + diff
            pred_ref[k] = c[b, 0]
        want = R.entropy(c, "420")
        assert sizes[i] == len(want) <= enc.capacity and buf[at:at + len(want)].tobytes() == want
        at += len(want)


def test_video_sink_equals_the_encoder(hiplib, tmp_path):
    """Five frames in batches of two (a tail batch of one) through the side stream and the AviWriter: the files of JpegEncoder.files."""
    from radnerf.video import AviWriter, JpegEncoder, VideoSink
    hw = (40, 24)
    frames = torch.from_numpy(np.stack([_frame(hw, s) for s in (1, 2, 3, 4, 5)])).cuda()
    enc = JpegEncoder(*hw, quality=90, subsampling="420")
    want = enc.files(frames)
    sink = VideoSink(AviWriter(tmp_path / "sink.avi", *hw, 25), JpegEncoder(*hw, quality=90, subsampling="420"), batch=2)
    for f in frames.unbind(0):
        sink.push(f.clone())
    path = sink.finish()
    avi = R.read_avi(open(path, "rb").read())
    assert [c[2] for c in avi["movi"]] == want and avi["avih"]["total_frames"] == 5 and sink.files == 5
    # a guess that is too small costs a second copy, not bytes, and the next guess follows the batch
    small = JpegEncoder(*hw, quality=90, subsampling="420")
    small.guess = 16
    assert small.files(frames) == want and small.guess >= sum(len(w) - len(enc.header) - 2 for w in want) // 5


@pytest.fixture(scope="module")
def clip(tmp_path_factory, hiplib):
    """One epoch on tests/dataset_dir.py's directory, then --test --video with a 16 kHz track."""
    from radnerf import cli
    root = str(tmp_path_factory.mktemp("dataset"))
    ws = str(tmp_path_factory.mktemp("workspace"))
    dd.write_dataset(root, 0)
    wav = os.path.join(root, "aud.wav")
    pcm = (np.arange(16000 * dd.N_AUD // 25) * 37 % 65536 - 32768).astype("<i2").tobytes()
    with wave.open(wav, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(pcm)
    base = [root, "--workspace", ws, "--num_rays", "256", "-O"]
    quiet = lambda *a: None
    cli.main(base + ["--iters", "24", "--ckpt", "scratch"], log=quiet, decode=dd.npy_decode)
    done = cli.main(base + ["--test", "--pose", os.path.join(root, "clip.json"), "--aud", os.path.join(root, "clip_aud.npy"), "--video",
                            "--audio_wav", wav], log=quiet, decode=dd.npy_decode)
    return done, pcm


def test_command_line_writes_a_playable_file(clip):
    done, pcm = clip
    video = np.load(done["video"])
    assert done["avi"] == done["video"][:-4] + ".avi" and os.path.isfile(done["avi"])
    avi = R.read_avi(open(done["avi"], "rb").read())
    frames = [c[2] for c in avi["movi"] if c[0] == b"00dc"]
    h = avi["avih"]
    assert (h["total_frames"], h["height"], h["width"]) == video.shape[:3] == (dd.N_AUD, dd.H, dd.W) and len(frames) == dd.N_AUD
    assert h["us_per_frame"] == 40000 and len(avi["streams"]) == 2
    assert b"".join(c[2] for c in avi["movi"] if c[0] == b"01wb") == pcm
    # the first frame: within 0.2 dB of the float64 encoder on that frame
    got, want = R.decode(frames[0]), R.decode(R.encode(video[0], 90, "420"))
    assert got.shape == video[0].shape
    print(f"first frame: {len(frames[0])} bytes, PSNR {R.psnr(got, video[0]):.3f} dB, float64 encoder {R.psnr(want, video[0]):.3f} dB")
    assert R.psnr(got, video[0]) >= R.psnr(want, video[0]) - 0.2
    for f in frames[1:]:
        R.parse(f)

