"""Playable video out of a render: Motion-JPEG in an AVI container with an optional PCM audio track -- what the reference's
test() gets from imageio.mimwrite(<name>.mp4, fps=25) plus ffmpeg (nerf/utils.py:971), without either.

    quant_tables   the Annex K tables under the IJG quality rule
    JpegEncoder    frames [F,H,W,3] uint8 on the device -> baseline JPEG.  The transform and the entropy coder are kernels
                   (csrc/rn_jpeg.hip; csrc/rn_jpeg_dev.h states every convention); the headers -- SOI, APP0, two DQT, SOF0, four DHT,
                   SOS -- are built here once per encoder.  One read-back per batch: the byte counts and the packed scans share a buffer,
                   and the copy takes half as much again as the last batch's frames needed (what it misses costs a second copy).
    AviWriter      RIFF 'AVI ' 1.0: hdrl (avih, a vids/MJPG stream, with audio an auds/PCM stream), movi (00dc and 01wb chunks
                   interleaved per frame), idx1.  Sizes and counts are patched on close().  Below 2 GiB; OpenDML is not written.
    VideoSink      takes device frames as they are rendered, encodes every `batch` of them on the render stream, copies the compressed
                   bytes to pinned memory on a side stream (FrameSink's event / record_stream discipline, radnerf/output.py) and
                   appends them to the AviWriter when the copy has landed.

numpy and the standard library; torch is plumbing (streams, events, pinned memory) and is imported where a device is used, so that
the writer and check_wav serve a command line that has not touched a GPU.
"""
import struct
import wave
from fractions import Fraction

import numpy as np

_LUM_Q = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
          18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100,
          103, 99)
_CHR_Q = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99) + (99,) * 36
_ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49,
           56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
# BITS then HUFFVAL of the Annex K.3 tables, as a DHT segment carries them: DC luma, DC chroma, AC luma, AC chroma
_DHT = (
    (0x00, "00010501010101010100000000000000" "000102030405060708090a0b"),
    (0x01, "00030101010101010101010000000000" "000102030405060708090a0b"),
    (0x10, "0002010303020403050504040000017d"
           "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748"
           "494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3"
           "c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"),
    (0x11, "00020102040403040705040400010277"
           "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445464748"
           "494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2"
           "c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"),
)
SUBSAMPLINGS = ("420", "444")


def quant_tables(quality):
    """(luma, chroma) quantisation steps, natural order, uint8 [64] each: s = 5000 / q below 50, 200 - 2 q from 50 on,
    (t s + 50) / 100 clamped to 1 .. 255."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"video: quality is 1 .. 100, got {quality}")
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((np.asarray(t, np.int64) * s + 50) // 100, 1, 255).astype(np.uint8) for t in (_LUM_Q, _CHR_Q))


def _segment(marker, payload):
    return struct.pack(">BBH", 0xFF, marker, len(payload) + 2) + payload


def jfif_header(H, W, quality, subsampling):
    """Everything of a baseline JFIF file before its scan: SOI, APP0, DQT x 2, SOF0, DHT x 4, SOS."""
    sub = str(subsampling)
    if sub not in SUBSAMPLINGS:
        raise ValueError(f"video: subsampling is one of {SUBSAMPLINGS}, got {subsampling}")
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError(f"video: a JPEG frame is 1 .. 65535 pixels a side, got {H} x {W}")
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0" + struct.pack(">BBBHHBB", 1, 1, 0, 1, 1, 0, 0))
    for i, t in enumerate(quant_tables(quality)):
        out += _segment(0xDB, bytes([i]) + bytes(int(t[z]) for z in _ZIGZAG))
    out += _segment(0xC0, struct.pack(">BHHB", 8, H, W, 3) + bytes([1, 0x22 if sub == "420" else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, spec in _DHT:
        out += _segment(0xC4, bytes([tc_th]) + bytes.fromhex(spec))
    return out + _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


_EOI = b"\xff\xd9"


class JpegEncoder:
    """Baseline JPEG of uint8 frames [F,H,W,3] that live on the device."""

    def __init__(self, H, W, quality=90, subsampling="420"):
        import radnerf_hip as hip
        self.H, self.W, self.quality, self.subsampling = int(H), int(W), int(quality), str(subsampling)
        self.header = jfif_header(self.H, self.W, self.quality, self.subsampling)
        self._hip, self._sub = hip, int(self.subsampling)
        self.blocks = int(hip._lib.rn_jpeg_blocks(self.H, self.W, self._sub))
        self.capacity = int(hip._lib.rn_jpeg_stream_capacity(self.H, self.W, self._sub))       # worst case of one frame's scan
        if not self.blocks:
            raise ValueError(f"video: {H} x {W} is not a frame the JPEG kernels take")
        self.guess = max(3 * self.H * self.W // 8, 4096)       # bytes per frame the next read-back brings along: follows the last batch

    def _frames(self, frames):
        import torch
        if frames.dim() == 3:
            frames = frames[None]
        if frames.dtype != torch.uint8 or not frames.is_cuda or tuple(frames.shape[1:]) != (self.H, self.W, 3):
            raise ValueError(f"video: frames are uint8 [F,{self.H},{self.W},3] on the device, got {frames.dtype} {tuple(frames.shape)}")
        return frames.contiguous()

    def coefficients(self, frames):
        """int16 [F, blocks, 64] on the device: quantised, zigzag order, blocks in MCU-interleaved scan order."""
        import torch
        hip, frames = self._hip, self._frames(frames)
        out = torch.empty(frames.shape[0], self.blocks, 64, dtype=torch.int16, device=frames.device)
        hip.call("rn_jpeg_coefficients", hip.ptr(frames), frames.shape[0], self.H, self.W, self._sub, self.quality, hip.ptr(out), hip.stream())
        return out

    @staticmethod
    def _head(n_frames):
        return (4 * n_frames + 15) // 16 * 16

    def entropy(self, coefficients):
        """The scans of a batch on the device: one uint8 buffer = F uint32 byte counts, padding to 16 bytes, then the scans one
        behind the other."""
        import torch
        hip, F = self._hip, int(coefficients.shape[0])
        if coefficients.dtype != torch.int16 or tuple(coefficients.shape[1:]) != (self.blocks, 64):
            raise ValueError(f"video: coefficients are int16 [F,{self.blocks},64]")
        dev = coefficients.device
        head = self._head(F)
        buf = torch.empty(head + F * self.capacity, dtype=torch.uint8, device=dev)
        ws = torch.empty(int(hip._lib.rn_jpeg_workspace(F, self.H, self.W, self._sub)), dtype=torch.uint8, device=dev)
        streams = buf[head:]
        hip.call("rn_jpeg_entropy", hip.ptr(coefficients), F, self.H, self.W, self._sub, hip.ptr(ws), hip.ptr(streams), F * self.capacity,
                 hip.ptr(buf), hip.stream())
        return buf

    def encode_device(self, frames):
        return self.entropy(self.coefficients(frames))

    def split(self, host, n_frames, rest=None):
        """(bytes of the packed scans, sizes) from the host copy of a batch's buffer; `rest(first, last)` fetches what the copy
        left out when the guess was short."""
        sizes = np.frombuffer(host, np.uint32, n_frames).astype(np.int64)
        head, total = self._head(n_frames), int(sizes.sum())
        have = len(host) - head
        self.guess = 3 * total // (2 * n_frames) + 4096        # half as much again as this batch's frames, and a header's worth
        if total > have:
            if rest is None:
                raise ValueError("video: the copy holds less than the scans")
            return bytes(host[head:]) + bytes(rest(head + have, head + total)), sizes
        return bytes(host[head:head + total]), sizes

    def encode(self, frames):
        """(bytes of the packed scans, int64 sizes [F]) after one read-back (a second one only when the frames grew by more than
        half since the last batch, or on the first batch of an encoder)."""
        frames = self._frames(frames)
        buf, F = self.encode_device(frames), int(frames.shape[0])
        n = min(self._head(F) + self.guess * F, buf.numel())
        host = buf[:n].cpu().numpy()
        return self.split(memoryview(host), F, lambda a, b: buf[a:b].cpu().numpy().tobytes())

    def wrap(self, data, sizes):
        """Complete JFIF files from packed scans."""
        out, at = [], 0
        for n in sizes:
            out.append(self.header + data[at:at + int(n)] + _EOI)
            at += int(n)
        return out

    def files(self, frames):
        return self.wrap(*self.encode(frames))


# ----------------------------------------------------------------------------------------------------------------------- audio
def read_wav(path):
    """(rate, channels, bytes per sample, PCM bytes) of a PCM .wav; ValueError for anything the `wave` module does not read as PCM."""
    try:
        with wave.open(str(path), "rb") as w:
            if w.getcomptype() != "NONE":
                raise ValueError(f"{path}: compressed audio ({w.getcomptype()})")
            return w.getframerate(), w.getnchannels(), w.getsampwidth(), w.readframes(w.getnframes())
    except (wave.Error, EOFError, OSError) as e:
        raise ValueError(f"{path}: not a readable PCM .wav ({e})") from None


def check_wav(path):
    """The header check of read_wav alone."""
    try:
        with wave.open(str(path), "rb") as w:
            if w.getcomptype() != "NONE" or w.getframerate() <= 0 or w.getnchannels() <= 0:
                raise ValueError(f"{path}: not PCM")
    except (wave.Error, EOFError, OSError) as e:
        raise ValueError(f"{path}: not a readable PCM .wav ({e})") from None


# ------------------------------------------------------------------------------------------------------------------------- AVI
class AviWriter:
    """with AviWriter(path, H, W, fps, audio="a.wav") as avi: avi.add_frame(jpeg_bytes) ...
    audio: a PCM .wav path, or (rate, channels, bytes per sample, PCM bytes).  Frame i is followed by the samples
    round(i rate / fps) .. round((i + 1) rate / fps): the rounding is of the running total, so nothing drifts when rate / fps is not
    whole; what the track holds beyond the last frame is written by close()."""
    LIMIT = (1 << 31) - 1

    def __init__(self, path, H, W, fps, audio=None):
        self.path, self.H, self.W = str(path), int(H), int(W)
        self.rate = Fraction(fps).limit_denominator(100000)
        if self.rate <= 0:
            raise ValueError(f"video: fps must be positive, got {fps}")
        self.audio = read_wav(audio) if isinstance(audio, (str, bytes)) or hasattr(audio, "__fspath__") else audio
        self.frames = self._audio_at = self._largest = self._largest_audio = 0
        self._index = []
        self._f = open(self.path, "wb")
        self._write_headers()

    # -- layout
    def _write_headers(self):
        f, n_streams = self._f, 2 if self.audio else 1
        us = int(round(1e6 / self.rate))
        f.write(b"RIFF\0\0\0\0AVI ")
        strl = self._strl_video() + (self._strl_audio() if self.audio else b"")
        avih = struct.pack("<14I", us, 0, 0, 0x10 | 0x100, 0, 0, n_streams, 0, self.W, self.H, 0, 0, 0, 0)
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", 56) + avih + strl
        at = f.tell()
        f.write(b"LIST" + struct.pack("<I", len(hdrl)) + hdrl)
        base = at + 12                                               # 'avih' fourcc
        self._at_total_frames, self._at_buffer = base + 8 + 16, base + 8 + 28
        v = base + 8 + 56 + 12                                       # 'strh' fourcc of the video strl
        self._at_video_length, self._at_video_buffer = v + 8 + 32, v + 8 + 36
        if self.audio:
            a = v + 8 + 56 + 8 + 40 + 12                             # behind strh, strf (BITMAPINFOHEADER): LIST size 'strl'
            self._at_audio_length, self._at_audio_buffer = a + 8 + 32, a + 8 + 36
        self._at_movi = f.tell()
        f.write(b"LIST\0\0\0\0movi")

    def _strl_video(self):
        strh = struct.pack("<4s4sIHHIIIIIIII4H", b"vids", b"MJPG", 0, 0, 0, 0, self.rate.denominator, self.rate.numerator, 0, 0, 0,
                           0xFFFFFFFF, 0, 0, 0, self.W, self.H)
        strf = struct.pack("<IiiHH4sIiiII", 40, self.W, self.H, 1, 24, b"MJPG", self.W * self.H * 3, 0, 0, 0, 0)
        body = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        return b"LIST" + struct.pack("<I", len(body)) + body

    def _strl_audio(self):
        rate, channels, width, _ = self.audio
        align = channels * width
        strh = struct.pack("<4s4sIHHIIIIIIII4H", b"auds", b"\0\0\0\0", 0, 0, 0, 0, 1, rate, 0, 0, 0, 0xFFFFFFFF, align, 0, 0, 0, 0)
        strf = struct.pack("<HHIIHHH", 1, channels, rate, rate * align, align, 8 * width, 0)
        body = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        return b"LIST" + struct.pack("<I", len(body)) + body

    def _position(self):
        return self._f.tell()

    def _chunk(self, fourcc, data, flags):
        # what the file would measure with this chunk, the index so far, this entry and the idx1 header
        after = self._position() + 8 + len(data) + (len(data) & 1) + 16 * (len(self._index) + 1) + 8
        if after > self.LIMIT:
            raise ValueError(f"{self.path}: frame {self.frames} would take the file past 2 GiB, the limit of AVI 1.0 "
                             "(OpenDML is not written); render the clip in parts")
        self._index.append((fourcc, flags, self._f.tell() - (self._at_movi + 8), len(data)))
        self._f.write(fourcc + struct.pack("<I", len(data)) + data + (b"\0" if len(data) & 1 else b""))

    def _audio_until(self, samples):
        rate, channels, width, pcm = self.audio
        align = channels * width
        data = pcm[self._audio_at * align:samples * align]
        data = data[:len(data) // align * align]
        if data:
            self._chunk(b"01wb", data, 0)
            self._audio_at += len(data) // align
            self._largest_audio = max(self._largest_audio, len(data))

    # -- use
    def add_frame(self, jpeg):
        self._chunk(b"00dc", bytes(jpeg), 0x10)
        self.frames += 1
        self._largest = max(self._largest, len(jpeg))
        if self.audio:
            self._audio_until(int(Fraction(self.frames * self.audio[0]) / self.rate + Fraction(1, 2)))

    def close(self):
        f = self._f
        if f is None:
            return
        if self.audio:
            self._audio_until(len(self.audio[3]))
        end_movi = f.tell()
        f.write(b"idx1" + struct.pack("<I", 16 * len(self._index)))
        for cc, flags, off, size in self._index:
            f.write(struct.pack("<4sIII", cc, flags, off, size))
        end = f.tell()
        for at, value in ((4, end - 8), (self._at_movi + 4, end_movi - self._at_movi - 8), (self._at_total_frames, self.frames),
                          (self._at_buffer, self._largest), (self._at_video_length, self.frames), (self._at_video_buffer, self._largest)):
            f.seek(at)
            f.write(struct.pack("<I", value))
        if self.audio:
            f.seek(self._at_audio_length)
            f.write(struct.pack("<I", self._audio_at))
            f.seek(self._at_audio_buffer)
            f.write(struct.pack("<I", self._largest_audio))
        f.close()
        self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ------------------------------------------------------------------------------------------------------------------------ sink
class VideoSink:
    """push(frame) device frames in display order; every `batch` of them is encoded on the current stream, its byte counts and
    scans copied to a pinned slot on a side stream, and written to the AviWriter once the copy's event has fired (at the latest
    when the slot comes round again).  finish() encodes the tail batch, drains every slot and closes the file."""

    def __init__(self, writer, encoder, batch=8, slots=2, device=None):
        import torch
        self.writer, self.encoder, self.batch, self.slots = writer, encoder, int(batch), int(slots)
        self.device = torch.device(device if device is not None else "cuda")
        self.copy_stream = torch.cuda.Stream(device=self.device)
        self._stage = None
        self._n = 0
        self._pinned = [None] * self.slots
        self._pending = [None] * self.slots                    # (copy-finished event, frames, device buffer, bytes copied)
        self._head = 0
        self.files = 0

    def push(self, frame_u8):
        import torch
        if self._stage is None:
            self._stage = torch.empty(self.batch, self.encoder.H, self.encoder.W, 3, dtype=torch.uint8, device=frame_u8.device)
        self._stage[self._n].copy_(frame_u8.reshape(self.encoder.H, self.encoder.W, 3))
        self._n += 1
        if self._n == self.batch:
            self._encode()

    def _encode(self):
        import torch
        enc, n = self.encoder, self._n
        slot = self._head % self.slots
        self._drain(slot)
        buf = enc.encode_device(self._stage[:n])               # reads the staging frames on the render stream, in order with push()
        nbytes = min(enc._head(n) + enc.guess * n, buf.numel())
        if self._pinned[slot] is None or self._pinned[slot].numel() < nbytes:      # page-locking is slow: in steps of 256 KiB, rarely
            self._pinned[slot] = torch.empty(-(-nbytes // (1 << 18)) << 18, dtype=torch.uint8).pin_memory()
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(self.device))   # the scans are complete at this point of the render stream
        with torch.cuda.stream(self.copy_stream):
            self.copy_stream.wait_event(ready)
            self._pinned[slot][:nbytes].copy_(buf[:nbytes], non_blocking=True)
            done = torch.cuda.Event()
            done.record(self.copy_stream)
        buf.record_stream(self.copy_stream)                    # the allocator must not recycle it before the copy ran
        self._pending[slot] = (done, n, buf, nbytes)
        self._head += 1
        self._n = 0

    def _drain(self, slot):
        if self._pending[slot] is None:
            return
        done, n, buf, nbytes = self._pending[slot]
        done.synchronize()
        host = memoryview(self._pinned[slot].numpy())[:nbytes]
        data, sizes = self.encoder.split(host, n, lambda a, b: buf[a:b].cpu().numpy().tobytes())
        for jpeg in self.encoder.wrap(data, sizes):
            self.writer.add_frame(jpeg)
            self.files += 1
        self._pending[slot] = None

    def finish(self):
        if self._n:
            self._encode()
        for k in range(self.slots):                            # oldest first
            self._drain((self._head + k) % self.slots)
        self.writer.close()
        return self.writer.path
