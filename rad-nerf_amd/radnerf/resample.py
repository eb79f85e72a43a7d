"""Any PCM audio -> the 16 kHz mono float32 signal the wav2vec2 path takes: the step the reference leaves to soundfile and resampy
(nerf/asr.py:255-264) and its preprocessing to ffmpeg's -ar 16000 (data_utils/process.py:9-12).

    x = samples_16k("talk_48k_stereo.wav", "cuda")                      # read_audio + Resampler.whole
    rs = Resampler(48000, 16000, "s16le", 2, device="cuda")             # a stream: the same bits as whole(), for any split
    for block in blocks: y = rs.push(block); ...
    y = rs.flush()

The filter is band-limited interpolation with a Kaiser-windowed sinc, after the design of resampy's `kaiser_best` (its parameters
written down from memory -- resampy is not a dependency and nothing here is pinned to its bits):

    prototype   Z = 64 zero crossings, roll-off rho = 0.9475937167399596, Kaiser beta = 14.769656459379492, tabulated at 512 points
                per crossing: win[j] = rho sinc(rho j / 512) I0(beta sqrt(1 - (j / (512 Z))^2)) / I0(beta), j = 0 .. 512 Z
    h(u)        s times the linear interpolation of win at |u| s 512, zero from Z / s on; s = min(1, dst / src)
    rates       g = gcd(src, dst), L = dst / g, M = src / g, W = ceil(Z / s).  Output t sits at input time n + p / L with
                n = (t M) // L and p = (t M) % L, exact integers: no float time accumulates, an endless stream does not drift
    table       tab[p][k + W] = float32(h(k - p / L)), computed in float64: [L, 2 W + 1]
    output      y[t] = sum over k = -W .. W of tab[p][k + W] x[n + k], x zero outside the signal; n_out = (n_in L) // M

On a GPU the decode (rn_pcm_decode) and the filter (rn_resample: one fmaf chain per output over k ascending, csrc/rn_resample.hip)
are kernels; on a CPU tensor the same sum runs in plain torch (one rounded product and one rounded add per tap, k ascending).
Either way an output's bits depend on its index and the signal alone, so push() + flush() equal whole() bit for bit.  When
src == dst nothing is filtered: the samples pass through with their bits.

read_audio is this module's own RIFF parser (the `wave` module does not read float files): format tags 1 (PCM: 8, 16, 24, 32 bits)
and 3 (IEEE float, 32 bits), and WAVE_FORMAT_EXTENSIBLE with those two sub-formats.  Not built: compressed audio, channel mixing
(the first channel is taken, as the reference does).
"""
import math
import struct

import numpy as np
import torch

ZEROS = 64
ROLLOFF = 0.9475937167399596
BETA = 14.769656459379492
PRECISION = 512
TABLE_LIMIT = 16 << 20                  # bytes
FORMATS = {"u8": 1, "s16le": 2, "s24le": 3, "s32le": 4, "f32le": 4}          # bytes per sample
_FORMAT_IDS = {"u8": 0, "s16le": 1, "s24le": 2, "s32le": 3, "f32le": 4}     # RN_PCM_*
_KSDATAFORMAT_TAIL = bytes.fromhex("000000001000800000aa00389b71")
_window_cache = []


def prototype():
    """win[0 .. 512 Z], float64."""
    if not _window_cache:
        j = np.arange(PRECISION * ZEROS + 1, dtype=np.float64)
        r = j / (PRECISION * ZEROS)
        _window_cache.append(ROLLOFF * np.sinc(ROLLOFF * j / PRECISION) * np.i0(BETA * np.sqrt(np.maximum(0.0, 1.0 - r * r))) / np.i0(BETA))
    return _window_cache[0]


def plan(src, dst=16000):
    """(L, M, W) of the rates; ValueError for a rate that is not positive or a table past 16 MiB.  Builds nothing."""
    src, dst = int(src), int(dst)
    if src <= 0 or dst <= 0:
        raise ValueError(f"resample: rates must be positive, got {src} Hz -> {dst} Hz")
    g = math.gcd(src, dst)
    L, M = dst // g, src // g
    W = ZEROS if M <= L else -(-ZEROS * M // L)
    nbytes = 4 * L * (2 * W + 1)
    if nbytes > TABLE_LIMIT:
        raise ValueError(f"resample: {src} Hz -> {dst} Hz needs a table of {L} phases x {2 * W + 1} taps ({nbytes} bytes, past {TABLE_LIMIT}): "
                         f"the rates share too small a divisor ({g})")
    return L, M, W


def n_out(n_in, L, M):
    return (int(n_in) * L) // M


def phase_table(src, dst=16000):
    """-> (tab float32 [L, 2 W + 1], L, M, W)."""
    L, M, W = plan(src, dst)
    win = prototype()
    k = np.arange(-W, W + 1, dtype=np.int64)[None, :]
    p = np.arange(L, dtype=np.int64)[:, None]
    num = np.abs(k * L - p).astype(np.float64)                       # |k - p / L| L, exact
    a = num * PRECISION / L if M <= L else num * PRECISION / M       # |u| s 512 with s = L / M below 1
    inside = a < PRECISION * ZEROS
    a = np.where(inside, a, 0.0)
    i = np.floor(a).astype(np.int64)
    frac = a - i
    i1 = np.minimum(i + 1, PRECISION * ZEROS)
    h = win[i] + frac * (win[i1] - win[i])
    s = 1.0 if M <= L else L / M
    return np.where(inside, s * h, 0.0).astype(np.float32), L, M, W


# ------------------------------------------------------------------------------------------------------------------- RIFF / WAVE
def _riff(path, want_data):
    with open(path, "rb") as fh:
        head = fh.read(12)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"WAVE":
            raise ValueError(f"{path} is not a RIFF/WAVE file")
        fmt = None
        while True:
            ck = fh.read(8)
            if len(ck) < 8:
                raise ValueError(f"{path} has no {'data' if fmt else 'fmt '} chunk")
            name, size = ck[:4], struct.unpack("<I", ck[4:])[0]
            if name == b"fmt ":
                fmt = fh.read(size)
                if len(fmt) < 16 or size < 16:
                    raise ValueError(f"{path}: the fmt chunk is {len(fmt)} bytes, shorter than a WAVEFORMAT")
            elif name == b"data":
                if fmt is None:
                    raise ValueError(f"{path} has its data chunk before its fmt chunk")
                at = fh.tell()
                fh.seek(0, 2)
                have = min(size, max(0, fh.tell() - at))                 # a data chunk longer than the file is clipped
                fh.seek(at)
                return fmt, have, (fh.read(have) if want_data else None)
            else:
                fh.seek(size, 1)
            if size & 1 and name != b"data":
                fh.seek(1, 1)                                            # chunks are padded to even sizes


def _describe(path, fmt):
    tag, channels, rate, _, align, bits = struct.unpack("<HHIIHH", fmt[:16])
    if tag == 0xFFFE:
        if len(fmt) < 40:
            raise ValueError(f"{path}: format tag 0xFFFE (extensible) with a fmt chunk of {len(fmt)} bytes, shorter than 40")
        sub = fmt[24:40]
        tag = struct.unpack("<H", sub[:2])[0]
        if sub[2:] != _KSDATAFORMAT_TAIL:
            raise ValueError(f"{path}: format tag 0xFFFE with a sub-format that is neither PCM nor IEEE float ({sub.hex()})")
    if tag not in (1, 3):
        raise ValueError(f"{path}: format tag {tag} is compressed or unknown audio; only PCM (1) and IEEE float (3) are read")
    if channels == 0:
        raise ValueError(f"{path}: channels = 0")
    if rate == 0:
        raise ValueError(f"{path}: sample rate = 0")
    if tag == 1 and bits in (8, 16, 24, 32):
        name = {8: "u8", 16: "s16le", 24: "s24le", 32: "s32le"}[bits]
    elif tag == 3 and bits == 32:
        name = "f32le"
    else:
        raise ValueError(f"{path}: bits per sample = {bits} with format tag {tag}; PCM of 8, 16, 24 or 32 bits and 32-bit float are read"
                         + (" (64-bit float is not)" if tag == 3 and bits == 64 else ""))
    if align != channels * FORMATS[name]:
        raise ValueError(f"{path}: block align = {align}, {channels} channels of {bits} bits make {channels * FORMATS[name]}")
    return rate, channels, name


def check_audio(path):
    """The header of a file read_audio reads -> (rate, channels, format, frames); ValueError otherwise.  Reads no samples."""
    try:
        fmt, have, _ = _riff(str(path), False)
    except OSError as e:
        raise ValueError(f"{path} cannot be read ({e})") from None
    rate, channels, name = _describe(path, fmt)
    return rate, channels, name, have // (channels * FORMATS[name])


def read_audio(path):
    """A RIFF/WAVE PCM or float file -> (rate, channels, format, raw bytes of whole frames); one [WARN] line for several channels."""
    try:
        fmt, have, raw = _riff(str(path), True)
    except OSError as e:
        raise ValueError(f"{path} cannot be read ({e})") from None
    rate, channels, name = _describe(path, fmt)
    frame = channels * FORMATS[name]
    if channels > 1:
        print(f"[WARN] audio has {channels} channels, only use the first.")
    return rate, channels, name, raw[:len(raw) // frame * frame]


def decode_numpy(raw, format, channels):
    """Raw interleaved frames -> float32 [N], the first channel: what rn_pcm_decode computes, in numpy."""
    width = FORMATS[format]
    b = np.frombuffer(raw, dtype=np.uint8)
    b = b[:len(b) // (width * channels) * (width * channels)].reshape(-1, channels, width)[:, 0, :]
    if format == "u8":
        return (b[:, 0].astype(np.float32) - np.float32(128)) / np.float32(128)
    if format == "s16le":
        return np.ascontiguousarray(b).view("<i2")[:, 0].astype(np.float32) / np.float32(32768)
    if format == "s24le":
        v = b[:, 0].astype(np.int32) | (b[:, 1].astype(np.int32) << 8) | (b[:, 2].astype(np.int8).astype(np.int32) << 16)
        return v.astype(np.float32) / np.float32(1 << 23)
    if format == "s32le":
        return np.ascontiguousarray(b).view("<i4")[:, 0].astype(np.float32) * np.float32(2.0 ** -31)
    return np.ascontiguousarray(b).view("<f4")[:, 0].copy()


def pcm16_track(samples):
    """Float samples at 16 kHz -> (rate, channels, bytes per sample, PCM bytes) as video.AviWriter takes it: rounded and clipped."""
    x = np.asarray(torch.as_tensor(samples).detach().cpu(), dtype=np.float64)
    return 16000, 1, 2, np.clip(np.rint(x * 32768.0), -32768, 32767).astype("<i2").tobytes()


# --------------------------------------------------------------------------------------------------------------------- Resampler
def _is_raw(data):
    return isinstance(data, (bytes, bytearray, memoryview)) or (isinstance(data, np.ndarray) and data.dtype == np.uint8)


class Resampler:
    def __init__(self, src, dst=16000, format="f32le", channels=1, device="cpu"):
        """format, channels: how raw bytes handed to whole() / push() are laid out; float samples (an array or a tensor) are taken
        as the mono signal itself.  Everything lives on `device`; the table is built here, once."""
        if format not in FORMATS:
            raise ValueError(f"Resampler: format = {format!r} is not one of {', '.join(FORMATS)}")
        if int(channels) < 1:
            raise ValueError(f"Resampler: channels = {channels}")
        self.src, self.dst, self.format, self.channels = int(src), int(dst), format, int(channels)
        self.device = torch.device(device)
        self.L, self.M, self.W = plan(self.src, self.dst)
        self.passthrough = self.src == self.dst
        self._hip = self.device.type == "cuda"
        self.taps = None
        if not self.passthrough:
            tab = phase_table(self.src, self.dst)[0]
            self.taps = torch.from_numpy(np.ascontiguousarray(tab.T)).to(self.device)      # tap-major [2 W + 1, L]
        self._hist = torch.zeros(0, dtype=torch.float32, device=self.device)   # the decoded samples the next outputs still read
        self._carry = b""               # bytes short of a frame
        self.n_in = 0                   # samples pushed so far
        self.n_done = 0                 # outputs handed out so far
        self.finished = False

    @property
    def latency(self):
        """Seconds of input an output waits for behind its own time: its right wing and the sample that closes it."""
        return 0.0 if self.passthrough else (self.W + 1) / self.src

    # -------------------------------------------------------------------------------------------------------------------- decode
    def _decode(self, data):
        if not _is_raw(data):
            if isinstance(data, np.ndarray):
                data = np.array(data, dtype=np.float32)             # a copy: the array may be read-only
            return torch.as_tensor(data).detach().to(self.device, torch.float32).reshape(-1)
        raw = bytes(data) if not isinstance(data, np.ndarray) else data.tobytes()
        frame = self.channels * FORMATS[self.format]
        n = len(raw) // frame
        if not self._hip:
            return torch.from_numpy(decode_numpy(raw[:n * frame], self.format, self.channels).copy())
        out = torch.empty(n, dtype=torch.float32, device=self.device)
        if n:
            import radnerf_hip as hip
            host = torch.frombuffer(bytearray(raw[:n * frame]), dtype=torch.uint8)
            dev = host.to(self.device)
            hip.call("rn_pcm_decode", hip.ptr(dev), n, self.channels, _FORMAT_IDS[self.format], hip.ptr(out), hip.stream())
        return out

    # -------------------------------------------------------------------------------------------------------------------- filter
    def _filter(self, buf, origin, t0, count):
        """Outputs t0 .. t0 + count - 1 from buf, whose element 0 is input index origin; zeros outside it."""
        L, M, W = self.L, self.M, self.W
        y = torch.empty(count, dtype=torch.float32, device=self.device)
        if count == 0:
            return y
        if self._hip:
            import radnerf_hip as hip
            buf = buf.contiguous()
            hip.call("rn_resample", hip.ptr(buf) if buf.numel() else None, buf.numel(), origin, hip.ptr(self.taps), L, M, W, t0, count, hip.ptr(y),
                     hip.stream())
            return y
        tm = (t0 + torch.arange(count, dtype=torch.int64)) * M
        n, p = tm // L, tm % L
        at = n - W - origin                                          # buffer index of the first tap, may leave the buffer
        lo, hi = int(at.min()), int(at.max()) + 2 * W
        front, back = max(0, -lo), max(0, hi + 1 - buf.numel())
        padded = torch.cat([buf.new_zeros(front), buf, buf.new_zeros(back)])
        at = at + front
        acc = torch.zeros(count, dtype=torch.float32)
        for j in range(2 * W + 1):
            acc = acc + self.taps[j][p] * padded[at + j]
        return acc

    # -------------------------------------------------------------------------------------------------------------------- public
    def whole(self, data):
        """A complete signal -> its (n_in L) // M outputs.  Keeps no state: a stream in progress is not disturbed."""
        x = self._decode(data)
        if self.passthrough:
            return x
        return self._filter(x, 0, 0, n_out(x.numel(), self.L, self.M))

    def push(self, data):
        """More of the stream -> the outputs that became complete: those whose right wing lies inside what was pushed."""
        if self.finished:
            raise RuntimeError("Resampler.push: the stream was flushed")
        if _is_raw(data):
            raw = self._carry + (bytes(data) if not isinstance(data, np.ndarray) else data.tobytes())
            frame = self.channels * FORMATS[self.format]
            keep = len(raw) // frame * frame
            self._carry, data = raw[keep:], raw[:keep]
        x = self._decode(data)
        if self.passthrough:
            self.n_in += x.numel()
            self.n_done = self.n_in
            return x
        origin = self.n_in - self._hist.numel()
        buf = torch.cat([self._hist, x]) if self._hist.numel() else x
        self.n_in += x.numel()
        q = self.n_in - self.W                                       # inputs whose right wing is in: indices below q
        t_end = min(-(-q * self.L // self.M), n_out(self.n_in, self.L, self.M)) if q > 0 else 0
        t_end = max(t_end, self.n_done)
        y = self._filter(buf, origin, self.n_done, t_end - self.n_done)
        self.n_done = t_end
        first = max(origin, (self.n_done * self.M) // self.L - self.W)     # the first input the next output reads
        self._hist = buf[first - origin:]
        return y

    def flush(self):
        """The stream has ended: the outputs that were still waiting for their right wing, which is zeros now."""
        if self.finished:
            return torch.empty(0, dtype=torch.float32, device=self.device)
        self.finished = True
        self._carry = b""
        if self.passthrough:
            return torch.empty(0, dtype=torch.float32, device=self.device)
        t_end = n_out(self.n_in, self.L, self.M)
        y = self._filter(self._hist, self.n_in - self._hist.numel(), self.n_done, t_end - self.n_done)
        self.n_done = t_end
        self._hist = self._hist[:0]
        return y


def samples_16k(path, device="cpu"):
    """Any file read_audio reads -> float32 [N] at 16 kHz on `device`."""
    rate, channels, format, raw = read_audio(path)
    return Resampler(rate, 16000, format, channels, device=device).whole(raw)
