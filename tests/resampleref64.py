"""Float64 restatement of radnerf/resample.py's filter, built differently: every output's weights come straight from the definition
h((n + k) - t src / dst) with exact integer times and no phase table, and the Kaiser window comes from scipy.signal.windows.kaiser
instead of np.i0.  Shared by test_resample_host.py and test_gpu_resample.py."""
import math
import struct

import numpy as np
from scipy.signal.windows import kaiser

Z = 64
ROLLOFF = 0.9475937167399596
BETA = 14.769656459379492
POINTS = 512
RATES = (8000, 11025, 22050, 32000, 44100, 48000, 96000)
U = 2.0 ** -24
_cache = {}


def window():
    if "win" not in _cache:
        j = np.arange(POINTS * Z + 1, dtype=np.float64)
        _cache["win"] = ROLLOFF * np.sinc(ROLLOFF * j / POINTS) * kaiser(2 * POINTS * Z + 1, BETA)[POINTS * Z:]
    return _cache["win"]


def ratio(src, dst=16000):
    g = math.gcd(src, dst)
    L, M = dst // g, src // g
    s = min(1.0, dst / src)
    return L, M, int(math.ceil(Z * M / L)) if M > L else Z, s


def h_num(num, L, M):
    """h(num / L) for an integer array num: the prototype, stretched by s = min(1, L / M), linearly interpolated."""
    win = window()
    s_num, s_den = (L, M) if M > L else (1, 1)
    a = np.abs(num).astype(np.float64) * (s_num * POINTS) / (s_den * L)
    out = np.zeros(a.shape)
    ok = a < POINTS * Z
    i = np.floor(a[ok]).astype(np.int64)
    f = a[ok] - i
    out[ok] = (win[i] * (1.0 - f) + win[np.minimum(i + 1, POINTS * Z)] * f) * (s_num / s_den)
    return out


def weights(src, dst, t):
    """Outputs t (an int array) -> (n [T], w [T, 2 W + 1]): w[i][k + W] = h((n_i + k) - t_i M / L), the weight of x[n_i + k]."""
    L, M, W, _ = ratio(src, dst)
    t = np.asarray(t, dtype=np.int64)
    n = (t * M) // L
    k = np.arange(-W, W + 1, dtype=np.int64)
    num = (n[:, None] + k[None, :]) * L - (t * M)[:, None]
    return n, h_num(num, L, M)


def resample(x, src, dst=16000, rows=2048):
    """x float [N] -> (y float64 [(N L) // M], bound float64: sum over k of |w x| per output, the scale of the float32 bound)."""
    L, M, W, _ = ratio(src, dst)
    x = np.asarray(x, dtype=np.float64)
    n_out = (len(x) * L) // M
    padded = np.concatenate([np.zeros(W), x, np.zeros(W + M + 1)])
    y, bound = np.zeros(n_out), np.zeros(n_out)
    for a in range(0, n_out, rows):
        t = np.arange(a, min(a + rows, n_out))
        n, w = weights(src, dst, t)
        taps = padded[n[:, None] + np.arange(2 * W + 1)[None, :]]           # x[n - W + j] sits at padded[n + j]
        y[t] = (w * taps).sum(axis=1)
        bound[t] = np.abs(w * taps).sum(axis=1)
    return y, bound


def f32_bound(src, dst, bound):
    """|y_f32 - y| <= (2 W + 3) 2^-24 sum |w x|: a float32 chain of 2 W + 1 terms whose coefficients were rounded to float32."""
    return (2 * ratio(src, dst)[2] + 3) * U * bound


def table(src, dst=16000):
    """[L, 2 W + 1] float64: what phase_table rounds to float32."""
    L, M, W, _ = ratio(src, dst)
    k = np.arange(-W, W + 1, dtype=np.int64)[None, :]
    p = np.arange(L, dtype=np.int64)[:, None]
    return h_num(k * L - p, L, M)


def tone(freq, rate, seconds=0.25, amp=1.0, phase=0.0):
    return amp * np.sin(2 * np.pi * freq * np.arange(int(round(seconds * rate))) / rate + phase)


# ------------------------------------------------------------------------------------------------- files and raw frames
GUID_TAIL = bytes.fromhex("000000001000800000aa00389b71")


def riff(tag, channels, rate, bits, body, extensible=False, before=(), data_size=None, riff_pad=b""):
    align = channels * bits // 8
    fmt = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, channels, rate, rate * align, align, bits)
    if extensible:
        fmt += struct.pack("<HHI", 22, bits, 0) + struct.pack("<H", tag) + GUID_TAIL
    chunks = b"fmt " + struct.pack("<I", len(fmt)) + fmt
    for name, payload in before:
        chunks += name + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")
    chunks += b"data" + struct.pack("<I", len(body) if data_size is None else data_size) + body + riff_pad
    return b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks


def numpy_decode(raw, fmt, channels):
    """Written apart from the module's: through int64 and float64 where the scaling is exact there."""
    if fmt == "u8":
        v = np.frombuffer(raw, np.uint8).astype(np.int64) - 128
        return (v.reshape(-1, channels)[:, 0] / 128.0).astype(np.float32)
    if fmt == "s16le":
        return (np.frombuffer(raw, "<i2").reshape(-1, channels)[:, 0] / 32768.0).astype(np.float32)
    if fmt == "s24le":
        b = np.frombuffer(raw, np.uint8).reshape(-1, channels, 3)[:, 0].astype(np.int64)
        v = b[:, 0] + (b[:, 1] << 8) + (b[:, 2] << 16)
        v = np.where(v >= 1 << 23, v - (1 << 24), v)
        return (v / float(1 << 23)).astype(np.float32)
    if fmt == "s32le":
        return np.frombuffer(raw, "<i4").reshape(-1, channels)[:, 0].astype(np.float32) * np.float32(2.0 ** -31)
    return np.frombuffer(raw, "<f4").reshape(-1, channels)[:, 0].copy()
