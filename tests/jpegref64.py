"""float64 numpy restatement of the Motion-JPEG write-out (rad-nerf_amd/csrc/rn_jpeg_dev.h states the conventions), written from
ITU-T T.81 and the JFIF note and sharing no code with the package: encoder, an independent decoder, a minimal RIFF reader written
from the AVI layout, and the test frame generator.  tests/test_video.py pins this file against libjpeg (PIL); everything else is
pinned against this file.

Conventions: JFIF full-range YCbCr; edge replication up to whole MCUs; 4:2:0 chroma = the plain mean of each 2 x 2; level shift,
orthonormal 8 x 8 DCT-II; Annex K tables under the IJG quality rule; quotient rounded half away from zero; zigzag order; the four
Annex K Huffman tables; blocks in MCU-interleaved scan order."""
import struct

import numpy as np

LUM_Q = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
                  80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
                  95, 98, 112, 100, 103, 99])
CHR_Q = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99] + [99] * 36)


def _zigzag():
    order = sorted(range(64), key=lambda i: (i // 8 + i % 8, (i // 8 if (i // 8 + i % 8) % 2 else i % 8)))
    return np.array(order)


ZZ = _zigzag()                                   # natural index of zigzag position z (built from the diagonals, not from a list)

DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
DC_VALS = (list(range(12)), list(range(12)))
AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77])
AC_VALS = (bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748"
    "494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3"
    "c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"), bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445464748"
    "494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2"
    "c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"))


def huff_codes(bits, vals):
    """{symbol: (code, length)} from BITS / HUFFVAL (T.81 Annex C)."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


DC_CODES = [huff_codes(DC_BITS[t], DC_VALS[t]) for t in range(2)]
AC_CODES = [huff_codes(AC_BITS[t], AC_VALS[t]) for t in range(2)]

_k = np.arange(8)
DCT = np.where(_k[:, None] == 0, np.sqrt(1 / 8), 0.5 * np.cos((2 * _k[None, :] + 1) * _k[:, None] * np.pi / 16))      # [u, x]


# ------------------------------------------------------------------------------------------------------------ frames
def scene(H, W, seed, turned=False):
    """uint8 [H, W, 3]: an RGB gradient, a flat disc, uniform noise (top left), random pure black / white (bottom left) and an
    8-pixel checkerboard (bottom right; on the block grid, every other 16 rows shifted by half a cell): together they reach every
    branch of the coder.  turned: by 180 degrees, so that the scan ends in the noise and not in the checkerboard, whose chroma
    blocks code to zero bits alone."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    img = np.stack([255 * x / max(W - 1, 1), 255 * y / max(H - 1, 1), 255 * (x + y) / max(H + W - 2, 1)], -1)
    disc = (y - 0.3 * H) ** 2 + (x - 0.6 * W) ** 2 <= (min(H, W) / 5) ** 2
    img[disc] = (200, 40, 90)
    tl = (y < H // 2) & (x < W // 3)
    img[tl] = rng.integers(0, 256, (int(tl.sum()), 3))
    bl = (y >= H // 2) & (x < W // 3)
    img[bl] = 255 * rng.integers(0, 2, (int(bl.sum()), 1))
    br = (y >= H // 2) & (x >= 2 * W // 3)
    check = (((x + 4 * ((y // 16) % 2)) // 8 + y // 8) % 2) * 255
    img[br] = check[br][:, None]
    img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(img[::-1, ::-1]) if turned else img


def dc_differences(coefs, sub):
    """int64 [blocks]: the DC difference every block codes (against the previous block of its component, 0 before the first)."""
    coefs = np.asarray(coefs).reshape(-1, 64)
    comps = np.tile(block_layout(1, 1, sub)[3], len(coefs) // block_layout(1, 1, sub)[2])
    out = np.zeros(len(coefs), np.int64)
    for c in range(3):
        out[comps == c] = np.diff(coefs[comps == c, 0].astype(np.int64), prepend=0)
    return out


def block_checker(H, W, cell):
    """uint8 [H, W, 3]: pure black and pure white cells of `cell` pixels from the origin (cell = 8 at 4:4:4, 16 at 4:2:0: on the
    block grid).  Every block is flat: DC -1024 or 1016 at quality 100, a difference of 2040 (category 11) between neighbours, every
    AC quotient zero up to rounding noise: nothing is near a tie."""
    y, x = np.mgrid[0:H, 0:W]
    v = (((y // cell + x // cell) % 2) * 255).astype(np.uint8)
    return np.repeat(v[..., None], 3, -1)


def dense_coefficients(blocks, seed):
    """int16 [blocks, 64] (zigzag) for the entropy coder alone: every AC of {+-1023, +-511, 255}, DC -1024 and 1023 in turns of three
    blocks (at 4:4:4 every component's predictor difference is then +-2047).  The positive values' extra bits are all ones, so
    about a fifth of the scan's bytes are 0xFF."""
    rng = np.random.default_rng(seed)
    out = rng.choice(np.array([-1023, -511, 255, 511, 1023], np.int16), (blocks, 64))
    out[:, 0] = np.where((np.arange(blocks) // 3) % 2 == 0, -1024, 1023)
    return out


def unstuffed(scan):
    """uint8 array of a scan's bytes before stuffing."""
    return np.frombuffer(scan.replace(b"\xff\x00", b"\xff"), np.uint8)


def ff_seams(scan, chunk=4096, vector=16):
    """Where the 0xFF bytes of a scan lie in its unstuffed stream: dict of counts -- 0xFF bytes in all (`ff`), at the last byte of a
    chunk / of a vector (`chunk_end`, `vector_end`), and pairs of 0xFF on both sides of such a seam (`chunk_pair`, `vector_pair`)."""
    ff = unstuffed(scan) == 0xFF
    at = np.flatnonzero(ff[:-1])
    pair = at[ff[at + 1]]
    return dict(ff=int(ff.sum()), chunk_end=int((at % chunk == chunk - 1).sum()), vector_end=int((at % vector == vector - 1).sum()),
                chunk_pair=int((pair % chunk == chunk - 1).sum()), vector_pair=int((pair % vector == vector - 1).sum()))


# Inputs of the tests that a CPU test (tests/test_video.py) holds to their conditions and the GPU tests (tests/test_gpu_video.py) run.
# (shape, subsampling, blocks): on both sides of the 1024 entries one round of the device's scan takes (1024 is no multiple of 3 or 6),
# and past two rounds.  They run on turned scenes: a round that ends in blocks of zero bits would not show a lost carry
ROUND_SHAPES = [((88, 248), "444", 1023), ((144, 152), "444", 1026), ((160, 272), "420", 1020), ((144, 304), "420", 1026),
                ((144, 304), "444", 2052)]
LOW_SHAPES = [((17, 19), "420"), ((17, 19), "444"), ((40, 24), "420"), ((40, 24), "444"), ((144, 304), "420")]
LOW_QUALITIES = [1, 10, 49]                                     # the 5000 / q branch of the IJG rule; every step is 255 at 1
CHECKERS = [((48, 64), "444", 8), ((48, 64), "420", 16), ((88, 248), "444", 8), ((160, 272), "420", 16)]      # (shape, subsampling, cell)
# Sides of 1, below one block, of exactly one MCU: {shape: the seeds of `scene` in use}; the reference alone flags at most 1.6 % of
# the coefficients of each at both subsamplings and qualities 50 and 100, so the tie rule's 2 % cap judges the device and not the seed.
TINY_SEEDS = {(1, 1): (1, 2, 3), (1, 40): (1, 2, 3), (40, 1): (1, 2, 3), (7, 33): (1, 2, 3), (8, 8): (2, 4, 6), (16, 16): (2, 4, 7),
              (3, 200): (1, 2, 3)}
# dense_coefficients seeds of the two long frames at 144 x 152, 4:4:4 (1026 blocks): each scan has a 0xFF at the end of a 4096-byte chunk
# and of a 16-byte vector, and a pair of 0xFF across both kinds of seam
DENSE_HW, DENSE_SEEDS = (144, 152), (1, 5)
# dense_coefficients seed of an 8 x 8 frame at 4:4:4 (3 blocks) whose last byte holds one bit of data and seven of padding, and is 0xFF
PADDED_FF_SEED = 8


def dense_batch():
    """int16 [3, 1026, 64]: the two long frames and a short one (zeros but for every 100th block) behind them."""
    blocks = block_layout(*DENSE_HW, "444")
    blocks = blocks[0] * blocks[1] * blocks[2]
    short = np.zeros((blocks, 64), np.int16)
    short[::100] = dense_coefficients(blocks, 3)[::100]
    return np.stack([dense_coefficients(blocks, DENSE_SEEDS[0]), dense_coefficients(blocks, DENSE_SEEDS[1]), short])


# ----------------------------------------------------------------------------------------------------------- encoder
def quant_tables(quality):
    """(luma, chroma) steps in natural order: the IJG rule."""
    q = min(max(int(quality), 1), 100)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((t * s + 50) // 100, 1, 255) for t in (LUM_Q, CHR_Q))


def mcu_side(sub):
    return {"420": 16, "444": 8}[str(sub)]


def block_layout(H, W, sub):
    """(mcus_h, mcus_w, blocks per MCU, component of each block of an MCU)."""
    m = mcu_side(sub)
    comps = [0, 0, 0, 0, 1, 2] if str(sub) == "420" else [0, 1, 2]
    return -(-H // m), -(-W // m), len(comps), comps


def planes(frame, sub):
    """Y, Cb, Cr float64 planes of the frame padded to whole MCUs (chroma at half size for 4:2:0)."""
    H, W, _ = frame.shape
    mh, mw, _, _ = block_layout(H, W, sub)
    m = mcu_side(sub)
    rgb = np.pad(frame.astype(np.float64), ((0, mh * m - H), (0, mw * m - W), (0, 0)), mode="edge")
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    out = [0.299 * r + 0.587 * g + 0.114 * b, -0.168735892 * r - 0.331264108 * g + 0.5 * b + 128, 0.5 * r - 0.418687589 * g - 0.081312411 * b + 128]
    if str(sub) == "420":
        out[1:] = [(p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]) / 4 for p in out[1:]]
    return out


def block_samples(frame, sub):
    """[blocks, 8, 8] float64 in scan order, and the component of every block."""
    H, W, _ = frame.shape
    mh, mw, per, comps = block_layout(H, W, sub)
    yy, cb, cr = planes(frame, sub)
    out = np.empty((mh * mw * per, 8, 8))
    i = 0
    for my in range(mh):
        for mx in range(mw):
            if per == 6:
                for k in range(4):
                    oy, ox = my * 16 + (k >> 1) * 8, mx * 16 + (k & 1) * 8
                    out[i + k] = yy[oy:oy + 8, ox:ox + 8]
                out[i + 4] = cb[my * 8:my * 8 + 8, mx * 8:mx * 8 + 8]
                out[i + 5] = cr[my * 8:my * 8 + 8, mx * 8:mx * 8 + 8]
            else:
                for k, p in enumerate((yy, cb, cr)):
                    out[i + k] = p[my * 8:my * 8 + 8, mx * 8:mx * 8 + 8]
            i += per
    return out, np.tile(comps, mh * mw)


def quotients(frame, quality, sub):
    """[blocks, 64] float64 in zigzag order BEFORE rounding, and the component of every block."""
    s, comp = block_samples(frame, sub)
    c = DCT @ (s - 128.0) @ DCT.T
    q = np.stack(quant_tables(quality))[np.minimum(comp, 1)].reshape(-1, 8, 8)
    return (c / q).reshape(-1, 64)[:, ZZ], comp


def round_half_away(v):
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)


def coefficients(frame, quality, sub):
    return round_half_away(quotients(frame, quality, sub)[0])


def flagged(quot, margin=4e-3):
    """Coefficients whose rounding fp32 may decide the other way: |v| within `margin` of a half-integer."""
    a = np.abs(quot)
    return np.abs(a - np.floor(a) - 0.5) <= margin


def compare_coefficients(got, frame, quality, sub, margin=4e-3, cap=0.02):
    """The tie rule: `got` equals the float64 coefficients except where the quotient is flagged; flagged ones are within 1 and
    at most `cap` of all.  -> the flags [blocks, 64]."""
    quot, _ = quotients(frame, quality, sub)
    want, flags = round_half_away(quot), flagged(quot, margin)
    got = np.asarray(got).reshape(want.shape).astype(np.int64)
    bad = (got != want) & ~flags
    assert not bad.any(), f"{int(bad.sum())} coefficients differ away from a tie, first at {np.argwhere(bad)[0]}: " \
                          f"{got[bad][0]} vs {want[bad][0]} (quotient {quot[bad][0]!r})"
    assert np.abs(got - want).max() <= 1
    assert flags.mean() <= cap, f"{flags.mean():.4f} of the coefficients are flagged"
    return flags


class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n, self.stuffed = bytearray(), 0, 0, 0

    def put(self, value, length):
        self.acc = (self.acc << length) | value
        self.n += length
        while self.n >= 8:
            self.n -= 8
            byte = (self.acc >> self.n) & 0xFF
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
                self.stuffed += 1
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def entropy(coefs, sub, stats=None):
    """The scan of one frame: coefs int [blocks, 64] (zigzag) -> bytes.  stats: a dict that collects symbol counts (and the
    last scan's `pad_bits`)."""
    per = 6 if str(sub) == "420" else 3
    comps = [0, 0, 0, 0, 1, 2] if per == 6 else [0, 1, 2]
    st = dict(zrl=0, eob=0, c63=0, dc11=0, ac10=0, stuffed=0, blocks=0) if stats is None else stats
    w, pred = BitWriter(), [0, 0, 0]
    for b, block in enumerate(np.asarray(coefs).reshape(-1, 64).tolist()):
        comp = comps[b % per]
        t = 1 if comp else 0
        diff = block[0] - pred[comp]
        pred[comp] = block[0]
        cat = abs(diff).bit_length()
        assert cat <= 11
        st["dc11"] += cat == 11
        w.put(*DC_CODES[t][cat])
        if cat:
            w.put((diff if diff >= 0 else diff - 1) & ((1 << cat) - 1), cat)
        run = 0
        for z in range(1, 64):
            v = block[z]
            if v == 0:
                run += 1
                continue
            while run > 15:
                w.put(*AC_CODES[t][0xF0])
                st["zrl"] += 1
                run -= 16
            cat = abs(v).bit_length()
            assert cat <= 10
            st["ac10"] += cat == 10
            w.put(*AC_CODES[t][(run << 4) | cat])
            w.put((v if v >= 0 else v - 1) & ((1 << cat) - 1), cat)
            run = 0
        if run:
            w.put(*AC_CODES[t][0])
            st["eob"] += 1
        else:
            st["c63"] += 1
        st["blocks"] += 1
    st["pad_bits"] = -w.n % 8                                     # of this scan: how many 1-bits fill its last byte
    w.flush()
    st["stuffed"] += w.stuffed
    return bytes(w.out)


def _segment(marker, payload):
    return struct.pack(">BBH", 0xFF, marker, len(payload) + 2) + payload


def headers(H, W, quality, sub):
    """SOI, APP0 (JFIF 1.01), two DQT, SOF0, four DHT, SOS."""
    lum, chr_ = quant_tables(quality)
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0" + struct.pack(">BBBHHBB", 1, 1, 0, 1, 1, 0, 0))
    for i, t in enumerate((lum, chr_)):
        out += _segment(0xDB, bytes([i]) + bytes(int(v) for v in t[ZZ]))
    hv = 0x22 if str(sub) == "420" else 0x11
    out += _segment(0xC0, struct.pack(">BHHB", 8, H, W, 3) + bytes([1, hv, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for cls, tables in ((0, (DC_BITS, DC_VALS)), (1, (AC_BITS, AC_VALS))):
        for t in range(2):
            out += _segment(0xC4, bytes([cls << 4 | t]) + bytes(tables[0][t]) + bytes(tables[1][t]))
    return out + _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def encode(frame, quality, sub, stats=None):
    """A complete JFIF file of the frame."""
    H, W, _ = frame.shape
    return headers(H, W, quality, sub) + entropy(coefficients(frame, quality, sub), sub, stats) + b"\xff\xd9"


# ----------------------------------------------------------------------------------------------------------- decoder
def _lookup(bits, vals):
    """16-bit prefix -> (length, symbol) arrays."""
    length, symbol = np.zeros(1 << 16, np.uint8), np.zeros(1 << 16, np.uint8)
    for sym, (code, n) in huff_codes(bits, vals).items():
        lo = code << (16 - n)
        length[lo:lo + (1 << (16 - n))] = n
        symbol[lo:lo + (1 << (16 - n))] = sym
    return length, symbol


def parse(data):
    """Segments of a baseline JFIF file: dict(H, W, sampling, qt {id: natural-order steps}, dc / ac {id: lookup}, comps, scan bytes)."""
    assert data[:2] == b"\xff\xd8", "no SOI"
    info, at = dict(qt={}, dc={}, ac={}), 2
    while True:
        assert data[at] == 0xFF, f"no marker at {at}"
        marker, n = data[at + 1], struct.unpack(">H", data[at + 2:at + 4])[0]
        body = data[at + 4:at + 2 + n]
        at += 2 + n
        if marker == 0xDB:
            while body:
                assert body[0] >> 4 == 0, "8-bit tables only"
                t = np.zeros(64, np.int64)
                t[ZZ] = list(body[1:65])
                info["qt"][body[0] & 15] = t
                body = body[65:]
        elif marker == 0xC0:
            p, info["H"], info["W"], nc = struct.unpack(">BHHB", body[:6])
            assert p == 8 and nc == 3
            info["comps"] = [dict(id=body[6 + 3 * i], h=body[7 + 3 * i] >> 4, v=body[7 + 3 * i] & 15, tq=body[8 + 3 * i]) for i in range(3)]
        elif marker == 0xC4:
            while body:
                cnt = sum(body[1:17])
                info["ac" if body[0] >> 4 else "dc"][body[0] & 15] = _lookup(list(body[1:17]), list(body[17:17 + cnt]))
                body = body[17 + cnt:]
        elif marker == 0xDA:
            assert body[0] == 3
            for i in range(3):
                assert body[1 + 2 * i] == info["comps"][i]["id"]
                info["comps"][i].update(td=body[2 + 2 * i] >> 4, ta=body[2 + 2 * i] & 15)
            assert tuple(body[7:10]) == (0, 63, 0)
            break
        else:
            assert 0xE0 <= marker <= 0xFE, f"marker {marker:#x} is not baseline"
    end = data.rindex(b"\xff\xd9")
    assert end == len(data) - 2, "EOI is not the end of the file"
    info["scan"] = data[at:end]
    return info


def decode_coefficients(data):
    """(info, coefs int64 [blocks, 64] in zigzag order, component of every block) of a file."""
    info = parse(data)
    scan = info["scan"]
    i = scan.find(b"\xff")
    while i >= 0:
        assert scan[i + 1] == 0, f"marker {scan[i + 1]:#x} inside the scan"
        i = scan.find(b"\xff", i + 2)
    raw = scan.replace(b"\xff\x00", b"\xff")
    bits = np.unpackbits(np.frombuffer(raw + b"\xff\xff\xff", np.uint8)).astype(np.int64)
    n = len(bits) - 16
    peek = np.zeros(n, np.int64)
    for k in range(16):
        peek += bits[k:k + n] << (15 - k)
    peek = peek.tolist()
    c0 = info["comps"][0]
    assert (c0["h"], c0["v"]) in ((2, 2), (1, 1)) and all((c["h"], c["v"]) == (1, 1) for c in info["comps"][1:])
    sub = "420" if c0["h"] == 2 else "444"
    mh, mw, per, comps = block_layout(info["H"], info["W"], sub)
    tables = [(info["dc"][c["td"]], info["ac"][c["ta"]]) for c in info["comps"]]
    tables = [((d[0].tolist(), d[1].tolist()), (a[0].tolist(), a[1].tolist())) for d, a in tables]
    out = np.zeros((mh * mw * per, 64), np.int64)
    pred, p = [0, 0, 0], 0

    def receive(cat):
        nonlocal p
        if not cat:
            return 0
        v = peek[p] >> (16 - cat)
        p += cat
        return v if v >> (cat - 1) else v - (1 << cat) + 1

    for b in range(len(out)):
        comp = comps[b % per]
        (dl, ds), (al, as_) = tables[comp]
        assert dl[peek[p]], "no such DC code"
        cat = ds[peek[p]]
        p += dl[peek[p]]
        pred[comp] += receive(cat)
        out[b, 0] = pred[comp]
        z = 1
        while z < 64:
            assert al[peek[p]], "no such AC code"
            rs = as_[peek[p]]
            p += al[peek[p]]
            if rs == 0:
                break
            if rs == 0xF0:
                z += 16
                continue
            z += rs >> 4
            assert z < 64, "run past the block"
            out[b, z] = receive(rs & 15)
            z += 1
    assert p <= 8 * len(raw) and 8 * len(raw) - p < 8, f"{8 * len(raw) - p} bits left over"
    assert bits[p:8 * len(raw)].all(), "padding is not 1-bits"
    return info, out, np.tile(comps, mh * mw), sub


def decode_planes(data):
    """(Y, Cb, Cr) float64 at full (padded) resolution -- chroma replicated 2 x for 4:2:0 -- and (H, W)."""
    info, coefs, comp, sub = decode_coefficients(data)
    nat = np.zeros_like(coefs)
    nat[:, ZZ] = coefs
    q = np.stack([info["qt"][info["comps"][c]["tq"]] for c in range(3)])[comp]
    s = DCT.T @ (nat * q).reshape(-1, 8, 8).astype(np.float64) @ DCT + 128.0
    mh, mw, per, _ = block_layout(info["H"], info["W"], sub)
    m = mcu_side(sub)
    yy = np.zeros((mh * m, mw * m))
    cb, cr = (np.zeros((mh * 8, mw * 8)) for _ in range(2))
    i = 0
    for my in range(mh):
        for mx in range(mw):
            if per == 6:
                for k in range(4):
                    oy, ox = my * 16 + (k >> 1) * 8, mx * 16 + (k & 1) * 8
                    yy[oy:oy + 8, ox:ox + 8] = s[i + k]
                cb[my * 8:my * 8 + 8, mx * 8:mx * 8 + 8], cr[my * 8:my * 8 + 8, mx * 8:mx * 8 + 8] = s[i + 4], s[i + 5]
            else:
                yy[my * 8:my * 8 + 8, mx * 8:mx * 8 + 8], cb[my * 8:my * 8 + 8, mx * 8:mx * 8 + 8] = s[i], s[i + 1]
                cr[my * 8:my * 8 + 8, mx * 8:mx * 8 + 8] = s[i + 2]
            i += per
    if per == 6:
        cb, cr = (np.repeat(np.repeat(p, 2, 0), 2, 1) for p in (cb, cr))
    return (yy, cb, cr), (info["H"], info["W"])


def decode(data):
    """uint8 [H, W, 3] RGB of a baseline JFIF file."""
    (yy, cb, cr), (H, W) = decode_planes(data)
    yy = np.clip(np.rint(yy), 0, 255)
    cb, cr = (np.clip(np.rint(p), 0, 255) - 128.0 for p in (cb, cr))
    rgb = np.stack([yy + 1.402 * cr, yy - 0.344136286 * cb - 0.714136286 * cr, yy + 1.772 * cb], -1)
    return np.clip(np.rint(rgb), 0, 255).astype(np.uint8)[:H, :W]


def decode_luma(data):
    (yy, _, _), (H, W) = decode_planes(data)
    return np.clip(np.rint(yy), 0, 255).astype(np.uint8)[:H, :W]


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return float("inf") if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


# -------------------------------------------------------------------------------------------------------------- RIFF
def _chunks(data, at, end):
    """[(fourcc, payload offset, size, list type or None)] of the chunks in data[at:end]; every chunk starts on an even offset."""
    out = []
    while at < end:
        assert at % 2 == 0 and at + 8 <= end, f"chunk header at {at} does not fit"
        cc, size = data[at:at + 4], struct.unpack("<I", data[at + 4:at + 8])[0]
        assert at + 8 + size <= end, f"chunk {cc} at {at}: {size} bytes pass the end of its parent"
        out.append((cc, at + 8, size, data[at + 8:at + 12] if cc in (b"RIFF", b"LIST") else None))
        at += 8 + size + (size & 1)
    assert at == end or at == end + 1, "chunks do not fill their parent"
    return out


def read_avi(data):
    """A RIFF 'AVI ' file as a dict: avih, streams [(strh, strf)], movi [(fourcc, offset of the chunk header from 'movi', payload)],
    idx1 [(fourcc, flags, offset, size)].  Checks the nesting and every size on the way."""
    (cc, at, size, kind), = _chunks(data, 0, len(data))
    assert cc == b"RIFF" and kind == b"AVI " and size == len(data) - 8
    out = dict(streams=[], movi=[], idx1=[])
    for cc, at, size, kind in _chunks(data, 12, len(data)):
        if cc == b"LIST" and kind == b"hdrl":
            for c2, a2, s2, k2 in _chunks(data, at + 4, at + size):
                if c2 == b"avih":
                    assert s2 == 56
                    names = ("us_per_frame", "max_bytes_per_sec", "padding", "flags", "total_frames", "initial_frames", "streams",
                             "suggested_buffer", "width", "height")
                    out["avih"] = dict(zip(names, struct.unpack("<10I", data[a2:a2 + 40])))
                elif c2 == b"LIST" and k2 == b"strl":
                    strh = strf = None
                    for c3, a3, s3, _ in _chunks(data, a2 + 4, a2 + s2):
                        if c3 == b"strh":
                            assert s3 == 56
                            v = struct.unpack("<4s4sIHHIIIIIIII4H", data[a3:a3 + 56])
                            strh = dict(type=v[0], handler=v[1], scale=v[6], rate=v[7], start=v[8], length=v[9], suggested_buffer=v[10],
                                        quality=v[11], sample_size=v[12])
                        elif c3 == b"strf":
                            strf = data[a3:a3 + s3]
                    out["streams"].append((strh, strf))
        elif cc == b"LIST" and kind == b"movi":
            out["movi_at"] = at                                  # offset of the 'movi' fourcc
            for c2, a2, s2, _ in _chunks(data, at + 4, at + size):
                out["movi"].append((c2, a2 - 8 - at, data[a2:a2 + s2]))
        elif cc == b"idx1":
            assert size % 16 == 0
            out["idx1"] = [struct.unpack("<4sIII", data[at + 16 * i:at + 16 * i + 16]) for i in range(size // 16)]
    return out
