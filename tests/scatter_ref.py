"""What the table-gradient scatters are held to, in numpy: the oracle's addends restated, their exact (float64) sums per table
element, the bound of one fp32 sum against the exact one, the plan of which level takes which path of rn_grid_scatter.hip, and
the input patterns that reach those paths.  Shared by test_gpu_scatter_ordered.py, test_gpu_scatter_atomic.py (GPU) and
test_scatter_ref.py (CPU: the reference against the oracle, and the preconditions of the patterns for the committed seeds).

Nothing here loads the HIP library at import: `Grid` stands in for a GridEncoder on the CPU (same attributes, numpy offsets).
"""
import ctypes as C

import numpy as np

U = 2.0 ** -24                     # unit roundoff of fp32
BASE, DESIRED = 16, 2048
# constants of rn_grid_scatter.hip, restated
SC_THREADS, SC_SLOTS, SC_PROBES = 256, 512, 24
FLUSH_ABOVE = SC_SLOTS // 2 - SC_SLOTS // 8          # a table with more occupied slots than this is flushed after the chunk
DIRECT_ROWS, CHUNK_ROWS, CHUNKS = 1 << 17, 1 << 16, 8
BUCKET_SHIFT, MIN_BUCKETS, MAX_BUCKETS, BIN_THREADS = 12, 16, 128, 256
MERGE_HEADS = 40                                     # sum_runs scans a wave with at most this many run heads

GRIDS = {
    "hash17": dict(input_dim=3, log2_hashmap_size=17, gridtype="hash"),
    "tiled2": dict(input_dim=2, log2_hashmap_size=16, gridtype="tiled"),
    "tiled3": dict(input_dim=3, log2_hashmap_size=16, gridtype="tiled"),
}


def level_offsets(input_dim, num_levels, per_level_scale, base_resolution, log2_hashmap_size):
    """gridencoder.encoder.level_offsets (align_corners = False), restated so that the CPU tests need no built library."""
    offsets, offset = [], 0
    for i in range(num_levels):
        resolution = int(np.ceil(base_resolution * per_level_scale ** i))
        rows = min(2 ** log2_hashmap_size, (resolution + 1) ** input_dim)
        offsets.append(offset)
        offset += int(np.ceil(rows / 8) * 8)
    return np.array(offsets + [offset], dtype=np.int32)


class Grid:
    """The attributes of a GridEncoder that this module reads, on the CPU."""

    def __init__(self, input_dim, log2_hashmap_size, gridtype, num_levels=16):
        self.input_dim, self.num_levels, self.gridtype = input_dim, num_levels, gridtype
        self.gridtype_id = {"hash": 0, "tiled": 1}[gridtype]
        self.per_level_scale = np.exp2(np.log2(DESIRED / BASE) / (num_levels - 1))
        self.offsets = level_offsets(input_dim, num_levels, self.per_level_scale, BASE, log2_hashmap_size)


def grid(name, num_levels=16):
    return Grid(num_levels=num_levels, **GRIDS[name])


def _offsets(enc):
    off = enc.offsets
    return (off.cpu().numpy() if hasattr(off, "cpu") else np.asarray(off)).astype(np.int64)


def _levels(enc):
    return int(_offsets(enc).shape[0]) - 1


def _gradients(L, cap, live, r):
    k = r.integers(-20, 4, size=(L, cap, 1))
    g = (r.standard_normal((L, cap, 2)) * np.exp2(k)).astype(np.float32)
    g[:, live:] = np.nan
    return g


def _inputs(D, cap, live, seed=7):
    """(inputs [cap, D], grad [16, cap, 2]) as numpy fp32: 300 samples in one cell, the others uniform, two outside [0, 1],
    gradients over 24 binades; rows past the live count are NaN."""
    r = np.random.default_rng(seed)
    x = r.random((cap, D), dtype=np.float32)
    n_cell = min(300, live)
    x[:n_cell] = (r.random((1, D), dtype=np.float32) * 0.9 + 0.01 * r.random((n_cell, D), dtype=np.float32)).astype(np.float32)
    if live > 402:
        x[400, 0] = 1.5
        x[401, D - 1] = -0.1
    k = r.integers(-20, 4, size=(16, cap, 1))
    g = (r.standard_normal((16, cap, 2)) * np.exp2(k)).astype(np.float32)
    x[live:] = np.nan
    g[:, live:] = np.nan
    return x, g


def _oracle(po, enc, x, g, live):
    """The oracle's table gradient of the first `live` samples, [rows, 2] fp32."""
    off = _offsets(enc).astype(np.int32)
    D, L = enc.input_dim, _levels(enc)
    emb = np.zeros((int(off[-1]), 2), np.float32)
    out, _ = po.grid_encode_backward(np.ascontiguousarray(g[:, :live]), np.ascontiguousarray(x[:live]), emb, off, live, D, 2, L,
                                     float(np.float32(np.log2(enc.per_level_scale))), 16, None, enc.gridtype_id, False, 0)
    return out


def _exp2f():
    f = C.CDLL("libm.so.6").exp2f
    f.restype, f.argtypes = C.c_float, [C.c_float]
    return f


def _level_consts(enc):
    """(scale fp32, resolution) per level, as make_level_consts / the oracle compute them (libm's exp2f)."""
    exp2f, S = _exp2f(), np.float32(np.log2(enc.per_level_scale))
    scale = [np.float32(np.float32(exp2f(np.float32(level) * S)) * np.float32(16) - np.float32(1)) for level in range(_levels(enc))]
    return scale, [np.uint32(np.ceil(s)) + np.uint32(1) for s in scale]


def _corners(enc, xs, level):
    """(level-local row int64 [n], weight fp32 [n]) of every corner, in corner order, for samples xs that all lie inside [0, 1]
    (orc_grid.c:212-256)."""
    off = _offsets(enc)
    D = enc.input_dim
    primes = np.array([1, 2654435761, 805459861], dtype=np.uint32)
    scales, ress = _level_consts(enc)
    size, scale, res = np.uint32(off[level + 1] - off[level]), scales[level], ress[level]
    pos = (xs * scale + np.float32(0.5)).astype(np.float32)
    pg = np.floor(pos).astype(np.uint32)
    pos = (pos - pg.astype(np.float32)).astype(np.float32)
    for corner in range(1 << D):
        w = np.ones(pos.shape[0], np.float32)
        stride, index = np.uint64(1), np.zeros(pos.shape[0], np.uint32)
        h = np.zeros(pos.shape[0], np.uint32)
        for d in range(D):
            bit = (corner >> d) & 1
            w = (w * (pos[:, d] if bit else (np.float32(1) - pos[:, d]))).astype(np.float32)
            p = pg[:, d] + np.uint32(bit)
            h ^= p * primes[d]
            if stride <= size:
                index = index + p * np.uint32(stride)
                stride = np.uint64(np.uint32(stride * np.uint64(res + 1)))       # uint32 arithmetic, as the oracle's
        if enc.gridtype_id == 0 and stride > size:
            index = h
        yield (index % size).astype(np.int64), w


def _inside(xs):
    return ~((xs < 0) | (xs > 1)).any(axis=1)


def _contributions(enc, x, g, live):
    """(global row, w * g [.., 2]) of every (level, sample, corner) the oracle adds, restated in numpy fp32 (orc_grid.c:212-256)."""
    off = _offsets(enc)
    xs, rows, vals = x[:live], [], []
    inside = _inside(xs)
    for level in range(_levels(enc)):
        for index, w in _corners(enc, xs[inside], level):
            rows.append(off[level] + index)
            vals.append((w[:, None] * g[level, :live][inside]).astype(np.float32))
    return np.concatenate(rows), np.concatenate(vals)


def _jobs(entries, host_offsets=True):
    """ScatterJobT array for [(grad, inputs, enc, grad_table), ...] + what must stay alive."""
    import radnerf_hip as hip
    from radnerf.fused import _grid_desc
    from radnerf_hip.abi import ScatterJobT
    arr, keep = (ScatterJobT * len(entries))(), []
    for i, (grad, inputs, enc, table) in enumerate(entries):
        gd, off = _grid_desc(enc, table), hip.host_offsets(enc.offsets)
        arr[i].grad, arr[i].inputs, arr[i].grid, arr[i].grad_table = grad.data_ptr(), inputs.data_ptr(), C.pointer(gd), table.data_ptr()
        arr[i].offsets_host = C.cast(off, C.c_void_p) if host_offsets else None
        keep += [gd, off]
    return arr, keep


def _bits(t):
    return (t.detach().cpu().numpy() if hasattr(t, "detach") else t).view(np.uint32)


def accumulate(rows, vals, n_rows):
    """(n [rows], mag [rows, 2], exact [rows, 2]) in float64: how many addends a row has, the sum of their magnitudes, their sum."""
    n, mag, exact = np.zeros(n_rows), np.zeros((n_rows, 2), np.float64), np.zeros((n_rows, 2), np.float64)
    with np.errstate(over="ignore"):
        np.add.at(n, rows, 1.0)
        np.add.at(mag, rows, np.abs(vals.astype(np.float64)))
        np.add.at(exact, rows, vals.astype(np.float64))
    return n, mag, exact


def gamma(k):
    k = np.asarray(k, np.float64)
    return k * U / (1.0 - k * U)


def bound(n, mag):
    """|fp32 sum of n terms, in any order - exact sum| <= gamma(n - 1) * sum |v_i| (Higham, Accuracy and Stability of Numerical
    Algorithms, eq. 4.4).  n [rows], mag [rows, 2] -> [rows, 2]; zero for n <= 1."""
    return gamma(np.maximum(np.asarray(n, np.float64) - 1.0, 0.0))[:, None] * mag


def reference(enc, x, g, live):
    rows, vals = _contributions(enc, x, g, live)
    return accumulate(rows, vals, int(_offsets(enc)[-1]))


def _limits(got, ref, prior):
    n, mag, exact = ref
    if prior is None:
        return exact, bound(n, mag)
    return exact + prior.astype(np.float64), bound(n, mag) + U * np.abs(got.astype(np.float64))


def verdict(got, ref, prior=None):
    """got [rows, 2] fp32 against ref = (n, mag, exact), element by element: n == 0 -> the bits of `prior` (zeros when None);
    n == 1 -> the addend itself; else within bound(n, mag).  With `prior`, a touched element is held to prior + sum with one more
    rounding, bound + U |got| (n == 1 included) -- sound where a row receives its whole sum in ONE addition to memory.
    -> dict(untouched_changed, single_wrong, over: elements that miss; nan; worst: largest err / bound; longest: longest run)."""
    n = ref[0]
    want, b = _limits(got, ref, prior)
    err = np.abs(got.astype(np.float64) - want)
    none, one, many = n == 0, n == 1, n > 1
    before = np.zeros_like(got) if prior is None else prior
    return dict(untouched_changed=int((_bits(np.ascontiguousarray(got[none])) != _bits(np.ascontiguousarray(before[none]))).sum()),
                single_wrong=int((~(err[one] <= b[one])).sum()), over=int((~(err[many] <= b[many])).sum()), nan=int(np.isnan(got).sum()),
                worst=float((err[many] / np.maximum(b[many], 1e-300)).max()) if many.any() else 0.0, longest=int(n.max()))


def first_failures(got, ref, enc, prior=None, k=5):
    """(level, local row, channel, n, got, wanted, bound) of the first k elements that miss: for the failure message."""
    n = ref[0]
    off = _offsets(enc)
    want, b = _limits(got, ref, prior)
    bad = np.argwhere(~(np.abs(got.astype(np.float64) - want) <= b))
    out = []
    for r, c in bad[:k]:
        level = int(np.searchsorted(off, r, side="right") - 1)
        out.append((level, int(r - off[level]), int(c), int(n[r]), float(got[r, c]), float(want[r, c]), float(b[r, c])))
    return out


# ---- which level takes which path ------------------------------------------------------------------------------------------
def plan(enc, host_offsets=True):
    """Per level: rows, hashed (the dense stride overflows the level's rows), direct (hashed and >= 2^17 rows, needs the host
    offsets), binned (hashed and 16 .. 128 buckets of 2^12 rows; taken only with a workspace), chunks (8 where rows <= 2^16 and
    the host offsets are given, else 1; a direct level has 1), n_buckets."""
    off = _offsets(enc)
    _, ress = _level_consts(enc)
    L = _levels(enc)
    rows = (off[1:] - off[:-1]).astype(np.int64)
    hashed = np.zeros(L, bool)
    for level in range(L):
        stride = 1
        for _ in range(enc.input_dim):
            if stride <= rows[level]:
                stride *= int(ress[level]) + 1
        hashed[level] = enc.gridtype_id == 0 and stride > rows[level]
    nb = (rows + (1 << BUCKET_SHIFT) - 1) >> BUCKET_SHIFT
    binned = hashed & (nb >= MIN_BUCKETS) & (nb <= MAX_BUCKETS)
    direct = hashed & (rows >= DIRECT_ROWS) & host_offsets
    chunks = np.where(~direct & (rows <= CHUNK_ROWS) & host_offsets, CHUNKS, 1)
    return dict(rows=rows, hashed=hashed, direct=direct, binned=binned, chunks=chunks, n_buckets=nb,
                binned_mask=int(sum(1 << level for level in range(L) if binned[level])))


def bucket_capacity(M, enc):
    """Entries a bucket has room for at row capacity M: 2 x the mean load of a bucket of the level with the fewest + slack."""
    p = plan(enc)
    if not p["binned"].any():
        return 0
    return 2 * ((M << enc.input_dim) // int(p["n_buckets"][p["binned"]].min())) + 2048


def sample_rows(enc, x, live, level):
    """[live, 2^D] level-local rows of every sample's corners; -1 for a sample outside [0, 1]."""
    xs = x[:live]
    inside = _inside(xs)
    out = np.full((live, 1 << enc.input_dim), -1, np.int64)
    for corner, (index, _) in enumerate(_corners(enc, xs[inside], level)):
        out[inside, corner] = index
    return out


def samples_per_chunk(enc):
    return SC_THREADS >> (enc.input_dim - 1)


def simulate_tables(enc, x, live, level, chunks):
    """The LDS table of every workgroup of `level`, chunk by chunk, as sets of 64-byte lines: -> (flushes before the last chunk
    [workgroups], peak number of distinct lines a table is offered between two flushes [workgroups], distinct lines per chunk
    [all chunks]).  A line that finds no slot within the probe limit goes to memory instead, so the true occupancy can be lower
    than the peak (never higher than the slot count)."""
    spc = samples_per_chunk(enc)
    lines = sample_rows(enc, x, live, level) >> 3
    flushes, peaks, per_chunk = [], [], []
    for wg in range(-(-live // (spc * chunks))):
        table, peak, fl = set(), 0, 0
        for c in range(chunks):
            lo = (wg * chunks + c) * spc
            if lo >= live:
                break
            ls = lines[lo:lo + spc]
            mine = set(ls[ls >= 0].tolist())
            per_chunk.append(len(mine))
            table |= mine
            peak = max(peak, len(table))
            if c + 1 == chunks or lo + spc >= live:
                break
            if len(table) > FLUSH_ABOVE:
                fl += 1
                table = set()
        flushes.append(fl)
        peaks.append(peak)
    return np.array(flushes), np.array(peaks), np.array(per_chunk)


def wave_heads(enc, x, live, level):
    """Run heads of every wave of the line-merge kernel on `level`: a lane holds the two rows of one x-pair of corners of one sample,
    the lanes of a wave are 64 consecutive samples of one pair, and a head is a lane whose rows differ from the lane before."""
    spc, P = samples_per_chunk(enc), 1 << (enc.input_dim - 1)
    rows = sample_rows(enc, x, live, level)
    pad = -(-live // spc) * spc
    keys = np.full((pad, P, 2), -1, np.int64)
    keys[:live] = rows.reshape(live, P, 2)                    # corner = x bit | pair << 1
    keys = keys.reshape(pad // spc, spc // 64, 64, P, 2).transpose(0, 3, 1, 2, 4)      # chunk, pair, wave, lane, row
    return 1 + (keys[..., 1:, :] != keys[..., :-1, :]).any(axis=-1).sum(axis=-1).reshape(-1)


def bucket_load(enc, x, live, level):
    """(entries per bucket [n_buckets], longest run per bucket) of a binned level."""
    rows = sample_rows(enc, x, live, level).reshape(-1)
    rows = rows[rows >= 0]
    nb = int(plan(enc)["n_buckets"][level])
    per_row = np.bincount(rows, minlength=nb << BUCKET_SHIFT)
    return np.bincount(rows >> BUCKET_SHIFT, minlength=nb), per_row.reshape(nb, -1).max(axis=1)


# ---- input patterns --------------------------------------------------------------------------------------------------------
CAP = 4608


def _finish(x, live, L, r, cap=CAP):
    out = np.full((cap, x.shape[1]), np.nan, np.float32)
    out[:live] = x[:live]
    return out, _gradients(L, cap, live, r), live


def uniform(enc, seed=7, live=4096, cap=CAP):
    """Spread-out samples: every chunk fills the table past the flush threshold, most touched rows of the fine levels have one
    addend.  Holds the corners of the unit cube, a coordinate exactly 0, one exactly 1, and two samples outside [0, 1]."""
    D, r = enc.input_dim, np.random.default_rng(seed)
    x = r.random((live, D), dtype=np.float32)
    if live > 6:
        x[0], x[1], x[2, 0], x[3, D - 1], x[4, 0], x[5, D - 1] = 0.0, 1.0, 0.0, 1.0, 1.5, -0.1
    return _finish(x, live, _levels(enc), r, cap)


def ray_runs(enc, seed=11, live=4096):
    """Runs of 16 samples stepping away from one point, as a ray's samples do: neighbouring lanes share their coarse rows."""
    D, r = enc.input_dim, np.random.default_rng(seed)
    base = r.random((live // 16, 1, D))
    x = (base + 0.02 * np.arange(16).reshape(1, 16, 1) * r.standard_normal((live // 16, 1, D))).reshape(-1, D)
    x = np.clip(x, 0, 1).astype(np.float32)
    x[:5] = 1.5
    return _finish(x, live, _levels(enc), r)


def coincident(enc, seed=3, live=CAP):
    """Every sample the same point: runs as long as the launch."""
    D, r = enc.input_dim, np.random.default_rng(seed)
    x = np.repeat(r.random((1, D), dtype=np.float32) * 0.8 + 0.1, live, axis=0)
    return _finish(x, live, _levels(enc), r)


MIXED_CLUSTERED = 3         # clustered chunks at the head of every group of 8


def mixed(enc, seed=5, live=4096):
    """Per group of 8 chunks: MIXED_CLUSTERED chunks inside one small box (few lines: no flush), then uniform chunks -- the first
    of them is inserted into a table that already holds the box's lines.  MIXED_SIDE makes the box hold just under the flush threshold on one level."""
    D, r = enc.input_dim, np.random.default_rng(seed)
    spc = samples_per_chunk(enc)
    x = r.random((live, D), dtype=np.float32)
    for wg in range(live // (spc * CHUNKS)):
        lo = wg * spc * CHUNKS
        side = MIXED_SIDE[enc.input_dim, enc.gridtype]
        corner = (r.random((1, D)) * (1 - side)).astype(np.float32)
        x[lo:lo + MIXED_CLUSTERED * spc] = corner + np.float32(side) * r.random((MIXED_CLUSTERED * spc, D), dtype=np.float32)
    return _finish(np.clip(x, 0, 1), live, _levels(enc), r)


# side of the box: the largest 8-chunk level at which the box still holds fewer than 190 lines decides it (level 2 of the 3-D hash
# grid, whose finer levels are not line-merged in chunks; level 8 of the 3-D tiled grid, the last that keeps z; level 15 in 2-D)
MIXED_SIDE = {(3, "hash"): 0.28, (3, "tiled"): 0.04, (2, "tiled"): 0.023}


OVERFULL_LEVEL = 15


def overfull_bucket(enc, seed=13, live=4096, pool=60000):
    """Samples with a corner in bucket 0 of level OVERFULL_LEVEL: that bucket gets more entries than it has room for, in short runs,
    so the rest goes through the spill list.  Capacity = live count (the bucket capacity follows the row capacity)."""
    r = np.random.default_rng(seed)
    x = r.random((pool, enc.input_dim), dtype=np.float32)
    rows = sample_rows(enc, x, pool, OVERFULL_LEVEL)
    keep = np.flatnonzero(((rows >> BUCKET_SHIFT) == 0).any(axis=1))
    assert keep.shape[0] >= live, (keep.shape[0], live)
    return _finish(x[keep[:live]], live, _levels(enc), r, cap=live)


PATTERNS = dict(uniform=uniform, ray_runs=ray_runs, mixed=mixed, coincident=coincident, overfull_bucket=overfull_bucket)


# ---- inputs for the accumulate-versus-write contract ---------------------------------------------------------------------------
def spread(enc, seed, live):
    """`live` samples at a capacity of live + 5 (the rest NaN): uniform ones, each with a partner 0.05 away along every axis -- the
    two share rows on the coarsest levels (cells of 1/15) and none from level 4 on (cells of 1/59 and less)."""
    r = np.random.default_rng(seed)
    x = r.random((live, enc.input_dim), dtype=np.float32) * np.float32(0.9)
    x[live // 2:] = x[:live - live // 2] + np.float32(0.05)
    return _finish(x, live, _levels(enc), r, cap=live + 5)


def longest_probe_cluster(lines):
    """Longest cyclic run of occupied slots once `lines` sit in the LDS table.  Which slots end up occupied does not depend on the
    order of insertion (linear probing), and no insertion probes further than the longest run + 1."""
    used = np.zeros(SC_SLOTS, bool)
    for line in lines:
        slot = ((int(line) * 2654435761) & 0xffffffff) >> (32 - 9)
        while used[slot]:
            slot = (slot + 1) & (SC_SLOTS - 1)
        used[slot] = True
    if used.all():
        return SC_SLOTS
    start = int(np.flatnonzero(~used)[0])
    run = best = 0
    for s in np.roll(used, -start):
        run = run + 1 if s else 0
        best = max(best, run)
    return best


def summed_once(enc, x, live, ref, binned):
    """None if every table row receives its whole sum in ONE addition to memory (else the reason): one workgroup and one chunk per
    level, every line placed in the LDS table within the probe limit, and on the levels that go straight to memory (direct ones,
    when not binned) no row with two addends."""
    if live > samples_per_chunk(enc):
        return "more than one chunk of samples"
    p, off = plan(enc), _offsets(enc)
    for level in range(_levels(enc)):
        if binned and p["binned"][level]:
            continue
        if p["direct"][level]:
            if ref[0][off[level]:off[level + 1]].max() > 1:
                return "level %d goes straight to memory and has a row with two addends" % level
            continue
        lines = np.unique(sample_rows(enc, x, live, level) >> 3)
        if longest_probe_cluster(lines[lines >= 0]) + 1 >= SC_PROBES:
            return "level %d may reach the probe limit" % level
    return None


# (grid, seed, live count, binned route) of the prefilled-table cases; test_scatter_ref.py asserts summed_once for each
SUMMED_ONCE = [("hash17", 1, 16, False), ("tiled2", 2, 100, False), ("tiled3", 1, 48, False), ("hash17", 1, 48, True)]
