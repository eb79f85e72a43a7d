"""rn_grid_dense_plan (csrc/rn_grid.hip): which hashed levels of a grid a dense image stores as whole lattices.  Host only -- no
GPU, nothing allocated.  The expectation is restated here from include/radnerf_fused.h: hashed levels in ascending order while
the whole image stays within the budget, below 4 GiB and below 2^31 rows; a taken level gets (R+1)^3 rows rounded up to 8,
every other level keeps its rows; tiled grids, D != 3 and a budget that fits no level give "no image"."""
import ctypes as C

import numpy as np
import pytest

L = 16


def level_resolutions(H, S, n=L):
    """resolution[l] as csrc/rn_grid_dev.h make_level_consts computes it (fp32 exp2f)."""
    out = []
    for l in range(n):
        scale = np.float32(np.exp2(np.float32(l) * np.float32(S))) * np.float32(H) - np.float32(1.0)
        out.append(int(np.ceil(scale)) + 1)
    return out


def table_offsets(D, H, S, log2_T, n=L):
    """offsets [n+1] in rows of a grid as gridencoder/encoder.py lays it out (align_corners off)."""
    off = [0]
    for R in level_resolutions(H, S, n):
        rows = min(2 ** log2_T, (R + 1) ** D)
        off.append(off[-1] + (rows + 7) // 8 * 8)
    return off


def plan_ref(off, res, row_bytes, budget, gridtype=0, D=3):
    """(image offsets, level mask, image bytes) or None."""
    if gridtype != 0 or D != 3:
        return None
    rows = [off[l + 1] - off[l] for l in range(len(res))]
    total, mask = sum(rows), 0
    for l, R in enumerate(res):
        if (R + 1) ** 3 <= rows[l]:
            continue                                            # dense already
        full = ((R + 1) ** 3 + 7) // 8 * 8
        new_total = total - rows[l] + full
        if new_total * row_bytes > budget or new_total * row_bytes >= 2 ** 32 or new_total >= 2 ** 31:
            break
        total, rows[l], mask = new_total, full, mask | (1 << l)
    if not mask:
        return None
    return list(np.cumsum([0] + rows)), mask, total * row_bytes


def grid_desc(hiplib, off, H, S, dtype, gridtype=0, D=3, embeddings=0, offsets_dev=0):
    from radnerf_hip.abi import GridT
    g = GridT()
    g.embeddings, g.offsets = embeddings, offsets_dev
    g.D, g.L, g.H, g.S, g.gridtype, g.dtype = D, len(off) - 1, H, float(S), gridtype, dtype
    return g


def plan(hiplib, g, off, budget):
    """The library's answer in the shape of plan_ref's."""
    oh = (C.c_int32 * len(off))(*off)
    out = (C.c_int32 * len(off))(*([-1] * len(off)))
    levels, nbytes = C.c_uint32(0xFFFFFFFF), C.c_size_t(0)
    rc = hiplib._lib.rn_grid_dense_plan(C.byref(g), oh, int(budget), out, C.byref(levels), C.byref(nbytes))
    assert rc in (0, 1), hiplib.last_error()
    if rc == 0:
        assert list(out) == [-1] * len(off) and levels.value == 0xFFFFFFFF      # "no image" writes nothing
        return None
    return list(out), levels.value, nbytes.value


S11 = float(np.log2(np.exp2(np.log2(2048 / 16) / 15)))      # the xyz grid of the shipped configurations: 16 -> 2048 over 16 levels


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("log2_T", [12, 19])
def test_plan_follows_the_budget_to_the_byte(hiplib, log2_T, dtype):
    row_bytes = 4 if dtype else 8
    off, res = table_offsets(3, 16, S11, log2_T), level_resolutions(16, S11)
    g = grid_desc(hiplib, off, 16, S11, dtype)
    first = next(l for l, R in enumerate(res) if (R + 1) ** 3 > off[l + 1] - off[l])
    assert first == (0 if log2_T == 12 else 5)
    table_bytes = off[-1] * row_bytes
    for n in (1, 3, 4):                                         # the budget that holds exactly n levels, and one byte less
        rows = off[-1] + sum(((res[l] + 1) ** 3 + 7) // 8 * 8 - (off[l + 1] - off[l]) for l in range(first, first + n))
        want = plan_ref(off, res, row_bytes, rows * row_bytes)
        assert want[1] == ((1 << n) - 1) << first and want[2] == rows * row_bytes
        assert plan(hiplib, g, off, rows * row_bytes) == want
        less = plan(hiplib, g, off, rows * row_bytes - 1)
        assert less == plan_ref(off, res, row_bytes, rows * row_bytes - 1)
        assert (less is None) if n == 1 else (less[1] == ((1 << (n - 1)) - 1) << first)
    for budget in (0, table_bytes):                             # no level fits
        assert plan(hiplib, g, off, budget) is None


@pytest.mark.parametrize("dtype", [0, 1])
def test_plan_never_reaches_4_gib(hiplib, dtype):
    row_bytes = 4 if dtype else 8
    off, res = table_offsets(3, 16, S11, 19), level_resolutions(16, S11)
    g = grid_desc(hiplib, off, 16, S11, dtype)
    got = plan(hiplib, g, off, 1 << 40)
    assert got == plan_ref(off, res, row_bytes, 1 << 40)
    image_off, mask, nbytes = got
    assert nbytes < 2 ** 32 and image_off[-1] < 2 ** 31 and nbytes == image_off[-1] * row_bytes
    last = mask.bit_length() - 1
    assert mask == sum(1 << l for l in range(5, last + 1)) and last == (12 if dtype else 11)
    # the next level is what would cross the line, not the budget
    assert (image_off[-1] - (off[last + 2] - off[last + 1]) + (res[last + 1] + 1) ** 3) * row_bytes >= 2 ** 32
    for l in range(L):
        rows = image_off[l + 1] - image_off[l]
        assert rows == (((res[l] + 1) ** 3 + 7) // 8 * 8 if (mask >> l) & 1 else off[l + 1] - off[l])


def test_no_image_for_tiled_grids_and_other_dimensions(hiplib):
    off = table_offsets(3, 16, S11, 12)
    assert plan(hiplib, grid_desc(hiplib, off, 16, S11, 0, gridtype=1), off, 1 << 30) is None
    off2 = table_offsets(2, 16, S11, 12)
    assert plan(hiplib, grid_desc(hiplib, off2, 16, S11, 0, D=2), off2, 1 << 30) is None
    # a grid whose levels are all dense already (T = 2^30 holds level 9's 296^3 rows; 10 levels) has nothing to take
    off3 = table_offsets(3, 16, S11, 30, n=10)
    assert plan(hiplib, grid_desc(hiplib, off3, 16, S11, 0), off3, 1 << 40) is None


def test_plan_rejects_bad_arguments(hiplib):
    off = table_offsets(3, 16, S11, 12)
    g = grid_desc(hiplib, off, 16, S11, 0)
    oh = (C.c_int32 * len(off))(*off)
    out = (C.c_int32 * len(off))()
    levels, nbytes = C.c_uint32(0), C.c_size_t(0)
    assert hiplib._lib.rn_grid_dense_plan(C.byref(g), None, 1 << 30, out, C.byref(levels), C.byref(nbytes)) < 0
    assert hiplib._lib.rn_grid_dense_plan(C.byref(g), oh, 1 << 30, None, C.byref(levels), C.byref(nbytes)) < 0
    bad = (C.c_int32 * len(off))(*([0] + off[:-1][::-1]))
    assert hiplib._lib.rn_grid_dense_plan(C.byref(g), bad, 1 << 30, out, C.byref(levels), C.byref(nbytes)) < 0
    g.dtype = 7
    assert hiplib._lib.rn_grid_dense_plan(C.byref(g), oh, 1 << 30, out, C.byref(levels), C.byref(nbytes)) < 0
