"""Seeded inputs of the compositor tests, shared by test_compref64.py (CPU: the oracle against compref64) and
test_gpu_composite.py (GPU: the kernels against compref64).  Plain numpy, nothing here loads a library.

The shapes are the smallest at which the kernels can go wrong: the workgroup is 256 rays, so N runs over 1, 255, 256, 257
and 1000 (four workgroups, the last partial); `rays[:, 0]` is a permutation, so a kernel that writes row n instead of row
rays[n, 0] is wrong on every ray; counts of 0 and rays past the budget M take the kernels' skip branch; deltas over three
cascades' step sizes and sigma = 400 u^4 (a fifth exactly 0) give transparent rays, rays that end after one sample and rays
with one nearly opaque sample that go on.
"""
import functools

import numpy as np

DTS = (2 * np.sqrt(3) / 1024, 2 * np.sqrt(3) / 128, 2 * np.sqrt(3) / 16)
SENTINEL = np.float32(7.25)             # what the gradient buffers hold before the backward: rows of no gradient keep it
SPARE = 5                               # rows past the last ray's slice
MAX_COUNT = 24

TRAIN_N = (1, 255, 256, 257, 1000)
TRAIN_T = (0.0, 1e-4, 0.3)


def _samples(r, M):
    """sigma, rgb, ambient, deltas[:, 0] of M samples."""
    sig = (400.0 * r.random(M) ** 4).astype(np.float32)
    sig[r.random(M) < 0.2] = 0.0
    sig[r.random(M) < 0.02] = np.float32(1e-9)      # sigma * delta ~ 1e-12: alpha is 0 in fp32
    rgb = r.random((M, 3)).astype(np.float32)
    amb = r.random(M).astype(np.float32)
    dt = np.asarray(DTS, np.float32)[r.integers(0, 3, M)]
    return sig, rgb, amb, dt


def _train_case(name, N, T_thresh, seed, counts=None, budget=True):
    r = np.random.default_rng(seed)
    if counts is None:
        counts = r.integers(0, MAX_COUNT + 1, N)
        counts[r.random(N) < 0.05] = 0
        if N == 1:
            counts[:] = 7
    counts = np.asarray(counts, np.int64)
    offs = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    total = int(counts.sum())
    rows = total + SPARE                # what is allocated: every offset stays inside it
    # the budget the operator is given ends inside the third ray from the end that has samples: the last rays are skipped
    M = total
    live = np.flatnonzero(counts)
    if budget and live.size >= 8:
        M = int(offs[live[-3]] + counts[live[-3]] - 1)
    rays = np.stack([r.permutation(N), offs, counts], 1).astype(np.int32)
    sig, rgb, amb, dt = _samples(r, rows)
    t = np.empty(rows, np.float32)
    for o, k in zip(offs, counts):
        t[o:o + k] = (3.0 + np.cumsum(dt[o:o + k].astype(np.float64))).astype(np.float32)
    t[total:] = 3.0
    deltas = np.stack([dt, t], 1).astype(np.float32)
    g_ws = r.standard_normal(N).astype(np.float32)
    g_am = r.standard_normal(N).astype(np.float32)
    g_im = r.standard_normal((N, 3)).astype(np.float32)
    if N > 1:
        g_ws[r.random(N) < 0.1] = 0.0
        g_im[r.random(N) < 0.1] = 0.0
    # the marcher's backward on the same rays: sample gradients, and buffers that hold something on entry
    gx = r.standard_normal((rows, 3)).astype(np.float32)
    gd = r.standard_normal((rows, 3)).astype(np.float32)
    go0 = r.standard_normal((N, 3)).astype(np.float32)
    gd0 = r.standard_normal((N, 3)).astype(np.float32)
    return dict(name=name, N=N, M=M, rows=rows, T_thresh=float(np.float32(T_thresh)), rays=rays, sigmas=sig, rgbs=rgb, ambient=amb,
                deltas=deltas, g_ws=g_ws, g_am=g_am, g_im=g_im, gx=gx, gd=gd, go0=go0, gd0=gd0)


def _as_training(name, icase):
    """The first call of an inference case as a training case at T_thresh = 0: entry n of the alive list is ray n with the
    slots of its chunk that hold a sample (outputs are compared by entry, since the alive ids exceed N)."""
    N, s = icase["N"], icase["n_step"]
    sig, rgb, dl = chunk(icase, icase["alive"], 0)
    counts = (dl[:, 0].reshape(N, s) > 0).sum(1)
    rays = np.stack([np.arange(N), np.arange(N) * s, counts], 1).astype(np.int32)
    z = np.zeros(N, np.float32)
    return dict(name=name, N=N, M=N * s, rows=N * s, T_thresh=0.0, rays=rays, sigmas=sig, rgbs=rgb, ambient=np.zeros(N * s, np.float32),
                deltas=dl, g_ws=z, g_am=z, g_im=np.zeros((N, 3), np.float32))


@functools.lru_cache(maxsize=None)
def train_case(name):
    if name.startswith("as-training:"):
        return _as_training(name, infer_case(name.split(":", 1)[1]))
    if name.endswith("/image"):         # nothing but the image is used downstream
        case = dict(train_case(name[:-6]), name=name)
        case["g_ws"], case["g_am"] = np.zeros_like(case["g_ws"]), np.zeros_like(case["g_am"])
        return case
    if name == "empty":
        return _train_case(name, 64, 1e-4, 900, counts=np.zeros(64, np.int64))
    if name == "single24":
        return _train_case(name, 1, 1e-4, 901, counts=[MAX_COUNT])
    N, T = name.split("-")
    N, T = int(N[1:]), float(T[1:])
    return _train_case(name, N, T, 1000 + 10 * TRAIN_N.index(N) + TRAIN_T.index(T))


TRAIN_CASES = [f"N{N}-T{T:g}" for N in TRAIN_N for T in TRAIN_T] + ["empty", "single24"]
MARCH_BWD_CASES = ["N1-T0", "N256-T0", "N257-T0"]       # T_thresh plays no part in the marcher's backward


# ------------------------------------------------------------------------------------------------ inference

INFER_N = (1, 257, 600)
INFER_STEP = (1, 4, 8)
INFER_T = (0.0, 1e-4)
CALLS = 3


def _infer_case(name, N, n_step, T_thresh, seed, limit=None):
    """R rays of which a shuffled subset of N is alive; ray `i` has `length[i]` samples (0 ... CALLS * n_step) in slots
    [i, 0 : length[i]], the slots after them are zero.  Call c composites slots [c * n_step, (c + 1) * n_step) of the rays that
    are still alive.  `limit`: the device-side count of the first call (the launch bound stays N)."""
    r = np.random.default_rng(seed)
    R = N + max(3, N // 4)
    S = CALLS * n_step
    alive = r.permutation(R)[:N].astype(np.int32)
    length = r.integers(0, S + 1, R)
    length[r.random(R) < 0.15] = S                  # rays that the walk never leaves
    if N == 1:
        length[alive[0]] = S
    sig, rgb, _, dt = _samples(r, R * S)
    sig, rgb, dt = sig.reshape(R, S), rgb.reshape(R, S, 3), dt.reshape(R, S)
    sig[r.random(R) < 0.3] *= np.float32(0.01)      # thin rays: they outlive the frame's three calls
    if T_thresh == 0.0:
        # without a threshold a ray stops only where fp32's `1 - weights_sum` goes negative, which no float64 restatement
        # decides: keep every ray's optical depth at 9 or less, so that T stays above e^-9 = 1.2e-4, far above the
        # resolution of `1 - weights_sum` (2^-24)
        depth = (sig.astype(np.float64) * dt).sum(1)
        sig = (sig * np.minimum(1.0, 9.0 / np.maximum(depth, 1e-30))[:, None] * 0.999).astype(np.float32)
    used = np.arange(S)[None] < length[:, None]
    t = (3.0 + np.cumsum(dt.astype(np.float64), 1)).astype(np.float32)
    deltas = np.stack([dt * used, t * used], -1).astype(np.float32)
    sig, rgb = sig * used, rgb * used[..., None]
    # rays outside the alive list hold values that no call may touch; alive rays start a frame: zero accumulators
    on = np.zeros(R, bool)
    on[alive] = True
    ws0 = np.where(on, 0, r.random(R)).astype(np.float32)
    dp0 = np.where(on, 0, r.random(R)).astype(np.float32)
    im0 = np.where(on[:, None], 0, r.random((R, 3))).astype(np.float32)
    t0 = r.uniform(2, 3, R).astype(np.float32)
    return dict(name=name, N=N, R=R, n_step=n_step, T_thresh=float(np.float32(T_thresh)), alive=alive, length=length, sigmas=sig,
                rgbs=rgb, deltas=deltas, ws0=ws0, depth0=dp0, image0=im0, rays_t0=t0, limit=limit,
                calls=1 if limit is not None else CALLS)


@functools.lru_cache(maxsize=None)
def infer_case(name):
    if name == "device-count":
        return _infer_case(name, 600, 4, 1e-4, 2900, limit=300)
    N, s, T = name.split("-")
    N, s, T = int(N[1:]), int(s[1:]), float(T[1:])
    return _infer_case(name, N, s, T, 2000 + 100 * INFER_N.index(N) + 10 * INFER_STEP.index(s) + INFER_T.index(T))


INFER_CASES = [f"N{N}-s{s}-T{T:g}" for N in INFER_N for s in INFER_STEP for T in INFER_T] + ["device-count"]


def chunk(case, alive, c):
    """The sample buffers of call `c` for the alive list `alive`: entry n holds slots [c * n_step, (c + 1) * n_step) of ray
    alive[n]."""
    s = case["n_step"]
    sl = slice(c * s, (c + 1) * s)
    return (np.ascontiguousarray(case["sigmas"][alive, sl]).reshape(-1), np.ascontiguousarray(case["rgbs"][alive, sl]).reshape(-1, 3),
            np.ascontiguousarray(case["deltas"][alive, sl]).reshape(-1, 2))


def run_inference(case, composite):
    """The per-frame pattern: CALLS calls of `composite(n_alive, n_step, T_thresh, alive, rays_t, sigmas, rgbs, deltas, ws, depth,
    image, limit)` (in place on numpy arrays, `limit` the device-side count or None), the alive list compacted on the host
    between them.  Returns, per call, what went in and what came out."""
    alive = case["alive"].copy()
    state = dict(rays_t=case["rays_t0"].copy(), ws=case["ws0"].copy(), depth=case["depth0"].copy(), image=case["image0"].copy())
    out = []
    for c in range(case["calls"]):
        sig, rgb, dl = chunk(case, alive, c)
        alive_out = alive.copy()
        if alive.size:
            composite(alive.size, case["n_step"], case["T_thresh"], alive_out, state["rays_t"], sig, rgb, dl, state["ws"],
                      state["depth"], state["image"], case["limit"])
        out.append(dict(alive_in=alive, alive_out=alive_out, **{k: v.copy() for k, v in state.items()}))
        alive = alive_out[alive_out >= 0]
    return out
