"""The two weight images of the torso layer (csrc/rn_torso_dev.h): rn_torso_pack_weights (inference, k_torso_fused) and
rn_train_torso_pack (training: forward | transposed | constants), element for element against a numpy restatement of the layout
written from

    rowmap(r, h) = (r & 3) + 8 (r >> 2) + 4 h        output row of register r, lane half h, of a 32-row accumulator tile
    kmap(s, h)   = 32 (s >> 4) + rowmap(s & 15, h)   k of MFMA step s when the B operand is the previous layer's accumulators

Random fp32 weights make every element distinct, so a swapped index cannot pass; ind_dim = 3 makes the leading dimensions of the
two first layers (96 + ind, 128 + ind) differ from their constant-free widths.

The weights are copied, so they compare with ==.  The constants block is arithmetic: every bias is a sum of 54 + ind_dim fp32
products of O(1) numbers added in sequence (error <= (54 + ind) * 2^-24 of the sum of their magnitudes, and that only if every
rounding goes the same way), and a cosine of enc_pose is sinf(a + fp32(pi / 2)) with |a| <= 8: half an ulp of an argument below
16 is 4.8e-7 before sinf's own 1 - 2 ulp.  Both are errors against the O(1) scale of the block, not against an element that
cancellation or a zero of the cosine makes small, so each of the three blocks is held to 1e-6 of its largest float64 magnitude."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K64, K32 = 128, 64                                             # floats per MFMA step of a 64-row / 32-row layer
T_D0, T_D1, T_D2, T_T0, T_T1, T_T2, N_FWD = 0, 2688, 6784, 6912, 9280, 10304, 10432
B_T2, B_T1, B_T0, B_D2, B_D1, N_BWD = 0, 128, 1152, 2176, 2304, 6400
N_CONST = 152


def rowmap(r, h):
    return (r & 3) + 8 * (r >> 2) + 4 * h


def kmap(s, h):
    return 32 * (s >> 4) + rowmap(s & 15, h)


def gather_column(s, h):
    """Grid column of step s, lane half h, in the order the training forward gathers: half h holds level 2 (s / 2) + h, its steps
    are the level's two channels."""
    return 2 * (2 * (s >> 1) + h) + (s & 1)


def mfma64(w, steps, k_of, transposed=False):
    """[step][h][col j][row tile] of a 64-row layer: W[32 rt + j, k(s, h)] (transposed: W[k(s, h), 32 rt + j])"""
    out = np.empty((steps, 2, 32, 2), np.float32)
    for s in range(steps):
        for h in range(2):
            for rt in range(2):
                rows = 32 * rt + np.arange(32)
                out[s, h, :, rt] = w[k_of(s, h), rows] if transposed else w[rows, k_of(s, h)]
    return out.reshape(-1)


def mfma32(w, steps, k_of):
    """[step][h][row j] of a 32-row layer: W[j, k(s, h)]"""
    return np.stack([w[:32, k_of(s, h)] for s in range(steps) for h in range(2)]).reshape(-1)


def narrow(w, regs):
    """[out][h][q] of a VALU layer over `regs` accumulator registers per lane (16 per row tile)"""
    return np.stack([[[w[o, 32 * (q >> 4) + rowmap(q & 15, h)] for q in range(regs)] for h in range(2)] for o in range(w.shape[0])]).reshape(-1)


def forward_image(ws, gather):
    d0, d1, d2, t0, t1, t2 = ws
    grid = gather_column if gather else (lambda s, h: 2 * s + h)
    img = np.concatenate([
        mfma64(d0, 21, lambda s, h: 2 * s + h), mfma64(d1, 32, kmap), narrow(d2, 32),
        mfma32(t0, 37, lambda s, h: grid(s, h) if s < 16 else 2 * s + h), mfma32(t1, 16, rowmap), narrow(t2, 16)])
    assert img.size == N_FWD
    return img


def transposed_image(ws):
    d0, d1, d2, t0, t1, t2 = ws
    # output row j of the grid-feature gradient sits in register r of lane half hh with rowmap(r, hh) == j, and is to be the
    # feature the forward gathered into that register: 4 (r >> 1) + 2 hh + (r & 1)
    feat = np.empty(32, np.int64)
    for r in range(16):
        for hh in range(2):
            feat[rowmap(r, hh)] = 4 * (r >> 1) + 2 * hh + (r & 1)
    img = np.concatenate([
        narrow(t2, 16), mfma32(t1.T, 16, rowmap), mfma32(t0[:, :32][:, feat].T, 16, rowmap),
        narrow(d2, 32), mfma64(d1, 32, kmap, transposed=True)])
    assert img.size == N_BWD
    return img


@pytest.mark.parametrize("ind_dim", [0, 3])
def test_torso_weight_images(hiplib, ind_dim):
    import torch
    from radnerf_hip import abi
    hip, lib = hiplib, hiplib._lib
    assert lib.rn_torso_packed_floats() == N_FWD and lib.rn_train_torso_image_floats() == N_FWD + N_BWD + N_CONST
    gen = torch.Generator().manual_seed(7 + ind_dim)
    shapes = [(64, 96 + ind_dim), (64, 64), (2, 64), (32, 128 + ind_dim), (32, 32), (4, 32)]
    sizes = [a * b for a, b in shapes]
    # a random permutation of evenly spaced values in (-1, 1): random, and distinct by construction
    flat = (torch.randperm(sum(sizes), generator=gen).float() + 0.5) * (2.0 / sum(sizes)) - 1.0
    ws_t = [f.reshape(s).cuda() for f, s in zip(flat.split(sizes), shapes)]
    poses6 = (torch.rand(6, generator=gen) * 2 - 1).cuda()
    code = torch.randn(ind_dim, generator=gen).cuda() if ind_dim else None
    ws = [w.cpu().numpy() for w in ws_t]
    assert np.unique(np.concatenate([w.reshape(-1) for w in ws])).size == sum(w.size for w in ws)

    tw = abi.TorsoWeightsT()
    (tw.def_w0, tw.def_w1, tw.def_w2, tw.tor_w0, tw.tor_w1, tw.tor_w2) = [w.data_ptr() for w in ws_t]
    tw.ind_dim = ind_dim
    infer = torch.full((N_FWD,), float("nan"), device="cuda")
    train = torch.full((N_FWD + N_BWD + N_CONST,), float("nan"), device="cuda")
    hip.call("rn_torso_pack_weights", C.byref(tw), hip.ptr(infer), hip.stream())
    hip.call("rn_train_torso_pack", C.byref(tw), hip.ptr(poses6), hip.ptr(code), hip.ptr(train), hip.stream())
    infer, train = infer.cpu().numpy(), train.cpu().numpy()

    # ---- forward part: the restatement, and the two images against each other
    assert np.array_equal(infer, forward_image(ws, gather=False))
    assert np.array_equal(train[:N_FWD], forward_image(ws, gather=True))
    grid_steps = np.zeros(N_FWD, bool)
    grid_steps[T_T0:T_T0 + 16 * K32] = True
    assert np.array_equal(infer[~grid_steps], train[:N_FWD][~grid_steps])
    for s in range(16):
        for h in range(2):
            c = gather_column(s, h)                              # level order holds column c at step c >> 1, lane half c & 1
            at, src = T_T0 + s * K32 + h * 32, T_T0 + (c >> 1) * K32 + (c & 1) * 32
            assert np.array_equal(train[at:at + 32], infer[src:src + 32]), (s, h)

    # ---- transposed part, block by block
    got, want = train[N_FWD:N_FWD + N_BWD], transposed_image(ws)
    for name, lo, hi in (("tor L2", B_T2, B_T1), ("tor L1", B_T1, B_T0), ("tor L0 grid", B_T0, B_D2), ("def L2", B_D2, B_D1),
                         ("def L1", B_D1, N_BWD)):
        assert np.array_equal(got[lo:hi], want[lo:hi]), name

    # ---- constants: biases of the constant columns [enc_pose | c] (deform 64 | torso 32), enc_pose [54], two zeros
    p = poses6.cpu().numpy().astype(np.float64)
    enc = np.empty(54)
    enc[:6] = p
    for c in range(6, 54):
        col, d = c // 6 - 1, c % 6
        enc[c] = (np.cos if col & 1 else np.sin)(2.0 ** (col // 2) * p[d])
    const = np.concatenate([enc, code.cpu().numpy().astype(np.float64)]) if ind_dim else enc
    want = {"def bias": ws[0][:, 42:].astype(np.float64) @ const, "tor bias": ws[3][:, 74:].astype(np.float64) @ const, "enc_pose": enc}
    got = train[N_FWD + N_BWD:]
    for name, lo in (("def bias", 0), ("tor bias", 64), ("enc_pose", 96)):
        ref = want[name]
        err = np.abs(got[lo:lo + ref.size] - ref).max() / np.abs(ref).max()
        print(f"ind_dim {ind_dim} {name}: max error / max magnitude = {err:.3e}")
        assert err <= 1e-6, name
    assert np.array_equal(got[150:], np.zeros(2, np.float32))
