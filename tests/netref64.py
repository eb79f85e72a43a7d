"""Float64 restatement of NeRFNetwork.forward and forward_torso (nerf/network.py:188-283), written from the math, for tests.

    ref = Net64(model)                             # float64 leaf copies of the module's parameters, on the module's device
    sigma, rgb, ambient = ref.forward(x, d, enc_a, c, e)        # c: individual code [ind_dim] or None; e: [1, 1] or None
    alpha, color, dx = ref.forward_torso(xy, poses6, ct)
    grads = torch.autograd.grad(loss, [ref.P[name], ...])       # float64 autograd: every parameter, the tables, enc_a, e, c

Grid encoding: the normalised coordinate, the lattice position and the cell are computed in fp32 exactly as the kernels do
(gridencoder.cu: pos = x * scale + 0.5, scale = exp2f(level * S) * H - 1), so both sides pick the same corners and weights
(on the finest levels one fp32 ulp of `pos` is 1.2e-4 of a cell: a float64 position would be a different function); the row of
a corner comes from the tiled / hash rule (`grid_rows`, the vector form of `py_grid_index`).  The fractional position enters
with derivative `scale` in the coordinate.  The interpolation and everything after it -- the
bias-free MLPs, ReLU, tanh, exp (trunc_exp's forward), sigmoid, SH of degree 4, the frequency encodings -- are float64.
An input outside [0, 1] (normalised) gives zero features, as in the kernels.
"""
import ctypes

import numpy as np
import torch

_EXP2F = ctypes.CDLL("libm.so.6").exp2f
_EXP2F.restype, _EXP2F.argtypes = ctypes.c_float, [ctypes.c_float]

PRIMES = [1, 2654435761, 805459861, 3674653429, 2097192037, 1434869437, 2165219737]


def py_grid_index(D, C, gridtype, align_corners, ch, hashmap_size, resolution, pos_grid):
    """gridencoder.cu:66-84 with Python ints, wrapping to uint32 explicitly."""
    M = 1 << 32
    stride, index, d = 1, 0, 0
    while d < D and stride <= hashmap_size:
        index = (index + pos_grid[d] * stride) % M
        stride = (stride * (resolution if align_corners else resolution + 1)) % M
        d += 1
    if gridtype == 0 and stride > hashmap_size:
        index = 0
        for i in range(D):
            index ^= (pos_grid[i] * PRIMES[i]) % M
    return (index % hashmap_size) * C + ch


def torch_grid(x, emb, off, S, H, D, C, L, gridtype, interp):
    """Pure-torch float64 formulation (differentiable in emb and x) using the Python integer indices."""
    outs = []
    for l in range(L):
        scale = float(np.float32(np.exp2(np.float32(np.float32(l) * np.float32(S)))) * np.float32(H) - np.float32(1))
        res = int(np.ceil(scale)) + 1
        hs = int(off[l + 1] - off[l])
        pos = x * scale + 0.5
        p0 = torch.floor(pos).detach()
        fr = pos - p0
        if interp == 1:
            fr = fr * fr * (3 - 2 * fr)
        acc = 0
        p0n = p0.long().numpy()
        for corner in range(1 << D):
            w = 1
            pg = p0n.copy()
            for d in range(D):
                bit = (corner >> d) & 1
                w = w * (fr[:, d] if bit else 1 - fr[:, d])
                pg[:, d] += bit
            rows = np.array([py_grid_index(D, 1, gridtype, False, 0, hs, res, [int(v) for v in r]) for r in pg])
            acc = acc + w[:, None] * emb[off[l] + torch.from_numpy(rows)]
        outs.append(acc)
    return torch.stack(outs, 0)  # [L,B,C]


def level_scale(l, S, H):
    """(scale, resolution) of level l in fp32 arithmetic with numpy's float32 exp2.  Not quite the library's: see level_scale_libm."""
    scale = np.float32(np.exp2(np.float32(np.float32(l) * np.float32(S)))) * np.float32(H) - np.float32(1)
    return scale, int(np.ceil(scale)) + 1


def level_scale_libm(l, S, H):
    """(scale, resolution) of level l as the library computes them on the host (make_level_consts, csrc/rn_grid_dev.h): libm's
    exp2f.  numpy's float32 exp2 is another function -- one ulp away on levels 1, 3, 6, 9 and 12 of a 16 -> 2048 grid, which moves
    a lattice position by up to 1e-4 of a cell and puts every fp32 gradient upstream of a grid 1e-4 .. 2e-2 from a float64
    reference built on it.  Net64Libm uses this one; Net64 and the tests written against it keep level_scale, with which their
    bars were measured (moving them is a change of its own: tests/test_gpu_train_camera.py's 4 e_ops bar at M = 31 holds only
    because both of its errors are that discrepancy)."""
    scale = np.float32(_EXP2F(np.float32(l) * np.float32(S))) * np.float32(H) - np.float32(1)
    return scale, int(np.ceil(scale)) + 1


def grid_rows(pg, gridtype, hashmap_size, resolution):
    """py_grid_index (align_corners off, C = 1, ch = 0) over an int64 tensor of lattice points [N, D]."""
    M = 1 << 32
    D = pg.shape[1]
    stride, index, d = 1, torch.zeros_like(pg[:, 0]), 0
    while d < D and stride <= hashmap_size:
        index = (index + pg[:, d] * stride) % M
        stride = (stride * (resolution + 1)) % M
        d += 1
    if gridtype == 0 and stride > hashmap_size:
        index = torch.zeros_like(pg[:, 0])
        for i in range(D):
            index = index ^ ((pg[:, i] * PRIMES[i]) % M)
    return index % hashmap_size


def grid_encode(x, table, enc, bound, scale_of=level_scale):
    """GridEncoder(x, bound) [N, L*C] in float64; x [N, D] (float64, may require grad), table [rows, C] float64; scale_of:
    level_scale or level_scale_libm."""
    D, L, H = int(enc.input_dim), int(enc.num_levels), int(enc.base_resolution)
    S = float(np.log2(enc.per_level_scale))
    gridtype = int(enc.gridtype_id)
    off = [int(v) for v in enc.offsets.tolist()]
    bound32 = torch.tensor(bound, dtype=torch.float32)
    xn32 = (x.detach().float() + bound32) / (2 * bound32)             # gridencoder/grid.py: (inputs + bound) / (2 * bound)
    xn = (x + bound) / (2 * bound)
    inside = ((xn32 >= 0) & (xn32 <= 1)).all(-1, keepdim=True).to(torch.float64)
    outs = []
    for l in range(L):
        scale, res = scale_of(l, S, H)
        pos32 = xn32 * torch.tensor(scale) + torch.tensor(np.float32(0.5))
        cell = torch.floor(pos32)
        # the fp32 fractional position as value (what the kernels interpolate with), d/dx = scale as derivative
        fr = (pos32 - cell).double() + (xn - xn.detach()) * float(scale)
        p0 = cell.long()
        acc = 0
        for corner in range(1 << D):
            w = 1
            pg = p0.clone()
            for d in range(D):
                bit = (corner >> d) & 1
                w = w * (fr[:, d] if bit else 1 - fr[:, d])
                pg[:, d] += bit
            rows = off[l] + grid_rows(pg, gridtype, off[l + 1] - off[l], res)
            acc = acc + w.unsqueeze(-1) * table[rows]
        outs.append(acc)
    return torch.cat(outs, -1) * inside


def sh4(d):
    """Real spherical harmonics of degree 4 (16 values) of the (unit) directions d [N, 3], closed form."""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xy, yz, xz, x2, y2, z2 = x * y, y * z, x * z, x * x, y * y, z * z
    return torch.stack([
        torch.full_like(x, 0.28209479177387814),
        -0.48860251190291987 * y, 0.48860251190291987 * z, -0.48860251190291987 * x,
        1.0925484305920792 * xy, -1.0925484305920792 * yz, 0.94617469575755997 * z2 - 0.31539156525251999,
        -1.0925484305920792 * xz, 0.54627421529603959 * x2 - 0.54627421529603959 * y2,
        0.59004358992664352 * y * (-3.0 * x2 + y2), 2.8906114426405538 * xy * z, 0.45704579946446572 * y * (1.0 - 5.0 * z2),
        0.3731763325901154 * z * (5.0 * z2 - 3.0), 0.45704579946446572 * x * (1.0 - 5.0 * z2), 1.4453057213202769 * z * (x2 - y2),
        0.59004358992664352 * x * (-x2 + 3.0 * y2)], -1)


def freq(x, n_freqs):
    """FreqEncoder: [x, sin(x), cos(x), sin(2x), cos(2x), ..., sin(2^(n-1) x), cos(2^(n-1) x)], each block [N, D]."""
    parts = [x]
    for f in range(n_freqs):
        parts += [torch.sin(x * 2.0 ** f), torch.cos(x * 2.0 ** f)]
    return torch.cat(parts, -1)


def mlp(ws, x):
    for i, w in enumerate(ws):
        x = x @ w.t()
        if i != len(ws) - 1:
            x = torch.relu(x)
    return x


class Net64:
    """Float64 copies of a NeRFNetwork's parameters (leaves that require grad: self.P[name]) and its forward passes."""

    def __init__(self, model, device=None):
        dev = device if device is not None else model.encoder.embeddings.device
        self.model = model
        self.bound = float(model.bound)
        self.P = {n: p.detach().to(dev, torch.float64).requires_grad_(True) for n, p in model.named_parameters()}

    def _grid(self, x, table, enc, bound):
        return grid_encode(x, table, enc, bound)

    def _ws(self, net):
        out, l = [], 0
        while f"{net}.net.{l}.weight" in self.P:
            out.append(self.P[f"{net}.net.{l}.weight"])
            l += 1
        return out

    def forward(self, x, d, enc_a, c=None, e=None):
        """(sigma [N], rgb [N, 3], ambient [N, 2]) = NeRFNetwork.forward(x, d, enc_a, c, e); enc_a [1, audio_dim]."""
        m, P = self.model, self.P
        x, d = x.double(), d.double()
        n = x.shape[0]
        enc_x = self._grid(x, P["encoder.embeddings"], m.encoder, self.bound)
        ambient = torch.tanh(mlp(self._ws("ambient_net"), torch.cat([enc_x, enc_a.reshape(1, -1).double().expand(n, -1)], -1)))
        enc_w = self._grid(ambient, P["encoder_ambient.embeddings"], m.encoder_ambient, 1.0)
        cols = [enc_x, enc_w] + ([e.reshape(1, -1).double().expand(n, -1)] if e is not None else [])
        h = mlp(self._ws("sigma_net"), torch.cat(cols, -1))
        sigma = torch.exp(h[:, 0])
        cols = [sh4(d), h[:, 1:]] + ([c.reshape(1, -1).double().expand(n, -1)] if c is not None else [])
        rgb = torch.sigmoid(mlp(self._ws("color_net"), torch.cat(cols, -1)))
        return sigma, rgb, ambient

    def forward_torso(self, x, poses, c=None):
        """(alpha [N, 1], color [N, 3], dx [N, 2]) = NeRFNetwork.forward_torso(x, poses, enc_a, c); x [N, 2] in [-1, 1]."""
        m, P = self.model, self.P
        n = x.shape[0]
        x = x.double() * float(np.float32(m.opt.torso_shrink))
        enc_pose = freq(poses.reshape(1, -1).double(), 4).expand(n, -1)
        enc_x = freq(x, 10)
        cols = [enc_x, enc_pose] + ([c.reshape(1, -1).double().expand(n, -1)] if c is not None else [])
        h = torch.cat(cols, -1)
        dx = mlp(self._ws("torso_deform_net"), h)
        xt = (x + dx).clamp(-1, 1)
        enc_t = self._grid(xt, P["torso_encoder.embeddings"], m.torso_encoder, 1.0)
        out = mlp(self._ws("torso_net"), torch.cat([enc_t, h], -1))
        return torch.sigmoid(out[:, :1]), torch.sigmoid(out[:, 1:]), dx


class Net64Libm(Net64):
    """Net64 with the level scales the library itself computes (level_scale_libm): the reference of tests/test_gpu_train_head_ref.py."""

    def _grid(self, x, table, enc, bound):
        return grid_encode(x, table, enc, bound, level_scale_libm)
