"""Which samples the fp32 fused training head (RN_TRAIN_MLP=f32, csrc/rn_train_head.hip) may be compared on gradient by
gradient with float64, and batches made of them -- computed in float64 with netref64.Net64Libm and the model alone, for tests.

A per-sample gradient is discontinuous where a ReLU switches or where a coordinate crosses a cell boundary of a grid (the
grid's derivative is piecewise constant).  Two fp32 evaluations of the network -- the fused kernels, the operator path --
and float64 agree on the side only where the deciding quantity is farther from the switch than its fp32 error.  `unstable32`
marks a sample if any of these holds:

* ReLU: a hidden pre-activation z = sum_k x_k W_k satisfies |z| < 2^-15 sum_k |x_k W_k|.  An fp32 dot product of at most 128
  terms errs by at most 128 * 2^-24 = 2^-17 of the sum of the magnitudes of its products; its inputs carry the same error
  from up to three layers before; 2^-15 covers the four of them.
* ambient cells: an ambient coordinate (ambient + 1) / 2 lies within 2e-5 scale_l (lattice units; 2e-5 in normalised units)
  of a cell boundary of some level l of the 2-D grid -- the margin of tests/test_gpu_train_head.py::_stable_samples; an fp32
  ambient output differs from float64 by about 1e-6.
* xyz cells: a normalised xyz coordinate lies within 2e-6 scale_l of a cell boundary of some level of the 3-D grid: 30 times
  the fp32 rounding (2^-24) of the coordinate.  It guards the gradient of the sample positions.
* ReLU behind the ambient grid: with the ambient coordinates moved by 1e-6 (the size of an fp32 ambient output's error) along
  either diagonal, a hidden pre-activation of sigma_net or color_net changes sign or enters the ReLU margin.  The 2-D grid
  multiplies an error of the ambient coordinate by up to scale_15 / 2 = 1023 table differences before sigma_net sees it, which
  the 2^-15 margin of the first clause -- one layer's own rounding -- does not contain: of 131 105 samples that passed the
  first three clauses, one (|z| = 1.14 * 2^-15 of its products in sigma_net's second layer, the kernels' ambient 1.7e-8 =
  4 ulp from float64) took the other side of its ReLU in the fused kernels and moved the xyz table's gradient by 2.5 %.

`stable_batch32` picks a batch the way netref16.stable_batch does: a pool of 4 M + 256 uniformly drawn candidates (the rule
excludes 52 - 57 % of them, so the pool holds about 1.8 M stable ones), the first M the rule lets through, min(2, M // 8)
rows outside the bound behind the first of them.  The excluded rows of a batch (only out-of-bound rows the rule happens to
mark) get zero upstream gradients; outputs are compared on every row."""
import numpy as np
import torch

from netref64 import level_scale_libm, sh4

RELU_MARGIN, AMBIENT_MARGIN, XYZ_MARGIN, AMBIENT_ERROR = 2.0 ** -15, 2e-5, 2e-6, 1e-6
CHUNK = 65536


def near_cell_boundary(xn, enc, margin):
    """xn [N, D] float64 normalised coordinates -> [N] bool: some coordinate within margin * scale_l (lattice units) of an integer
    lattice position pos = xn * scale_l + 0.5 of some level l of GridEncoder `enc`."""
    S = float(np.log2(enc.per_level_scale))
    near = torch.zeros(xn.shape[0], dtype=torch.bool, device=xn.device)
    for l in range(int(enc.num_levels)):
        scale = float(level_scale_libm(l, S, int(enc.base_resolution))[0])
        pos = xn * scale + 0.5
        frac = pos - torch.floor(pos)
        near |= ((frac <= margin * scale) | (frac >= 1.0 - margin * scale)).any(-1)
    return near


def _layers(ref, net, x, const, relu_near, signs=None):
    """mlp(net) on cat[x, const] with the ReLU rule applied to every hidden pre-activation (relu_near is updated in place; the
    signs of the hidden pre-activations are appended to `signs`)."""
    ws = ref._ws(net)
    if const is not None:
        x = torch.cat([x, const.reshape(1, -1).double().expand(x.shape[0], -1)], -1)
    for i, w in enumerate(ws):
        z = x @ w.t()
        if i == len(ws) - 1:
            return z
        relu_near |= (z.abs() < RELU_MARGIN * (x.abs() @ w.abs().t())).any(-1)
        if signs is not None:
            signs.append(z > 0)
        x = torch.relu(z)


def _behind_ambient(ref, enc_x, ambient, sh, c, e, relu_near):
    """sigma_net and color_net on the ambient coordinates `ambient` -> the signs of their hidden pre-activations."""
    m, signs = ref.model, []
    enc_w = ref._grid(ambient, ref.P["encoder_ambient.embeddings"], m.encoder_ambient, 1.0)
    h = _layers(ref, "sigma_net", torch.cat([enc_x, enc_w], -1), e, relu_near, signs)
    _layers(ref, "color_net", torch.cat([sh, h[:, 1:]], -1), c, relu_near, signs)
    return torch.cat(signs, -1)


def unstable32(ref, x, d, enc_a, c=None, e=None):
    """The rule for samples (x, d) of Net64Libm `ref` -> dict(relu, ambient, xyz, relu_behind_ambient, any): [N] bool each.  enc_a [1, audio_dim], c: the
    individual code or None, e: [1, 1] or None (as Net64.forward)."""
    m, P = ref.model, ref.P
    parts = {k: [] for k in ("relu", "ambient", "xyz", "relu_behind_ambient")}
    with torch.no_grad():
        for at in range(0, x.shape[0], CHUNK):
            xc, dc = x[at:at + CHUNK].double(), d[at:at + CHUNK].double()
            relu = torch.zeros(xc.shape[0], dtype=torch.bool, device=xc.device)
            enc_x = ref._grid(xc, P["encoder.embeddings"], m.encoder, ref.bound)
            ambient = torch.tanh(_layers(ref, "ambient_net", enc_x, enc_a, relu))
            sh = sh4(dc)
            signs = _behind_ambient(ref, enc_x, ambient, sh, c, e, relu)
            moved = torch.zeros_like(relu)
            for s0, s1 in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
                shift = torch.tensor([s0, s1], dtype=torch.float64, device=xc.device) * AMBIENT_ERROR
                moved |= (_behind_ambient(ref, enc_x, ambient + shift, sh, c, e, moved) != signs).any(-1)
            parts["relu"].append(relu)
            parts["relu_behind_ambient"].append(moved)
            parts["ambient"].append(near_cell_boundary((ambient + 1.0) / 2.0, m.encoder_ambient, AMBIENT_MARGIN))
            parts["xyz"].append(near_cell_boundary((xc + ref.bound) / (2.0 * ref.bound), m.encoder, XYZ_MARGIN))
    out = {k: torch.cat(v) for k, v in parts.items()}
    out["any"] = out["relu"] | out["ambient"] | out["xyz"] | out["relu_behind_ambient"]
    return out


def stable_batch32(ref, M, seed, oob=2):
    """A batch of M samples on the device of `ref` (a Net64Libm), drawn with a CPU generator so that the same seed names the same
    batch everywhere.  -> dict(xyzs, dirs, enc_a [1, audio_dim], eye [1, 1], up = upstream gradients (netref16.head_loss),
    excluded [M] bool: rows whose upstream gradients are zero because the rule excludes them, pool_excluded: the share of the
    uniformly drawn candidates the rule excludes, shares: the same per rule).  "At most one third of the rows excluded" holds
    for such a batch by construction."""
    m = ref.model
    dev = ref.P["encoder.embeddings"].device
    g = torch.Generator().manual_seed(seed)
    pool, n_oob = 4 * M + 256, min(oob, M // 8)
    xyzs = (torch.rand(pool, 3, generator=g) * 2 - 1) * 0.98
    xyzs[:n_oob] = 1.25
    dirs = torch.nn.functional.normalize(torch.randn(pool, 3, generator=g), dim=-1)
    enc_a = torch.randn(1, int(m.audio_dim), generator=g) * 0.5
    eye = torch.full((1, 1), 0.25)
    up = [torch.randn(pool, generator=g), torch.randn(pool, 3, generator=g), torch.randn(pool, generator=g) * 0.3,
          torch.randn(pool, 2, generator=g) * 0.3]
    xyzs, dirs, enc_a, eye = (t.to(dev) for t in (xyzs, dirs, enc_a, eye))
    rule = unstable32(ref, xyzs, dirs, enc_a, ref.P["individual_codes"][0].detach() if m.individual_dim else None,
                      eye if m.exp_eye else None)
    bad = rule["any"]
    free = torch.nonzero(~bad[n_oob:]).reshape(-1)[:M - n_oob] + n_oob
    assert free.numel() == M - n_oob, "the pool holds too few stable samples"
    rows = torch.cat([free[:1], torch.arange(n_oob, device=dev), free[1:]])   # a stable sample first: a live count of 1 keeps one
    excluded = bad[rows]
    keep = (~excluded).float()
    up = [u.to(dev)[rows] * (keep if u.dim() == 1 else keep.unsqueeze(-1)) for u in up]
    return dict(xyzs=xyzs[rows].contiguous(), dirs=dirs[rows].contiguous(), enc_a=enc_a, eye=eye, up=up, excluded=excluded,
                pool_excluded=float(bad[n_oob:].float().mean()),
                shares={k: float(v[n_oob:].float().mean()) for k, v in rule.items()})
