"""Float64 restatement of the fused training head with 16-bit matrix products (RN_TRAIN_MLP=f16, csrc/rn_train_head_f16.hip),
built on netref64.Net64, for tests.  It states the arithmetic of that mode and nothing of its kernels:

* the weights of the 64-row contractions -- W_amb0[:, 0:32], W_amb1, W_sig0[:, 0:64], W_sig1, W_sig2[1:65], W_col0[:, 0:80] --
  are rounded to half (nearest even); so is every input of such a contraction (grid features, SH basis, the previous layer's
  activations).  Products and sums are float64;
* the weight gradients see the unrounded operands: dW = dZ X^T with the unrounded X and dZ;
* in the backward pass dX = W^T dY with the rounded W, and the dY of each 32-sample tile (rows 32 t .. 32 t + 31, in sample
  order) is multiplied by the power of two that brings its largest magnitude into [2^14, 2^15), rounded to half and divided
  again; a tile whose dY is zero gives zero;
* the columns of the per-call constants (audio code, eye, individual code) are float64 products with unrounded weights (the
  kernels fold them into fp32 biases), the narrow layers (W_amb2, W_sig2[0], W_col1), the grids, SH and the activations are
  Net64's, and the gradient of the SH basis is taken with the unrounded W_col0[:, 0:16] and the unrounded dZ (the kernels'
  input-gradient launch reads the fp32 image and the fp32 workspace).

After a forward, `unstable` [N] marks the samples with a hidden pre-activation smaller in magnitude than 2^-9 times the sum of
the magnitudes of its products: one rounding of an operand could flip their ReLU mask."""
import torch

from netref64 import Net64, grid_encode, sh4

TILE = 32


def round_half(x):
    """x (float64) rounded to the nearest binary16 value, ties to even, subnormals kept, overflow to infinity -- in one rounding
    (a cast through float32 would round twice)."""
    _, e = torch.frexp(x)
    e = torch.clamp(e - 1, min=-14)                       # floor(log2 |x|), held at the subnormal exponent
    ulp = torch.ldexp(torch.ones_like(x), e - 10)
    r = torch.round(x / ulp) * ulp                        # torch.round: halves to even
    return torch.where(r.abs() >= 65520.0, torch.sign(r) * float("inf"), r)


def round_tiles(g):
    """g [N, K]: each tile of 32 rows scaled by a power of two so that its largest magnitude lies in [2^14, 2^15), rounded to
    half and unscaled; zero tiles stay zero."""
    n, k = g.shape
    pad = (-n) % TILE
    t = torch.cat([g, g.new_zeros(pad, k)]).reshape(-1, TILE * k)
    amax = t.abs().amax(-1, keepdim=True)
    _, e = torch.frexp(amax)
    e = torch.clamp(e - 1, min=-112, max=127)             # the kernels keep both factors normal fp32 numbers
    scale = torch.ldexp(torch.ones_like(amax), 14 - e)
    q = torch.where(amax > 0, round_half(t * scale) / scale, torch.zeros_like(t))
    return q.reshape(-1, k)[:n]


class _Lin16(torch.autograd.Function):
    """y = half(x) half(W)^T; backward: dx = tiles(dy) half(W) (the first `plain` columns: dy W), dW = dy^T x."""

    @staticmethod
    def forward(ctx, x, w, plain):
        ctx.save_for_backward(x, w)
        ctx.plain = plain
        return round_half(x) @ round_half(w).t()

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        gx = round_tiles(g) @ round_half(w)
        if ctx.plain:
            gx = torch.cat([g @ w[:, :ctx.plain], gx[:, ctx.plain:]], -1)
        return gx, g.t() @ x, None


HEAD = ("encoder", "encoder_ambient", "ambient_net", "sigma_net", "color_net")


def head_loss(sigma, rgb, amb, up):
    """The scalar the head tests differentiate: upstream gradients up = (sigma [N], rgb [N, 3], |ambient| sum [N], ambient [N, 2])."""
    return (sigma * up[0]).sum() + (rgb * up[1]).sum() + (amb.abs().sum(-1) * up[2]).sum() + (amb * up[3]).sum()


def run_reference(ref, xyzs, dirs, enc_a, eye, up, input_grads=False, row=0):
    """Outputs and every gradient of `ref` (a Net64 or a Net16) under head_loss: the head's parameters by their module names,
    "enc_a", "eye" (model with the eye input), "individual_codes" (model with the code, row `row` used), and "xyzs" / "dirs"
    with input_grads.  eye: [1, 1] or None."""
    m = ref.model
    leaves = {n: p for n, p in ref.P.items() if n.split(".")[0] in HEAD}
    leaves["enc_a"] = enc_a.double().clone().requires_grad_(True)
    e = c = None
    if m.exp_eye:
        e = leaves["eye"] = eye.double().clone().requires_grad_(True)
    if m.individual_dim:
        leaves["individual_codes"] = ref.P["individual_codes"]
        c = ref.P["individual_codes"][row]
    x, d = xyzs.double(), dirs.double()
    if input_grads:
        x, d = x.clone().requires_grad_(True), d.clone().requires_grad_(True)
        leaves["xyzs"], leaves["dirs"] = x, d
    sigma, rgb, amb = ref.forward(x, d, leaves["enc_a"], c, e)
    names = sorted(leaves)
    gs = torch.autograd.grad(head_loss(sigma, rgb, amb, [u.double() for u in up]), [leaves[n] for n in names])
    out = {"sigma": sigma.detach(), "rgb": rgb.detach(), "ambient": amb.detach()}
    return out, dict(zip(names, gs))


def max_normalised(a, ref):
    """max |a - ref| / max |ref|."""
    return float((a.double() - ref.double()).abs().max()) / (float(ref.double().abs().max()) + 1e-300)


# The models and batches of tests/test_gpu_train_head_f16.py, named here so that tests/test_netref16.py checks the same ones on
# the CPU.  tag -> default_opt overrides ("aud32": also audio_dim = 32 instead of 64)
MODELS = {"default": {}, "hash19": dict(xyz_grid="hashgrid", xyz_log2_hashmap_size=19), "noeye_noind": dict(exp_eye=False, ind_dim=0),
          "aud32": {}}
# (tag, M, live count or None, row-indexed individual code).  Tile edges 1 / 31 / 32 / 33 / 95 and a capacity of 64 with a device
# live count; the seed of a batch is 1600 + its position here
CASES = [("default", 1, None, False), ("default", 31, None, False), ("default", 32, None, False), ("default", 33, None, True),
         ("default", 95, None, False), ("default", 64, 1, False), ("default", 64, 40, True), ("hash19", 95, None, False),
         ("noeye_noind", 33, None, False), ("aud32", 33, None, False)]


def head_scene(tag, device):
    """The seeded synthetic scene of MODELS[tag] (no torso, 16 x 16 pixels: only its model is used)."""
    from radnerf.scene import SyntheticScene, default_opt
    opt = default_opt(engine="ops", torso=False, smooth_lips=False, **MODELS[tag])
    model = None
    torch.manual_seed(0)
    if tag == "aud32":
        from radnerf.network import NeRFNetwork
        model = NeRFNetwork(opt, audio_dim=32)
    return SyntheticScene(H=16, W=16, n_frames=8, device=device, opt=opt, model=model)


def stable_batch(ref, M, seed, oob=2):
    """A batch of M samples for the gradient comparisons, on the device of `ref` (a Net16), drawn with a CPU generator so that
    the same seed names the same batch everywhere.  Of a uniformly drawn sample ~90 % are `unstable` by Net16's rule (320 hidden
    units each), so the batch is picked from a pool of 24 M + 768 candidates with the model alone: the first candidates the rule lets through, with
    min(oob, M // 8) rows outside [-bound, bound] (zero grid features; kept whatever the rule says) behind the first of them.
    -> dict(xyzs, dirs, enc_a [1, audio_dim], eye [1, 1], up = upstream gradients (head_loss), excluded [M] bool: rows whose
    upstream gradients are zero because the rule excludes them, pool_excluded: the share of the uniformly drawn candidates the
    rule excludes).  A consequence the callers state next to their assertions: the gradients are compared on samples chosen to
    be well conditioned, and "at most one third excluded" holds for such a batch by construction."""
    m = ref.model
    dev = ref.P["encoder.embeddings"].device
    g = torch.Generator().manual_seed(seed)
    pool, n_oob = 24 * M + 768, min(oob, M // 8)
    xyzs = (torch.rand(pool, 3, generator=g) * 2 - 1) * 0.98
    xyzs[:n_oob] = 1.25
    dirs = torch.nn.functional.normalize(torch.randn(pool, 3, generator=g), dim=-1)
    enc_a = torch.randn(1, int(m.audio_dim), generator=g) * 0.5
    eye = torch.full((1, 1), 0.25)
    up = [torch.randn(pool, generator=g), torch.randn(pool, 3, generator=g), torch.randn(pool, generator=g) * 0.3,
          torch.randn(pool, 2, generator=g) * 0.3]
    xyzs, dirs, enc_a, eye = (t.to(dev) for t in (xyzs, dirs, enc_a, eye))
    with torch.no_grad():
        ref.forward(xyzs, dirs, enc_a.double(), ref.P["individual_codes"][0] if m.individual_dim else None,
                    eye.double() if m.exp_eye else None)
    free = torch.nonzero(~ref.unstable[n_oob:]).reshape(-1)[:M - n_oob] + n_oob
    assert free.numel() == M - n_oob, "the pool holds too few stable samples"
    rows = torch.cat([free[:1], torch.arange(n_oob, device=dev), free[1:]])   # a stable sample first: a live count of 1 keeps one
    excluded = ref.unstable[rows]
    keep = (~excluded).float()
    up = [u.to(dev)[rows] * (keep if u.dim() == 1 else keep.unsqueeze(-1)) for u in up]
    return dict(xyzs=xyzs[rows].contiguous(), dirs=dirs[rows].contiguous(), enc_a=enc_a, eye=eye, up=up, excluded=excluded,
                pool_excluded=float(ref.unstable[n_oob:].float().mean()))   # the rule's rate on the uniformly drawn candidates


class Net16(Net64):
    """Net64 with the 16-bit matrix products of RN_TRAIN_MLP=f16 in `forward` (forward_torso is Net64's)."""

    def _hidden(self, x, w, cols, const=None, plain=0):
        """Pre-activation of a 64-row layer: _Lin16 on the first `cols` columns + the float64 product of the constant's."""
        z = _Lin16.apply(x, w[:, :cols], plain)
        mag = round_half(x.detach()).abs() @ round_half(w[:, :cols].detach()).abs().t()
        if const is not None:
            c = const.reshape(1, -1).double()
            z = z + c @ w[:, cols:].t()
            mag = mag + c.detach().abs() @ w[:, cols:].detach().abs().t()
        self.unstable = self.unstable | (z.detach().abs() < 2.0 ** -9 * mag).any(-1)
        return z

    def forward(self, x, d, enc_a, c=None, e=None):
        m, P = self.model, self.P
        x, d = x.double(), d.double()
        self.unstable = torch.zeros(x.shape[0], dtype=torch.bool, device=x.device)
        a, s, cn = self._ws("ambient_net"), self._ws("sigma_net"), self._ws("color_net")
        enc_x = grid_encode(x, P["encoder.embeddings"], m.encoder, self.bound)
        h = torch.relu(self._hidden(enc_x, a[0], 32, enc_a))
        h = torch.relu(self._hidden(h, a[1], 64))
        ambient = torch.tanh(h @ a[2].t())
        enc_w = grid_encode(ambient, P["encoder_ambient.embeddings"], m.encoder_ambient, 1.0)
        h = torch.relu(self._hidden(torch.cat([enc_x, enc_w], -1), s[0], 64, e))
        h = torch.relu(self._hidden(h, s[1], 64))
        sigma = torch.exp(h @ s[2][0])
        geo = _Lin16.apply(h, s[2][1:], 0)
        h = torch.relu(self._hidden(torch.cat([sh4(d), geo], -1), cn[0], 80, c, plain=16))
        rgb = torch.sigmoid(h @ cn[1].t())
        return sigma, rgb, ambient
