"""The perceptual term of lip fine-tuning: lpips.LPIPS(net='alex') in eval mode (nerf/utils.py:649-650, 766, 781) and the metric
of LPIPSMeter (:438-466), as a frozen torch.nn.Module.

    crit = PerceptualAlex.from_lpips_state_dict(torch.load("alex_full.pth"))      # or from_parts(alexnet_sd, lin_sd)
    Trainer(model, opt, patch_criterion=crit.cuda())

forward(pred, target, normalize=False) -> [P,1,1,1] for [P,3,h,w] inputs in [0, 1] (normalize=True: both become 2x - 1 first, which
is what LPIPSMeter does with images in [0, 1]).  On a GPU in fp32 with RN_PERCEP=hip (the default) the value and the gradient
with respect to `pred` come from rn_percep_forward / rn_percep_backward (csrc/rn_percep.hip): about two dozen launches, no float
atomics.  Otherwise -- CPU tensors, another dtype, a `target` that requires grad, RN_PERCEP=torch -- the same arithmetic runs in
plain torch with the convolutions written as unfold + matmul.

The arithmetic: x' = (x - shift) / scale; five convolutions with bias and ReLU (3->64 k11 s4 p2 | 64->192 k5 p2 | 192->384 k3 p1 |
384->256 k3 p1 | 256->256 k3 p1), conv2 and conv3 on the 3 x 3 / stride 2 max-pool of the tap before; per tap
n(x) = x / (sqrt(sum_c x^2) + 1e-10), d = sum_c lin[c] (n(x) - n(y))^2, mean over positions; the value is the sum over the taps.
Two decisions where torch's autograd is silent or NaN: at a position whose channels are all zero the kernels take d|x|/dx = 0
(torch's sqrt backward gives inf * 0 = NaN there, so does the torch path), and a pool window's gradient goes to its first maximum
in row-major order, as torch's does.  The smallest image is 31 x 31 (the second pool needs a 3 x 3 map): anything smaller is a
ValueError.

The key names of the loaders are written from the public layout of the `lpips` and `torchvision` packages; neither was available
when this was written, so identity with the package's numbers was NOT checked -- only identity with the arithmetic above.
Every tensor's shape is checked, and a missing or unexpected key is named.
"""
import ctypes as C

import torch

from . import switches

LAYERS = ((3, 64, 11, 4, 2), (64, 192, 5, 1, 2), (192, 384, 3, 1, 1), (384, 256, 3, 1, 1), (256, 256, 3, 1, 1))   # cin, cout, k, stride, pad
POOL_BEFORE = (False, True, True, False, False)
SHIFT, SCALE = (-.030, -.088, -.188), (.458, .448, .450)
MIN_SIDE = 31
_LPIPS_SLICES = ("net.slice1.0", "net.slice2.3", "net.slice3.6", "net.slice4.8", "net.slice5.10")
_ALEX_FEATURES = ("features.0", "features.3", "features.6", "features.8", "features.10")


def _check_images(pred, target):
    if pred.dim() != 4 or pred.shape[1] != 3 or pred.shape != target.shape or pred.shape[0] == 0:
        raise ValueError(f"PerceptualAlex: pred and target must be [P,3,h,w] with P >= 1, got {tuple(pred.shape)} and {tuple(target.shape)}")
    if pred.shape[2] < MIN_SIDE or pred.shape[3] < MIN_SIDE:
        raise ValueError(f"PerceptualAlex: {pred.shape[2]} x {pred.shape[3]} is below the smallest image, {MIN_SIDE} x {MIN_SIDE}")


def _take(sd, key, shape, used):
    if key not in sd:
        raise KeyError(f"PerceptualAlex: the state dict has no '{key}'")
    t = torch.as_tensor(sd[key])
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"PerceptualAlex: '{key}' has shape {tuple(t.shape)}, expected {tuple(shape)}")
    used.add(key)
    return t.detach().to(torch.float32)


class PerceptualAlex(torch.nn.Module):
    def __init__(self, weights=None, biases=None, lins=None, shift=SHIFT, scale=SCALE):
        """weights / biases: five conv tensors [Cout,Cin,k,k] / [Cout]; lins: five [1,C,1,1] (or [C]) vectors.  None: zeros, to be
        filled by a loader."""
        super().__init__()
        for l, (cin, cout, k, _, _) in enumerate(LAYERS):
            w = torch.zeros(cout, cin, k, k) if weights is None else torch.as_tensor(weights[l]).detach().float().reshape(cout, cin, k, k)
            b = torch.zeros(cout) if biases is None else torch.as_tensor(biases[l]).detach().float().reshape(cout)
            lin = torch.zeros(cout) if lins is None else torch.as_tensor(lins[l]).detach().float().reshape(cout)
            self.register_buffer(f"w{l + 1}", w.clone().contiguous())
            self.register_buffer(f"b{l + 1}", b.clone().contiguous())
            self.register_buffer(f"lin{l}", lin.clone().contiguous())
        self.register_buffer("shift_scale", torch.tensor(list(shift) + list(scale), dtype=torch.float32))
        self._image = None

    # ------------------------------------------------------------------------------------------------------------- loading
    def _set(self, weights, biases, lins, shift_scale=None):
        with torch.no_grad():
            for l in range(5):
                getattr(self, f"w{l + 1}").copy_(weights[l])
                getattr(self, f"b{l + 1}").copy_(biases[l])
                getattr(self, f"lin{l}").copy_(lins[l].reshape(-1))
            if shift_scale is not None:
                self.shift_scale.copy_(shift_scale)
        return self

    def load_lpips_state_dict(self, sd):
        """The key layout of lpips.LPIPS(net='alex').state_dict(): net.slice{1..5}.{0,3,6,8,10}.weight/bias,
        lin{0..4}.model.1.weight [1,C,1,1], optional scaling_layer.shift / scale [1,3,1,1]; duplicate `lins.*` entries are ignored."""
        used = set()
        ws = [_take(sd, f"{p}.weight", (co, ci, k, k), used) for p, (ci, co, k, _, _) in zip(_LPIPS_SLICES, LAYERS)]
        bs = [_take(sd, f"{p}.bias", (co,), used) for p, (ci, co, k, _, _) in zip(_LPIPS_SLICES, LAYERS)]
        lins = [_take(sd, f"lin{l}.model.1.weight", (1, LAYERS[l][1], 1, 1), used) for l in range(5)]
        ss = None
        if "scaling_layer.shift" in sd or "scaling_layer.scale" in sd:
            ss = torch.cat([_take(sd, "scaling_layer.shift", (1, 3, 1, 1), used).reshape(3), _take(sd, "scaling_layer.scale", (1, 3, 1, 1), used).reshape(3)])
        extra = sorted(k for k in sd if k not in used and not k.startswith("lins."))
        if extra:
            raise KeyError(f"PerceptualAlex: unexpected keys in the state dict: {extra}")
        return self._set(ws, bs, lins, ss)

    @classmethod
    def from_lpips_state_dict(cls, sd):
        return cls().load_lpips_state_dict(sd)

    @classmethod
    def from_parts(cls, alexnet_sd, lin_sd):
        """torchvision's AlexNet state dict (features.{0,3,6,8,10}.weight/bias; classifier.* ignored) plus the package's lin-only
        file (lin{0..4}.model.1.weight)."""
        used = set()
        ws = [_take(alexnet_sd, f"{p}.weight", (co, ci, k, k), used) for p, (ci, co, k, _, _) in zip(_ALEX_FEATURES, LAYERS)]
        bs = [_take(alexnet_sd, f"{p}.bias", (co,), used) for p, (ci, co, k, _, _) in zip(_ALEX_FEATURES, LAYERS)]
        extra = sorted(k for k in alexnet_sd if k not in used and not k.startswith("classifier."))
        if extra:
            raise KeyError(f"PerceptualAlex: unexpected keys in the AlexNet state dict: {extra}")
        used = set()
        lins = [_take(lin_sd, f"lin{l}.model.1.weight", (1, LAYERS[l][1], 1, 1), used) for l in range(5)]
        extra = sorted(k for k in lin_sd if k not in used and not k.startswith("lins."))
        if extra:
            raise KeyError(f"PerceptualAlex: unexpected keys in the lin state dict: {extra}")
        return cls()._set(ws, bs, lins)

    def lpips_state_dict(self):
        """The tensors under the package's key names (what load_lpips_state_dict reads)."""
        sd = {}
        for l, p in enumerate(_LPIPS_SLICES):
            sd[f"{p}.weight"], sd[f"{p}.bias"] = getattr(self, f"w{l + 1}").clone(), getattr(self, f"b{l + 1}").clone()
            sd[f"lin{l}.model.1.weight"] = getattr(self, f"lin{l}").reshape(1, -1, 1, 1).clone()
        sd["scaling_layer.shift"] = self.shift_scale[:3].reshape(1, 3, 1, 1).clone()
        sd["scaling_layer.scale"] = self.shift_scale[3:].reshape(1, 3, 1, 1).clone()
        return sd

    # ---------------------------------------------------------------------------------------------------------- torch path
    def taps_torch(self, x, normalize=False):
        """The five ReLU outputs of one batch of images [P,3,h,w]."""
        dt = x.dtype
        if normalize:
            x = 2 * x - 1
        ss = self.shift_scale.to(dt)
        x = (x - ss[:3].view(1, 3, 1, 1)) / ss[3:].view(1, 3, 1, 1)
        taps = []
        for l, (cin, cout, k, stride, pad) in enumerate(LAYERS):
            if POOL_BEFORE[l]:
                x = torch.nn.functional.max_pool2d(x, 3, 2)
            P, _, h, w = x.shape
            oh, ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
            cols = torch.nn.functional.unfold(x, k, padding=pad, stride=stride)
            x = getattr(self, f"w{l + 1}").to(dt).view(cout, -1) @ cols + getattr(self, f"b{l + 1}").to(dt).view(1, cout, 1)
            x = torch.relu(x.view(P, cout, oh, ow))
            taps.append(x)
        return taps

    def distance_torch(self, taps_x, taps_y):
        value = 0
        for l, (x, y) in enumerate(zip(taps_x, taps_y)):
            nx = x / (torch.sqrt((x * x).sum(1, keepdim=True)) + 1e-10)
            ny = y / (torch.sqrt((y * y).sum(1, keepdim=True)) + 1e-10)
            lin = getattr(self, f"lin{l}").to(x.dtype).view(1, -1, 1, 1)
            value = value + (lin * (nx - ny) ** 2).sum(1, keepdim=True).mean((2, 3), keepdim=True)
        return value

    def forward_torch(self, pred, target, normalize=False):
        return self.distance_torch(self.taps_torch(pred, normalize), self.taps_torch(target, normalize))

    # ------------------------------------------------------------------------------------------------------------ HIP path
    def packed_image(self):
        """The kernels' weight image, packed once per change of a tensor (its address or version)."""
        import radnerf_hip as hip
        tensors = [getattr(self, f"w{l + 1}") for l in range(5)] + [getattr(self, f"b{l + 1}") for l in range(5)]
        tensors += [getattr(self, f"lin{l}") for l in range(5)] + [self.shift_scale]
        key = tuple((t.data_ptr(), t._version) for t in tensors)
        if self._image is None or self._image[0] != key:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("PerceptualAlex: the weight image must be packed before a step is captured (call it once eagerly)")
            image = torch.empty(int(hip._lib.rn_percep_image_floats()), dtype=torch.float32, device=self.shift_scale.device)
            arrays = [(C.c_void_p * 5)(*[hip.ptr(t, torch.float32) for t in tensors[5 * i:5 * i + 5]]) for i in range(3)]
            hip.call("rn_percep_pack", arrays[0], arrays[1], arrays[2], hip.ptr(self.shift_scale), hip.ptr(image), hip.stream())
            self._image = (key, image)
        return self._image[1]

    def _hip_usable(self, pred, target):
        return (pred.is_cuda and target.is_cuda and pred.dtype == torch.float32 and target.dtype == torch.float32
                and self.shift_scale.is_cuda and not target.requires_grad and switches.get("RN_PERCEP") == "hip")

    def forward(self, pred, target, normalize=False):
        _check_images(pred, target)
        if self._hip_usable(pred, target):
            return _PercepFn.apply(pred, target, self, bool(normalize))
        return self.forward_torch(pred, target, normalize)


def _strides(t):
    """(image, pixel, channel) element strides of a [P,3,h,w] view whose rows are `w` pixels apart, or None."""
    s = t.stride()
    if s[2] != t.shape[3] * s[3] or min(s) < 0:
        return None
    return s[0], s[3], s[1]


def _strided(t):
    return t if _strides(t) is not None else t.contiguous()


class _PercepFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, module, normalize):
        import radnerf_hip as hip
        pred, target = _strided(pred.detach()), _strided(target.detach())
        P, _, h, w = pred.shape
        image = module.packed_image()
        nbytes = int(hip._lib.rn_percep_workspace(P, h, w))
        if nbytes == 0:
            raise ValueError(f"PerceptualAlex: unsupported shape P = {P}, {h} x {w}")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=pred.device)
        value = torch.empty(P, dtype=torch.float32, device=pred.device)
        hip.call("rn_percep_forward", hip.ptr(image), ws.data_ptr(), nbytes, pred.data_ptr(), *_strides(pred), target.data_ptr(),
                 *_strides(target), P, h, w, int(normalize), hip.ptr(value), hip.stream())
        ctx.saved = (image, ws, pred, normalize)
        return value.view(P, 1, 1, 1)

    @staticmethod
    def backward(ctx, grad_value):
        import radnerf_hip as hip
        image, ws, pred, normalize = ctx.saved
        P, _, h, w = pred.shape
        g_pred = torch.empty_like(pred)
        if _strides(g_pred) is None:
            g_pred = torch.empty(pred.shape, dtype=torch.float32, device=pred.device)
        up = grad_value.reshape(P)
        stride = 0 if (P == 1 or up.stride(0) == 0) else 1
        up = up if (stride == 0 or up.is_contiguous()) and up.dtype == torch.float32 else up.float().contiguous()
        hip.call("rn_percep_backward", hip.ptr(image), ws.data_ptr(), ws.numel(), up.data_ptr(), stride, g_pred.data_ptr(),
                 *_strides(g_pred), P, h, w, int(normalize), None, hip.stream())
        return g_pred, None, None, None
