"""Audio features from samples: the wav2vec2 CTC model the reference runs in nerf/asr.py, in its file mode, as a frozen
torch.nn.Module, plus the window loop around it restated as a pure function.

    asr = Wav2Vec2CTC.from_files("w2v.pth", "config.json").cuda()        # nothing is fetched: the user names the files
    feats = asr.features_from_samples(read_wav("intro.wav"))             # [F,16,C], the layout of aud_eo.npy
    python -m radnerf.asr --wav intro.wav --weights w2v.pth [--config config.json] [-l 10 -m 50 -r 10] [--resample] --out aud_eo.npy

The model is `transformers`' Wav2Vec2ForCTC with feat_extract_norm = "layer", conv_bias = True and do_stable_layer_norm = True in
eval mode without an attention mask (asr.py:324-328) -- the family both of the reference's --asr_model names belong to:

    input       one window: (x - mean) / sqrt(var + 1e-7), population variance (the processor's do_normalize)
    encoder     conv layers without padding, each + bias, LayerNorm over the channels, exact (erf) GELU
    projection  LayerNorm, Linear -> hidden
    position    h += GELU(conv(h)): K taps (even), G groups, padding K / 2, the last step dropped; the weight is weight-normed over
                dim 2 (w = v * g / |v|, the norm over dims (0, 1) per tap)
    layers      h += out_proj(attn(LN(h))); h += W2 GELU(W1 LN(h)); queries scaled by head_dim ** -0.5, softmax(Q K^T) V per head
    output      LayerNorm, lm_head: the raw logits [T, vocab], T = N - 1 for a window of N chunks of 320 samples

Any other variant is a ValueError naming the config field (`supported`).  On a GPU in fp32 with RN_ASR=hip forward and the
cut + unfold run in the kernels of csrc/rn_asr.hip (no float atomics: two calls give the same bits, and a window's logits do not
depend on which other windows share its launch); otherwise -- CPU tensors, float64, RN_ASR=torch -- the same arithmetic runs in
plain torch.  RN_ASR=torch is the default: at the real size the torch path measured faster (DESIGN.md section 3 has the numbers);
set RN_ASR=hip where the bits must not depend on the batching.  RN_ASR_TILE (auto | 32 | 128) names the tiling of the kernels' matrix
products: 32 x 32 tiles for the few rows of one window, 128 x 128 for a batch, chosen per product from its shape; the same bits either way.

The windows (asr.py:35-251): chunks of 320 samples, `l` zero chunks in front, a window whenever l + m + r chunks have collected,
the last l + r kept for the next; when the samples run out one terminal window over whatever is held.  Of a window's T logits
rows l .. min(T, T - r + 1) - 1 are kept (all from l on for the terminal window); the kept rows [M,C] are unfolded (window 16,
padding 8, stride 2) to [M // 2 + 1, 16, C].  The reference runs the model once per window, one after the other; the windows are
independent (each normalised on its own, none padded, no mask), so here all windows of one length go through the model together.
A terminal window shorter than the encoder's receptive field (400 samples) contributes no rows -- the reference would raise
inside the first convolution there.

The live loop around this model -- samples arriving 20 ms at a time, one window per m chunks into a ring of logits, one attention
window per video frame -- is radnerf/live.py.  Audio at another rate or in another sample format goes through radnerf/resample.py
first (--resample).  Microphone capture and playback, the text decode and DeepSpeech features are not built here.
"""
import ctypes as C
import json
import wave

import numpy as np
import torch
import torch.nn.functional as F

from . import switches

CHUNK = 320
SAMPLE_RATE = 16000
MAX_STEPS = 96                      # the attention kernel's longest sequence
LARGE = dict(conv_dim=[512] * 7, conv_kernel=[10, 3, 3, 3, 3, 2, 2], conv_stride=[5, 2, 2, 2, 2, 2, 2], hidden_size=1024,
             num_attention_heads=16, intermediate_size=4096, num_hidden_layers=24, num_conv_pos_embeddings=128,
             num_conv_pos_embedding_groups=16, vocab_size=44, layer_norm_eps=1e-5, feat_extract_norm="layer", conv_bias=True,
             do_stable_layer_norm=True)
_LAYER_PARTS = ("layer_norm", "attention.q_proj", "attention.k_proj", "attention.v_proj", "attention.out_proj", "final_layer_norm",
                "feed_forward.intermediate_dense", "feed_forward.output_dense")
_POS = "wav2vec2.encoder.pos_conv_embed.conv"


def normalized_config(config):
    """A dict or a transformers config -> the dict of the fields this module reads, defaults as Wav2Vec2Config has them."""
    get = (lambda k, d: config.get(k, d)) if isinstance(config, dict) else (lambda k, d: getattr(config, k, d))
    c = dict(conv_dim=list(get("conv_dim", LARGE["conv_dim"])), conv_kernel=list(get("conv_kernel", LARGE["conv_kernel"])),
             conv_stride=list(get("conv_stride", LARGE["conv_stride"])), hidden_size=int(get("hidden_size", 768)),
             num_attention_heads=int(get("num_attention_heads", 12)), intermediate_size=int(get("intermediate_size", 3072)),
             num_hidden_layers=int(get("num_hidden_layers", 12)), num_conv_pos_embeddings=int(get("num_conv_pos_embeddings", 128)),
             num_conv_pos_embedding_groups=int(get("num_conv_pos_embedding_groups", 16)), vocab_size=int(get("vocab_size", 32)),
             layer_norm_eps=float(get("layer_norm_eps", 1e-5)), feat_extract_norm=get("feat_extract_norm", "group"),
             conv_bias=bool(get("conv_bias", False)), do_stable_layer_norm=bool(get("do_stable_layer_norm", False)),
             add_adapter=bool(get("add_adapter", False)), feat_extract_activation=get("feat_extract_activation", "gelu"),
             hidden_act=get("hidden_act", "gelu"))
    return c


def supported(config):
    """The normalised config when the arithmetic above covers it; ValueError naming the field otherwise."""
    c = normalized_config(config)
    def no(field, why):
        raise ValueError(f"Wav2Vec2CTC: {field} = {c.get(field)!r}: {why}")
    if c["feat_extract_norm"] != "layer":
        no("feat_extract_norm", "only the 'layer' variant (a LayerNorm after every conv layer) is built, not group norm")
    if not c["do_stable_layer_norm"]:
        no("do_stable_layer_norm", "only the pre-norm (stable layer norm) encoder is built, not post-norm")
    if not c["conv_bias"]:
        no("conv_bias", "only conv layers with a bias are built")
    if c["add_adapter"]:
        no("add_adapter", "adapters are not built")
    if c["feat_extract_activation"] != "gelu":
        no("feat_extract_activation", "only the exact GELU is built")
    if c["hidden_act"] != "gelu":
        no("hidden_act", "only the exact GELU is built")
    n = len(c["conv_dim"])
    if not (1 <= n <= 8) or len(c["conv_kernel"]) != n or len(c["conv_stride"]) != n:
        no("conv_dim", "1 .. 8 conv layers, with one kernel and one stride each")
    if any(d <= 0 or d % 4 or d > 4096 for d in c["conv_dim"]):
        no("conv_dim", "every width must be a multiple of 4, at most 4096")
    if any(not 1 <= k <= 64 for k in c["conv_kernel"]):
        no("conv_kernel", "every kernel must be 1 .. 64")
    if any(not 1 <= s <= 64 for s in c["conv_stride"]):
        no("conv_stride", "every stride must be 1 .. 64")
    if c["num_conv_pos_embeddings"] < 2 or c["num_conv_pos_embeddings"] % 2 or c["num_conv_pos_embeddings"] > 1024:
        no("num_conv_pos_embeddings", "only an even K (the last output step is dropped) up to 1024 is built")
    if c["num_attention_heads"] < 1 or c["hidden_size"] != 64 * c["num_attention_heads"] or c["hidden_size"] > 8192:
        no("num_attention_heads", f"hidden_size / num_attention_heads must be 64 (hidden_size = {c['hidden_size']}), the attention kernel's head width")
    g = c["num_conv_pos_embedding_groups"]
    if g < 1 or c["hidden_size"] % g or (c["hidden_size"] // g) % 4:
        no("num_conv_pos_embedding_groups", "hidden_size / groups must be a multiple of 4")
    if c["intermediate_size"] < 4 or c["intermediate_size"] % 4 or c["intermediate_size"] > 32768:
        no("intermediate_size", "must be a multiple of 4, at most 32768")
    if not 1 <= c["num_hidden_layers"] <= 128:
        no("num_hidden_layers", "must be 1 .. 128")
    if not 1 <= c["vocab_size"] <= 65536:
        no("vocab_size", "must be 1 .. 65536")
    if not 0 < c["layer_norm_eps"] < 1:
        no("layer_norm_eps", "must be in (0, 1)")
    return c


def tensor_names(c):
    """The state-dict keys in the order rn_asr_pack reads them; the positional conv under the older spelling."""
    names = []
    for i in range(len(c["conv_dim"])):
        p = f"wav2vec2.feature_extractor.conv_layers.{i}"
        names += [f"{p}.conv.weight", f"{p}.conv.bias", f"{p}.layer_norm.weight", f"{p}.layer_norm.bias"]
    names += ["wav2vec2.feature_projection.layer_norm.weight", "wav2vec2.feature_projection.layer_norm.bias",
              "wav2vec2.feature_projection.projection.weight", "wav2vec2.feature_projection.projection.bias"]
    names += [f"{_POS}.weight_g", f"{_POS}.weight_v", f"{_POS}.bias"]
    names += ["wav2vec2.encoder.layer_norm.weight", "wav2vec2.encoder.layer_norm.bias"]
    for l in range(c["num_hidden_layers"]):
        for part in _LAYER_PARTS:
            names += [f"wav2vec2.encoder.layers.{l}.{part}.weight", f"wav2vec2.encoder.layers.{l}.{part}.bias"]
    return names + ["lm_head.weight", "lm_head.bias"]


def tensor_shapes(c):
    shapes, cin = [], 1
    for d, k in zip(c["conv_dim"], c["conv_kernel"]):
        shapes += [(d, cin, k), (d,), (d,), (d,)]
        cin = d
    H, I, K, G, V = c["hidden_size"], c["intermediate_size"], c["num_conv_pos_embeddings"], c["num_conv_pos_embedding_groups"], c["vocab_size"]
    shapes += [(cin,), (cin,), (H, cin), (H,), (1, 1, K), (H, H // G, K), (H,), (H,), (H,)]
    layer = [(H,), (H,)] + [(H, H), (H,)] * 4 + [(H,), (H,), (I, H), (I,), (H, I), (H,)]
    return shapes + layer * c["num_hidden_layers"] + [(V, H), (V,)]


def frames_of(c, samples):
    """Logit rows of a window of `samples` samples (0: below the receptive field)."""
    t = int(samples)
    for k, s in zip(c["conv_kernel"], c["conv_stride"]):
        if t < k:
            return 0
        t = (t - k) // s + 1
    return t


def receptive_field(c):
    n = 1
    for k, s in zip(reversed(c["conv_kernel"]), reversed(c["conv_stride"])):
        n = (n - 1) * s + k
    return n


def plan_windows(n_samples, l=10, m=50, r=10, config=None):
    """One (samples, T, left, right) per window the reference's loop runs on n_samples samples, in order."""
    return [w[1:] for w in _windows(n_samples, l, m, r, supported(LARGE if config is None else config))]


def _windows(n_samples, l, m, r, c):
    """(first sample in the zero-padded stream, samples, T, left, right) per window."""
    n_samples, l, m, r = int(n_samples), int(l), int(m), int(r)
    if n_samples < 0 or l < 0 or r < 0 or m < 1:
        raise ValueError(f"plan_windows: n_samples = {n_samples}, l, m, r = {l}, {m}, {r} (n_samples, l, r >= 0; m >= 1)")
    total = l * CHUNK + n_samples
    chunks = l + -(-n_samples // CHUNK)
    size = l + m + r
    full = (chunks - size) // m + 1 if chunks >= size else 0
    out = []
    for j in range(full):
        samples = min((j * m + size) * CHUNK, total) - j * m * CHUNK
        T = frames_of(c, samples)
        out.append((j * m * CHUNK, samples, T, max(0, l), min(T, T - r + 1)))
    first = full * m
    samples = total - first * CHUNK
    if samples > 0:
        T = frames_of(c, samples)
        out.append((first * CHUNK, samples, T, max(0, l), T))
    return out


def unfold_rows(rows):
    """Kept logits [M,C] -> [M // 2 + 1, 16, C] (asr.py:238-243)."""
    M, Cc = rows.shape
    if M == 0:
        return rows.new_zeros(1, 16, Cc)
    u = F.unfold(rows.t().reshape(1, Cc, M, 1), kernel_size=(16, 1), padding=(8, 0), stride=(2, 1))
    return u.view(Cc, 16, -1).permute(2, 1, 0).contiguous()


def check_wav(path):
    """The header of a .wav this module can read (16 kHz PCM16) -> (channels, frames); ValueError otherwise.  Reads no samples."""
    try:
        with wave.open(path, "rb") as w:
            channels, width, rate, n, comp = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes(), w.getcomptype()
    except (wave.Error, EOFError) as e:
        raise ValueError(f"{path} is not a PCM .wav file ({e})") from None
    if comp != "NONE":
        raise ValueError(f"{path} is compressed ({comp}); only PCM16 is read")
    if width != 2:
        raise ValueError(f"{path} has {8 * width}-bit samples; only PCM16 is read")
    if rate != SAMPLE_RATE:
        raise ValueError(f"{path} is sampled at {rate} Hz; resample it to {SAMPLE_RATE} Hz first, or pass --resample (radnerf/resample.py)")
    return channels, n


def read_wav(path):
    """A 16 kHz PCM16 .wav -> float32 [N] in [-1, 1) (int16 / 32768), the first channel of several (one [WARN] line)."""
    channels, n = check_wav(path)
    with wave.open(path, "rb") as w:
        raw = w.readframes(n)
    x = np.frombuffer(raw, dtype="<i2").reshape(-1, channels)
    if channels > 1:
        print(f"[WARN] audio has {channels} channels, only use the first.")
    return (x[:, 0].astype(np.float32) / np.float32(32768)).copy()


def _take(sd, key, shape, used):
    if key not in sd:
        raise KeyError(f"Wav2Vec2CTC: the state dict has no '{key}'")
    t = torch.as_tensor(sd[key])
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"Wav2Vec2CTC: '{key}' has shape {tuple(t.shape)}, expected {tuple(shape)}")
    used.add(key)
    return t.detach().to(torch.float32)


class Wav2Vec2CTC(torch.nn.Module):
    def __init__(self, config):
        """Zero weights of the config's shapes, to be filled by a loader."""
        super().__init__()
        self.config = supported(config)
        self.names = tensor_names(self.config)
        for i, shape in enumerate(tensor_shapes(self.config)):
            self.register_buffer(f"t{i}", torch.zeros(shape))
        self._image = None

    # ------------------------------------------------------------------------------------------------------------- loading
    def load_hf_state_dict(self, sd):
        """The key layout of Wav2Vec2ForCTC.state_dict(); the positional conv's weight under `parametrizations.weight.original0 |
        original1` or the older `weight_g | weight_v`; wav2vec2.masked_spec_embed is ignored."""
        used = set()
        new = (f"{_POS}.parametrizations.weight.original0", f"{_POS}.parametrizations.weight.original1")
        rename = {f"{_POS}.weight_g": new[0], f"{_POS}.weight_v": new[1]} if new[0] in sd or new[1] in sd else {}
        tensors = [_take(sd, rename.get(name, name), shape, used) for name, shape in zip(self.names, tensor_shapes(self.config))]
        extra = sorted(k for k in sd if k not in used and k != "wav2vec2.masked_spec_embed")
        if extra:
            raise KeyError(f"Wav2Vec2CTC: unexpected keys in the state dict: {extra}")
        with torch.no_grad():
            for i, t in enumerate(tensors):
                getattr(self, f"t{i}").copy_(t)
        return self

    @classmethod
    def from_state_dict(cls, sd, config):
        return cls(config).load_hf_state_dict(sd)

    @classmethod
    def from_files(cls, weights, config_json=None):
        """weights: a torch.save'd state dict (or a .safetensors file when `safetensors` imports); config_json: the model's
        config.json.  Without one the large shape is taken, vocab_size read from lm_head.weight."""
        if str(weights).endswith(".safetensors"):
            try:
                from safetensors.torch import load_file
            except ImportError:
                raise ImportError(f"Wav2Vec2CTC: reading {weights} needs the `safetensors` package; torch.save the state dict instead") from None
            sd = load_file(str(weights))
        else:
            sd = torch.load(str(weights), map_location="cpu", weights_only=True)
        if config_json:
            with open(config_json, "r") as fh:
                config = json.load(fh)
        else:
            if "lm_head.weight" not in sd:
                raise KeyError("Wav2Vec2CTC: the state dict has no 'lm_head.weight'")
            config = dict(LARGE, vocab_size=int(sd["lm_head.weight"].shape[0]))
        return cls.from_state_dict(sd, config)

    def hf_state_dict(self, old_names=False):
        """The tensors under the package's key names (what load_hf_state_dict reads)."""
        sd = {name: getattr(self, f"t{i}").clone() for i, name in enumerate(self.names)}
        if not old_names:
            sd[f"{_POS}.parametrizations.weight.original0"] = sd.pop(f"{_POS}.weight_g")
            sd[f"{_POS}.parametrizations.weight.original1"] = sd.pop(f"{_POS}.weight_v")
        return sd

    def _tensors(self):
        return [getattr(self, f"t{i}") for i in range(len(self.names))]

    @property
    def vocab_size(self):
        return self.config["vocab_size"]

    # ---------------------------------------------------------------------------------------------------------- torch path
    def forward_torch(self, windows):
        c, dt = self.config, windows.dtype
        t = iter(w.to(dt) for w in self._tensors())
        eps = c["layer_norm_eps"]
        x = (windows - windows.mean(-1, keepdim=True)) / torch.sqrt(windows.var(-1, unbiased=False, keepdim=True) + 1e-7)
        h = x[:, None, :]
        for s in c["conv_stride"]:
            w, b, g, be = next(t), next(t), next(t), next(t)
            h = F.conv1d(h, w, b, stride=s)
            h = F.gelu(F.layer_norm(h.transpose(1, 2), (h.shape[1],), g, be, eps)).transpose(1, 2)
        h = h.transpose(1, 2)
        g, be, w, b = next(t), next(t), next(t), next(t)
        h = F.linear(F.layer_norm(h, (h.shape[-1],), g, be, eps), w, b)
        wg, wv, b = next(t), next(t), next(t)
        K = c["num_conv_pos_embeddings"]
        w = wv * (wg / wv.norm(dim=(0, 1), keepdim=True))
        pos = F.conv1d(h.transpose(1, 2), w, b, padding=K // 2, groups=c["num_conv_pos_embedding_groups"])[:, :, :-1]
        h = h + F.gelu(pos).transpose(1, 2)
        enc_g, enc_b = next(t), next(t)
        heads = c["num_attention_heads"]
        B, T, H = h.shape
        for _ in range(c["num_hidden_layers"]):
            p = [next(t) for _ in range(16)]
            y = F.layer_norm(h, (H,), p[0], p[1], eps)
            q = (F.linear(y, p[2], p[3]) * (H // heads) ** -0.5).view(B, T, heads, -1).transpose(1, 2)
            k = F.linear(y, p[4], p[5]).view(B, T, heads, -1).transpose(1, 2)
            v = F.linear(y, p[6], p[7]).view(B, T, heads, -1).transpose(1, 2)
            a = torch.softmax(q @ k.transpose(-1, -2), dim=-1) @ v
            h = h + F.linear(a.transpose(1, 2).reshape(B, T, H), p[8], p[9])
            y = F.layer_norm(h, (H,), p[10], p[11], eps)
            h = h + F.linear(F.gelu(F.linear(y, p[12], p[13])), p[14], p[15])
        h = F.layer_norm(h, (H,), enc_g, enc_b, eps)
        return F.linear(h, next(t), next(t))

    # ------------------------------------------------------------------------------------------------------------ HIP path
    def c_config(self):
        from radnerf_hip import abi
        c, cfg = self.config, None
        cfg = abi.AsrConfigT()
        cfg.n_conv = len(c["conv_dim"])
        for i in range(cfg.n_conv):
            cfg.conv_dim[i], cfg.conv_kernel[i], cfg.conv_stride[i] = c["conv_dim"][i], c["conv_kernel"][i], c["conv_stride"][i]
        cfg.hidden, cfg.heads, cfg.intermediate, cfg.layers = c["hidden_size"], c["num_attention_heads"], c["intermediate_size"], c["num_hidden_layers"]
        cfg.pos_taps, cfg.pos_groups, cfg.vocab, cfg.layer_norm_eps = c["num_conv_pos_embeddings"], c["num_conv_pos_embedding_groups"], c["vocab_size"], c["layer_norm_eps"]
        return cfg

    def packed_image(self):
        """The kernels' weight image, packed once per change of a tensor (its address or version)."""
        import radnerf_hip as hip
        tensors = self._tensors()
        key = tuple((t.data_ptr(), t._version) for t in tensors)
        if self._image is None or self._image[0] != key:
            cfg = self.c_config()
            n = int(hip._lib.rn_asr_image_floats(C.byref(cfg)))
            if n == 0:
                raise ValueError(f"Wav2Vec2CTC: the kernels do not take this config: {self.config}")
            image = torch.empty(n, dtype=torch.float32, device=tensors[0].device)
            ptrs = (C.c_void_p * len(tensors))(*[hip.ptr(t, torch.float32) for t in tensors])
            hip.call("rn_asr_pack", C.byref(cfg), ptrs, len(tensors), hip.ptr(image), hip.stream())
            self._image = (key, image)
        return self._image[1]

    def _hip_usable(self, windows):
        return windows.is_cuda and windows.dtype == torch.float32 and self.t0.is_cuda and switches.get("RN_ASR") == "hip"

    def workspace_bytes(self, B, samples):
        import radnerf_hip as hip
        return int(hip._lib.rn_asr_workspace(C.byref(self.c_config()), int(B), int(samples)))

    def forward_hip(self, windows, out=None, workspace=None):
        """workspace: a uint8 device tensor of at least workspace_bytes(B, S) bytes to run in (a caller that runs one window
        after the other keeps one); without it one is allocated per call.  RN_ASR_TILE names the tiling of the matrix
        products (auto: per product from its shape; the logits have the same bits under every value)."""
        import radnerf_hip as hip
        windows = windows.contiguous()
        B, S = windows.shape
        T = frames_of(self.config, S)
        nbytes = self.workspace_bytes(B, S)
        if nbytes == 0:
            raise ValueError(f"Wav2Vec2CTC: unsupported shape: {B} windows of {S} samples ({T} steps; the kernels take 1 .. {MAX_STEPS} steps)")
        image = self.packed_image()
        ws = workspace if workspace is not None and workspace.numel() >= nbytes else torch.empty(nbytes, dtype=torch.uint8, device=windows.device)
        if out is None:
            out = torch.empty(B, T, self.vocab_size, dtype=torch.float32, device=windows.device)
        tile = {"auto": 0, "32": 32, "128": 128}[switches.get("RN_ASR_TILE")]
        hip.call("rn_asr_forward_tile", C.byref(self.c_config()), hip.ptr(image), ws.data_ptr(), ws.numel(), hip.ptr(windows), B, S, hip.ptr(out),
                 tile, hip.stream())
        return out

    def forward(self, windows):
        """windows [B,S] -> logits [B,T,C]."""
        if windows.dim() != 2 or windows.shape[0] < 1:
            raise ValueError(f"Wav2Vec2CTC: windows must be [B,S] with B >= 1, got {tuple(windows.shape)}")
        if frames_of(self.config, windows.shape[1]) < 1:
            raise ValueError(f"Wav2Vec2CTC: a window of {windows.shape[1]} samples is below the receptive field, {receptive_field(self.config)}")
        with torch.no_grad():
            if self._hip_usable(windows):
                return self.forward_hip(windows)
            return self.forward_torch(windows)

    # ------------------------------------------------------------------------------------------------------------ features
    def default_max_batch(self, samples, cap_bytes=2 << 30):
        """Windows per launch under a workspace cap; a function of the window length alone."""
        if not self.t0.is_cuda:
            return 16
        one = self.workspace_bytes(1, samples)
        return max(1, min(4096, cap_bytes // max(one, 1)))

    def features_from_samples(self, x, l=10, m=50, r=10, max_batch=None, layout="F16C"):
        """Samples [N] (a tensor or an array; float32 in [-1, 1)) -> features [F,16,C] on the module's device: every window the
        reference's loop would run, all windows of one length through the model together, at most max_batch at a time.
        layout="FC16": the same values as [F,C,16], the layout the renderer reads."""
        dev = self.t0.device
        x = torch.as_tensor(x)
        x = x.to(dev, x.dtype if x.dtype == torch.float64 else torch.float32).reshape(-1)
        wins = [w for w in _windows(x.numel(), l, m, r, self.config)]
        stream = torch.cat([x.new_zeros(int(l) * CHUNK), x])
        Cv = self.vocab_size
        groups = []                                   # runs of windows of one length: [samples, T, left, right, [first sample, ...]]
        for first, samples, T, left, right in wins:
            if T < 1:
                continue
            if groups and groups[-1][:4] == [samples, T, left, right]:
                groups[-1][4].append(first)
            else:
                groups.append([samples, T, left, right, [first]])
        rows_total = sum(g[1] * len(g[4]) for g in groups)
        hip_path = self._hip_usable(stream)
        logits = torch.empty(max(rows_total, 1), Cv, dtype=stream.dtype, device=dev)
        segments, at = [], 0
        with torch.no_grad():
            for samples, T, left, right, firsts in groups:
                segments.append((at, len(firsts), T, min(left, right), right))
                step = int(max_batch) if max_batch else self.default_max_batch(samples)
                for i in range(0, len(firsts), step):
                    batch = torch.stack([stream[f:f + samples] for f in firsts[i:i + step]])
                    out = logits[at:at + len(batch) * T].view(len(batch), T, Cv)
                    if hip_path:
                        self.forward_hip(batch, out=out)
                    else:
                        out.copy_(self.forward_torch(batch))
                    at += len(batch) * T
            M = sum(n * (right - left) for _, n, _, left, right in segments)
            if hip_path and len(segments) <= 4 and segments:
                import radnerf_hip as hip
                feats = torch.empty(M // 2 + 1, Cv, 16, dtype=torch.float32, device=dev)
                flat = (C.c_uint32 * (5 * len(segments)))(*[v for s in segments for v in s])
                hip.call("rn_asr_features", hip.ptr(logits), logits.shape[0], Cv, flat, len(segments), hip.ptr(feats), M // 2 + 1, hip.stream())
                return feats if layout == "FC16" else feats.permute(0, 2, 1)
            kept = [logits[a:a + n * T].view(n, T, Cv)[:, left:right].reshape(-1, Cv) for a, n, T, left, right in segments]
            rows = torch.cat(kept) if kept else logits[:0]
            feats = unfold_rows(rows)
        return feats.permute(0, 2, 1).contiguous() if layout == "FC16" else feats


def main(argv=None, log=print):
    """python -m radnerf.asr --wav F --weights W [--config J] [-l -m -r] --out aud_eo.npy: the file asr.py:390-420 writes."""
    import argparse
    p = argparse.ArgumentParser(prog="python -m radnerf.asr", description="wav2vec2 CTC logits of a .wav, as the [F,16,C] file --aud reads")
    p.add_argument("--wav", type=str, required=True)
    p.add_argument("--weights", type=str, required=True, help="state dict of Wav2Vec2ForCTC; nothing is fetched")
    p.add_argument("--config", type=str, default="", help="the model's config.json (default: the large shape)")
    p.add_argument("-l", type=int, default=10)
    p.add_argument("-m", type=int, default=50)
    p.add_argument("-r", type=int, default=10)
    p.add_argument("--out", type=str, required=True)
    p.add_argument("--resample", action="store_true", help="take any PCM or float .wav, resampled to 16 kHz (radnerf/resample.py)")
    opt = p.parse_args(argv)
    if opt.resample:
        from .resample import samples_16k
        x = samples_16k(opt.wav, "cuda" if torch.cuda.is_available() else "cpu")
    else:
        x = read_wav(opt.wav)
    model = Wav2Vec2CTC.from_files(opt.weights, opt.config or None)
    if torch.cuda.is_available():
        model = model.cuda()
    feats = model.features_from_samples(x, opt.l, opt.m, opt.r).cpu().numpy()
    np.save(opt.out, feats)
    log(f"[INFO] saved logits to {opt.out}: {feats.shape}")
    return feats


if __name__ == "__main__":
    import sys
    main(sys.argv[1:])
