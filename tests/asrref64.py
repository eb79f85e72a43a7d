"""float64 restatement of the wav2vec2 CTC model radnerf/asr.py runs (Wav2Vec2ForCTC, feat_extract_norm = "layer", conv_bias,
do_stable_layer_norm, eval mode, no mask) and of the reference's window loop (nerf/asr.py:185-251) written chunk by chunk like
run_step.  Plain torch functional calls; nothing but torch and numpy is imported, and nothing of the product.

    forward(sd, cfg, windows[B,S])            -> logits [B,T,C] float64
    features(sd, cfg, x[N], l, m, r)          -> ([F,16,C] float64, [(samples, T, left, right), ...])
    random_state_dict(cfg, seed, old_names)   -> a state dict under Wav2Vec2ForCTC's key names, values exact in float16
"""
import numpy as np
import torch
import torch.nn.functional as F

CHUNK = 320
POS = "wav2vec2.encoder.pos_conv_embed.conv"
TINY = dict(conv_dim=[32] * 7, conv_kernel=[10, 3, 3, 3, 3, 2, 2], conv_stride=[5, 2, 2, 2, 2, 2, 2], hidden_size=128,
            num_attention_heads=2, intermediate_size=128, num_hidden_layers=2, num_conv_pos_embeddings=8,
            num_conv_pos_embedding_groups=2, vocab_size=44, layer_norm_eps=1e-5, feat_extract_norm="layer", conv_bias=True,
            do_stable_layer_norm=True)


def _ln(x, sd, prefix, eps):
    w, b = sd[prefix + ".weight"].double(), sd[prefix + ".bias"].double()
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def _lin(x, sd, prefix):
    return x @ sd[prefix + ".weight"].double().t() + sd[prefix + ".bias"].double()


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / np.sqrt(2.0)))


def forward(sd, cfg, windows):
    x = torch.as_tensor(windows).double()
    eps = cfg["layer_norm_eps"]
    mu = x.mean(-1, keepdim=True)
    x = (x - mu) / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + 1e-7)
    h = x[:, None, :]                                                   # [B, C, T]
    for i, s in enumerate(cfg["conv_stride"]):
        p = f"wav2vec2.feature_extractor.conv_layers.{i}"
        h = F.conv1d(h, sd[p + ".conv.weight"].double(), sd[p + ".conv.bias"].double(), stride=s)
        h = _gelu(_ln(h.transpose(1, 2), sd, p + ".layer_norm", eps)).transpose(1, 2)
    h = h.transpose(1, 2)                                               # [B, T, C]
    h = _lin(_ln(h, sd, "wav2vec2.feature_projection.layer_norm", eps), sd, "wav2vec2.feature_projection.projection")
    if POS + ".weight_g" in sd:
        g, v = sd[POS + ".weight_g"].double(), sd[POS + ".weight_v"].double()
    else:
        g, v = sd[POS + ".parametrizations.weight.original0"].double(), sd[POS + ".parametrizations.weight.original1"].double()
    w = v * g / torch.sqrt((v * v).sum((0, 1), keepdim=True))
    K, G = cfg["num_conv_pos_embeddings"], cfg["num_conv_pos_embedding_groups"]
    assert K % 2 == 0
    pos = F.conv1d(h.transpose(1, 2), w, sd[POS + ".bias"].double(), padding=K // 2, groups=G)[:, :, :-1]
    h = h + _gelu(pos).transpose(1, 2)
    B, T, H = h.shape
    nh = cfg["num_attention_heads"]
    hd = H // nh
    for l in range(cfg["num_hidden_layers"]):
        p = f"wav2vec2.encoder.layers.{l}"
        y = _ln(h, sd, p + ".layer_norm", eps)
        q = (_lin(y, sd, p + ".attention.q_proj") * hd ** -0.5).view(B, T, nh, hd).transpose(1, 2)
        k = _lin(y, sd, p + ".attention.k_proj").view(B, T, nh, hd).transpose(1, 2)
        v = _lin(y, sd, p + ".attention.v_proj").view(B, T, nh, hd).transpose(1, 2)
        a = torch.softmax(q @ k.transpose(-1, -2), dim=-1) @ v
        h = h + _lin(a.transpose(1, 2).reshape(B, T, H), sd, p + ".attention.out_proj")
        y = _ln(h, sd, p + ".final_layer_norm", eps)
        h = h + _lin(_gelu(_lin(y, sd, p + ".feed_forward.intermediate_dense")), sd, p + ".feed_forward.output_dense")
    h = _ln(h, sd, "wav2vec2.encoder.layer_norm", eps)
    return _lin(h, sd, "lm_head")


def min_samples(cfg):
    n = 1
    for k, s in zip(reversed(cfg["conv_kernel"]), reversed(cfg["conv_stride"])):
        n = (n - 1) * s + k
    return n


def features(sd, cfg, x, l=10, m=50, r=10, model=None):
    """The reference's loop, one chunk at a time.  model: another `windows[1,S] -> logits[1,T,C]` (default: forward above)."""
    x = np.asarray(x, dtype=np.float64)
    model = (lambda w: forward(sd, cfg, w)) if model is None else model
    frames = [np.zeros(CHUNK)] * l
    idx, terminated, kept, windows = 0, False, [], []
    while not terminated:
        frame = x[idx:idx + CHUNK] if idx < x.shape[0] else None              # get_audio_frame
        idx += CHUNK
        if frame is None:
            terminated = True
        else:
            frames.append(frame)
            if len(frames) < l + m + r:
                continue
        inputs = np.concatenate(frames) if frames else np.zeros(0)
        if not terminated:
            frames = frames[-(l + r):] if l + r > 0 else []
        if inputs.shape[0] < min_samples(cfg):                              # the reference would raise in the first convolution
            windows.append((int(inputs.shape[0]), 0, max(0, l), 0))
            continue
        logits = model(torch.from_numpy(inputs)[None])[0]
        T = logits.shape[0]
        left = max(0, l)
        right = T if terminated else min(T, T - r + 1)
        windows.append((int(inputs.shape[0]), int(T), left, int(right)))
        kept.append(logits[left:right])
    C = cfg["vocab_size"]
    rows = torch.cat(kept) if kept else torch.zeros(0, C, dtype=torch.float64)
    M = rows.shape[0]
    padded = torch.cat([rows.new_zeros(8, C), rows, rows.new_zeros(8, C)])
    out = torch.stack([padded[2 * f:2 * f + 16] for f in range(M // 2 + 1)])   # window 16, padding 8, stride 2
    return out, windows


def shapes(cfg):
    out, cin = {}, 1
    for i, (d, k) in enumerate(zip(cfg["conv_dim"], cfg["conv_kernel"])):
        p = f"wav2vec2.feature_extractor.conv_layers.{i}"
        out[p + ".conv.weight"], out[p + ".conv.bias"] = (d, cin, k), (d,)
        out[p + ".layer_norm.weight"], out[p + ".layer_norm.bias"] = (d,), (d,)
        cin = d
    H, I, K, G, V = (cfg["hidden_size"], cfg["intermediate_size"], cfg["num_conv_pos_embeddings"], cfg["num_conv_pos_embedding_groups"],
                     cfg["vocab_size"])
    def lin(p, o, i):
        out[p + ".weight"], out[p + ".bias"] = (o, i), (o,)
    def ln(p, n):
        out[p + ".weight"], out[p + ".bias"] = (n,), (n,)
    ln("wav2vec2.feature_projection.layer_norm", cin)
    lin("wav2vec2.feature_projection.projection", H, cin)
    out[POS + ".weight_g"], out[POS + ".weight_v"], out[POS + ".bias"] = (1, 1, K), (H, H // G, K), (H,)
    ln("wav2vec2.encoder.layer_norm", H)
    for l in range(cfg["num_hidden_layers"]):
        p = f"wav2vec2.encoder.layers.{l}"
        ln(p + ".layer_norm", H)
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            lin(f"{p}.attention.{n}", H, H)
        ln(p + ".final_layer_norm", H)
        lin(p + ".feed_forward.intermediate_dense", I, H)
        lin(p + ".feed_forward.output_dense", H, I)
    lin("lm_head", V, H)
    return out


def random_state_dict(cfg, seed=0, old_names=True, dtype=torch.float32):
    """Weights of a plausible scale (fan-in scaled matrices, LayerNorm gains near 1), rounded to float16 values."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in shapes(cfg).items():
        if name.endswith("layer_norm.weight") or name.endswith("weight_g"):
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        elif name.endswith(".bias"):
            t = 0.1 * torch.randn(shape, generator=g)
        else:
            fan_in = int(np.prod(shape[1:]))
            t = torch.randn(shape, generator=g) * (1.5 / np.sqrt(fan_in))
        sd[name] = t.half().to(dtype)
    if not old_names:
        sd[POS + ".parametrizations.weight.original0"] = sd.pop(POS + ".weight_g")
        sd[POS + ".parametrizations.weight.original1"] = sd.pop(POS + ".weight_v")
    return sd


def err(got, want):
    """Max-normalised error against the float64 side."""
    got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double().cpu()
    return float((got - want).abs().max() / want.abs().max())
