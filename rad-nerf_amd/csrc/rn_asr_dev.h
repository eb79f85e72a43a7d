// rn_asr_dev.h -- the supported shapes, the packed weight image and the workspace plan of the wav2vec2 CTC kernels
// (rn_asr.hip), shared by the host entry points.  See include/radnerf_fused.h for the arithmetic.
//
// Activations are time-major [B][T][C] floats.  Every weight matrix of the image is the B operand of a GEMM, [K][ld] with
// ld = N rounded up to 4 (zero filled), K ordered as the GEMM's A rows are laid out in memory:
//   conv layer i >= 1   k = tap * Cin + ci        (the taps of output step t are k * Cin contiguous floats from row t * stride)
//   positional conv     per group: k = tap * (H / G) + ci, the weight norm folded in (w = v * g[tap] / |v[:, :, tap]|)
//   linear layers       k = input feature; q, k and v side by side as one [H][3 H] matrix
// Every piece of the image and of the workspace starts at a multiple of 4 floats (16-byte vector loads).
#pragma once

#include "rn_common.h"

#include "../../include/radnerf_fused.h"

namespace rn {
namespace asr {

constexpr uint32_t kMaxConv = 8;
constexpr uint32_t kHeadDim = 64;       // the attention kernel's head width (one lane per feature)
constexpr uint32_t kMaxT = 96;          // the attention kernel's longest sequence (keys and values of one head stay in LDS)
constexpr uint32_t kLayerTensors = 16, kFixedTensors = 4 + 3 + 2 + 2;

static inline size_t up4(size_t n) { return (n + 3u) & ~(size_t)3u; }

// NULL when the kernels take the config, else what they do not take (a static string naming the field)
static inline const char *unsupported(const rn_asr_config_t *c) {
    if (!c) return "null config";
    if (c->n_conv < 1 || c->n_conv > kMaxConv) return "n_conv must be 1 .. 8";
    for (uint32_t i = 0; i < c->n_conv; i++) {
        if (c->conv_dim[i] == 0 || c->conv_dim[i] % 4u || c->conv_dim[i] > 4096u) return "conv_dim must be a multiple of 4, at most 4096";
        if (c->conv_kernel[i] == 0 || c->conv_kernel[i] > 64u) return "conv_kernel must be 1 .. 64";
        if (c->conv_stride[i] == 0 || c->conv_stride[i] > 64u) return "conv_stride must be 1 .. 64";
    }
    if (c->heads == 0 || c->hidden != c->heads * kHeadDim) return "hidden_size / num_attention_heads must be 64";
    if (c->hidden > 8192u) return "hidden_size must be at most 8192";
    if (c->intermediate == 0 || c->intermediate % 4u || c->intermediate > 32768u) return "intermediate_size must be a multiple of 4, at most 32768";
    if (c->layers == 0 || c->layers > 128u) return "num_hidden_layers must be 1 .. 128";
    if (c->pos_taps == 0 || c->pos_taps % 2u || c->pos_taps > 1024u) return "num_conv_pos_embeddings must be even, at most 1024";
    if (c->pos_groups == 0 || c->hidden % c->pos_groups || (c->hidden / c->pos_groups) % 4u)
        return "hidden_size / num_conv_pos_embedding_groups must be a multiple of 4";
    if (c->vocab == 0 || c->vocab > 65536u) return "vocab_size must be 1 .. 65536";
    if (!(c->layer_norm_eps > 0.0f) || !(c->layer_norm_eps < 1.0f)) return "layer_norm_eps must be in (0, 1)";
    return nullptr;
}

static inline uint32_t tensor_count(const rn_asr_config_t &c) { return 4u * c.n_conv + kFixedTensors + kLayerTensors * c.layers; }

// ---- packed weight image (offsets in floats) ---------------------------------------------------------------------------------
struct LayerLayout {       // relative to the layer's start
    size_t ln1_w, ln1_b, wqkv, bqkv, wo, bo, ln2_w, ln2_b, w1, b1, w2, b2, size;
};
struct ImageLayout {
    size_t conv_w[kMaxConv], conv_b[kMaxConv], conv_lnw[kMaxConv], conv_lnb[kMaxConv];
    size_t proj_lnw, proj_lnb, proj_w, proj_b;
    size_t pos_scale, pos_w, pos_b;      // pos_scale [taps]: g / |v| per tap, written by the pack and read by it alone
    size_t enc_lnw, enc_lnb, layers, head_w, head_b, total;
    LayerLayout layer;
};
static inline ImageLayout image_layout(const rn_asr_config_t &c) {
    ImageLayout L{};
    size_t at = 0;
    auto take = [&at](size_t n) { const size_t o = at; at += up4(n); return o; };
    for (uint32_t i = 0; i < c.n_conv; i++) {
        const size_t cin = i ? c.conv_dim[i - 1] : 1u;
        L.conv_w[i] = take(cin * c.conv_kernel[i] * c.conv_dim[i]);
        L.conv_b[i] = take(c.conv_dim[i]); L.conv_lnw[i] = take(c.conv_dim[i]); L.conv_lnb[i] = take(c.conv_dim[i]);
    }
    const size_t cl = c.conv_dim[c.n_conv - 1], H = c.hidden, I = c.intermediate;
    L.proj_lnw = take(cl); L.proj_lnb = take(cl); L.proj_w = take(cl * H); L.proj_b = take(H);
    L.pos_scale = take(c.pos_taps); L.pos_w = take((size_t)c.pos_taps * (H / c.pos_groups) * H); L.pos_b = take(H);
    L.enc_lnw = take(H); L.enc_lnb = take(H);
    {
        size_t in = 0;
        auto sub = [&in](size_t n) { const size_t o = in; in += up4(n); return o; };
        LayerLayout &y = L.layer;
        y.ln1_w = sub(H); y.ln1_b = sub(H); y.wqkv = sub(H * 3u * H); y.bqkv = sub(3u * H); y.wo = sub(H * H); y.bo = sub(H);
        y.ln2_w = sub(H); y.ln2_b = sub(H); y.w1 = sub(H * I); y.b1 = sub(I); y.w2 = sub(I * H); y.b2 = sub(H);
        y.size = in;
    }
    L.layers = take(L.layer.size * c.layers);
    L.head_w = take(H * up4(c.vocab)); L.head_b = take(c.vocab);
    L.total = at;
    return L;
}

// ---- workspace (offsets in floats) -------------------------------------------------------------------------------------------
struct Plan {
    uint32_t T[kMaxConv];        // steps after conv layer i
    uint32_t Tout;
    size_t xn, conv_a, conv_b, h, pad, x, qkv, att, ff, total;     // total = 0: unsupported (B, samples)
};
static inline Plan make_plan(const rn_asr_config_t &c, uint32_t B, uint32_t samples) {
    Plan p{};
    if (B == 0 || B > 4096u || samples == 0 || samples > (1u << 22)) return p;
    uint32_t t = samples;
    size_t widest = 0;
    for (uint32_t i = 0; i < c.n_conv; i++) {
        if (t < c.conv_kernel[i]) return p;
        t = (t - c.conv_kernel[i]) / c.conv_stride[i] + 1u;
        p.T[i] = t;
        const size_t n = (size_t)B * t * c.conv_dim[i];
        widest = n > widest ? n : widest;
    }
    if (t > kMaxT) return p;
    p.Tout = t;
    const size_t rows = (size_t)B * t, H = c.hidden;
    if ((size_t)B * p.T[0] >= (1u << 31)) return p;
    size_t at = 0;
    auto take = [&at](size_t n) { const size_t o = at; at += up4(n); return o; };
    p.xn = take((size_t)B * samples);
    p.conv_a = take(widest); p.conv_b = take(widest);
    p.h = take(rows * H); p.pad = take((size_t)B * (t + c.pos_taps) * H); p.x = take(rows * H); p.qkv = take(rows * 3u * H);
    p.att = take(rows * H); p.ff = take(rows * c.intermediate);
    p.total = at;
    return p;
}

// ---- the GEMM's tiling ----------------------------------------------------------------------------------------------------------
// 32 or 128: which of the two tilings of C = A W runs a product of M x N x K in `groups` groups on a device of `cus` compute
// units.  Both give the same bits, so the choice moves nothing but time, and it is a function of the shape alone: never of the data
// or of what else shares the batch.  The 32-row tiling (one wave per 32 x 32 tile) is taken while the 128-row grid would leave
// compute units idle and its own tiles still find a SIMD each (four per compute unit); K does not enter: both walk it whole.
static inline uint32_t pick_tile(uint32_t M, uint32_t N, uint32_t K, uint32_t groups, uint32_t cus) {
    (void)K;
    const uint64_t wg128 = (uint64_t)((M + 127u) / 128u) * ((N + 127u) / 128u) * groups;
    const uint64_t waves32 = (uint64_t)((M + 31u) / 32u) * ((N + 31u) / 32u) * groups;
    return (wg128 < cus && waves32 <= 4ull * cus) ? 32u : 128u;
}

}  // namespace asr
}  // namespace rn
