// rn_jpeg_dev.h -- the arithmetic of the Motion-JPEG write-out (rn_jpeg.hip; DESIGN.md section 3, "video write-out"), plain functions
// for host and device.  No HIP header is needed: a host compiler builds the same text (tests/test_video.py does, as tests/test_mesh.py
// does with rn_mesh_dev.h), the kernels include it as it is.
//
// Baseline sequential JPEG (ITU-T T.81) with the Annex K tables, one scan, components interleaved:
//   * colour: JFIF full-range YCbCr in fp32, nothing rounded between the stages,
//       Y = .299 R + .587 G + .114 B,  Cb = -.168735892 R - .331264108 G + .5 B + 128,  Cr = .5 R - .418687589 G - .081312411 B + 128;
//   * a frame whose sides are no multiple of the MCU is padded by edge replication (pixel (min(x, W-1), min(y, H-1)));
//   * subsampling 420: MCU 16 x 16 = Y00 Y01 Y10 Y11 Cb Cr, a chroma sample is the plain mean of its 2 x 2 pixels,
//     ((a + b) + (c + d)) / 4 with a, b the upper row; subsampling 444: MCU 8 x 8 = Y Cb Cr.  MCUs in raster order;
//   * transform: sample - 128, then the orthonormal 8 x 8 DCT-II, rows first then columns, every sum in index order 0..7;
//   * quantisation: the Annex K tables scaled by the IJG rule (s = 5000 / q below 50, 200 - 2 q from 50 on, (t s + 50) / 100 clamped to
//     1..255), coefficient / step, rounded half away from zero: sign(v) floor(|v| + 0.5).  int16, stored in zigzag order.
//     Invariants (8-bit samples, steps >= 1): |DC| <= 1024, so a DC difference has category <= 11; |AC| <= 1023: category <= 10;
//   * entropy coding: the four Annex K Huffman tables (BITS / HUFFVAL below), never optimised ones: a frame's stream depends on its
//     own coefficients alone.  DC: the difference against the previous block of the same component in scan order, 0 before a
//     frame's first; AC: (run << 4 | size) symbols, one ZRL (0xF0) per 16 zeros of a longer run, EOB (0x00) after the last non-zero
//     coefficient unless that is coefficient 63; a negative value's extra bits are the low bits of value - 1 (one's complement).
// Table index 0 serves Y, 1 serves Cb and Cr.  All arithmetic rounds as written (the tree builds with -ffp-contract=off).
#pragma once

#include <stdint.h>

#ifndef RN_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define RN_HD __host__ __device__ inline
#else
#define RN_HD inline
#endif
#endif

namespace rn {
namespace jpeg {

constexpr uint32_t kSub420 = 420, kSub444 = 444;
constexpr uint32_t kMaxDcCategory = 11, kMaxAcCategory = 10;
// Worst case of one coded block: DC at most 11 bits of code (the chroma table's longest) + 11 extra bits; each of the 63 AC coefficients
// at most 16 bits of code + 10 extra bits when none is zero.  A ZRL (11 or 10 bits) stands for 16 zeros, an EOB for at least one, so
// zeros only shorten the block.  22 + 63 * 26 = 1660 bits = 207.5 bytes < 208; byte stuffing at most doubles it.
constexpr uint32_t kMaxBlockBits = 22 + 63 * 26;
constexpr uint32_t kMaxBlockBytes = 208;
static_assert(kMaxBlockBits <= 8 * kMaxBlockBytes, "a coded block fits its worst-case slot");

RN_HD bool subsampling_ok(uint32_t sub) { return sub == kSub420 || sub == kSub444; }
RN_HD uint32_t mcu_side(uint32_t sub) { return sub == kSub420 ? 16u : 8u; }
RN_HD uint32_t blocks_per_mcu(uint32_t sub) { return sub == kSub420 ? 6u : 3u; }
RN_HD uint32_t mcus_across(uint32_t extent, uint32_t sub) { return (extent + mcu_side(sub) - 1u) / mcu_side(sub); }
// component (0 Y, 1 Cb, 2 Cr) of block k of an MCU
RN_HD uint32_t block_component(uint32_t k, uint32_t sub) { return sub == kSub420 ? (k < 4u ? 0u : k - 3u) : k; }
// Block b of a frame (MCU-interleaved scan order): the index of the previous block of the same component, -1 for an MCU 0 block
// whose component has none before it.
RN_HD int32_t previous_block(uint32_t b, uint32_t sub) {
    const uint32_t per = blocks_per_mcu(sub), k = b % per;
    if (sub == kSub420 && k >= 1u && k < 4u) return (int32_t)b - 1;
    if (b < per) return -1;
    return (int32_t)b - (sub == kSub420 && k == 0u ? 3 : (int32_t)per);
}

// ---- colour ---------------------------------------------------------------------------------------------------------------
RN_HD float luma(float r, float g, float b) { return 0.299f * r + 0.587f * g + 0.114f * b; }
RN_HD float chroma_b(float r, float g, float b) { return -0.168735892f * r - 0.331264108f * g + 0.5f * b + 128.0f; }
RN_HD float chroma_r(float r, float g, float b) { return 0.5f * r - 0.418687589f * g - 0.081312411f * b + 128.0f; }
RN_HD float component_of(uint32_t comp, float r, float g, float b) {
    return comp == 0u ? luma(r, g, b) : comp == 1u ? chroma_b(r, g, b) : chroma_r(r, g, b);
}
RN_HD float mean4(float a, float b, float c, float d) { return ((a + b) + (c + d)) * 0.25f; }

// Sample (x, y) of 0..7 of block k of the MCU at (mcu_x, mcu_y), level-shifted: frame = [H, W, 3] uint8
RN_HD float block_sample(const uint8_t *frame, uint32_t H, uint32_t W, uint32_t sub, uint32_t mcu_x, uint32_t mcu_y, uint32_t k, uint32_t x,
                         uint32_t y) {
    const uint32_t comp = block_component(k, sub);
    float v[4];
    const bool mean = sub == kSub420 && comp != 0u;
    const uint32_t n = mean ? 4u : 1u;
    for (uint32_t i = 0; i < n; i++) {
        uint32_t px, py;
        if (mean) {
            px = mcu_x * 16u + 2u * x + (i & 1u);
            py = mcu_y * 16u + 2u * y + (i >> 1);
        } else if (sub == kSub420) {
            px = mcu_x * 16u + (k & 1u) * 8u + x;
            py = mcu_y * 16u + (k >> 1) * 8u + y;
        } else {
            px = mcu_x * 8u + x;
            py = mcu_y * 8u + y;
        }
        px = px < W ? px : W - 1u;
        py = py < H ? py : H - 1u;
        const uint8_t *p = frame + ((size_t)py * W + px) * 3u;
        v[i] = component_of(comp, (float)p[0], (float)p[1], (float)p[2]);
    }
    return (mean ? mean4(v[0], v[1], v[2], v[3]) : v[0]) - 128.0f;
}

// ---- transform ------------------------------------------------------------------------------------------------------------
// a(u) cos((2 x + 1) u pi / 16), a(0) = sqrt(1/8), a(u > 0) = 1/2: the orthonormal DCT-II basis
RN_HD float dct_basis(uint32_t u, uint32_t x) {
    const float half_cos[9] = {0.5f, 0.49039264020161522f, 0.46193976625564337f, 0.41573480615127262f, 0.35355339059327379f,
                               0.27778511650980114f, 0.19134171618254492f, 0.09754516100806417f, 0.0f};      // cos(i pi / 16) / 2
    if (u == 0u) return 0.35355339059327379f;
    uint32_t m = ((2u * x + 1u) * u) & 31u;
    if (m > 16u) m = 32u - m;
    return m > 8u ? -half_cos[16u - m] : half_cos[m];
}
// One output of the 8-point transform of in[0], in[stride], ..; basis_row = dct_basis(u, 0 .. 7) where a caller keeps a table of them
RN_HD float dct8(const float *in, uint32_t stride, const float *basis_row) {
    float s = 0.0f;
    for (uint32_t x = 0; x < 8u; x++) s += in[x * stride] * basis_row[x];
    return s;
}
RN_HD float dct8(const float *in, uint32_t stride, uint32_t u) {
    float row[8];
    for (uint32_t x = 0; x < 8u; x++) row[x] = dct_basis(u, x);
    return dct8(in, stride, row);
}

// ---- quantisation ---------------------------------------------------------------------------------------------------------
RN_HD uint32_t base_quant(uint32_t table, uint32_t natural) {
    const uint8_t lum[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                             69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55,  64,
                             81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
    const uint8_t chr[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                             99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
    return table == 0u ? lum[natural] : chr[natural];
}
// the IJG rule; quality 1..100
RN_HD uint32_t quant_step(uint32_t table, uint32_t natural, uint32_t quality) {
    const uint32_t q = quality < 1u ? 1u : quality > 100u ? 100u : quality;
    const uint32_t scale = q < 50u ? 5000u / q : 200u - 2u * q;
    const uint32_t v = (base_quant(table, natural) * scale + 50u) / 100u;
    return v < 1u ? 1u : v > 255u ? 255u : v;
}
// natural (row-major) index of zigzag position z, and back
RN_HD uint32_t zigzag_natural(uint32_t z) {
    const uint8_t zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                            35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return zz[z];
}
RN_HD uint32_t zigzag_position(uint32_t natural) {
    const uint8_t pos[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                             10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};
    return pos[natural];
}
RN_HD int16_t quantise(float coefficient, uint32_t step) {
    const float r = coefficient / (float)step;
    const float m = __builtin_floorf(__builtin_fabsf(r) + 0.5f);
    return (int16_t)(r < 0.0f ? -m : m);
}

// ---- Huffman tables (Annex K.3) -------------------------------------------------------------------------------------------
struct HuffSpec { uint8_t bits[16]; uint8_t n; uint8_t vals[162]; };
struct HuffSpecs { HuffSpec dc[2], ac[2]; };
constexpr HuffSpecs kHuffSpecs = {
    {{{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}},
     {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}}},
    {{{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, 162,
      {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
       0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
       0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
       0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
       0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
       0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
       0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
       0xfa}},
     {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}, 162,
      {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
       0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
       0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
       0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
       0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
       0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
       0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
       0xfa}}}};

// code | length << 16 of every symbol (0 where the table has none), built from BITS / HUFFVAL as Annex C does
struct HuffCodes { uint32_t dc[2][16]; uint32_t ac[2][256]; };
constexpr void assign_codes(const HuffSpec &s, uint32_t *out) {
    uint32_t code = 0, k = 0;
    for (uint32_t len = 1; len <= 16; len++) {
        for (uint32_t i = 0; i < s.bits[len - 1]; i++) out[s.vals[k++]] = code++ | (len << 16);
        code <<= 1;
    }
}
constexpr HuffCodes make_huff_codes() {
    HuffCodes c = {};
    for (uint32_t t = 0; t < 2; t++) {
        assign_codes(kHuffSpecs.dc[t], c.dc[t]);
        assign_codes(kHuffSpecs.ac[t], c.ac[t]);
    }
    return c;
}

// ---- symbols --------------------------------------------------------------------------------------------------------------
// `len` bits, the first one transmitted at bit len - 1
struct Bits { uint64_t bits; uint32_t len; };

// bits |v| needs, at most `cap`: a value beyond the invariant is coded as the largest of its category, so that no length ever
// passes the worst case the buffers are sized by (the coefficient pass never produces one)
RN_HD int32_t clamp_to_category(int32_t v, uint32_t cap) {
    const int32_t lim = (int32_t)(1u << cap) - 1;
    return v > lim ? lim : v < -lim ? -lim : v;
}
RN_HD uint32_t category(int32_t v) {
    uint32_t a = (uint32_t)(v < 0 ? -v : v), n = 0;
    while (a) { n++; a >>= 1; }
    return n;
}
RN_HD uint32_t extra_bits(int32_t v, uint32_t cat) { return (uint32_t)(v < 0 ? v - 1 : v) & ((1u << cat) - 1u); }
RN_HD Bits append(Bits a, uint32_t code_len, uint32_t extra, uint32_t n_extra) {
    a.bits = (a.bits << (code_len >> 16)) | (code_len & 0xffffu);
    a.bits = (a.bits << n_extra) | extra;
    a.len += (code_len >> 16) + n_extra;
    return a;
}
RN_HD Bits dc_symbol(const HuffCodes &h, uint32_t table, int32_t diff) {
    diff = clamp_to_category(diff, kMaxDcCategory);
    const uint32_t cat = category(diff);
    return append(Bits{0, 0}, h.dc[table][cat], extra_bits(diff, cat), cat);
}
// A non-zero AC coefficient after `run` zeros (run <= 62): run / 16 ZRLs, then the run/size symbol and the extra bits: <= 59 bits
RN_HD Bits ac_symbol(const HuffCodes &h, uint32_t table, uint32_t run, int32_t v) {
    v = clamp_to_category(v, kMaxAcCategory);
    Bits b{0, 0};
    for (uint32_t z = run >> 4; z > 0; z--) b = append(b, h.ac[table][0xf0], 0, 0);
    const uint32_t cat = category(v);
    return append(b, h.ac[table][((run & 15u) << 4) | cat], extra_bits(v, cat), cat);
}
RN_HD Bits eob_symbol(const HuffCodes &h, uint32_t table) { return append(Bits{0, 0}, h.ac[table][0], 0, 0); }

// What position z (zigzag) of a block contributes, given the block's non-zero mask (bit z = coefficient z != 0): position 0 the DC
// difference, a non-zero AC coefficient its ZRLs and symbol, position 63 holding a zero the EOB, everything else nothing.
RN_HD Bits position_bits(const HuffCodes &h, uint32_t table, uint32_t z, int32_t value, int32_t dc_pred, uint64_t nonzero) {
    if (z == 0u) return dc_symbol(h, table, value - dc_pred);
    if (value == 0) return z == 63u ? eob_symbol(h, table) : Bits{0, 0};
    const uint64_t below = (nonzero | 1u) & ((1ull << z) - 1u);                  // position 0 bounds every run
    const uint32_t prev = 63u - (uint32_t)__builtin_clzll(below);
    return ac_symbol(h, table, z - prev - 1u, value);
}

}  // namespace jpeg
}  // namespace rn
