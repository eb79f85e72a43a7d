// rn_jpeg.hip -- Motion-JPEG write-out as gfx950 kernels: a batch of finished uint8 frames [F,H,W,3] on the device becomes one
// baseline JPEG scan per frame, so that a few tens of KB per frame cross to the host and not 3 H W bytes.  Every convention and all
// arithmetic is in rn_jpeg_dev.h; the host writes the headers around the scan (radnerf/video.py).
//
// One wave is one 8 x 8 block everywhere: lane = sample (y, x) in the coefficient pass, lane = zigzag position in the entropy pass.
//   k_jpeg_coefficients  colour, 2 x 2 chroma mean, level shift, DCT (rows, then columns, through LDS), quantisation: int16
//                        [F, blocks, 64], blocks in MCU-interleaved scan order, coefficients in zigzag order.
//   k_jpeg_block_bits    the coded length of every block: each lane's symbol (rn_jpeg_dev.h position_bits; the run before a non-zero
//                        coefficient is a bit distance in the wave's __ballot mask), summed over the wave.
//   k_jpeg_scan          one workgroup per frame: exclusive scan of its entries in place, the total to a per-frame word.  Used twice:
//                        block lengths -> bit offsets, and 0xFF counts per chunk -> stuffing offsets.
//   k_jpeg_pack          the symbols again, a wave prefix sum of their lengths for each one's bit position; the wave ORs them into its
//                        own words in LDS and writes those to the frame's unstuffed stream: whole words by plain stores, the first
//                        and the last one -- shared with the neighbouring blocks, which other workgroups may write -- by an
//                        integer atomicOr on the zeroed buffer.  OR commutes: the bytes do not depend on the order of arrival.
//   k_jpeg_ff_count      per chunk of 4096 unstuffed bytes: how many are 0xFF (the last byte of a frame padded with 1-bits first).
//   k_jpeg_stuff         per chunk: byte i goes to i + (0xFF bytes before it), a 0x00 after every 0xFF, behind the streams of the
//                        batch's earlier frames (the output is packed); thread 0 of a frame's first chunk writes its byte count.
// No write is data-dependent in its bound: the unstuffed stream has kMaxBlockBytes per block, the output twice that (rn_jpeg_dev.h
// derives both), the entropy coder clamps a coefficient beyond the invariants to its category's largest value, and every store is
// also tested against the capacity it was given.
#include "rn_common.h"
#include "rn_jpeg_dev.h"

#include "../../include/radnerf_fused.h"

namespace rn {
namespace jpeg {

constexpr int kThreads = 256, kWaves = kThreads / kWave;                  // four blocks per workgroup
constexpr int kBlockWords = (kMaxBlockBits + 31 + 31) / 32 + 1;           // a block's bits from any bit offset within a word: 54 (+1)
constexpr int kScanThreads = 1024;
constexpr uint32_t kChunkBytes = 4096, kBytesPerThread = kChunkBytes / kThreads;      // 16: one uint4 of the unstuffed stream

__constant__ const HuffCodes d_huff = make_huff_codes();

struct Shape { uint32_t F, H, W, sub, mcus_w, blocks; };                   // blocks: per frame
struct QuantSteps { uint8_t step[2][64]; };                                // natural order

__global__ void __launch_bounds__(kThreads)
k_jpeg_coefficients(const uint8_t *__restrict__ frames, Shape s, QuantSteps q, int16_t *__restrict__ coefficients) {
    __shared__ float tile[kWaves][64], rows[kWaves][64], basis[64];                       // basis[u * 8 + x]
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, x = lane & 7u, y = lane >> 3;
    if (wave == 0u) basis[lane] = dct_basis(y, x);
    const size_t gb = (size_t)blockIdx.x * kWaves + wave;
    const bool live = gb < (size_t)s.F * s.blocks;
    uint32_t table = 0;
    if (live) {
        const uint32_t f = (uint32_t)(gb / s.blocks), b = (uint32_t)(gb % s.blocks);
        const uint32_t per = blocks_per_mcu(s.sub), mcu = b / per, k = b % per;
        table = block_component(k, s.sub) ? 1u : 0u;
        tile[wave][lane] = block_sample(frames + (size_t)f * s.H * s.W * 3u, s.H, s.W, s.sub, mcu % s.mcus_w, mcu / s.mcus_w, k, x, y);
    }
    __syncthreads();
    if (live) rows[wave][lane] = dct8(&tile[wave][y * 8u], 1u, &basis[x * 8u]);           // rows[y][u]
    __syncthreads();
    if (live) {
        const float c = dct8(&rows[wave][x], 8u, &basis[y * 8u]);                          // coefficient (v = y, u = x)
        coefficients[gb * 64u + zigzag_position(lane)] = quantise(c, q.step[table][lane]);
    }
}

// lane z of the wave that holds block b of a frame: its coefficient, and what it contributes to the stream
__device__ __forceinline__ Bits lane_bits(const int16_t *__restrict__ frame_coefficients, uint32_t b, uint32_t sub, uint32_t lane) {
    const int32_t value = frame_coefficients[(size_t)b * 64u + lane];
    const unsigned long long nonzero = __ballot(value != 0);
    const int32_t prev = previous_block(b, sub);
    int32_t pred = 0;
    if (lane == 0u && prev >= 0) pred = frame_coefficients[(size_t)prev * 64u];
    return position_bits(d_huff, block_component(b % blocks_per_mcu(sub), sub) ? 1u : 0u, lane, value, pred, nonzero);
}
// inclusive prefix sum over the wave
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v) {
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

__global__ void __launch_bounds__(kThreads)
k_jpeg_block_bits(const int16_t *__restrict__ coefficients, Shape s, uint32_t *__restrict__ block_bits) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const size_t gb = (size_t)blockIdx.x * kWaves + wave;
    if (gb >= (size_t)s.F * s.blocks) return;                                              // wave-uniform
    const uint32_t f = (uint32_t)(gb / s.blocks), b = (uint32_t)(gb % s.blocks);
    const Bits mine = lane_bits(coefficients + (size_t)f * s.blocks * 64u, b, s.sub, lane);
    const uint32_t total = wave_inclusive_scan(mine.len);
    if (lane == 63u) block_bits[gb] = total;
}

// In place: values[f * n + i] -> the sum of the frame's entries before i; totals[f] = the frame's sum
__global__ void __launch_bounds__(kScanThreads)
k_jpeg_scan(uint32_t *__restrict__ values, uint32_t n, uint32_t *__restrict__ totals) {
    __shared__ uint32_t lds[kScanThreads / kWave];
    uint32_t *mine = values + (size_t)blockIdx.x * n;
    uint32_t carry = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += kScanThreads) {
        const uint32_t i = i0 + threadIdx.x;
        const uint32_t v = i < n ? mine[i] : 0u;
        uint32_t all;
        const uint32_t before = block_exclusive_scan<kScanThreads>(v, lds, &all);
        if (i < n) mine[i] = carry + before;
        carry += all;
        __syncthreads();                                                                   // lds is read until here
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

__global__ void __launch_bounds__(kThreads)
k_jpeg_pack(const int16_t *__restrict__ coefficients, Shape s, const uint32_t *__restrict__ block_offsets, uint32_t words_per_frame,
            uint32_t *__restrict__ words) {
    __shared__ uint32_t lds[kWaves][kBlockWords];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const size_t gb = (size_t)blockIdx.x * kWaves + wave;
    const bool live = gb < (size_t)s.F * s.blocks;
    if (lane < (uint32_t)kBlockWords) lds[wave][lane] = 0u;
    __syncthreads();
    uint32_t first_bit = 0, n_bits = 0, f = 0;
    if (live) {
        f = (uint32_t)(gb / s.blocks);
        const uint32_t b = (uint32_t)(gb % s.blocks);
        const Bits mine = lane_bits(coefficients + (size_t)f * s.blocks * 64u, b, s.sub, lane);
        const uint32_t end = wave_inclusive_scan(mine.len);
        n_bits = __shfl(end, 63, 64);
        first_bit = block_offsets[gb] & 31u;
        if (mine.len) {
            // the symbol's `len` <= 59 bits start at bit `at` of the wave's words, most significant bit first: at most three words
            const uint32_t at = first_bit + end - mine.len, w = at >> 5, shift = at & 31u;
            const unsigned long long top = mine.bits << (64u - mine.len);              // the symbol at the top of 64 bits
            // words w, w + 1, w + 2 are the 96 bits of top * 2^(32 - shift)
            const uint32_t w0 = (uint32_t)(top >> (32u + shift)), w1 = (uint32_t)(top >> shift), w2 = (uint32_t)(top << (32u - shift));
            if (w < (uint32_t)kBlockWords) atomicOr(&lds[wave][w], w0);
            if (w1 && w + 1u < (uint32_t)kBlockWords) atomicOr(&lds[wave][w + 1u], w1);
            if (w2 && w + 2u < (uint32_t)kBlockWords) atomicOr(&lds[wave][w + 2u], w2);
        }
    }
    __syncthreads();
    if (!live || n_bits == 0u) return;
    const uint32_t n_words = (first_bit + n_bits + 31u) >> 5;
    if (lane >= n_words || lane >= (uint32_t)kBlockWords) return;
    const uint32_t gw = (block_offsets[gb] >> 5) + lane;
    if (gw >= words_per_frame) return;
    uint32_t *dst = words + (size_t)f * words_per_frame + gw;
    const bool whole = (lane > 0u || first_bit == 0u) && (lane + 1u < n_words || ((first_bit + n_bits) & 31u) == 0u);
    if (whole) *dst = lds[wave][lane];
    else atomicOr(dst, lds[wave][lane]);
}

// byte i of a frame's unstuffed stream (big-endian within the words), the last one padded with 1-bits
__device__ __forceinline__ uint32_t stream_byte(uint32_t word, uint32_t i, uint32_t frame_bits) {
    uint32_t v = (word >> (24u - 8u * (i & 3u))) & 0xffu;
    if (i == (frame_bits - 1u) >> 3 && (frame_bits & 7u)) v |= 0xffu >> (frame_bits & 7u);
    return v;
}
// A thread's 16 bytes of chunk `blockIdx.x` of frame `blockIdx.y`: the words, the index of the first byte, how many are in the stream
__device__ __forceinline__ uint32_t thread_bytes(const uint32_t *__restrict__ words, uint32_t words_per_frame, uint32_t frame_bits,
                                                 uint32_t w[4], uint32_t *first) {
    const uint32_t n_bytes = (frame_bits + 7u) >> 3;
    *first = blockIdx.x * kChunkBytes + threadIdx.x * kBytesPerThread;
    w[0] = w[1] = w[2] = w[3] = 0u;
    if (*first >= n_bytes) return 0u;
    const uint32_t w0 = *first >> 2;                                                     // a multiple of 4; words_per_frame is one too
    if (w0 + 4u <= words_per_frame) {
        const uint4 v = *reinterpret_cast<const uint4 *>(words + (size_t)blockIdx.y * words_per_frame + w0);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    }
    return n_bytes - *first < kBytesPerThread ? n_bytes - *first : kBytesPerThread;
}

__global__ void __launch_bounds__(kThreads)
k_jpeg_ff_count(const uint32_t *__restrict__ words, uint32_t words_per_frame, const uint32_t *__restrict__ frame_bits,
                uint32_t *__restrict__ ff_counts) {
    __shared__ uint32_t red[kWaves];
    const uint32_t bits = frame_bits[blockIdx.y];
    uint32_t w[4], first, count = 0;
    const uint32_t n = thread_bytes(words, words_per_frame, bits, w, &first);
    for (uint32_t j = 0; j < n; j++) count += stream_byte(w[j >> 2], first + j, bits) == 0xffu ? 1u : 0u;
    const uint32_t total = block_sum_first<uint32_t, kThreads>(count, red);
    if (threadIdx.x == 0) ff_counts[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
}

__global__ void __launch_bounds__(kThreads)
k_jpeg_stuff(const uint32_t *__restrict__ words, uint32_t words_per_frame, const uint32_t *__restrict__ frame_bits,
             const uint32_t *__restrict__ ff_offsets, const uint32_t *__restrict__ ff_totals, uint32_t capacity, uint8_t *__restrict__ out,
             uint32_t *__restrict__ sizes) {
    __shared__ uint32_t lds[kWaves], frame_base;
    const uint32_t bits = frame_bits[blockIdx.y];
    if ((uint32_t)(blockIdx.x * kChunkBytes) >= ((bits + 7u) >> 3) && blockIdx.x > 0) return;      // a chunk beyond the frame's stream
    if (threadIdx.x == 0) {                                   // the frames are packed: this one starts where the earlier ones end
        uint32_t base = 0;
        for (uint32_t f = 0; f < blockIdx.y; f++) base += ((frame_bits[f] + 7u) >> 3) + ff_totals[f];
        frame_base = base;
    }
    uint32_t w[4], first, count = 0;
    const uint32_t n = thread_bytes(words, words_per_frame, bits, w, &first);
    for (uint32_t j = 0; j < n; j++) count += stream_byte(w[j >> 2], first + j, bits) == 0xffu ? 1u : 0u;
    const uint32_t before = block_exclusive_scan<kThreads>(count, lds);          // its barrier also publishes frame_base
    uint32_t at = frame_base + first + ff_offsets[(size_t)blockIdx.y * gridDim.x + blockIdx.x] + before;
    for (uint32_t j = 0; j < n; j++) {
        const uint32_t v = stream_byte(w[j >> 2], first + j, bits);
        if (at < capacity) out[at] = (uint8_t)v;
        at++;
        if (v == 0xffu) {
            if (at < capacity) out[at] = 0u;
            at++;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) sizes[blockIdx.y] = ((bits + 7u) >> 3) + ff_totals[blockIdx.y];
}

// What a shape needs; ok = false: not a shape these entry points take
struct Plan {
    bool ok;
    Shape shape;
    uint32_t words_per_frame, chunks;                 // per frame: words of the unstuffed stream (a multiple of 4), chunks of it
    size_t capacity;                                  // bytes of one frame's stuffed stream, worst case
    size_t total_blocks;
    // workspace: block bit offsets uint32 [F * blocks] | frame bits uint32 [F] | 0xFF offsets uint32 [F * chunks] | 0xFF totals uint32 [F]
    //            | unstuffed words uint32 [F * words_per_frame] (16-byte aligned)
    size_t off_frame_bits, off_ff, off_ff_totals, off_words, bytes;
};
static Plan plan(uint32_t F, uint32_t H, uint32_t W, uint32_t sub) {
    Plan p = {};
    if (F == 0 || H == 0 || W == 0 || H > 65535u || W > 65535u || !subsampling_ok(sub)) return p;
    const uint64_t blocks = (uint64_t)mcus_across(W, sub) * mcus_across(H, sub) * blocks_per_mcu(sub);
    // a frame's bit count and every byte offset inside it fit 31 bits; the launch grids fit 31 bits
    if (blocks * 2u * kMaxBlockBytes * 8u >= (1ull << 31) || blocks * F / kWaves >= (1ull << 31)) return p;
    p.shape = Shape{F, H, W, sub, mcus_across(W, sub), (uint32_t)blocks};
    p.words_per_frame = ((uint32_t)blocks * (kMaxBlockBytes / 4u) + 3u) & ~3u;
    p.chunks = div_up(p.words_per_frame * 4u, kChunkBytes);
    p.capacity = (size_t)blocks * 2u * kMaxBlockBytes;
    p.total_blocks = (size_t)blocks * F;
    auto align16 = [](size_t v) { return (v + 15u) & ~(size_t)15u; };
    p.off_frame_bits = align16(p.total_blocks * 4u);
    p.off_ff = align16(p.off_frame_bits + (size_t)F * 4u);
    p.off_ff_totals = align16(p.off_ff + (size_t)F * p.chunks * 4u);
    p.off_words = align16(p.off_ff_totals + (size_t)F * 4u);
    p.bytes = p.off_words + (size_t)F * p.words_per_frame * 4u;
    p.ok = p.chunks <= 65535u * 16u && F <= 65535u;
    return p;
}

}  // namespace jpeg
}  // namespace rn

using namespace rn;
using namespace rn::jpeg;

extern "C" {

size_t rn_jpeg_workspace(uint32_t F, uint32_t H, uint32_t W, uint32_t subsampling) {
    const Plan p = plan(F, H, W, subsampling);
    return p.ok ? p.bytes : 0;
}

size_t rn_jpeg_stream_capacity(uint32_t H, uint32_t W, uint32_t subsampling) {
    const Plan p = plan(1, H, W, subsampling);
    return p.ok ? p.capacity : 0;
}

size_t rn_jpeg_blocks(uint32_t H, uint32_t W, uint32_t subsampling) {
    const Plan p = plan(1, H, W, subsampling);
    return p.ok ? p.shape.blocks : 0;
}

int rn_jpeg_coefficients(const uint8_t *frames, uint32_t F, uint32_t H, uint32_t W, uint32_t subsampling, uint32_t quality,
                         int16_t *coefficients, rn_stream_t stream) {
    const Plan p = plan(F, H, W, subsampling);
    RN_REQUIRE(p.ok, "jpeg_coefficients: F, H, W >= 1, sides <= 65535, subsampling 420 or 444, a frame's worst case below 2^31 bits "
               "(got %u frames of %u x %u, subsampling %u)", F, H, W, subsampling);
    RN_REQUIRE(quality >= 1 && quality <= 100, "jpeg_coefficients: quality is 1 .. 100 (got %u)", quality);
    RN_REQUIRE(frames && coefficients, "jpeg_coefficients: null pointer");
    QuantSteps q;
    for (uint32_t t = 0; t < 2; t++)
        for (uint32_t i = 0; i < 64; i++) q.step[t][i] = (uint8_t)quant_step(t, i, quality);
    hipLaunchKernelGGL(k_jpeg_coefficients, dim3((uint32_t)((p.total_blocks + kWaves - 1) / kWaves)), dim3(kThreads), 0, as_stream(stream),
                       frames, p.shape, q, coefficients);
    return check_launch("jpeg_coefficients");
}

int rn_jpeg_entropy(const int16_t *coefficients, uint32_t F, uint32_t H, uint32_t W, uint32_t subsampling, void *workspace, uint8_t *streams,
                    size_t capacity, uint32_t *sizes, rn_stream_t stream) {
    const Plan p = plan(F, H, W, subsampling);
    RN_REQUIRE(p.ok, "jpeg_entropy: F, H, W >= 1, sides <= 65535, subsampling 420 or 444, a frame's worst case below 2^31 bits "
               "(got %u frames of %u x %u, subsampling %u)", F, H, W, subsampling);
    RN_REQUIRE(coefficients && workspace && streams && sizes, "jpeg_entropy: null pointer");
    RN_REQUIRE(capacity >= (size_t)F * p.capacity, "jpeg_entropy: %zu bytes are below the worst case of %u frames, %zu each "
               "(rn_jpeg_stream_capacity)", capacity, F, p.capacity);
    RN_REQUIRE((size_t)F * p.capacity < ((size_t)1 << 31), "jpeg_entropy: the worst case of %u frames passes 2^31 bytes: encode fewer at a time", F);
    if (capacity >= ((size_t)1 << 31)) capacity = ((size_t)1 << 31) - 1;                 // byte offsets are 32-bit; no stream reaches that far
    RN_REQUIRE(((uintptr_t)workspace & 15u) == 0, "jpeg_entropy: workspace must be 16-byte aligned");
    uint8_t *ws = static_cast<uint8_t *>(workspace);
    uint32_t *block_bits = reinterpret_cast<uint32_t *>(ws), *frame_bits = reinterpret_cast<uint32_t *>(ws + p.off_frame_bits);
    uint32_t *ff = reinterpret_cast<uint32_t *>(ws + p.off_ff), *ff_totals = reinterpret_cast<uint32_t *>(ws + p.off_ff_totals);
    uint32_t *words = reinterpret_cast<uint32_t *>(ws + p.off_words);
    hipStream_t s = as_stream(stream);
    const dim3 per_block((uint32_t)((p.total_blocks + kWaves - 1) / kWaves)), per_chunk(p.chunks, F);
    if (hipMemsetAsync(words, 0, (size_t)F * p.words_per_frame * 4u, s) != hipSuccess) return check_launch("jpeg_entropy (memset)");
    hipLaunchKernelGGL(k_jpeg_block_bits, per_block, dim3(kThreads), 0, s, coefficients, p.shape, block_bits);
    hipLaunchKernelGGL(k_jpeg_scan, dim3(F), dim3(kScanThreads), 0, s, block_bits, p.shape.blocks, frame_bits);
    hipLaunchKernelGGL(k_jpeg_pack, per_block, dim3(kThreads), 0, s, coefficients, p.shape, block_bits, p.words_per_frame, words);
    hipLaunchKernelGGL(k_jpeg_ff_count, per_chunk, dim3(kThreads), 0, s, words, p.words_per_frame, frame_bits, ff);
    hipLaunchKernelGGL(k_jpeg_scan, dim3(F), dim3(kScanThreads), 0, s, ff, p.chunks, ff_totals);
    hipLaunchKernelGGL(k_jpeg_stuff, per_chunk, dim3(kThreads), 0, s, words, p.words_per_frame, frame_bits, ff, ff_totals, (uint32_t)capacity,
                       streams, sizes);
    return check_launch("jpeg_entropy");
}

}  // extern "C"
