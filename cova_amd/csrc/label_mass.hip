// Label mass of resident training frames (include/covahip.h, covahip_train_data_label_mass): per frame, the number of macroblocks
// with gt != 0 that the keep map keeps.  A bandwidth kernel over gt u8 [capacity][h][w] (train_data.hip owns the storage and the
// entry point); every offset is 64-bit.
//
// A frame is read by a TEAM of lanes: one wave while it has at most MASS_WAVE_MAX bytes (a 45x80 frame is 3600: a workgroup
// takes four frames a round, and a 16x16 frame costs a quarter of one), the whole workgroup above (68x120 is 8160).  A frame of
// an odd h * w starts on any byte, so the team peels the up to 15 bytes before the first 16-byte boundary and the up to 15
// behind the last, a byte per lane, and reads the words between with one 16-byte load per lane, two in flight; non-zero bytes
// are counted a word at a time.  The keep map is aligned to the FRAME, not to memory: it comes as bits packed by the host (bit p
// = macroblock p is kept, at most 128 KiB), and the 16 bits of a label word are one funnel shift of two table words.  The
// table is an eighth of a frame's bytes and stays in cache; a byte table off the labels' alignment would take two more 16-byte
// loads and four byte alignments per word.  A frame belongs to one team, so its count is reduced in the wave (and through LDS
// in the workgroup) and stored once: no atomics.
#include "internal.h"

namespace {

constexpr int BLK = 256;
constexpr int MASS_WAVE_MAX = 4096;           // bytes of a frame that one wave still reads alone
constexpr unsigned MASS_BLOCKS_MAX = 2048;    // workgroups of a launch: 8 per CU of 256; the grid strides over the frames

// bit 7 of every byte of x that is not zero
__device__ inline uint32_t nz_bytes(uint32_t x) { return (((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u; }
// bits 0..3 of b to bit 7 of bytes 0..3 (the four partial products do not overlap)
__device__ inline uint32_t keep_bytes(uint32_t b) { return (((b & 0xFu) * 0x00204081u) & 0x01010101u) << 7; }
// bits pos .. pos + 31 of the keep table of nw words; past the table: the last word again, in bits no caller looks at
__device__ inline uint32_t keep_bits(const uint32_t *__restrict__ bits, int nw, int pos) {
    const int i = pos >> 5;
    const uint64_t two = (uint64_t)bits[min(i + 1, nw - 1)] << 32 | bits[i];
    return (uint32_t)(two >> (pos & 31));
}
// non-zero kept bytes of the 16 label bytes v, which are macroblocks pos .. pos + 15 of their frame
template <bool KEEP>
__device__ inline uint32_t mass16(uint4 v, const uint32_t *__restrict__ bits, int nw, int pos) {
    uint32_t a = nz_bytes(v.x), b = nz_bytes(v.y), c = nz_bytes(v.z), d = nz_bytes(v.w);
    if (KEEP) {
        const uint32_t k = keep_bits(bits, nw, pos);
        a &= keep_bytes(k), b &= keep_bytes(k >> 4), c &= keep_bytes(k >> 8), d &= keep_bytes(k >> 12);
    }
    return (uint32_t)__popc(a | b >> 1 | c >> 2 | d >> 3);
}

// WAVES: 1 (a frame per wave, BLK / 64 frames per workgroup and round) or BLK / 64 (a frame per workgroup).  KEEP false: the
// table is never read.  mass[i] for i in [0, n): frame first + i.
template <bool KEEP, int WAVES>
__global__ __launch_bounds__(BLK) void k_label_mass(const uint8_t *__restrict__ gt, const uint32_t *__restrict__ bits,
                                                    uint32_t *__restrict__ mass, int64_t first, int64_t n, int hw) {
    constexpr int TEAM = WAVES * 64, TEAMS = BLK / TEAM;
    __shared__ uint32_t part[BLK / 64];
    const int lane = (int)threadIdx.x % TEAM, team = (int)threadIdx.x / TEAM;
    const int nw = (hw + 31) >> 5;
    for (int64_t f = (int64_t)blockIdx.x * TEAMS + team; f < n; f += (int64_t)gridDim.x * TEAMS) {
        const uint8_t *p = gt + (first + f) * hw;
        const int head = (int)((16u - (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u);
        const int words = (hw - head) >> 4, tail = (hw - head) & 15;   // hw >= 256: words >= 15
        uint32_t c = 0;
        if (lane < head + tail) {                                      // at most 30 lanes, a byte each
            const int pos = lane < head ? lane : words * 16 + lane;    // (head + words * 16 + (lane - head))
            c = p[pos] != 0 && (!KEEP || (bits[pos >> 5] >> (pos & 31) & 1u));
        }
        const uint4 *body = reinterpret_cast<const uint4 *>(p + head);
        for (int j = lane; j < words; j += 2 * TEAM) {
            const int j2 = min(j + TEAM, words - 1);                   // always a load, its value dropped past the end
            const uint4 v = body[j];
            uint4 v2 = body[j2];
            if (j + TEAM >= words) v2 = make_uint4(0, 0, 0, 0);
            c += mass16<KEEP>(v, bits, nw, head + 16 * j) + mass16<KEEP>(v2, bits, nw, head + 16 * j2);
        }
#pragma unroll
        for (int s = 32; s; s >>= 1) c += __shfl_down(c, s, 64);
        if (WAVES == 1) {
            if (lane == 0) mass[f] = c;
        } else {                                                       // f is uniform over the workgroup
            if ((lane & 63) == 0) part[lane >> 6] = c;
            __syncthreads();
            if (lane == 0) {
                uint32_t t = 0;
#pragma unroll
                for (int i = 0; i < WAVES; i++) t += part[i];
                mass[f] = t;
            }
            __syncthreads();                                           // `part` is written again in the next round
        }
    }
}

}  // namespace

int covahip_label_mass_launch(covahip_ctx *ctx, const uint8_t *d_gt, const uint32_t *d_bits, uint32_t *d_mass, int64_t first,
                              int64_t n, int hw) {
    const bool wave = hw <= MASS_WAVE_MAX;
    const int64_t per = wave ? BLK / 64 : 1;   // frames of a workgroup and round
    const unsigned blocks = (unsigned)std::min<int64_t>((n + per - 1) / per, MASS_BLOCKS_MAX);
    const hipStream_t s = ctx->stream;
    ProfScope prof(ctx, "train_data_mass");
    if (d_bits && wave) k_label_mass<true, 1><<<blocks, BLK, 0, s>>>(d_gt, d_bits, d_mass, first, n, hw);
    else if (d_bits) k_label_mass<true, BLK / 64><<<blocks, BLK, 0, s>>>(d_gt, d_bits, d_mass, first, n, hw);
    else if (wave) k_label_mass<false, 1><<<blocks, BLK, 0, s>>>(d_gt, nullptr, d_mass, first, n, hw);
    else k_label_mass<false, BLK / 64><<<blocks, BLK, 0, s>>>(d_gt, nullptr, d_mass, first, n, hw);
    COVAHIP_CHECK_HIP(ctx, hipGetLastError());
    return COVAHIP_OK;
}
