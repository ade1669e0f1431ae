// Label alignment of resident training frames (include/covahip.h, covahip_train_data_align): per frame f of ONE recording and per
// shift s in -S .. S, the number of kept macroblocks that MOVE in the records of frame f and are SET in the labels of frame
// f + s, with the two marginal counts.  A bandwidth kernel over rec u16 / gt u8 [capacity][h][w] (train_data.hip owns the storage
// and the entry point); every offset is 64-bit.
//
// A workgroup owns a RUN of consecutive frames and walks the frame in tiles of TILE positions.  Per tile it turns the records of
// its RUN frames and the labels of the RUN + 2 S frames around them into BIT PLANES in LDS, a bit per macroblock with the keep map
// and the frame's edge already ANDed in; the (2 S + 1) RUN counts of the tile are then popcounts of ANDed plane words, so the
// (2 S + 1)-fold pass goes over a bit per macroblock, an LDS read, and every record and label byte is read from memory once (the
// 2 S label frames of the halo: once more per run).  LDS does not depend on the geometry.  A count belongs to one thread of one
// workgroup from the first tile to the last and is stored once: no atomics.
//
// A frame of an odd h * w starts on any byte (labels) or any even byte (records), and the planes of different frames must line up
// by POSITION.  A plane word is therefore built from the 16-byte aligned chunks that cover its 32 macroblocks -- three label
// chunks or five record chunks, one fewer when the frame happens to sit on the boundary -- and the bits are shifted into place
// as a 64-bit word; neighbouring lanes share the extra chunk in cache.  A chunk that would reach past the array is read a byte
// at a time (the last 16 bytes of a full data set).
#include "internal.h"

namespace {

constexpr int BLK = 256;
constexpr int RUN = 32;                         // frames of a run
constexpr int S_MAX = 32;                       // the largest shift scored
constexpr int TILE = 1024;                      // macroblocks of a tile: a plane row is TILE / 32 words
constexpr int ROW = TILE / 32 + 4;              // words between plane rows: consecutive rows, one ds_read_b128 each, miss each other's banks
constexpr int ROWS = 2 * RUN + 2 * S_MAX;       // RUN planes of `moves`, then RUN + 2 S of `set`
constexpr int ACC = (RUN * (2 * S_MAX + 3) + BLK - 1) / BLK;   // counts of a run a thread keeps
constexpr unsigned ALIGN_BLOCKS_MAX = 2048;     // workgroups of a launch: 8 per CU of 256; the grid strides over the runs

// bit 7 of every byte of x that is not zero
__device__ inline uint32_t nz_bytes(uint32_t x) { return (((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u; }
// bit k = byte k of x is not zero (the four partial products do not overlap)
__device__ inline uint32_t nz4(uint32_t x) { return ((nz_bytes(x) >> 7) * 0x00204081u >> 21) & 0xFu; }
__device__ inline uint32_t set16(uint4 v) { return nz4(v.x) | nz4(v.y) << 4 | nz4(v.z) << 8 | nz4(v.w) << 12; }

// The predicate on two packed records: lut bit (mv_x | mv_y << 3) = the vectors say it moves, cmask bit class = the class does.
__device__ inline uint32_t moves2(uint32_t x, uint64_t lut, uint32_t cmask) {
    const uint32_t a = (uint32_t)(lut >> ((x >> 3) & 63u)) | cmask >> (x & 7u);
    const uint32_t b = (uint32_t)(lut >> ((x >> 19) & 63u)) | cmask >> ((x >> 16) & 7u);
    return (a & 1u) | (b & 1u) << 1;
}
__device__ inline uint32_t moves8(uint4 v, uint64_t lut, uint32_t cmask) {
    return moves2(v.x, lut, cmask) | moves2(v.y, lut, cmask) << 2 | moves2(v.z, lut, cmask) << 4 | moves2(v.w, lut, cmask) << 6;
}

// the 16 bytes at p (16-byte aligned, inside the array); bytes at or past `end` read as zero
__device__ inline uint4 load16(const uint8_t *p, const uint8_t *end) {
    if (p + 16 <= end) return *reinterpret_cast<const uint4 *>(p);
    uint32_t v[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 16; k++)
        if (p + k < end) v[k >> 2] |= (uint32_t)p[k] << (8 * (k & 3));
    return make_uint4(v[0], v[1], v[2], v[3]);
}

// bit k = label byte a[k] != 0, k in 0 .. 31
__device__ inline uint32_t set_word(const uint8_t *a, const uint8_t *end) {
    const uint32_t off = (uint32_t)(reinterpret_cast<uintptr_t>(a) & 15u);
    const uint8_t *c = a - off;
    uint64_t b = set16(load16(c, end)) | (uint64_t)set16(load16(c + 16, end)) << 16;
    if (off) b |= (uint64_t)set16(load16(c + 32, end)) << 32;
    return (uint32_t)(b >> off);
}

// bit k = the record at a + 2 k moves, k in 0 .. 31 (a is 2-byte aligned)
__device__ inline uint32_t moves_word(const uint8_t *a, const uint8_t *end, uint64_t lut, uint32_t cmask) {
    const uint32_t off = (uint32_t)(reinterpret_cast<uintptr_t>(a) & 15u);
    const uint8_t *c = a - off;
    uint64_t b = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) b |= (uint64_t)moves8(load16(c + 16 * k, end), lut, cmask) << (8 * k);
    if (off) b |= (uint64_t)moves8(load16(c + 64, end), lut, cmask) << 32;
    return (uint32_t)(b >> (off >> 1));
}

// count q of a run: q < RUN * W: both[i][j], i = q / W; then RUN of mov[i]; then RUN of lab[i].  The two plane rows it ANDs.
__device__ inline void count_rows(int q, int W, int S, int *i, int *j, int *ra, int *rb) {
    if (q < RUN * W) {
        *i = q / W, *j = q - *i * W;
        *ra = *i, *rb = RUN + *i + *j;           // set plane p holds frame run0 - S + p: frame i at shift j - S is plane i + j
    } else if (q < RUN * (W + 1)) {
        *i = q - RUN * W, *j = -1;
        *ra = *rb = *i;
    } else {
        *i = q - RUN * (W + 1), *j = -2;
        *ra = *rb = RUN + S + *i;
    }
}

// The recording is frames [first, first + n) of the arrays; this launch serves its frames [at, at + m), outputs indexed from `at`.
// KEEP false: `bits` is never read.
template <bool KEEP>
__global__ __launch_bounds__(BLK) void k_align(const uint16_t *__restrict__ rec, const uint8_t *__restrict__ gt,
                                               const uint8_t *rec_end, const uint8_t *gt_end, const uint32_t *__restrict__ bits,
                                               uint64_t lut, uint32_t cmask, int S, int64_t first, int64_t n, int64_t at, int64_t m,
                                               int hw, uint32_t *__restrict__ both, uint32_t *__restrict__ mov,
                                               uint32_t *__restrict__ lab) {
    __shared__ uint4 planes[ROWS * ROW / 4];
    uint32_t *pl = reinterpret_cast<uint32_t *>(planes);
    const int tid = (int)threadIdx.x;
    const int W = 2 * S + 1, n_counts = RUN * (W + 2), n_rows = 2 * RUN + 2 * S;
    const int64_t runs = (m + RUN - 1) / RUN;
    for (int64_t run = blockIdx.x; run < runs; run += gridDim.x) {
        const int64_t i0 = at + run * RUN;                        // the run's first frame, counted from the recording's
        const int rn = at + m - i0 < RUN ? (int)(at + m - i0) : RUN;   // frames of this run
        uint32_t acc[ACC];
#pragma unroll
        for (int a = 0; a < ACC; a++) acc[a] = 0;
        for (int t0 = 0; t0 < hw; t0 += TILE) {
            const int n_words = (min(TILE, hw - t0) + 31) >> 5;
            for (int it = tid; it < n_rows * (TILE / 32); it += BLK) {
                const int row = it / (TILE / 32), w = it % (TILE / 32);
                const int p0 = t0 + 32 * w;
                uint32_t word = 0;
                if (w < n_words) {
                    uint32_t mask = KEEP ? bits[p0 >> 5] : ~0u;
                    if (hw - p0 < 32) mask &= (1u << (hw - p0)) - 1u;
                    if (row < RUN) {
                        if (row < rn)
                            word = mask & moves_word(reinterpret_cast<const uint8_t *>(rec + (first + i0 + row) * hw + p0), rec_end, lut, cmask);
                    } else {
                        const int64_t i = i0 - S + (row - RUN);   // outside the recording: the plane stays empty
                        if (i >= 0 && i < n) word = mask & set_word(gt + (first + i) * hw + p0, gt_end);
                    }
                }
                pl[row * ROW + w] = word;
            }
            __syncthreads();
            const int n_quads = (n_words + 3) >> 2;               // words n_words .. of a row are zero
#pragma unroll
            for (int a = 0; a < ACC; a++) {
                const int q = a * BLK + tid;
                if (q < n_counts) {
                    int i, j, ra, rb;
                    count_rows(q, W, S, &i, &j, &ra, &rb);
                    const uint4 *pa = planes + ra * (ROW / 4), *pb = planes + rb * (ROW / 4);
                    uint32_t c = 0;
                    for (int k = 0; k < n_quads; k++) {
                        const uint4 x = pa[k], y = pb[k];
                        c += __popc(x.x & y.x) + __popc(x.y & y.y) + __popc(x.z & y.z) + __popc(x.w & y.w);
                    }
                    acc[a] += c;
                }
            }
            __syncthreads();                                      // the planes are written again by the next tile
        }
#pragma unroll
        for (int a = 0; a < ACC; a++) {
            const int q = a * BLK + tid;
            if (q < n_counts) {
                int i, j, ra, rb;
                count_rows(q, W, S, &i, &j, &ra, &rb);
                if (i < rn) {
                    const int64_t o = i0 - at + i;
                    if (j >= 0) both[o * W + j] = acc[a];
                    else if (j == -1) mov[o] = acc[a];
                    else lab[o] = acc[a];
                }
            }
        }
    }
}

}  // namespace

int covahip_align_launch(covahip_ctx *ctx, const uint16_t *d_rec, const uint8_t *d_gt, int64_t capacity, const uint32_t *d_bits,
                         uint64_t lut, uint32_t cmask, int S, int64_t first, int64_t n, int64_t at, int64_t m, int hw,
                         uint32_t *d_both, uint32_t *d_mov, uint32_t *d_lab) {
    static_assert(ROW % 4 == 0 && TILE % 128 == 0 && (RUN * (TILE / 32)) % 64 == 0, "plane rows are read 16 bytes at a time");
    if (S < 0 || S > S_MAX || m < 1 || at < 0 || at + m > n || first < 0 || first + n > capacity) return COVAHIP_ERR_INVALID_ARG;
    // the chunks of a plane word start at or above the arrays' first byte only while the arrays sit on a 16-byte boundary
    if ((reinterpret_cast<uintptr_t>(d_rec) | reinterpret_cast<uintptr_t>(d_gt)) & 15u) return COVAHIP_ERR_INVALID_ARG;
    const uint8_t *rec_end = reinterpret_cast<const uint8_t *>(d_rec + capacity * hw), *gt_end = d_gt + capacity * hw;
    const unsigned blocks = (unsigned)std::min<int64_t>((m + RUN - 1) / RUN, ALIGN_BLOCKS_MAX);
    const hipStream_t s = ctx->stream;
    ProfScope prof(ctx, "train_data_align");
    if (d_bits)
        k_align<true><<<blocks, BLK, 0, s>>>(d_rec, d_gt, rec_end, gt_end, d_bits, lut, cmask, S, first, n, at, m, hw, d_both, d_mov, d_lab);
    else
        k_align<false><<<blocks, BLK, 0, s>>>(d_rec, d_gt, rec_end, gt_end, nullptr, lut, cmask, S, first, n, at, m, hw, d_both, d_mov, d_lab);
    COVAHIP_CHECK_HIP(ctx, hipGetLastError());
    return COVAHIP_OK;
}
