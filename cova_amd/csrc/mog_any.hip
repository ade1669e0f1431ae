// MoG labels on the macroblock grid of any even source size from 256 to 4096 in both axes (covahip_mog_create_any): the working
// image is mw x mh = half the source, and the geometry is an argument of the kernels, not a template parameter.  A row of the
// bit plane is roww = ceil(mw / 64) words, and everything per pixel lies on that padded pitch of 64 roww: pixel (x, y) is lane
// p = y * 64 roww + x of the update grid and entry p of the model's arrays (W[5][P], V[5][P], M[5][3][P] f32, nmodes[P] u8 with
// P = 64 roww mh, as Geom lays them out at its NPIX).  The entries at x >= mw are never read or written.
//
//   k_mog_any_update  the update body of mog_dev.h with runtime sizes (update_any, in mog_update.h with the kernel): a wave
//                     is 64 consecutive x of one padded row, so its ballot is one plane word.  Lanes at x >= mw load nothing,
//                     keep no model and ballot 0; the last block may be partial (P is a multiple of 64, not of 256).  BGR24
//                     (the 2x2 mean of LoadHalf) and, with
//                     LoadYuv<.., HALF> of mog_dev.h, NV12 / I420.  mog2_pixel is the one of mog_dev.h.
//   k_mog_any_post    k_mog_band_post (mog_band.hip) with runtime sizes: planes in global memory, the morphology band by band
//                     with the 10-row-up / 6-row-down halo, the hole fill swept over the bands to its fixed point, then the
//                     labels.  The row fill keeps the row's words in LDS, where the templated form keeps them in registers.
//
// The bits at x >= mw of a row's last word (`tail` = the mask of the bits inside the image) are outside the image:
//   * every horizontal pass reads them as its neutral element (0 for dilate, 1 for erode) whatever the pass before left there;
//     a vertical pass works column by column, so what it leaves there comes from there only;
//   * the planes the kernel writes (plane, filled_bits) have them clear;
//   * for the fill they are wall: the band's copy of A in LDS has them set, so ~A, the background the fill walks through, has
//     them clear; the seeds are the image's edge pixels, column mw - 1 on the right.
//
// No contraction in this file (see mog_dev.h); it is built with the flags of mog.hip.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include "covahip.h"
#include "internal.h"
#include "mog_dev.h"
#include "mog_update.h"

namespace {

using namespace mogdev;
using u64 = unsigned long long;

constexpr int POST_BLOCK = 512;                // one lane per word column and row segment of the column sweep at 32 words

// ------------------------------------------------------------------------------------------------ post passes, runtime width
// hpass_band / vpass_band of mog_dev.h on rows of `roww` words whose last word holds the image in the bits of `tail`
template <bool DIL, int K>
__device__ __forceinline__ void hpass_any(const u64 *in, u64 *out, int nrows, int roww, u64 tail) {
    constexpr int A = K / 2, B = K - 1 - K / 2;
    constexpr u64 NEU = DIL ? 0ull : ~0ull;
    const int nword = nrows * roww;
    for (int i = threadIdx.x; i < nword; i += POST_BLOCK) {
        const int w = i % roww;
        // the last word's bits beyond the image read as the neutral element (w - 1 is never the last word)
        const u64 c = w < roww - 1 ? in[i] : (DIL ? in[i] & tail : in[i] | ~tail);
        const u64 pv = w > 0 ? in[i - 1] : NEU;
        const u64 nx = w < roww - 2 ? in[i + 1] : (w == roww - 2 ? (DIL ? in[i + 1] & tail : in[i + 1] | ~tail) : NEU);
        u64 r = c;
#pragma unroll
        for (int d = -A; d <= B; d++) {
            if (d == 0) continue;
            const u64 v = d > 0 ? (c >> d) | (nx << (64 - d)) : (c << -d) | (pv >> (64 + d));
            r = DIL ? (r | v) : (r & v);
        }
        out[i] = r;
    }
}

template <bool DIL, int K>
__device__ __forceinline__ void vpass_any(const u64 *in, u64 *out, int nrows, int roww) {
    constexpr int A = K / 2, B = K - 1 - K / 2;
    constexpr u64 NEU = DIL ? 0ull : ~0ull;
    const int nword = nrows * roww;
    for (int i = threadIdx.x; i < nword; i += POST_BLOCK) {
        const int y = i / roww;
        u64 r = in[i];
#pragma unroll
        for (int d = -A; d <= B; d++) {
            if (d == 0) continue;
            const u64 v = (y + d >= 0 && y + d < nrows) ? in[i + d * roww] : NEU;
            r = DIL ? (r | v) : (r & v);
        }
        out[i] = r;
    }
}

template <bool DIL, int K>
__device__ __forceinline__ void morph_pass_any(u64 *X, u64 *Y, int nrows, int roww, u64 tail) {
    hpass_any<DIL, K>(X, Y, nrows, roww, tail);
    __syncthreads();
    vpass_any<DIL, K>(Y, X, nrows, roww);
    __syncthreads();
}

// the hole fill's seed in word w of row y: the image's edge pixels, rows 0 and mh - 1, columns 0 and mw - 1
__device__ __forceinline__ u64 edge_seed_any(int y, int w, int mw, int mh, int roww, u64 tail) {
    u64 edge = (y == 0 || y == mh - 1) ? ~0ull : 0ull;
    if (w == 0) edge |= 1ull;
    if (w == roww - 1) edge = (edge | 1ull << ((mw - 1) & 63)) & tail;
    return edge;
}

// col_sweep_band of mog_dev.h with a runtime row width: roww * FILL_SEG <= POST_BLOCK
template <bool DOWN>
__device__ __forceinline__ bool col_sweep_any(const u64 *A, u64 *T, int nrows, int roww, u64 *carry) {
    const int tid = threadIdx.x;
    const bool active = tid < roww * FILL_SEG;
    const int w = tid % roww, sg = tid / roww;
    const int len = (nrows + FILL_SEG - 1) / FILL_SEG;
    const int ya = sg * len < nrows ? sg * len : nrows, yb = ya + len < nrows ? ya + len : nrows;   // this lane's rows (may be none)
    u64 *out = carry, *pass = carry + FILL_SEG * roww;
    bool ch = false;
    if (active) {
        u64 r = 0, p = ~0ull;
        for (int k = 0; k < yb - ya; k++) {
            const int i = (DOWN ? ya + k : yb - 1 - k) * roww + w;
            const u64 na = ~A[i], old = T[i], nw = old | (na & r);
            if (nw != old) {
                T[i] = nw;
                ch = true;
            }
            r = nw;
            p &= na;
        }
        out[tid] = r;
        pass[tid] = p;
    }
    __syncthreads();
    if (active) {
        u64 d = 0;                             // what the segments walked before this one carry into it
        if (DOWN)
            for (int k = 0; k < sg; k++) d = out[k * roww + w] | (pass[k * roww + w] & d);
        else
            for (int k = FILL_SEG - 1; k > sg; k--) d = out[k * roww + w] | (pass[k * roww + w] & d);
        for (int k = 0; k < yb - ya && d; k++) {
            const int i = (DOWN ? ya + k : yb - 1 - k) * roww + w;
            d &= ~A[i];
            const u64 old = T[i], nw = old | d;
            if (nw != old) {
                T[i] = nw;
                ch = true;
            }
        }
    }
    __syncthreads();
    return ch;
}

// fill_band of mog_dev.h with a runtime row width.  The row fill works on T in LDS word by word: the pass towards higher x
// leaves the seeds and what they reached in T, the pass towards lower x starts from that.
__device__ __forceinline__ bool fill_any(const u64 *A, u64 *T, int nrows, int roww, int *changed, u64 *carry) {
    const int tid = threadIdx.x;
    bool any = false;
    for (;;) {
        if (tid == 0) *changed = 0;
        __syncthreads();
        const bool chd = col_sweep_any<true>(A, T, nrows, roww, carry);
        const bool chu = col_sweep_any<false>(A, T, nrows, roww, carry);
        if (chd || chu) *changed = 1;
        for (int y = tid; y < nrows; y += POST_BLOCK) {
            const u64 *a = A + y * roww;
            u64 *t = T + y * roww;
            bool ch = false;
            u64 c = 0;
            for (int w = 0; w < roww; w++) {           // towards higher x: m + seeds ripples through each seeded run
                const u64 m = ~a[w], sd = t[w];
                const u64 s1 = sd | (c & m & 1ull);
                const u64 r = m + s1;
                const u64 nw = ((r ^ m) | s1) & m;     // a superset of sd
                c = r < m ? 1ull : 0ull;               // carried out of bit 63: the run goes on in the next word
                if (nw != sd) {
                    t[w] = nw;
                    ch = true;
                }
            }
            c = 0;
            for (int w = roww - 1; w >= 0; w--) {      // towards lower x: the same on bit-reversed words
                const u64 rm = __builtin_bitreverse64(~a[w]), sd = t[w];
                const u64 s1 = __builtin_bitreverse64(sd) | (c & rm & 1ull);
                const u64 r = rm + s1;
                const u64 nw = __builtin_bitreverse64(((r ^ rm) | s1) & rm);
                c = r < rm ? 1ull : 0ull;
                if (nw != sd) {
                    t[w] = nw;
                    ch = true;
                }
            }
            if (ch) *changed = 1;
        }
        __syncthreads();
        const int again = *changed;
        __syncthreads();
        if (!again) break;
        any = true;
    }
    return any;
}

// bits: raw masks [F][S][roww mh]; filled_bits: the filled masks, same layout (T while the fill runs); plane: the mask after
// the morphology, same layout; labels [F][S][lh][lw]; rows: band height, >= 1; mode, ncover: MogLabelArgs.
// Dynamic LDS: band_lds_bytes(64 roww, mh, rows).
__global__ __launch_bounds__(POST_BLOCK) void k_mog_any_post(const u64 *__restrict__ bits, u64 *filled_bits, u64 *plane,
                                                             uint8_t *__restrict__ labels, const int32_t *__restrict__ nvalid, int S,
                                                             int rows, int mw, int mh, int mode, int ncover) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int roww = (mw + 63) / 64, nword = roww * mh, lw = (mw + 7) / 8, nlab = lw * ((mh + 7) / 8);
    const u64 tail = (mw & 63) ? (1ull << (mw & 63)) - 1 : ~0ull;
    // the layout band_lds_bytes sizes: flags ([0] fill loop, [1] a visit's seeds, [2] the sweep), carries, two windows
    int *flags = reinterpret_cast<int *>(smem);
    u64 *carry = reinterpret_cast<u64 *>(smem + BAND_FLAG_BYTES);
    u64 *P = reinterpret_cast<u64 *>(smem + BAND_FLAG_BYTES + band_carry_bytes(roww));
    const int fs = blockIdx.x;
    const int f = fs / S, s = fs % S;
    if (f >= nvalid[s]) return;
    const int tid = threadIdx.x;
    const u64 *src = bits + (size_t)fs * nword;
    u64 *Ag = plane + (size_t)fs * nword, *Tg = filled_bits + (size_t)fs * nword;
    const int nb = (mh + rows - 1) / rows;

    // 1. morphology: close 4x4, open 6x6 on the band and its halo, clipped to the frame
    for (int b = 0; b < nb; b++) {
        const int y0 = b * rows, y1 = y0 + rows < mh ? y0 + rows : mh;
        const int lo = y0 - HALO_UP > 0 ? y0 - HALO_UP : 0, hi = y1 + HALO_DOWN < mh ? y1 + HALO_DOWN : mh;
        const int n = hi - lo;
        u64 *X = P, *Y = P + n * roww;
        for (int i = tid; i < n * roww; i += POST_BLOCK) X[i] = src[lo * roww + i];
        __syncthreads();
        morph_pass_any<true, 4>(X, Y, n, roww, tail);
        morph_pass_any<false, 4>(X, Y, n, roww, tail);
        morph_pass_any<false, 6>(X, Y, n, roww, tail);
        morph_pass_any<true, 6>(X, Y, n, roww, tail);
        for (int i = tid; i < (y1 - y0) * roww; i += POST_BLOCK) {
            const int gi = y0 * roww + i, w = gi % roww;
            const u64 a = X[(y0 - lo) * roww + i] & (w == roww - 1 ? tail : ~0ull);
            Ag[gi] = a;
            Tg[gi] = ~a & edge_seed_any(gi / roww, w, mw, mh, roww, tail);
        }
        __syncthreads();                                   // X is free for the next band; A and T are visible
    }

    // 2. hole fill: sweeps over the bands, down then up, until one changes nothing
    for (bool first = true;; first = false) {
        if (tid == 0) flags[2] = 0;                        // (every visit starts with a barrier)
        for (int v = 0; v < 2 * nb - 1; v++) {
            const int b = v < nb ? v : 2 * nb - 2 - v;
            const int y0 = b * rows, y1 = y0 + rows < mh ? y0 + rows : mh;
            const int n = y1 - y0;
            if (tid == 0) flags[1] = 0;
            __syncthreads();
            // what the neighbouring bands' adjacent rows add to this band's first and last row (T has no bit beyond the image)
            u64 st = 0, sb = 0;
            if (tid < roww) {
                if (y0 > 0) st = ~Ag[y0 * roww + tid] & Tg[(y0 - 1) * roww + tid] & ~Tg[y0 * roww + tid];
                if (y1 < mh) sb = ~Ag[(y1 - 1) * roww + tid] & Tg[y1 * roww + tid] & ~Tg[(y1 - 1) * roww + tid];
                if (st | sb) flags[1] = 1;
            }
            __syncthreads();
            const bool seeded = flags[1] != 0;
            __syncthreads();                               // (the next visit clears the flag)
            // a band visited before is at its own fixed point: without new seeds there is nothing to do in it
            if (!(seeded || (first && v < nb))) continue;
            u64 *A = P, *T = P + n * roww;
            for (int i = tid; i < n * roww; i += POST_BLOCK) {
                A[i] = Ag[y0 * roww + i] | (i % roww == roww - 1 ? ~tail : 0ull);   // beyond the image is wall
                T[i] = Tg[y0 * roww + i];
            }
            __syncthreads();
            if (tid < roww) {
                T[tid] |= st;
                T[(n - 1) * roww + tid] |= sb;
            }
            const bool grew = fill_any(A, T, n, roww, &flags[0], carry);   // (starts and ends with a barrier)
            if (seeded || grew) {
                for (int i = tid; i < n * roww; i += POST_BLOCK) Tg[y0 * roww + i] = T[i];
                if (tid == 0) flags[2] = 1;
            }
        }
        __syncthreads();
        const int again = flags[2];
        __syncthreads();
        if (!again) break;
    }

    // 3. labels from T (the bits beyond the image are still clear in it: cover_labels masks them itself), then filled = ~T
    // inside the image, in place
    uint8_t *lab = labels + (size_t)fs * nlab;
    if (mode == COVAHIP_MOG_LABELS_CORNER) {
        for (int i = tid; i < nlab; i += POST_BLOCK) lab[i] = label_bit(Tg, i / lw, i % lw, roww);
    } else {
        cover_labels<POST_BLOCK>(Tg, lab, mw, mh, roww, mode, ncover);
    }
    __syncthreads();
    for (int i = tid; i < nword; i += POST_BLOCK) Tg[i] = ~Tg[i] & (i % roww == roww - 1 ? tail : ~0ull);
}

}  // namespace

int covahip_mog_any_update(covahip_ctx *ctx, int mw, int mh, const uint8_t *frames, size_t src_bytes, const MogUpdateArgs &a) {
    return mog_launch_update_any(ctx, "mog_any_update", k_mog_any_update<false>, mw, mh, frames, src_bytes, a);
}

int covahip_mog_any_yuv_update(covahip_ctx *ctx, int format, int mw, int mh, const uint8_t *frames, const covahip_mog_yuv_src &src,
                               const MogUpdateArgs &a) {
    if (format != COVAHIP_MOG_FMT_NV12 && format != COVAHIP_MOG_FMT_I420) return COVAHIP_ERR_INVALID_ARG;
    const auto kernel = format == COVAHIP_MOG_FMT_NV12 ? k_mog_any_yuv_update<COVAHIP_MOG_FMT_NV12, false>
                                                       : k_mog_any_yuv_update<COVAHIP_MOG_FMT_I420, false>;
    return mog_launch_update_any(ctx, "mog_any_yuv_update", kernel, mw, mh, frames, src, a);
}

int covahip_mog_any_post(covahip_ctx *ctx, int mw, int mh, const unsigned long long *bits, unsigned long long *filled_bits,
                         unsigned long long *plane, uint8_t *labels, const int32_t *nvalid, int S, size_t FS, int rows,
                         MogLabelArgs la) {
    const int pitch = mog_any_pitch(mw);
    if (pitch / 64 * FILL_SEG > POST_BLOCK || rows < 16 || rows > mh) return COVAHIP_ERR_UNSUPPORTED;
    const size_t lds = band_lds_bytes(pitch, mh, rows);
    if (lds > COVAHIP_MOG_BAND_LDS_MAX) return COVAHIP_ERR_UNSUPPORTED;
    // opened to the maximum: `rows` differs between launches
    if (int rc = covahip_open_lds(ctx, k_mog_any_post, lds, COVAHIP_MOG_BAND_LDS_MAX)) return rc;
    return mog_launch(ctx, "mog_any_post", k_mog_any_post, dim3((unsigned)FS), POST_BLOCK, lds, bits, filled_bits, plane, labels, nvalid, S,
                      rows, mw, mh, la.mode, la.ncover);
}
