// MoG labels on the macroblock grid of 2560x1440 and 3840x2160 sources: working images of 1280x720 (90x160 labels) and
// 1920x1080 (135x240 labels), whose two bit planes (230 KB, 518 KB) do not fit a CU's 160 KiB of LDS as k_mog_grid_post keeps
// them.  The planes stay in global memory (L2-resident: 259 KB each at 1920x1080) and the post kernel works on them in bands
// of `rows` whole rows.  MOG2, the morphology passes and the fill loop are the device code of mog_dev.h.
//
//   k_mog_band_update  update_body with LoadHalf, as k_mog_grid_update: a row is 20 (30) waves wide, so a wave's ballot is
//                      still one word of the plane.
//   k_mog_band_post    one workgroup per (frame, stream), three stages:
//     1. morphology, band by band.  Output row y of close 4x4 + open 6x6 depends on input rows y - 10 .. y + 6 (the vertical
//        passes reach 2 + 2 + 3 + 3 rows up and 1 + 1 + 2 + 2 down), so a band y0 .. y1 - 1 stages rows y0 - 10 .. y1 + 5 of
//        the raw plane, clipped to the frame, runs the eight passes on the whole window between two LDS planes and writes its
//        own rows to `plane` (A) and T = ~A & edge to filled_bits.  A row outside the frame is the pass's neutral element; a
//        row of the frame outside the window is not available, and the rows it spoils end exactly outside the band.
//     2. hole fill across bands.  T (the background reached from the frame edge) lives in filled_bits.  A visit of a band ORs
//        ~A & T of the neighbouring bands' adjacent rows into its first and last row and, if that added a pixel (or on the
//        band's first visit), runs the two-phase loop on the band in LDS until nothing changes, then writes T back.  (The
//        loop's column sweep runs on 16 row segments per word column with carries between them, mog_dev.h: 480 lanes at
//        1920 wide where the resident kernel's has 30.)  The
//        bands are visited downwards, then upwards, until a whole such sweep changed nothing.  The fixed point is the
//        background 4-connected to the edge whatever the band plan, so the result equals the resident kernel's bit for bit.
//        Termination is a flag in LDS; there is no iteration cap.
//     3. filled = ~T and the labels, label (r, c) = filled pixel (8 c, 8 r), or by block coverage (cover_labels of mog_dev.h).
//   One workgroup reads what another of its threads wrote to global memory only across __syncthreads(), whose fences order
//   global memory within the workgroup; the planes are not __restrict__.
//
// <960, 540> of the post kernel exists for tests (covahip_dev_mog_set_post_form): there it can be held against
// k_mog_grid_post on identical planes.
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

// bits: raw masks [F][S][NWORD]; filled_bits: the filled masks, same layout (T while the fill runs); plane: the mask after the
// morphology, same layout; labels [F][S][LH][LW]; rows: band height, >= 1; mode, ncover: MogLabelArgs
template <int MW, int MH, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_mog_band_post(const unsigned long long *__restrict__ bits, unsigned long long *filled_bits,
                                                         unsigned long long *plane, uint8_t *__restrict__ labels,
                                                         const int32_t *__restrict__ nvalid, int S, int rows, int mode,
                                                         int ncover) {
    using G = Geom<MW, MH>;
    constexpr int NWORD = G::NWORD, NLAB = G::NLAB, LW = G::LW, ROWW = G::ROWW;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    // the layout band_lds_bytes sizes: flags ([0] fill loop, [1] a visit's seeds, [2] the sweep), carries, two windows
    int *flags = reinterpret_cast<int *>(smem);
    unsigned long long *carry = reinterpret_cast<unsigned long long *>(smem + BAND_FLAG_BYTES);
    unsigned long long *P = reinterpret_cast<unsigned long long *>(smem + BAND_FLAG_BYTES + band_carry_bytes(ROWW));
    const int fs = blockIdx.x;
    const int f = fs / S, s = fs % S;
    if (f >= nvalid[s]) return;
    const int tid = threadIdx.x;
    const unsigned long long *src = bits + (size_t)fs * NWORD;
    unsigned long long *Ag = plane + (size_t)fs * NWORD, *Tg = filled_bits + (size_t)fs * NWORD;
    const int nb = (MH + rows - 1) / rows;

    // 1. morphology
    for (int b = 0; b < nb; b++) {
        const int y0 = b * rows, y1 = y0 + rows < MH ? y0 + rows : MH;
        const int lo = y0 - HALO_UP > 0 ? y0 - HALO_UP : 0, hi = y1 + HALO_DOWN < MH ? y1 + HALO_DOWN : MH;
        const int n = hi - lo;
        unsigned long long *X = P, *Y = P + n * ROWW;
        for (int i = tid; i < n * ROWW; i += BLOCK) X[i] = src[lo * ROWW + i];
        __syncthreads();
        morph_band<ROWW, BLOCK>(X, Y, n);
        for (int i = tid; i < (y1 - y0) * ROWW; i += BLOCK) {
            const int gi = y0 * ROWW + i;
            const unsigned long long a = X[(y0 - lo) * ROWW + i];
            Ag[gi] = a;
            Tg[gi] = ~a & edge_seed<ROWW>(gi / ROWW, gi % ROWW, MH);
        }
        __syncthreads();                                   // X is free for the next band; A and T are visible
    }

    // 2. hole fill: sweeps over the bands, down then up, until one changes nothing
    for (bool first = true;; first = false) {
        if (tid == 0) flags[2] = 0;                        // (every visit starts with a barrier)
        for (int v = 0; v < 2 * nb - 1; v++) {
            const int b = v < nb ? v : 2 * nb - 2 - v;
            const int y0 = b * rows, y1 = y0 + rows < MH ? y0 + rows : MH;
            const int n = y1 - y0;
            if (tid == 0) flags[1] = 0;
            __syncthreads();
            // what the neighbouring bands' adjacent rows add to this band's first and last row
            unsigned long long st = 0, sb = 0;
            if (tid < ROWW) {
                if (y0 > 0) st = ~Ag[y0 * ROWW + tid] & Tg[(y0 - 1) * ROWW + tid] & ~Tg[y0 * ROWW + tid];
                if (y1 < MH) sb = ~Ag[(y1 - 1) * ROWW + tid] & Tg[y1 * ROWW + tid] & ~Tg[(y1 - 1) * ROWW + tid];
                if (st | sb) flags[1] = 1;
            }
            __syncthreads();
            const bool seeded = flags[1] != 0;
            __syncthreads();                               // (the next visit clears the flag)
            // a band visited before is at its own fixed point: without new seeds there is nothing to do in it
            if (!(seeded || (first && v < nb))) continue;
            unsigned long long *A = P, *T = P + n * ROWW;
            for (int i = tid; i < n * ROWW; i += BLOCK) {
                A[i] = Ag[y0 * ROWW + i];
                T[i] = Tg[y0 * ROWW + i];
            }
            __syncthreads();
            if (tid < ROWW) {
                T[tid] |= st;
                T[(n - 1) * ROWW + tid] |= sb;
            }
            const bool grew = fill_band<ROWW, BLOCK>(A, T, n, &flags[0], carry);   // (starts and ends with a barrier)
            if (seeded || grew) {
                for (int i = tid; i < n * ROWW; i += BLOCK) Tg[y0 * ROWW + i] = T[i];
                if (tid == 0) flags[2] = 1;
            }
        }
        __syncthreads();
        const int again = flags[2];
        __syncthreads();
        if (!again) break;
    }

    // 3. labels from T, then filled = ~T in place
    uint8_t *lab = labels + (size_t)fs * NLAB;
    if (mode == COVAHIP_MOG_LABELS_CORNER) {
        for (int i = tid; i < NLAB; i += BLOCK) lab[i] = label_bit(Tg, i / LW, i % LW, ROWW);
    } else {
        cover_labels<BLOCK>(Tg, lab, MW, MH, ROWW, mode, ncover);
    }
    __syncthreads();
    for (int i = tid; i < NWORD; i += BLOCK) Tg[i] = ~Tg[i];
}

// 512 lanes: the row fill holds 2 x ROWW 64-bit words per lane (120 VGPRs at 1920 wide) and 512 lanes leave 256 VGPRs each
constexpr int POST_BLOCK = 512;

}  // namespace

int covahip_mog_band_update(covahip_ctx *ctx, int mw, const uint8_t *frames, size_t src_bytes, const MogUpdateArgs &a) {
    return with_geom<G1920, G1280>(mw, [&](auto g) {
        using G = decltype(g);
        return mog_launch_update<G>(ctx, "mog_band_update", k_mog_band_update<G::MW, G::MH, false>, frames, src_bytes, a);
    });
}

int covahip_mog_band_post(covahip_ctx *ctx, int mw, const unsigned long long *bits, unsigned long long *filled_bits,
                          unsigned long long *plane, uint8_t *labels, const int32_t *nvalid, int S, size_t FS, int rows,
                          MogLabelArgs la) {
    return with_geom<G1920, G1280, G960>(mw, [&](auto g) -> int {
        using G = decltype(g);
        if (rows < 16 || rows > G::MH) return COVAHIP_ERR_UNSUPPORTED;
        const size_t lds = band_lds_bytes(G::MW, G::MH, rows);
        if (lds > COVAHIP_MOG_BAND_LDS_MAX) return COVAHIP_ERR_UNSUPPORTED;
        // opened to the maximum: `rows` differs between launches
        if (int rc = covahip_open_lds(ctx, k_mog_band_post<G::MW, G::MH, POST_BLOCK>, lds, COVAHIP_MOG_BAND_LDS_MAX)) return rc;
        return mog_launch(ctx, "mog_band_post", k_mog_band_post<G::MW, G::MH, POST_BLOCK>, dim3((unsigned)FS), POST_BLOCK, lds, bits,
                          filled_bits, plane, labels, nvalid, S, rows, la.mode, la.ncover);
    });
}
