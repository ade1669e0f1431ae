// The post kernels of the MoG labeller: from a call's raw bit planes to filled masks and labels (close 4x4, open 6x6, hole fill,
// then one label per 8x8 block of the working image; include/covahip.h, "MoG labels", steps 3 to 6).  The passes, the resident
// form's body (post_planes) and the banded form's (post_banded) are the device code of mog_dev.h; this file has the kernels
// around them and their two launch functions.  One workgroup per (frame, stream).
//
//   k_mog_grid_post    the resident form: both bit planes in LDS.  640x360 (the reference grid and 1280x720 on either
//                      grid: 2 x 28,800 B) and 320x180 in static LDS, 960x540 in dynamic LDS (2 x 64,800 B, above the static
//                      limit and within a CU's 160 KiB, so one workgroup owns a CU there).  The label loop runs over the
//                      labels, which are more than the words of a plane off 640x360 (8,160 > 8,100; 920 > 900), and the last
//                      label row reads working row 536 (176): the height is no multiple of 8.
//   k_mog_band_post    the banded form, for working images of 1280x720 (90x160 labels) and 1920x1080 (135x240 labels), whose
//                      two planes (230 KB, 518 KB) do not fit LDS.  The planes stay in global memory (L2-resident: 259 KB each
//                      at 1920x1080) and the kernel works on them in bands of `rows` whole rows, in three stages:
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
//     One workgroup reads what another of its threads wrote to global memory only across __syncthreads(), whose fences order
//     global memory within the workgroup; the planes are not __restrict__.
//     <960, 540> exists for tests (covahip_dev_mog_set_post_form): there it can be held against k_mog_grid_post on identical
//     planes.
//   k_mog_any_post     the banded form with the geometry as arguments (covahip_mog_create_any: half of any even source size
//                      from 256 to 4096 in both axes).  A row is roww = ceil(mw / 64) words; mog_dev.h (AnyRows) says how the
//                      bits beyond the image in a row's last word are treated.  The row fill keeps the row's words in LDS,
//                      where the templated form keeps them in registers.
//
// No contraction in this file (see mog_dev.h); it is built with the flags of mog.hip.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include "covahip.h"
#include "internal.h"
#include "mog_dev.h"

namespace {

using namespace mogdev;

// the resident kernel's dynamic LDS: the two planes and the `changed` word, or 0 where they fit the 64 KiB of static LDS
constexpr size_t resident_lds_bytes(size_t nword) { return 2 * nword * 8 + 16 <= 64 * 1024 ? 0 : 2 * nword * 8 + 16; }

// bits: raw masks [F][S][NWORD]; filled_bits: the filled masks, same layout; labels [F][S][LH][LW]; mode, ncover: MogLabelArgs
template <int MW, int MH, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_mog_grid_post(const unsigned long long *__restrict__ bits,
                                                         unsigned long long *__restrict__ filled_bits, uint8_t *__restrict__ labels,
                                                         const int32_t *__restrict__ nvalid, int S, int mode, int ncover) {
    using G = Geom<MW, MH>;
    constexpr int NWORD = G::NWORD, NLAB = G::NLAB, LW = G::LW, ROWW = G::ROWW;
    // The planes as arrays of their own where they fit the static limit: the compiler then knows that a store to T is no store
    // to A, and the 640x360 kernel was measured 5 % slower without that.  Above the limit one dynamic block.
    unsigned long long *A, *T;
    int *changed;
    if constexpr (resident_lds_bytes(NWORD) == 0) {
        __shared__ unsigned long long planes[2][NWORD];
        __shared__ int flag;
        A = planes[0], T = planes[1], changed = &flag;
    } else {
        extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
        A = reinterpret_cast<unsigned long long *>(smem), T = A + NWORD;
        changed = reinterpret_cast<int *>(T + NWORD);
    }
    const int fs = blockIdx.x;
    const int f = fs / S, s = fs % S;
    if (f >= nvalid[s]) return;
    const int tid = threadIdx.x;
    const unsigned long long *src = bits + (size_t)fs * NWORD;
    for (int i = tid; i < NWORD; i += BLOCK) A[i] = src[i];
    __syncthreads();
    post_planes<G, BLOCK>(A, T, changed);
    unsigned long long *dst = filled_bits + (size_t)fs * NWORD;
    uint8_t *lab = labels + (size_t)fs * NLAB;
    if (NLAB == NWORD && mode == COVAHIP_MOG_LABELS_CORNER) {      // 640x360: as many labels as words, one loop writes both
        for (int i = tid; i < NWORD; i += BLOCK) {
            dst[i] = ~T[i];
            lab[i] = label_bit(T, i / LW, i % LW, ROWW);
        }
        return;
    }
    for (int i = tid; i < NWORD; i += BLOCK) dst[i] = ~T[i];
    if (mode == COVAHIP_MOG_LABELS_CORNER) {
        for (int i = tid; i < NLAB; i += BLOCK) lab[i] = label_bit(T, i / LW, i % LW, ROWW);
    } else {
        cover_labels<BLOCK>(T, lab, MW, MH, ROWW, mode, ncover);
    }
}

// 512 lanes: the row fill holds 2 x ROWW 64-bit words per lane (120 VGPRs at 1920 wide) and 512 lanes leave 256 VGPRs each; in the
// general kernel they are one lane per word column and row segment of the column sweep at 32 words
constexpr int BAND_BLOCK = 512;

// the arguments are post_banded's; dynamic LDS: band_lds_bytes
template <int MW, int MH, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_mog_band_post(const unsigned long long *__restrict__ bits, unsigned long long *filled_bits,
                                                         unsigned long long *plane, uint8_t *__restrict__ labels,
                                                         const int32_t *__restrict__ nvalid, int S, int rows, int mode,
                                                         int ncover) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    post_banded<BLOCK>(FixedRows<MW, MH>{}, smem, bits, filled_bits, plane, labels, nvalid, S, rows, mode, ncover);
}

__global__ __launch_bounds__(BAND_BLOCK) void k_mog_any_post(const unsigned long long *__restrict__ bits, unsigned long long *filled_bits,
                                                             unsigned long long *plane, uint8_t *__restrict__ labels,
                                                             const int32_t *__restrict__ nvalid, int S, int rows, int mw, int mh,
                                                             int mode, int ncover) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    post_banded<BAND_BLOCK>(AnyRows(mw, mh), smem, bits, filled_bits, plane, labels, nvalid, S, rows, mode, ncover);
}

}  // namespace

int covahip_mog_grid_post(covahip_ctx *ctx, int mw, const unsigned long long *bits, unsigned long long *filled_bits,
                          uint8_t *labels, const int32_t *nvalid, int S, size_t FS, MogLabelArgs la) {
    return with_geom<G640, G960, G320>(mw, [&](auto g) -> int {
        using G = decltype(g);
        constexpr int BLOCK = G::MW == 960 ? 512 : 256;    // (the results do not depend on it) at 960x540 one workgroup owns the CU
        constexpr size_t lds = resident_lds_bytes(G::NWORD);
        static_assert(lds <= 160 * 1024 - 64, "the two planes must fit a CU's LDS");
        if (int rc = covahip_open_lds(ctx, k_mog_grid_post<G::MW, G::MH, BLOCK>, lds, lds)) return rc;   // (a constant of the kernel)
        return mog_launch(ctx, "mog_post", k_mog_grid_post<G::MW, G::MH, BLOCK>, dim3((unsigned)FS), BLOCK, lds, bits, filled_bits, labels,
                          nvalid, S, la.mode, la.ncover);
    });
}

int covahip_mog_band_post(covahip_ctx *ctx, bool any, int mw, int mh, const unsigned long long *bits, unsigned long long *filled_bits,
                          unsigned long long *plane, uint8_t *labels, const int32_t *nvalid, int S, size_t FS, int rows,
                          MogLabelArgs la) {
    const int pitch = mog_any_pitch(mw);
    if (pitch / 64 * FILL_SEG > BAND_BLOCK || rows < 16 || rows > mh) return COVAHIP_ERR_UNSUPPORTED;
    const size_t lds = band_lds_bytes(pitch, mh, rows);
    if (lds > COVAHIP_MOG_BAND_LDS_MAX) return COVAHIP_ERR_UNSUPPORTED;
    // `dims`: what the kernel takes between `rows` and the label arguments
    const auto launch = [&](const char *scope, auto kernel, auto... dims) -> int {
        // opened to the maximum: `rows` differs between launches
        if (int rc = covahip_open_lds(ctx, kernel, lds, COVAHIP_MOG_BAND_LDS_MAX)) return rc;
        return mog_launch(ctx, scope, kernel, dim3((unsigned)FS), BAND_BLOCK, lds, bits, filled_bits, plane, labels, nvalid, S, rows,
                          dims..., la.mode, la.ncover);
    };
    if (any) return launch("mog_any_post", k_mog_any_post, mw, mh);
    return with_geom<G1920, G1280, G960>(mw, [&](auto g) -> int {
        using G = decltype(g);
        if (mh != G::MH) return COVAHIP_ERR_UNSUPPORTED;
        return launch("mog_band_post", k_mog_band_post<G::MW, G::MH, BAND_BLOCK>);
    });
}
