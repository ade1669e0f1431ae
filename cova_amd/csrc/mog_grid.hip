// MoG labels on the source's macroblock grid (COVAHIP_MOG_GRID_MACROBLOCK): the working image is half the source in both axes
// ((a + b + c + d + 2) >> 2 per channel over the 2x2 block, the rule of the reference grid's 1280x720 case) and there is one
// label per 16x16 macroblock of the source, i.e. per 8x8 block of the working image.  MOG2, morphology, hole fill and the
// subsample are the device code of mog_dev.h, the same as in mog.hip, instantiated here for
//   1920x1080 -> 960x540 working, 68x120 labels     and     640x360 -> 320x180 working, 23x40 labels.
// (1280x720 -> 640x360 is the reference grid itself and runs mog.hip's kernels.)
//
//   k_mog_grid_update  as k_mog_update: one lane per working pixel and stream, the five modes in registers across the call.  A
//                      row is 15 (5) waves wide, so a wave's ballot is still one word of the plane.
//   k_mog_grid_post    one workgroup per (stream, frame) with both bit planes in dynamic LDS: 2 x 64,800 B at 960x540, above
//                      the static limit and within a CU's 160 KiB, so one workgroup owns a CU there.  The label loop runs
//                      over the labels, which are more than the words of a plane here (8,160 > 8,100; 920 > 900), and the
//                      last label row reads working row 536 (176): the height is no multiple of 8.
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

// bits: raw masks [F][S][NWORD]; filled_bits: the filled masks, same layout; labels [F][S][LH][LW]; mode, ncover: MogLabelArgs
template <int MW, int MH, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_mog_grid_post(const unsigned long long *__restrict__ bits,
                                                         unsigned long long *__restrict__ filled_bits, uint8_t *__restrict__ labels,
                                                         const int32_t *__restrict__ nvalid, int S, int mode, int ncover) {
    using G = Geom<MW, MH>;
    constexpr int NWORD = G::NWORD, NLAB = G::NLAB, LW = G::LW, ROWW = G::ROWW;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    unsigned long long *A = reinterpret_cast<unsigned long long *>(smem), *T = A + NWORD;
    int *changed = reinterpret_cast<int *>(T + NWORD);
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
    for (int i = tid; i < NWORD; i += BLOCK) dst[i] = ~T[i];
    if (mode == COVAHIP_MOG_LABELS_CORNER) {
        for (int i = tid; i < NLAB; i += BLOCK) lab[i] = label_bit(T, i / LW, i % LW, ROWW);
    } else {
        cover_labels<BLOCK>(T, lab, MW, MH, ROWW, mode, ncover);
    }
}

}  // namespace

int covahip_mog_grid_update(covahip_ctx *ctx, int mw, const uint8_t *frames, size_t src_bytes, const MogUpdateArgs &a) {
    return with_geom<G960, G320>(mw, [&](auto g) {
        using G = decltype(g);
        return mog_launch_update<G>(ctx, "mog_update", k_mog_grid_update<G::MW, G::MH, false>, frames, src_bytes, a);
    });
}

int covahip_mog_grid_post(covahip_ctx *ctx, int mw, const unsigned long long *bits, unsigned long long *filled_bits,
                          uint8_t *labels, const int32_t *nvalid, int S, size_t FS, MogLabelArgs la) {
    return with_geom<G960, G320>(mw, [&](auto g) -> int {
        using G = decltype(g);
        constexpr int BLOCK = G::MW == 960 ? 512 : 256;    // (the results do not depend on it) at 960x540 one workgroup owns the CU
        constexpr size_t lds = (size_t)2 * G::NWORD * 8 + 16;   // the two planes and the `changed` word
        static_assert(lds <= 160 * 1024 - 64, "the two planes must fit a CU's LDS");
        if (int rc = covahip_open_lds(ctx, k_mog_grid_post<G::MW, G::MH, BLOCK>, lds, lds)) return rc;   // (a constant of the kernel)
        return mog_launch(ctx, "mog_post", k_mog_grid_post<G::MW, G::MH, BLOCK>, dim3((unsigned)FS), BLOCK, lds, bits, filled_bits, labels,
                          nvalid, S, la.mode, la.ncover);
    });
}

