// MoG labels with MOG2's shadow detection (covahip_mog_set_shadows; include/covahip.h, "MoG labels", step 2a): the SHADOW = true
// instances of all six update kernels of mog_update.h, the dispatch among them, and the kernel behind covahip_mog_shadow_counts.
// They are kept out of mog.hip, mog_grid.hip, mog_band.hip, mog_yuv.hip and mog_any.hip, which hold the kernels a labeller in
// COVAHIP_MOG_SHADOWS_OFF runs and nothing else.
//
//   k_mog_*update<.., true>  the update body with shadow_pixel behind mog2_pixel on the model in registers, and two ballots per
//                            frame: the raw plane the post kernels read (fg && !shadow in DROP, fg in KEEP: a wave-uniform
//                            select on the ballot, so one instance serves both) and the shadow plane, laid out alike.  The post
//                            kernels are the labeller's own, unchanged.
//   k_mog_counts             one workgroup per (frame, stream): popcounts of the two planes, added in LDS.
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

// covahip_mog_shadow_counts: one workgroup per (frame, stream) over the call's planes of nword words each.  counts [F][S][2]:
// the pixels at 127 (the shadow plane's bits; none without one) and at 255 (the raw plane's bits that are no shadow: in DROP
// mode the raw plane holds none anyway, in KEEP mode it holds them all).  The planes have no bit set beyond the image, so these
// are the counts inside it.
constexpr int COUNT_BLOCK = 256;
__global__ __launch_bounds__(COUNT_BLOCK) void k_mog_counts(const unsigned long long *__restrict__ bits,
                                                            const unsigned long long *__restrict__ shadow, unsigned nword,
                                                            uint32_t *__restrict__ counts) {
    __shared__ unsigned acc[2];
    if (threadIdx.x < 2) acc[threadIdx.x] = 0;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * nword;
    unsigned ns = 0, nf = 0;
    for (unsigned i = threadIdx.x; i < nword; i += COUNT_BLOCK) {
        const unsigned long long s = shadow ? shadow[base + i] : 0ull;
        ns += __popcll(s);
        nf += __popcll(bits[base + i] & ~s);
    }
    atomicAdd(&acc[0], ns);
    atomicAdd(&acc[1], nf);
    __syncthreads();
    if (threadIdx.x < 2) counts[2 * (size_t)blockIdx.x + threadIdx.x] = acc[threadIdx.x];
}

template <class G, int KIND>
int launch_yuv(covahip_ctx *ctx, int format, const uint8_t *frames, const covahip_mog_yuv_src &src, const MogUpdateArgs &a) {
    constexpr int NV12 = COVAHIP_MOG_FMT_NV12, I420 = COVAHIP_MOG_FMT_I420;
    const auto kernel = format == NV12 ? k_mog_yuv_update<G::MW, G::MH, NV12, KIND, true> : k_mog_yuv_update<G::MW, G::MH, I420, KIND, true>;
    return mog_launch_update<G>(ctx, "mog_yuv_update", kernel, frames, src, a);
}

}  // namespace

// the dispatch of mog.hip's launch_update and of the five files' own entries, on the SHADOW = true instances
int covahip_mog_shadow_update(covahip_ctx *ctx, const MogShadowRoute &r, const uint8_t *frames, size_t src_bytes,
                              const covahip_mog_yuv_src &src, const MogUpdateArgs &a) {
    constexpr int NV12 = COVAHIP_MOG_FMT_NV12, I420 = COVAHIP_MOG_FMT_I420;
    if (a.shadows == COVAHIP_MOG_SHADOWS_OFF || !a.shadow) return COVAHIP_ERR_INVALID_ARG;
    if (r.format != 0 && r.format != NV12 && r.format != I420) return COVAHIP_ERR_INVALID_ARG;
    if (r.any) {
        if (!r.format) return mog_launch_update_any(ctx, "mog_any_update", k_mog_any_update<true>, r.mw, r.mh, frames, src_bytes, a);
        const auto kernel = r.format == NV12 ? k_mog_any_yuv_update<NV12, true> : k_mog_any_yuv_update<I420, true>;
        return mog_launch_update_any(ctx, "mog_any_yuv_update", kernel, r.mw, r.mh, frames, src, a);
    }
    if (r.format)
        return with_geom<G640, G320, G960, G1280, G1920>(r.mw, [&](auto g) -> int {
            using G = decltype(g);
            if (r.load == MOG_LOAD_HALF) return launch_yuv<G, YUV_HALF>(ctx, r.format, frames, src, a);
            if constexpr (G::MW == 640) {      // copy and centre pick exist at the reference grid's working size only
                if (r.load == MOG_LOAD_COPY) return launch_yuv<G, YUV_COPY>(ctx, r.format, frames, src, a);
                if (r.load == MOG_LOAD_PICK) return launch_yuv<G, YUV_PICK>(ctx, r.format, frames, src, a);
            }
            return COVAHIP_ERR_UNSUPPORTED;
        });
    if (r.mw == G640::MW) {
        const auto kernel = r.load == MOG_LOAD_COPY ? k_mog_update<MOG_LOAD_COPY, true>
                                                    : (r.load == MOG_LOAD_HALF ? k_mog_update<MOG_LOAD_HALF, true> : k_mog_update<MOG_LOAD_PICK, true>);
        return mog_launch_update<G640>(ctx, "mog_update", kernel, frames, src_bytes, a);
    }
    if (r.resident)
        return with_geom<G960, G320>(r.mw, [&](auto g) {
            using G = decltype(g);
            return mog_launch_update<G>(ctx, "mog_update", k_mog_grid_update<G::MW, G::MH, true>, frames, src_bytes, a);
        });
    return with_geom<G1920, G1280>(r.mw, [&](auto g) {
        using G = decltype(g);
        return mog_launch_update<G>(ctx, "mog_band_update", k_mog_band_update<G::MW, G::MH, true>, frames, src_bytes, a);
    });
}

int covahip_mog_counts(covahip_ctx *ctx, const unsigned long long *bits, const unsigned long long *shadow, size_t nword, size_t FS,
                       uint32_t *counts) {
    return mog_launch(ctx, "mog_counts", k_mog_counts, dim3((unsigned)FS), COUNT_BLOCK, 0, bits, shadow, (unsigned)nword, counts);
}
