// MoG labels with MOG2's shadow detection (covahip_mog_set_shadows; include/covahip.h, "MoG labels", step 2a): the SHADOW = true
// instances of all five update kernels of mog_update.h, through the dispatch's, and the kernel behind covahip_mog_shadow_counts.
// They are kept out of mog_update.hip, which holds the kernels a labeller in COVAHIP_MOG_SHADOWS_OFF runs and nothing else.
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

}  // namespace

MOG_ROUTE_INSTANCE(true, false);

int covahip_mog_counts(covahip_ctx *ctx, const unsigned long long *bits, const unsigned long long *shadow, size_t nword, size_t FS,
                       uint32_t *counts) {
    return mog_launch(ctx, "mog_counts", k_mog_counts, dim3((unsigned)FS), COUNT_BLOCK, 0, bits, shadow, (unsigned)nword, counts);
}
