// The MoG labeller's model as an object that is only read (include/covahip.h, "MoG labels": frozen labelling, the background
// image): the FROZEN = true instances of all five update kernels of mog_update.h, without and with the shadow test, through the
// dispatch's, and the kernel behind covahip_mog_background.  They are kept out of mog_update.hip and mog_shadow.hip, which hold the
// kernels a labeller with no frozen stream runs and nothing else.
//
//   k_mog_*update<.., true>  the update body up to its write-back: the model is read once per call into registers, every frame of
//                            the call is classified against it (frozen_pixel; with SHADOW shadow_pixel behind it, on the model
//                            as it is) and nothing of it is written.  No read of `par`, no division.
//   k_mog_background         one lane per pixel of the padded pitch and stream: the weighted mean of the modes that make up the
//                            background, as u8 BGR.  The geometry and the pitch are arguments: one kernel serves every labeller.
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

// covahip_mog_background: grid (ceil(pitch * mh / BG_BLOCK), streams of the call).  state: the first stream's model, laid out
// as the update kernels have it at P = pitch * mh, one stream every state_bytes; out: u8 [streams][mh][mw][3], dense.  A lane at
// x >= mw does nothing.  The modes are read as far as the walk goes: W and the three means of mode k only where the sum of the
// weights before it has not passed TB.  A lane stores its three bytes one by one: a wave's stores cover 192 contiguous bytes.
constexpr int BG_BLOCK = 256;
__global__ __launch_bounds__(BG_BLOCK) void k_mog_background(const uint8_t *__restrict__ state, size_t state_bytes, int pitch, int mw,
                                                             int mh, uint8_t *__restrict__ out) {
    const size_t P = (size_t)pitch * mh;
    const size_t p = (size_t)blockIdx.x * BG_BLOCK + threadIdx.x;
    if (p >= P) return;
    const int x = (int)(p % pitch), y = (int)(p / pitch);
    if (x >= mw) return;
    const uint8_t *st = state + (size_t)blockIdx.y * state_bytes;
    const float *gW = reinterpret_cast<const float *>(st), *gM = gW + 2 * NMIX * P;
    const int nm = st[(size_t)5 * NMIX * 4 * P + p];
    float acc[3] = {0.f, 0.f, 0.f}, tw = 0.f;
    bool done = false;
#pragma unroll
    for (int k = 0; k < NMIX; k++) {
        if (k < nm && !done) {
            const float w = gW[(size_t)k * P + p];
#pragma unroll
            for (int c = 0; c < 3; c++) acc[c] = acc[c] + w * gM[(size_t)(k * 3 + c) * P + p];
            tw = tw + w;
            if (tw > TB) done = true;
        }
    }
    const float inv = fabsf(tw) > FLT_EPSILON ? div_rn(1.f, tw) : 0.f;
    uint8_t *o = out + ((size_t)blockIdx.y * mh * mw + (size_t)y * mw + x) * 3;
#pragma unroll
    for (int c = 0; c < 3; c++) o[c] = (uint8_t)sat8(__float2int_rn(acc[c] * inv));   // round half to even, then saturate
}

}  // namespace

MOG_ROUTE_INSTANCE(false, true);
MOG_ROUTE_INSTANCE(true, true);

int covahip_mog_background_launch(covahip_ctx *ctx, const uint8_t *state, size_t state_bytes, int pitch, int mw, int mh, int streams,
                                  uint8_t *out) {
    const size_t P = (size_t)pitch * mh;
    return mog_launch(ctx, "mog_background", k_mog_background, dim3((unsigned)((P + BG_BLOCK - 1) / BG_BLOCK), streams), BG_BLOCK, 0, state,
                      state_bytes, pitch, mw, mh, out);
}
