// MoG labels from decoder surfaces: the update kernels of all seven working geometries on NV12 and I420 frames that lie at a
// row pitch, plane offsets and frame / stream strides of the caller's (covahip_mog_apply_yuv; include/covahip.h, "MoG labels",
// states the conversion).  Everything behind the working pixel is the device code of mog_dev.h, the same as for BGR24 frames:
// mog2_pixel, the ballot word, the model's layout; the post kernels are those of mog.hip, mog_grid.hip and mog_band.hip.
//
//   k_mog_yuv_update<G, FMT, KIND>  update_body_strided (the one update body; LoadYuv::WAIT makes it wait once before its
//                                   loop) with LoadYuv (mog_dev.h): one lane per working pixel and stream, a wave owns 64 consecutive x
//                                   of one row.  KIND is how the working pixel comes from the source:
//     HALF  (the macroblock grid's half sizes and 1280x720 on either grid) a 16-bit word at byte 2x of Y rows 2y and 2y + 1 and,
//           NV12, a 16-bit word at byte 2x of UV row y: three loads of 128 contiguous bytes per wave.  I420 loads one byte each
//           of U and V at x of row y.  The four pixels of the 2x2 block share the chroma sample; each is converted, then the
//           rounded mean per channel.
//     COPY  (640x360 on the reference grid) the Y byte at (x, y) and the chroma sample at (x >> 1, y >> 1).
//     PICK  (1920x1080 on the reference grid) the same at source pixel (3x + 1, 3y + 1).
//   The functor hands back the raw words; they become a pixel where mog2_pixel consumes it, so the loads of frame f + 1 are in
//   flight across frame f's update.  The range (limited / full) is six integers passed by value, not a template axis.
//
// No contraction in this file (see mog_dev.h); it is built with the flags of mog.hip.  The conversion itself is integer.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include "covahip.h"
#include "internal.h"
#include "mog_dev.h"
#include "mog_update.h"

namespace {

using namespace mogdev;

constexpr int HALF = YUV_HALF, COPY = YUV_COPY, PICK = YUV_PICK;   // LoadYuv's kinds (mog_dev.h)
constexpr int NV12 = COVAHIP_MOG_FMT_NV12, I420 = COVAHIP_MOG_FMT_I420;

template <class G, int KIND>
int launch(covahip_ctx *ctx, int format, const uint8_t *frames, const covahip_mog_yuv_src &src, const MogUpdateArgs &a) {
    const auto kernel = format == NV12 ? k_mog_yuv_update<G::MW, G::MH, NV12, KIND, false> : k_mog_yuv_update<G::MW, G::MH, I420, KIND, false>;
    return mog_launch_update<G>(ctx, "mog_yuv_update", kernel, frames, src, a);
}

}  // namespace

int covahip_mog_yuv_update(covahip_ctx *ctx, int format, int load, int mw, const uint8_t *frames, const covahip_mog_yuv_src &src,
                           const MogUpdateArgs &a) {
    if (format != NV12 && format != I420) return COVAHIP_ERR_INVALID_ARG;
    return with_geom<G640, G320, G960, G1280, G1920>(mw, [&](auto g) -> int {
        using G = decltype(g);
        if (load == MOG_LOAD_HALF) return launch<G, HALF>(ctx, format, frames, src, a);
        if constexpr (G::MW == 640) {          // copy and centre pick exist at the reference grid's working size only
            if (load == MOG_LOAD_COPY) return launch<G, COPY>(ctx, format, frames, src, a);
            if (load == MOG_LOAD_PICK) return launch<G, PICK>(ctx, format, frames, src, a);
        }
        return COVAHIP_ERR_UNSUPPORTED;
    });
}
