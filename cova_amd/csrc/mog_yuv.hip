// MoG labels from decoder surfaces: the update kernels of all seven working geometries on NV12 and I420 frames that lie at a
// row pitch, plane offsets and frame / stream strides of the caller's (covahip_mog_apply_yuv; include/covahip.h, "MoG labels",
// states the conversion).  Everything behind the working pixel is the device code of mog_dev.h, the same as for BGR24 frames:
// mog2_pixel, the ballot word, the model's layout; the post kernels are those of mog.hip, mog_grid.hip and mog_band.hip.
//
//   k_mog_yuv_update<G, FMT, KIND>  update_body_strided (the one update body; LoadYuv::WAIT makes it wait once before its
//                                   loop) with LoadYuv: one lane per working pixel and stream, a wave owns 64 consecutive x
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

namespace {

using namespace mogdev;

enum { HALF = 0, COPY = 1, PICK = 2 };
constexpr int NV12 = COVAHIP_MOG_FMT_NV12, I420 = COVAHIP_MOG_FMT_I420;

__device__ __forceinline__ int sat8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

template <int FMT, int KIND>
struct LoadYuv {
    static constexpr bool WAIT = true;         // the body waits for the model and the first frame once, before its loop
    covahip_mog_yuv_src a;
    struct At { long long y, u, v; };          // bytes from the plane's first byte: Y sample(s), U (NV12: the UV pair), V
    struct Raw { unsigned y0, y1, u, v; };     // HALF: two Y pairs; else y0 = Y.  NV12: u = the UV pair as loaded

    __device__ __forceinline__ At at(int x, int y) const {
        int yr, yb, cr, cc;                        // Y row and byte, chroma row and sample
        if constexpr (KIND == HALF) {
            yr = 2 * y, yb = 2 * x, cr = y, cc = x;
        } else if constexpr (KIND == COPY) {
            yr = y, yb = x, cr = y >> 1, cc = x >> 1;
        } else {
            yr = 3 * y + 1, yb = 3 * x + 1, cr = yr >> 1, cc = yb >> 1;
        }
        At t;
        t.y = (long long)yr * a.pitch[0] + yb;
        if constexpr (FMT == NV12) {
            t.u = (long long)cr * a.pitch[1] + 2 * cc;
            t.v = 0;
        } else {
            t.u = (long long)cr * a.pitch[1] + cc;
            t.v = (long long)cr * a.pitch[2] + cc;
        }
        return t;
    }

    __device__ __forceinline__ Raw operator()(const uint8_t *__restrict__ fr, const At &t) const {
        Raw r;
        const uint8_t *py = fr + a.off[0] + t.y, *pu = fr + a.off[1] + t.u;
        if constexpr (KIND == HALF) {
            r.y0 = *reinterpret_cast<const uint16_t *>(py);
            r.y1 = *reinterpret_cast<const uint16_t *>(py + a.pitch[0]);
        } else {
            r.y0 = *py;
            r.y1 = 0;
        }
        if constexpr (FMT == NV12) {
            r.u = *reinterpret_cast<const uint16_t *>(pu);
            r.v = 0;
        } else {
            r.u = *pu;
            r.v = *(fr + a.off[2] + t.v);
        }
        return r;
    }

    __device__ __forceinline__ Px px(const Raw &r) const {
        const int U = FMT == NV12 ? (int)(r.u & 255u) : (int)r.u, V = FMT == NV12 ? (int)(r.u >> 8) : (int)r.v;
        // every factor fits 24 bits (|uu|, |vv| <= 128, Y <= 255, the constants < 2^22) and every product 32, so the full-rate
        // 24-bit multiply gives the int32 product of the header exactly
        const int uu = U - 128, vv = V - 128, h = 1 << 19;
        const int cb = h + __mul24(a.bu, uu), cg = h - __mul24(a.gv, vv) - __mul24(a.gu, uu), cr = h + __mul24(a.rv, vv);
        auto yy = [&](unsigned Y) {
            const int d = (int)Y - a.ysub;
            return __mul24(d < 0 ? 0 : d, a.ymul);
        };
        if constexpr (KIND == HALF) {
            const int q[4] = {yy(r.y0 & 255u), yy(r.y0 >> 8), yy(r.y1 & 255u), yy(r.y1 >> 8)};
            int b = 2, g = 2, c = 2;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                b += sat8((q[i] + cb) >> 20);
                g += sat8((q[i] + cg) >> 20);
                c += sat8((q[i] + cr) >> 20);
            }
            return {(float)(b >> 2), (float)(g >> 2), (float)(c >> 2)};
        } else {
            const int q = yy(r.y0);
            return {(float)sat8((q + cb) >> 20), (float)sat8((q + cg) >> 20), (float)sat8((q + cr) >> 20)};
        }
    }
};

// frames: the launch's first frame of stream 0; par: (alphaT, prune) [F][S] of the call; bits: raw masks [F][S][G::NWORD]
template <int MW, int MH, int FMT, int KIND>
__global__ __launch_bounds__(UPD_BLOCK) void k_mog_yuv_update(const uint8_t *__restrict__ frames, covahip_mog_yuv_src src,
                                                              uint8_t *__restrict__ state, const float2 *__restrict__ par,
                                                              const int32_t *__restrict__ nvalid, int f0, int nf, int S, float Tb,
                                                              unsigned long long *__restrict__ bits) {
    update_body_strided<Geom<MW, MH>>(LoadYuv<FMT, KIND>{src}, frames, src.frame_stride, src.stream_stride, state, par, nvalid, f0,
                                      nf, S, Tb, bits);
}

template <class G, int KIND>
int launch(covahip_ctx *ctx, int format, const uint8_t *frames, const covahip_mog_yuv_src &src, const MogUpdateArgs &a) {
    const auto kernel = format == NV12 ? k_mog_yuv_update<G::MW, G::MH, NV12, KIND> : k_mog_yuv_update<G::MW, G::MH, I420, KIND>;
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
