// The update kernels of the MoG labeller, all five, as templates over `bool SHADOW` (mog_dev.h: update_body_strided, shadow_pixel),
// and the one dispatch among them (mog_launch_route):
//   k_mog_update          the reference grid's 640x360 working frames: one lane per working-size pixel and stream.  The five
//                         modes (weight, variance, mean) are read once per call into registers, every frame of the call is
//                         applied to them, and they are written back once.  The source is resized while it is read (copy,
//                         2x2 mean or centre pick).  The foreground of a wave's 64 pixels (a row is exactly ten waves wide) is
//                         one __ballot word: a frame's raw mask is 3,600 words, 28.8 KB.
//   k_mog_grid_update     the macroblock grid's other working sizes (half the source: the 2x2 mean of LoadHalf): 960x540 and
//                         320x180, and 1280x720 and 1920x1080 of 1440p and 4K sources.  A row is 15, 5, 20 or 30 waves wide, so
//                         a wave's ballot is still one word of the plane.
//   k_mog_yuv_update      all of those on NV12 / I420 surfaces that lie at a row pitch, plane offsets and frame / stream strides
//                         of the caller's (covahip_mog_apply_yuv; include/covahip.h, "MoG labels", states the conversion):
//                         update_body_strided with LoadYuv of mog_dev.h, whose WAIT makes it wait once before its loop.  KIND
//                         is how the working pixel comes from the source:
//     HALF  (the macroblock grid's half sizes and 1280x720 on either grid) a 16-bit word at byte 2x of Y rows 2y and 2y + 1 and,
//           NV12, a 16-bit word at byte 2x of UV row y: three loads of 128 contiguous bytes per wave.  I420 loads one byte each
//           of U and V at x of row y.  The four pixels of the 2x2 block share the chroma sample; each is converted, then the
//           rounded mean per channel.
//     COPY  (640x360 on the reference grid) the Y byte at (x, y) and the chroma sample at (x >> 1, y >> 1).
//     PICK  (1920x1080 on the reference grid) the same at source pixel (3x + 1, 3y + 1).
//                         The functor hands back the raw words; they become a pixel where mog2_pixel consumes it, so the loads
//                         of frame f + 1 are in flight across frame f's update.  The range (limited / full) is six integers
//                         passed by value, not a template axis.
//   k_mog_any_update, k_mog_any_yuv_update   any size (covahip_mog_create_any), the geometry as arguments: the update body with
//                         runtime sizes (update_any).  Everything per pixel lies on the padded pitch of 64 roww, roww =
//                         ceil(mw / 64): pixel (x, y) is lane p = y * 64 roww + x of the update grid and entry p of the model's
//                         arrays (W[5][P], V[5][P], M[5][3][P] f32, nmodes[P] u8 with P = 64 roww mh, as Geom lays them out at its
//                         NPIX).  A wave is 64 consecutive x of one padded row, so its ballot is one plane word.  Lanes at
//                         x >= mw load nothing, keep no model and ballot 0; the last block may be partial (P is a multiple of 64,
//                         not of 256).  BGR24 (LoadHalfAny) and, with LoadYuv<.., HALF>, NV12 / I420.
// mog_update.hip instantiates the dispatch, and with it the kernels, for SHADOW = false: those are instruction for instruction
// the kernels from before the shadow test existed, and that file's object holds no other.  mog_shadow.hip instantiates it for
// SHADOW = true (covahip_mog_set_shadows in a mode other than OFF).  FROZEN, the last axis of every kernel (false in both of
// those files), is covahip_mog_set_frozen: the lane reads its model into registers as ever, classifies every frame of the call
// against it (frozen_pixel of mog_dev.h, then the shadow test on the model as it is) and returns: no write-back, `par` is not
// read, no division.  The ballots and the next frame's loads in flight are the update's.  mog_frozen.hip instantiates those.
//
// No contraction in this code (see mog_dev.h); every file that includes it is built with the flags of mog.hip.
#pragma once
#pragma clang fp contract(off)

#include <type_traits>

#include "mog_dev.h"

namespace mogdev {

// source pixel(s) of working pixel (x, y) of one frame, resized as cv.resize INTER_LINEAR does for the three sizes: the copy
// (640x360 sources), the 2x2 mean (1280x720) and the centre pick (1920x1080)
template <int SRC>
struct LoadPx {
    __device__ __forceinline__ Px operator()(const uint8_t *__restrict__ fr, int x, int y) const {
        if constexpr (SRC == MOG_LOAD_HALF) return LoadHalf<G640::MW>()(fr, x, y);
        const uint8_t *q = SRC == MOG_LOAD_COPY ? fr + ((size_t)y * 640 + x) * 3 : fr + ((size_t)(3 * y + 1) * 1920 + 3 * x + 1) * 3;
        return {(float)q[0], (float)q[1], (float)q[2]};
    }
};

// SRC: MOG_LOAD_*.  frames: this launch's first frame, [nf][S][src]; par: (alphaT, prune) [F][S] of the call; bits: raw masks
// [F][S][3600]; SHADOW, sh: the shadow test (update_body_strided)
template <int SRC, bool SHADOW, bool FROZEN>
__global__ __launch_bounds__(UPD_BLOCK) void k_mog_update(const uint8_t *__restrict__ frames, size_t src_bytes, uint8_t *__restrict__ state,
                                                          const float2 *__restrict__ par, const int32_t *__restrict__ nvalid, int f0,
                                                          int nf, int S, float Tb, unsigned long long *__restrict__ bits, MogShadowDev sh) {
    update_body<G640, SHADOW, FROZEN>(LoadPx<SRC>(), frames, src_bytes, state, par, nvalid, f0, nf, S, Tb, bits, sh);
}

// frames: this launch's first frame, [nf][S][2 MH][2 MW][3]; par: (alphaT, prune) [F][S]; bits: raw masks [F][S][NWORD].  All four
// working sizes off 640x360, whichever form their post kernel has.
template <int MW, int MH, bool SHADOW, bool FROZEN>
__global__ __launch_bounds__(UPD_BLOCK) void k_mog_grid_update(const uint8_t *__restrict__ frames, size_t src_bytes,
                                                               uint8_t *__restrict__ state, const float2 *__restrict__ par,
                                                               const int32_t *__restrict__ nvalid, int f0, int nf, int S, float Tb,
                                                               unsigned long long *__restrict__ bits, MogShadowDev sh) {
    update_body<Geom<MW, MH>, SHADOW, FROZEN>(LoadHalf<MW>(), frames, src_bytes, state, par, nvalid, f0, nf, S, Tb, bits, sh);
}

// frames: the launch's first frame of stream 0; par: (alphaT, prune) [F][S] of the call; bits: raw masks [F][S][G::NWORD]
template <int MW, int MH, int FMT, int KIND, bool SHADOW, bool FROZEN>
__global__ __launch_bounds__(UPD_BLOCK) void k_mog_yuv_update(const uint8_t *__restrict__ frames, covahip_mog_yuv_src src,
                                                              uint8_t *__restrict__ state, const float2 *__restrict__ par,
                                                              const int32_t *__restrict__ nvalid, int f0, int nf, int S, float Tb,
                                                              unsigned long long *__restrict__ bits, MogShadowDev sh) {
    update_body_strided<Geom<MW, MH>, SHADOW, FROZEN>(LoadYuv<FMT, KIND>{src}, frames, src.frame_stride, src.stream_stride, state, par, nvalid,
                                              f0, nf, S, Tb, bits, sh);
}

// working pixel (x, y) of a BGR24 frame src_w wide: LoadHalf with the width as a member
struct LoadHalfAny {
    int src_w;
    __device__ __forceinline__ Px operator()(const uint8_t *__restrict__ fr, int x, int y) const {
        const uint8_t *a = fr + ((size_t)(2 * y) * src_w + 2 * x) * 3;
        const uint8_t *b = a + (size_t)src_w * 3;
        unsigned s0 = ((unsigned)a[0] + a[3] + b[0] + b[3] + 2) >> 2;
        unsigned s1 = ((unsigned)a[1] + a[4] + b[1] + b[4] + 2) >> 2;
        unsigned s2 = ((unsigned)a[2] + a[5] + b[2] + b[5] + 2) >> 2;
        return {(float)s0, (float)s1, (float)s2};
    }
};

// update_body_strided of mog_dev.h on the padded pitch: grid (ceil(P / UPD_BLOCK), S), bits [F][S][roww mh].  SHADOW, sh: as
// there; a lane at x >= mw is no foreground, so it is in neither plane.
template <bool SHADOW, bool FROZEN, class Load>
__device__ __forceinline__ void update_any(Load load, const uint8_t *__restrict__ frames, long long frame_stride, long long stream_stride,
                                           uint8_t *__restrict__ state, const float2 *__restrict__ par,
                                           const int32_t *__restrict__ nvalid, int f0, int nf, int S, float Tb,
                                           unsigned long long *__restrict__ bits, int mw, int mh, const MogShadowDev &sh) {
    const int s = blockIdx.y;
    int fend = nvalid[s] - f0;
    fend = fend < nf ? fend : nf;
    if (fend <= 0) return;                     // the same for the whole block
    const int pitch = (mw + 63) / 64 * 64;
    const size_t P = (size_t)pitch * mh;
    const size_t p = (size_t)blockIdx.x * UPD_BLOCK + threadIdx.x;
    if (p >= P) return;                        // whole waves: P is a multiple of 64
    const int x = (int)(p % pitch), y = (int)(p / pitch);
    const bool live = x < mw;                  // lane 0 of a wave always is
    uint8_t *st = state + (size_t)s * (P * (5 * NMIX * 4 + 1));
    float *gW = reinterpret_cast<float *>(st), *gV = gW + NMIX * P, *gM = gW + 2 * NMIX * P;
    uint8_t *gN = st + (size_t)5 * NMIX * 4 * P;
    float W[NMIX] = {}, V[NMIX] = {}, M[NMIX][3] = {};
    int nm = 0;
    const uint8_t *fr = frames + (long long)s * stream_stride;
    typename Load::At at{};
    typename Load::Raw cur{};
    if (live) {
#pragma unroll
        for (int k = 0; k < NMIX; k++) {
            W[k] = gW[(size_t)k * P + p];
            V[k] = gV[(size_t)k * P + p];
#pragma unroll
            for (int c = 0; c < 3; c++) M[k][c] = gM[(size_t)(k * 3 + c) * P + p];
        }
        nm = gN[p];
        at = load.at(x, y);
        cur = load(fr, at);
    }
    for (int f = 0; f < fend; f++) {
        typename Load::Raw nxt = cur;
        if (live && f + 1 < fend) nxt = load(fr + (long long)(f + 1) * frame_stride, at);   // next frame's words in flight
        if constexpr (FROZEN) {
            Px px{};
            bool fg = false;
            if (live) {
                px = load.px(cur);
                fg = frozen_pixel(W, V, M, nm, px, Tb);
            }
            frame_ballots<SHADOW>(fg, W, V, M, nm, px, Tb, sh, ((size_t)(f0 + f) * S + s) * (P / 64) + p / 64, bits);
        } else {                               // (the update's own lines, left as they were)
            const float2 pr = par[(size_t)(f0 + f) * S + s];
            bool fg = false;
            if constexpr (SHADOW) {
                Px px{};
                if (live) {
                    px = load.px(cur);
                    fg = mog2_pixel(W, V, M, nm, px, pr.x, pr.y, Tb);
                }
                shadow_ballots(fg, W, V, M, nm, px, Tb, sh, ((size_t)(f0 + f) * S + s) * (P / 64) + p / 64, bits);
            } else {
                if (live) fg = mog2_pixel(W, V, M, nm, load.px(cur), pr.x, pr.y, Tb);
                const unsigned long long word = __ballot(fg);
                if ((threadIdx.x & 63) == 0) bits[((size_t)(f0 + f) * S + s) * (P / 64) + p / 64] = word;
            }
        }
        cur = nxt;
    }
    if constexpr (FROZEN) return;              // the model is as it was
    if (live) {
#pragma unroll
        for (int k = 0; k < NMIX; k++) {
            gW[(size_t)k * P + p] = W[k];
            gV[(size_t)k * P + p] = V[k];
#pragma unroll
            for (int c = 0; c < 3; c++) gM[(size_t)(k * 3 + c) * P + p] = M[k][c];
        }
        gN[p] = (uint8_t)nm;
    }
}

// frames: this launch's first frame, [nf][S][2 mh][2 mw][3]
template <bool SHADOW, bool FROZEN>
__global__ __launch_bounds__(UPD_BLOCK) void k_mog_any_update(const uint8_t *__restrict__ frames, size_t src_bytes, uint8_t *__restrict__ state,
                                                              const float2 *__restrict__ par, const int32_t *__restrict__ nvalid, int f0,
                                                              int nf, int S, float Tb, unsigned long long *__restrict__ bits, int mw, int mh,
                                                              MogShadowDev sh) {
    update_any<SHADOW, FROZEN>(PlainLoad<LoadHalfAny>{LoadHalfAny{2 * mw}}, frames, (long long)((size_t)S * src_bytes), (long long)src_bytes, state,
                       par, nvalid, f0, nf, S, Tb, bits, mw, mh, sh);
}

// frames: the launch's first frame of stream 0, surfaces as `src` describes them
template <int FMT, bool SHADOW, bool FROZEN>
__global__ __launch_bounds__(UPD_BLOCK) void k_mog_any_yuv_update(const uint8_t *__restrict__ frames, covahip_mog_yuv_src src,
                                                                  uint8_t *__restrict__ state, const float2 *__restrict__ par,
                                                                  const int32_t *__restrict__ nvalid, int f0, int nf, int S, float Tb,
                                                                  unsigned long long *__restrict__ bits, int mw, int mh, MogShadowDev sh) {
    update_any<SHADOW, FROZEN>(LoadYuv<FMT, YUV_HALF>{src}, frames, src.frame_stride, src.stream_stride, state, par, nvalid, f0, nf, S, Tb, bits, mw,
                       mh, sh);
}

}  // namespace mogdev

// One update launch of the any-size kernels at working size mw x mh (as mog_launch_update for the templated geometries)
template <class K, class Src>
int mog_launch_update_any(covahip_ctx *ctx, const char *scope, K kernel, int mw, int mh, const uint8_t *frames, const Src &src,
                          const MogUpdateArgs &a) {
    constexpr int BLOCK = mogdev::UPD_BLOCK;
    const size_t P = (size_t)mog_any_pitch(mw) * mh;
    return mog_launch(ctx, scope, kernel, dim3((unsigned)((P + BLOCK - 1) / BLOCK), a.S), BLOCK, 0, frames, src, a.state, a.par, a.nvalid,
                      a.f0, a.nf, a.S, a.Tb, a.bits, mw, mh, mog_shadow_dev(a));
}

// Which update kernel a labeller runs, as a value.  format: COVAHIP_MOG_FMT_* of the surfaces, 0 for BGR24 frames of src_bytes
// each (then src is not read); load: MOG_LOAD_*; mw x mh: the working size; resident: the row's post form, which names the
// profile scope of a BGR24 labeller off the 640 wide working size (mog_update, or mog_band_update beside the banded post kernel).
struct MogRoute {
    bool any;
    int format, load, mw, mh;
    bool resident;
};

// One update launch of the route's kernel, in its (SHADOW, FROZEN) instance.  The only copy of the dispatch: the learning
// instances are instantiated in mog_update.hip (SHADOW = false) and mog_shadow.hip (true), the frozen ones in mog_frozen.hip, and
// nowhere else (the declarations below).
template <bool SHADOW, bool FROZEN>
int mog_launch_route(covahip_ctx *ctx, const MogRoute &r, const uint8_t *frames, size_t src_bytes, const covahip_mog_yuv_src &src,
                     const MogUpdateArgs &a) {
    using namespace mogdev;
    constexpr int NV12 = COVAHIP_MOG_FMT_NV12, I420 = COVAHIP_MOG_FMT_I420;
    if (r.any) {
        if (!r.format) return mog_launch_update_any(ctx, "mog_any_update", k_mog_any_update<SHADOW, FROZEN>, r.mw, r.mh, frames, src_bytes, a);
        const auto kernel = r.format == NV12 ? k_mog_any_yuv_update<NV12, SHADOW, FROZEN> : k_mog_any_yuv_update<I420, SHADOW, FROZEN>;
        return mog_launch_update_any(ctx, "mog_any_yuv_update", kernel, r.mw, r.mh, frames, src, a);
    }
    if (r.format)
        return with_geom<G640, G320, G960, G1280, G1920>(r.mw, [&](auto g) -> int {
            using G = decltype(g);
            const auto launch = [&](auto kind) {
                constexpr int KIND = decltype(kind)::value;
                const auto kernel = r.format == NV12 ? k_mog_yuv_update<G::MW, G::MH, NV12, KIND, SHADOW, FROZEN>
                                                     : k_mog_yuv_update<G::MW, G::MH, I420, KIND, SHADOW, FROZEN>;
                return mog_launch_update<G>(ctx, "mog_yuv_update", kernel, frames, src, a);
            };
            if (r.load == MOG_LOAD_HALF) return launch(std::integral_constant<int, YUV_HALF>{});
            if constexpr (G::MW == 640) {      // copy and centre pick exist at the reference grid's working size only
                if (r.load == MOG_LOAD_COPY) return launch(std::integral_constant<int, YUV_COPY>{});
                if (r.load == MOG_LOAD_PICK) return launch(std::integral_constant<int, YUV_PICK>{});
            }
            return COVAHIP_ERR_UNSUPPORTED;
        });
    if (r.mw == G640::MW) {
        const auto kernel = r.load == MOG_LOAD_COPY ? k_mog_update<MOG_LOAD_COPY, SHADOW, FROZEN>
                                                    : (r.load == MOG_LOAD_HALF ? k_mog_update<MOG_LOAD_HALF, SHADOW, FROZEN> : k_mog_update<MOG_LOAD_PICK, SHADOW, FROZEN>);
        return mog_launch_update<G640>(ctx, "mog_update", kernel, frames, src_bytes, a);
    }
    const auto grid = [&](auto g) {
        using G = decltype(g);
        return mog_launch_update<G>(ctx, r.resident ? "mog_update" : "mog_band_update", k_mog_grid_update<G::MW, G::MH, SHADOW, FROZEN>, frames,
                                    src_bytes, a);
    };
    return r.resident ? with_geom<G960, G320>(r.mw, grid) : with_geom<G1920, G1280>(r.mw, grid);
}
#define MOG_ROUTE_INSTANCE(SHADOW, FROZEN)                                                                                     \
    template int mog_launch_route<SHADOW, FROZEN>(covahip_ctx *, const MogRoute &, const uint8_t *, size_t, const covahip_mog_yuv_src &, \
                                                  const MogUpdateArgs &)
extern MOG_ROUTE_INSTANCE(false, false);       // mog_update.hip
extern MOG_ROUTE_INSTANCE(true, false);        // mog_shadow.hip
extern MOG_ROUTE_INSTANCE(false, true);        // mog_frozen.hip, both
extern MOG_ROUTE_INSTANCE(true, true);

// counts [FS][2] (u32, device) = the set bits of shadow and of bits & ~shadow in each of FS planes of nword words; shadow may be
// nullptr (then none).  mog_shadow.hip.
int covahip_mog_counts(covahip_ctx *ctx, const unsigned long long *bits, const unsigned long long *shadow, size_t nword, size_t FS,
                       uint32_t *counts);

// out u8 [streams][mh][mw][3] (device) = the background image of `streams` models from `state` on, one every state_bytes, laid
// out at row pitch `pitch` (include/covahip.h, covahip_mog_background).  mog_frozen.hip.
int covahip_mog_background_launch(covahip_ctx *ctx, const uint8_t *state, size_t state_bytes, int pitch, int mw, int mh, int streams,
                                  uint8_t *out);
