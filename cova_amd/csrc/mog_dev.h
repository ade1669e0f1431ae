// Device code shared by the MoG label kernels, whatever their geometry (the reference grid: 640x360 working frames; the
// macroblock grid: half-resolution working frames, those of 1440p and 4K sources worked on in row bands; covahip_mog_create_any:
// the geometry as kernel arguments): the MOG2 pixel update and the shadow test, the update kernel's body and its loads, and the
// post kernels' morphology and hole-fill passes.  The arithmetic is stated in include/covahip.h ("MoG labels").  There is one
// update body for the table's geometries (update_body_strided; update_body adapts a BGR24 load to it; mog_update.h has the
// kernels and the general sizes' update_any) and one set of post passes, which take the shape of a plane's rows as a policy
// (FixedRows: a geometry of the table, all constants; AnyRows: values).  The resident post kernels run the passes on the whole
// frame (post_planes), the banded ones band by band (post_banded, one driver for both row shapes); mog_post.hip has the kernels.
// Below the namespace is the host side the files share: the table of admitted geometries, Geom's runtime twin, the dispatch on
// the working width, the launch helpers and the post kernels' launch functions.
//
// No contraction in this code: every product and sum is rounded on its own, as the x86 builds of OpenCV compute it (every
// translation unit that includes this is also built with -ffp-contract=off).  The f32 divisions go through double: the f64 quotient is
// correctly rounded and 53 >= 2 * 24 + 2 bits, so rounding it to f32 gives the correctly rounded f32 quotient (double rounding
// is innocuous for division at that width); unlike the f32 divide expansion this needs no f32 fused multiply-add, so the
// update kernels' ISA has none at all (DESIGN.md checks it).
#pragma once
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstddef>
#include <cstdint>
#include <type_traits>
#include <utility>
#include <vector>

#include "covahip.h"
#include "internal.h"

// An NV12 / I420 surface as a kernel sees it: plane offsets from a frame's first byte, pitches and the two strides in bytes (all
// even), and the range's constants of include/covahip.h ("MoG labels", conversion): yy = max(0, Y - ysub) * ymul,
// B += bu * uu, G -= gv * vv + gu * uu, R += rv * vv.
struct covahip_mog_yuv_src {
    long long off[3], pitch[3], frame_stride, stream_stride;
    int ysub, ymul, bu, gv, gu, rv;
};

namespace mogdev {

constexpr int NMIX = 5;
constexpr int UPD_BLOCK = 256;
constexpr float TB = 0.9f, TG = 9.0f, VAR_INIT = 15.0f, VAR_MIN = 4.0f, VAR_MAX = 75.0f, FCT = 0.05f;

// A working geometry: W x H pixels, a row is W / 64 ballot words of the bit plane, one label per 8x8 block (the block's
// top-left pixel, or its coverage: label_bit and cover_labels below; the last label row of a height that is no multiple of 8
// reads the last started block).
template <int W, int H>
struct Geom {
    static constexpr int MW = W, MH = H;
    static constexpr int NPIX = MW * MH;
    static constexpr int ROWW = MW / 64;               // 64-bit words per row
    static constexpr int NWORD = NPIX / 64;            // words per frame
    static constexpr int LW = (MW + 7) / 8, LH = (MH + 7) / 8, NLAB = LW * LH;
    // state of one stream, structure of arrays: W[5][P], V[5][P], M[5][3][P] (f32), nmodes[P] (u8)
    static constexpr size_t OFF_W = 0, OFF_V = (size_t)NMIX * NPIX * 4, OFF_M = (size_t)2 * NMIX * NPIX * 4;
    static constexpr size_t OFF_N = (size_t)5 * NMIX * NPIX * 4;
    static constexpr size_t STATE_BYTES = OFF_N + NPIX;
    static_assert(NPIX % UPD_BLOCK == 0 && MW % 64 == 0 && 8 * (LH - 1) < MH && (LW - 1) / 8 < ROWW, "geometry");
};
using G320 = Geom<320, 180>;                   // the five working geometries
using G640 = Geom<640, 360>;
using G960 = Geom<960, 540>;
using G1280 = Geom<1280, 720>;
using G1920 = Geom<1920, 1080>;

// correctly rounded a / b through an f64 quotient (see the head of the file).  The empty asm keeps the optimiser from folding
// the widened division back into the f32 one, whose expansion uses f32 fused multiply-adds.
__device__ __forceinline__ float div_rn(float a, float b) {
    double da = a, db = b;
    asm("" : "+v"(da), "+v"(db));
    return (float)(da / db);
}

struct Px { float c0, c1, c2; };

// entries i and i - 1 trade places where `sel` (i is a constant after unrolling: the arrays stay in registers)
__device__ __forceinline__ void swap_sel(float (&W)[NMIX], float (&V)[NMIX], float (&M)[NMIX][3], int i, bool sel) {
    float a = W[i], b = W[i - 1];
    W[i] = sel ? b : a;
    W[i - 1] = sel ? a : b;
    a = V[i], b = V[i - 1];
    V[i] = sel ? b : a;
    V[i - 1] = sel ? a : b;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        a = M[i][c], b = M[i - 1][c];
        M[i][c] = sel ? b : a;
        M[i - 1][c] = sel ? a : b;
    }
}

// one MOG2 update of one pixel (include/covahip.h, "MoG labels"); returns true when the pixel is foreground
__device__ __forceinline__ bool mog2_pixel(float (&W)[NMIX], float (&V)[NMIX], float (&M)[NMIX][3], int &nm, const Px &px,
                                           float alphaT, float prune, float Tb) {
    const float alpha1 = 1.f - alphaT;
    bool fits = false, bg = false;
    float tw = 0.f;
#pragma unroll
    for (int mode = 0; mode < NMIX; mode++) {
        if (mode < nm) {                       // nm shrinks when a mode is pruned
            float w = alpha1 * W[mode] + prune;
            int swaps = 0;
            if (!fits) {
                const float d0 = M[mode][0] - px.c0, d1 = M[mode][1] - px.c1, d2 = M[mode][2] - px.c2;
                const float dist2 = (d0 * d0 + d1 * d1) + d2 * d2;
                const float var = V[mode];
                if (tw < TB && dist2 < Tb * var) bg = true;
                if (dist2 < TG * var) {
                    fits = true;
                    w = w + alphaT;
                    const float k = div_rn(alphaT, w);
                    M[mode][0] = M[mode][0] - k * d0;
                    M[mode][1] = M[mode][1] - k * d1;
                    M[mode][2] = M[mode][2] - k * d2;
                    float vn = var + k * (dist2 - var);
                    vn = vn < VAR_MIN ? VAR_MIN : vn;
                    vn = VAR_MAX < vn ? VAR_MAX : vn;
                    V[mode] = vn;
                    bool go = true;
#pragma unroll
                    for (int i = mode; i > 0; i--) {
                        go = go && !(w < W[i - 1]);
                        swap_sel(W, V, M, i, go);
                        swaps += go ? 1 : 0;
                    }
                }
            }
            if (w < -prune) {
                w = 0.f;
                nm--;
            }
#pragma unroll
            for (int j = 0; j <= mode; j++)
                if (mode - swaps == j) W[j] = w;
            tw = tw + w;
        }
    }
    const float inv = fabsf(tw) > FLT_EPSILON ? div_rn(1.f, tw) : 0.f;
#pragma unroll
    for (int i = 0; i < NMIX; i++)
        if (i < nm) W[i] = W[i] * inv;
    if (!fits) {
        const int m = nm == NMIX ? NMIX - 1 : nm++;
#pragma unroll
        for (int j = 0; j < NMIX; j++)
            if (j == m) {
                W[j] = nm == 1 ? 1.f : alphaT;
                M[j][0] = px.c0;
                M[j][1] = px.c1;
                M[j][2] = px.c2;
                V[j] = VAR_INIT;
            }
        if (nm != 1) {
#pragma unroll
            for (int i = 0; i < NMIX - 1; i++)
                if (i < nm - 1) W[i] = W[i] * alpha1;
        }
        bool go = true;
#pragma unroll
        for (int i = NMIX - 1; i > 0; i--) {
            if (i < nm) {
                const bool stop = alphaT < W[i - 1];
                swap_sel(W, V, M, i, go && !stop);
                go = go && !stop;
            }
        }
    }
    return !bg;
}

// One pixel classified against its model, which is only read (include/covahip.h, "MoG labels", frozen labelling): the walk of
// mog2_pixel's step 2 without its writes, up to the first mode that fits; returns true when the pixel is foreground.  The mask
// is the one mog2_pixel gives at alphaT = 0 on a model of finite values.  No division, nothing stored: `done` is the statement's
// stop, so the unrolled loop keeps W, V and M in registers.
__device__ __forceinline__ bool frozen_pixel(const float (&W)[NMIX], const float (&V)[NMIX], const float (&M)[NMIX][3], int nm,
                                             const Px &px, float Tb) {
    bool done = false, bg = false;
    float tw = 0.f;
#pragma unroll
    for (int mode = 0; mode < NMIX; mode++) {
        if (mode < nm && !done) {
            const float d0 = M[mode][0] - px.c0, d1 = M[mode][1] - px.c1, d2 = M[mode][2] - px.c2;
            const float dist2 = (d0 * d0 + d1 * d1) + d2 * d2;
            const float var = V[mode];
            if (tw < TB && dist2 < Tb * var) bg = true;
            if (dist2 < TG * var) done = true;
            tw = tw + W[mode];                 // (not read again where the walk has just ended)
        }
    }
    return !bg;
}

// The shadow test of one foreground pixel on the model mog2_pixel has just left (include/covahip.h, "MoG labels", step 2a;
// detectShadowGMM of OpenCV's MOG2): true when the pixel is a darker copy, by a factor a in [tau, 1], of a background mode's
// mean.  The model is only read.  The returns of the statement are the `done` flag here, so the unrolled loop keeps W, V and M
// in registers; a mode past `done` costs nothing but the test of the flag.
__device__ __forceinline__ bool shadow_pixel(const float (&W)[NMIX], const float (&V)[NMIX], const float (&M)[NMIX][3], int nm,
                                             const Px &px, float Tb, float tau) {
    bool done = false, shadow = false;
    float tw = 0.f;
#pragma unroll
    for (int mode = 0; mode < NMIX; mode++) {
        if (mode < nm && !done) {
            const float m0 = M[mode][0], m1 = M[mode][1], m2 = M[mode][2];
            const float num = ((0.f + px.c0 * m0) + px.c1 * m1) + px.c2 * m2;
            const float den = ((0.f + m0 * m0) + m1 * m1) + m2 * m2;
            if (den == 0.f) {
                done = true;
            } else {
                if (num <= den && num >= tau * den) {
                    const float a = div_rn(num, den);
                    const float d0 = a * m0 - px.c0, d1 = a * m1 - px.c1, d2 = a * m2 - px.c2;
                    const float dist2a = ((0.f + d0 * d0) + d1 * d1) + d2 * d2;
                    if (dist2a < ((Tb * V[mode]) * a) * a) shadow = done = true;
                }
                if (!done) {
                    tw = tw + W[mode];
                    if (tw > TB) done = true;
                }
            }
        }
    }
    return shadow;
}

// What the update kernels take for the shadow test (covahip_mog_set_shadows), behind their other arguments; the instances
// without the test (SHADOW = false) take it too and read none of it.  plane: the shadow planes [F][S][NWORD], laid out as the raw
// planes; drop: COVAHIP_MOG_SHADOWS_DROP (the raw plane is fg && !shadow) or _KEEP (it is fg), the same for the whole launch.
struct MogShadowDev {
    unsigned long long *plane;
    float tau;
    int drop;
};

// The two words a wave stores for a frame when the shadow test is on: `fg` is mog2_pixel's answer (false in a lane without a
// pixel), and the test runs on the model as that call left it.  word: where the wave's word lies in either plane.
__device__ __forceinline__ void shadow_ballots(bool fg, const float (&W)[NMIX], const float (&V)[NMIX], const float (&M)[NMIX][3],
                                               int nm, const Px &px, float Tb, const MogShadowDev &sh, size_t word,
                                               unsigned long long *__restrict__ bits) {
    const bool shd = fg && shadow_pixel(W, V, M, nm, px, Tb, sh.tau);
    const unsigned long long sw = __ballot(shd), fw = __ballot(fg);
    if ((threadIdx.x & 63) == 0) {
        bits[word] = sh.drop ? fw & ~sw : fw;      // wave-uniform select
        sh.plane[word] = sw;
    }
}

// What a wave stores for a frame in the frozen instances: with SHADOW the two words of shadow_ballots (the test on the model
// as it is), without it the one ballot word of the raw plane.  fg is false in a lane without a pixel.
template <bool SHADOW>
__device__ __forceinline__ void frame_ballots(bool fg, const float (&W)[NMIX], const float (&V)[NMIX], const float (&M)[NMIX][3], int nm,
                                              const Px &px, float Tb, const MogShadowDev &sh, size_t word,
                                              unsigned long long *__restrict__ bits) {
    if constexpr (SHADOW) {
        shadow_ballots(fg, W, V, M, nm, px, Tb, sh, word, bits);
    } else {
        const unsigned long long w = __ballot(fg);
        if ((threadIdx.x & 63) == 0) bits[word] = w;
    }
}

// The update kernel's body: one lane per working pixel and stream, grid (G::NPIX / UPD_BLOCK, S).  frames: the launch's first
// frame of stream 0, with frames and streams at byte strides of the caller's; par: (alphaT, prune) [F][S] of the call; bits: raw
// masks [F][S][G::NWORD].  A wave's 64 pixels lie in one row, so its ballot is one word of the plane.  `load.at(x, y)` gives
// what the lane needs to address its pixel within a frame (Load::At), once; `load(frame, at)` gives the raw words of working
// pixel (x, y) (Load::Raw) and `load.px(raw)` makes the pixel of them where it is consumed, so that the next frame's words stay
// in flight across this frame's mog2_pixel.  Load::WAIT says whether the body waits once before its loop (below).  SHADOW: the
// shadow test runs on every foreground pixel and the wave stores two words per frame (shadow_ballots); without it `sh` is not
// read and the body is the one it was before the test existed.
template <class G, bool SHADOW, bool FROZEN, class Load>
__device__ __forceinline__ void update_body_strided(Load load, const uint8_t *__restrict__ frames, long long frame_stride,
                                                    long long stream_stride, uint8_t *__restrict__ state,
                                                    const float2 *__restrict__ par, const int32_t *__restrict__ nvalid, int f0, int nf,
                                                    int S, float Tb, unsigned long long *__restrict__ bits, const MogShadowDev &sh) {
    constexpr int NPIX = G::NPIX;
    const int s = blockIdx.y;
    int fend = nvalid[s] - f0;
    fend = fend < nf ? fend : nf;
    if (fend <= 0) return;                     // the same for the whole block
    const int p = blockIdx.x * UPD_BLOCK + threadIdx.x;
    const int x = p % G::MW, y = p / G::MW;
    uint8_t *st = state + (size_t)s * G::STATE_BYTES;
    float *gW = reinterpret_cast<float *>(st + G::OFF_W), *gV = reinterpret_cast<float *>(st + G::OFF_V);
    float *gM = reinterpret_cast<float *>(st + G::OFF_M);
    float W[NMIX], V[NMIX], M[NMIX][3];
#pragma unroll
    for (int k = 0; k < NMIX; k++) {
        W[k] = gW[(size_t)k * NPIX + p];
        V[k] = gV[(size_t)k * NPIX + p];
#pragma unroll
        for (int c = 0; c < 3; c++) M[k][c] = gM[(size_t)(k * 3 + c) * NPIX + p];
    }
    int nm = st[G::OFF_N + p];
    const uint8_t *fr = frames + (long long)s * stream_stride;
    const typename Load::At at = load.at(x, y);
    typename Load::Raw cur = load(fr, at);
    // The model and the first frame's words land here, once (s_waitcnt vmcnt(0), gfx9 encoding).  Left to the compiler, the one
    // wait for them sits at the head of the loop body, where it also waits for the next frame's words in every later iteration:
    // that is where the BGR24 kernels have it (WAIT = false), and moving it is a change of speed that wants a measurement.
    if constexpr (Load::WAIT) __builtin_amdgcn_s_waitcnt(0x0F70);
    for (int f = 0; f < fend; f++) {
        typename Load::Raw nxt = cur;
        if (f + 1 < fend) nxt = load(fr + (long long)(f + 1) * frame_stride, at);   // next frame's words in flight
        if constexpr (FROZEN) {
            const Px px = load.px(cur);
            frame_ballots<SHADOW>(frozen_pixel(W, V, M, nm, px, Tb), W, V, M, nm, px, Tb, sh,
                                  ((size_t)(f0 + f) * S + s) * G::NWORD + p / 64, bits);
        } else {                               // (the update's own lines, left as they were: its ISA is held to the letter)
            const float2 pr = par[(size_t)(f0 + f) * S + s];
            const Px px = load.px(cur);
            const bool fg = mog2_pixel(W, V, M, nm, px, pr.x, pr.y, Tb);
            if constexpr (SHADOW) {
                shadow_ballots(fg, W, V, M, nm, px, Tb, sh, ((size_t)(f0 + f) * S + s) * G::NWORD + p / 64, bits);
            } else {
                const unsigned long long word = __ballot(fg);
                if ((threadIdx.x & 63) == 0) bits[((size_t)(f0 + f) * S + s) * G::NWORD + p / 64] = word;
            }
        }
        cur = nxt;
    }
    if constexpr (FROZEN) return;              // the model is as it was
#pragma unroll
    for (int k = 0; k < NMIX; k++) {
        gW[(size_t)k * NPIX + p] = W[k];
        gV[(size_t)k * NPIX + p] = V[k];
#pragma unroll
        for (int c = 0; c < 3; c++) gM[(size_t)(k * 3 + c) * NPIX + p] = M[k][c];
    }
    st[G::OFF_N + p] = (uint8_t)nm;
}

// The body on dense BGR24 frames [nf][S][src_bytes]: `load(frame, x, y)` gives working pixel (x, y) of one source frame.
template <class L>
struct PlainLoad {
    static constexpr bool WAIT = false;
    L load;
    struct At { int x, y; };
    using Raw = Px;
    __device__ __forceinline__ At at(int x, int y) const { return {x, y}; }
    __device__ __forceinline__ Px operator()(const uint8_t *__restrict__ fr, const At &t) const { return load(fr, t.x, t.y); }
    __device__ __forceinline__ Px px(const Px &r) const { return r; }
};
template <class G, bool SHADOW, bool FROZEN, class L>
__device__ __forceinline__ void update_body(L load, const uint8_t *__restrict__ frames, size_t src_bytes, uint8_t *__restrict__ state,
                                            const float2 *__restrict__ par, const int32_t *__restrict__ nvalid, int f0, int nf, int S,
                                            float Tb, unsigned long long *__restrict__ bits, const MogShadowDev &sh) {
    update_body_strided<G, SHADOW, FROZEN>(PlainLoad<L>{load}, frames, (long long)((size_t)S * src_bytes), (long long)src_bytes, state, par,
                                   nvalid, f0, nf, S, Tb, bits, sh);
}

// working pixel (x, y) of a frame of 2 MW x 2 MH: the rounded mean of its 2x2 block (the macroblock grid's load)
template <int MW>
struct LoadHalf {
    __device__ __forceinline__ Px operator()(const uint8_t *__restrict__ fr, int x, int y) const {
        const uint8_t *a = fr + ((size_t)(2 * y) * (2 * MW) + 2 * x) * 3;
        const uint8_t *b = a + 2 * MW * 3;
        unsigned s0 = ((unsigned)a[0] + a[3] + b[0] + b[3] + 2) >> 2;
        unsigned s1 = ((unsigned)a[1] + a[4] + b[1] + b[4] + 2) >> 2;
        unsigned s2 = ((unsigned)a[2] + a[5] + b[2] + b[5] + 2) >> 2;
        return {(float)s0, (float)s1, (float)s2};
    }
};

// Working pixel (x, y) of an NV12 / I420 surface (mog_update.h states the loads; the general kernels use the HALF kind too).  KIND is how
// the working pixel comes from the source: YUV_HALF the 2x2 mean, YUV_COPY the pixel itself, YUV_PICK source pixel (3x + 1, 3y + 1).
enum { YUV_HALF = 0, YUV_COPY = 1, YUV_PICK = 2 };

__device__ __forceinline__ int sat8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

template <int FMT, int KIND>
struct LoadYuv {
    static constexpr bool WAIT = true;         // the body waits for the model and the first frame once, before its loop
    static constexpr int NV12 = COVAHIP_MOG_FMT_NV12, HALF = YUV_HALF, COPY = YUV_COPY;
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

// ------------------------------------------------------------------------------------------------ post passes
// The shape of a plane's rows as the passes see it: roww() words per row, of which the last holds the image in the bits of
// tail(), in a frame mw() x mh().  Two models.  FixedRows: a working geometry of the table, everything a constant, the rows
// full (tail() is all ones, so every expression on it folds away) and ROWW usable as an array bound.  AnyRows: the sizes as
// values, of a labeller of covahip_mog_create_any, whose rows lie at a pitch of 64 roww pixels.  The bits at x >= mw of a row's
// last word are outside the image:
//   * every horizontal pass reads them as its neutral element (0 for dilate, 1 for erode) whatever the pass before left there;
//     a vertical pass works column by column, so what it leaves there comes from there only;
//   * the planes the banded driver writes (plane, filled_bits) have them clear;
//   * for the fill they are wall: the band's copy of A in LDS has them set, so ~A, the background the fill walks through, has
//     them clear; the seeds are the image's edge pixels, column mw - 1 on the right.
template <int MW, int MH>
struct FixedRows {
    static constexpr bool FIXED = true;
    static constexpr int ROWW = MW / 64;
    static_assert(MW % 64 == 0, "full rows");
    static constexpr int roww() { return ROWW; }
    static constexpr int mw() { return MW; }
    static constexpr int mh() { return MH; }
    static constexpr unsigned long long tail() { return ~0ull; }
};
struct AnyRows {
    static constexpr bool FIXED = false;
    int roww_, mw_, mh_;
    unsigned long long tail_;
    __device__ __forceinline__ AnyRows(int mw, int mh)
        : roww_((mw + 63) / 64), mw_(mw), mh_(mh), tail_((mw & 63) ? (1ull << (mw & 63)) - 1 : ~0ull) {}
    __device__ __forceinline__ int roww() const { return roww_; }
    __device__ __forceinline__ int mw() const { return mw_; }
    __device__ __forceinline__ int mh() const { return mh_; }
    __device__ __forceinline__ unsigned long long tail() const { return tail_; }
};

// Bit x of word w of a row is pixel 64 w + x.  A k x k window at x covers x - k/2 .. x + k - 1 - k/2 (OpenCV's anchor, the same
// offsets for dilate and erode); outside the image is 0 for dilate and 1 for erode.  BLOCK = threads of the workgroup.
// The passes work on a window of `nrows` whole rows of a frame of shape `rs`: the whole frame in the resident kernels (nrows
// is G::MH there and folds away), a band and its halo in the banded driver (frames whose planes do not fit LDS).  That window is
// clipped to the frame, so a row beyond it is either outside the frame, where the neutral element is
// what the pass wants, or a row of the frame that was not staged: then the neutral element is a stand-in, and the rows it
// reaches (K/2 rows at the top, K - 1 - K/2 at the bottom of the window, per vertical pass) are not valid any more.  The
// caller stages enough rows around its band for the valid region to end on the band.  nrows (N) is an int, or where the window
// is the whole frame (post_planes) an integral_constant: those instances are then the resident kernels' own, with the height
// a constant from the start, which the banded driver's instances of the same row shape would otherwise keep from them.
template <int BLOCK, bool DIL, int K, class R, class N>
__device__ __forceinline__ void hpass(R rs, const unsigned long long *in, unsigned long long *out, N nrows) {
    constexpr int A = K / 2, B = K - 1 - K / 2;
    constexpr unsigned long long NEU = DIL ? 0ull : ~0ull;
    const int roww = rs.roww();
    const unsigned long long tail = rs.tail();
    const int nword = nrows * roww;
    for (int i = threadIdx.x; i < nword; i += BLOCK) {
        const int w = i % roww;
        unsigned long long c = in[i];
        const unsigned long long pv = w > 0 ? in[i - 1] : NEU;
        unsigned long long nx = w < roww - 1 ? in[i + 1] : NEU;
        if constexpr (!R::FIXED) {     // the last word's bits beyond the image read as the neutral element (w - 1 is never the last word)
            if (w == roww - 1) c = DIL ? c & tail : c | ~tail;
            if (w == roww - 2) nx = DIL ? nx & tail : nx | ~tail;
        }
        unsigned long long r = c;
#pragma unroll
        for (int d = -A; d <= B; d++) {
            if (d == 0) continue;
            const unsigned long long v = d > 0 ? (c >> d) | (nx << (64 - d)) : (c << -d) | (pv >> (64 + d));
            r = DIL ? (r | v) : (r & v);
        }
        out[i] = r;
    }
}

template <int BLOCK, bool DIL, int K, class R, class N>
__device__ __forceinline__ void vpass(R rs, const unsigned long long *in, unsigned long long *out, N nrows) {
    constexpr int A = K / 2, B = K - 1 - K / 2;
    constexpr unsigned long long NEU = DIL ? 0ull : ~0ull;
    const int roww = rs.roww();
    const int nword = nrows * roww;
    for (int i = threadIdx.x; i < nword; i += BLOCK) {
        const int y = i / roww;
        unsigned long long r = in[i];
#pragma unroll
        for (int d = -A; d <= B; d++) {
            if (d == 0) continue;
            const unsigned long long v = (y + d >= 0 && y + d < nrows) ? in[i + d * roww] : NEU;
            r = DIL ? (r | v) : (r & v);
        }
        out[i] = r;
    }
}

// one separable dilate (DIL) or erode K x K of the window in X (LDS, nrows x roww words, behind a barrier) through Y (the same
// size); the result is in X, behind a barrier
template <int BLOCK, bool DIL, int K, class R, class N>
__device__ __forceinline__ void morph_pass(R rs, unsigned long long *X, unsigned long long *Y, N nrows) {
    hpass<BLOCK, DIL, K>(rs, X, Y, nrows);
    __syncthreads();
    vpass<BLOCK, DIL, K>(rs, Y, X, nrows);
    __syncthreads();
}

// close 4x4 and open 6x6 of the window in X, with Y as the other plane of the ping-pong.  Of the result's rows, 10 at the top
// and 6 at the bottom are valid only where the window ends on the frame edge.
template <int BLOCK, class R, class N>
__device__ __forceinline__ void morph_band(R rs, unsigned long long *X, unsigned long long *Y, N nrows) {
    morph_pass<BLOCK, true, 4>(rs, X, Y, nrows);
    morph_pass<BLOCK, false, 4>(rs, X, Y, nrows);
    morph_pass<BLOCK, false, 6>(rs, X, Y, nrows);
    morph_pass<BLOCK, true, 6>(rs, X, Y, nrows);
}

// the hole fill's seed in word w of row y: the image's edge pixels, rows 0 and mh - 1, columns 0 and mw - 1
template <class R>
__device__ __forceinline__ unsigned long long edge_seed(R rs, int y, int w) {
    unsigned long long edge = (y == 0 || y == rs.mh() - 1) ? ~0ull : 0ull;
    if (w == 0) edge |= 1ull;
    if (w == rs.roww() - 1) edge = (edge | 1ull << ((rs.mw() - 1) & 63)) & rs.tail();
    return edge;
}

// label (r, c) = filled pixel (8 c, 8 r) of the plane whose reached background is T (rows of roww words): 8 r < MH by Geom's assert
__device__ __forceinline__ uint8_t label_bit(const unsigned long long *T, unsigned r, unsigned c, unsigned roww) {
    return (uint8_t)((~T[8 * r * roww + c / 8] >> (8 * (c % 8))) & 1ull);
}

// The labels by block coverage (COVAHIP_MOG_LABELS_COVER and _COUNT; include/covahip.h, "MoG labels", step 6) of one frame
// mw x mh whose reached background is T (rows of roww words, LDS or global memory), by all BLOCK threads of the workgroup; lab
// is the frame's [lh][lw].  One thread per (label row, plane word): the word's eight bytes are the rows of eight blocks, so
// the block's up-to-8 rows are each reduced to per-byte popcounts (the 64-bit SWAR steps) and added -- a byte reaches at most
// 8 x 8 = 64, so nothing carries -- and the eight bytes of the sum are the counts of the word's eight labels.  Consecutive
// threads read consecutive 64-bit words of a row.  `live` masks the bits at x >= mw of a row's last word (T has them clear, so ~T
// has them set): they are neither counted nor inside, nor are the rows at y >= mh, which are not read.
template <int BLOCK>
__device__ __forceinline__ void cover_labels(const unsigned long long *T, uint8_t *lab, unsigned mw, unsigned mh, unsigned roww,
                                             int mode, unsigned ncover) {
    constexpr unsigned long long M1 = 0x5555555555555555ull, M2 = 0x3333333333333333ull, M4 = 0x0f0f0f0f0f0f0f0full;
    const unsigned lw = (mw + 7) / 8, lh = (mh + 7) / 8;
    const unsigned long long tail = (mw & 63) ? (1ull << (mw & 63)) - 1 : ~0ull;
    for (unsigned i = threadIdx.x; i < lh * roww; i += BLOCK) {
        const unsigned r = i / roww, wc = i % roww;
        const unsigned long long live = wc == roww - 1 ? tail : ~0ull;
        const unsigned rows_in = mh - 8 * r < 8 ? mh - 8 * r : 8;
        unsigned long long sum = 0;
#pragma unroll
        for (unsigned k = 0; k < 8; k++) {
            if (k < rows_in) {
                unsigned long long v = ~T[(8 * r + k) * roww + wc] & live;
                v = v - ((v >> 1) & M1);
                v = (v & M2) + ((v >> 2) & M2);
                sum += (v + (v >> 4)) & M4;
            }
        }
#pragma unroll
        for (unsigned j = 0; j < 8; j++) {
            const unsigned c = 8 * wc + j;
            if (c < lw) {
                const unsigned count = (unsigned)(sum >> (8 * j)) & 255u;
                const unsigned inside = rows_in * (mw - 8 * c < 8 ? mw - 8 * c : 8);
                lab[r * lw + c] = mode == COVAHIP_MOG_LABELS_COUNT ? (uint8_t)count : (uint8_t)(64u * count >= ncover * inside);
            }
        }
    }
}

// A (LDS, G::NWORD words, the raw mask; all threads have passed a barrier after writing it) becomes the mask after close 4x4
// and open 6x6; T (LDS, the same size) becomes the background reached from the frame edge through 4-connected background,
// so ~T is the filled mask.  Ends behind a barrier.  `changed` is one LDS int.
template <class G, int BLOCK>
__device__ __forceinline__ void post_planes(unsigned long long *A, unsigned long long *T, int *changed) {
    constexpr int ROWW = G::ROWW, NWORD = G::NWORD, MH = G::MH;
    constexpr FixedRows<G::MW, MH> rs;
    const int tid = threadIdx.x;
    morph_band<BLOCK>(rs, A, T, std::integral_constant<int, MH>{});   // close 4x4, open 6x6 (separable) on the whole frame
    // hole fill: T = background reached from the frame edge through 4-connected background (~A)
    for (int i = tid; i < NWORD; i += BLOCK) T[i] = ~A[i] & edge_seed(rs, i / ROWW, i % ROWW);
    for (;;) {
        if (tid == 0) *changed = 0;
        __syncthreads();
        // vertical: one lane per word column sweeps down, then up
        if (tid < ROWW) {
            bool ch = false;
            unsigned long long r = 0;
            for (int y = 0; y < MH; y++) {
                const int i = y * ROWW + tid;
                const unsigned long long old = T[i], nw = old | (~A[i] & r);
                if (nw != old) {
                    T[i] = nw;
                    ch = true;
                }
                r = nw;
            }
            r = 0;
            for (int y = MH - 1; y >= 0; y--) {
                const int i = y * ROWW + tid;
                const unsigned long long old = T[i], nw = old | (~A[i] & r);
                if (nw != old) {
                    T[i] = nw;
                    ch = true;
                }
                r = nw;
            }
            if (ch) *changed = 1;
        }
        __syncthreads();
        // horizontal: one lane per row fills every background run that holds a reached pixel, carrying across words
        for (int y = tid; y < MH; y += BLOCK) {
            unsigned long long m[ROWW], sd[ROWW], up[ROWW];
#pragma unroll
            for (int w = 0; w < ROWW; w++) {
                m[w] = ~A[y * ROWW + w];
                sd[w] = T[y * ROWW + w];
            }
            unsigned long long c = 0;
#pragma unroll
            for (int w = 0; w < ROWW; w++) {           // towards higher x: m + seeds ripples through each seeded run
                const unsigned long long s1 = sd[w] | (c & m[w] & 1ull);
                const unsigned long long t = m[w] + s1;
                up[w] = ((t ^ m[w]) | s1) & m[w];
                c = t < m[w] ? 1ull : 0ull;           // carried out of bit 63: the run goes on in the next word
            }
            c = 0;
            bool ch = false;
#pragma unroll
            for (int w = ROWW - 1; w >= 0; w--) {      // towards lower x: the same on bit-reversed words
                const unsigned long long rm = __builtin_bitreverse64(m[w]);
                const unsigned long long s1 = __builtin_bitreverse64(sd[w]) | (c & rm & 1ull);
                const unsigned long long t = rm + s1;
                const unsigned long long dn = __builtin_bitreverse64(((t ^ rm) | s1) & rm);
                c = t < rm ? 1ull : 0ull;
                const unsigned long long nw = sd[w] | up[w] | dn;
                if (nw != sd[w]) {
                    T[y * ROWW + w] = nw;
                    ch = true;
                }
            }
            if (ch) *changed = 1;
        }
        __syncthreads();
        const int again = *changed;
        __syncthreads();
        if (!again) break;
    }
}

// ------------------------------------------------------------------------------------------------ hole fill on a row band
// One direction of the band's column sweep on FILL_SEG row segments per word column: r(y) = T(y) | (~A(y) & r(y - 1)) is linear in
// OR, so every lane first sweeps its own segment with nothing carried in and notes what leaves the segment (`out`) and which
// columns are background in all of its rows (`pass`: what a carry would cross the segment through); the carry into a segment
// then follows from the segments before it, and a second walk ORs in what the carry reaches, ending where it is blocked.  The
// result is that of one lane walking the whole column.  carry: LDS, 2 x FILL_SEG x roww words; all threads call this, and
// roww x FILL_SEG of them have a segment.
constexpr int FILL_SEG = 16;
template <bool DOWN, class R>
__device__ __forceinline__ bool col_sweep(R rs, const unsigned long long *A, unsigned long long *T, int nrows,
                                          unsigned long long *carry) {
    const int roww = rs.roww();
    const int tid = threadIdx.x;
    const bool active = tid < roww * FILL_SEG;
    const int w = tid % roww, sg = tid / roww;
    const int len = (nrows + FILL_SEG - 1) / FILL_SEG;
    const int ya = sg * len < nrows ? sg * len : nrows, yb = ya + len < nrows ? ya + len : nrows;   // this lane's rows (may be none)
    unsigned long long *out = carry, *pass = carry + FILL_SEG * roww;
    bool ch = false;
    if (active) {
        unsigned long long r = 0, p = ~0ull;
        for (int k = 0; k < yb - ya; k++) {
            const int i = (DOWN ? ya + k : yb - 1 - k) * roww + w;
            const unsigned long long na = ~A[i], old = T[i], nw = old | (na & r);
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
        unsigned long long d = 0;                      // what the segments walked before this one carry into it
        if (DOWN)
            for (int k = 0; k < sg; k++) d = out[k * roww + w] | (pass[k * roww + w] & d);
        else
            for (int k = FILL_SEG - 1; k > sg; k--) d = out[k * roww + w] | (pass[k * roww + w] & d);
        for (int k = 0; k < yb - ya && d; k++) {
            const int i = (DOWN ? ya + k : yb - 1 - k) * roww + w;
            d &= ~A[i];
            const unsigned long long old = T[i], nw = old | d;
            if (nw != old) {
                T[i] = nw;
                ch = true;
            }
        }
    }
    __syncthreads();
    return ch;
}

// The banded post kernel's dynamic LDS at band height `rows` (post_banded lays it out, mog_post.hip sizes its launch with this, mog.hip
// plans and validates band heights with it): the flags (fill loop, seeds of a visit, sweep), the column sweep's carries, then
// two windows of a band and its halo, clipped to the frame.  The morphology stage is the larger of the two stages; the fill
// needs only 2 x rows.
constexpr int HALO_UP = 10, HALO_DOWN = 6;     // rows of input above / below an output row of close 4x4 + open 6x6
constexpr size_t BAND_FLAG_BYTES = 16;
constexpr size_t band_carry_bytes(int roww) { return (size_t)2 * FILL_SEG * roww * 8; }
constexpr size_t band_lds_bytes(int mw, int mh, int rows) {
    const int win = rows + HALO_UP + HALO_DOWN < mh ? rows + HALO_UP + HALO_DOWN : mh;
    return BAND_FLAG_BYTES + band_carry_bytes(mw / 64) + (size_t)2 * win * (mw / 64) * 8;
}

// The two-phase loop of post_planes on a band: T (LDS, nrows x roww words, seeded by the caller, behind a barrier) grows
// through the background ~A (LDS, the same size) until nothing changes.  Returns whether T changed at all (the same value in
// every thread); ends behind a barrier.  The column sweep runs on FILL_SEG row segments per column (above).  The row fill has two
// bodies that differ in where the row lives.  With ROWW a constant it is 2 x ROWW words in the lane's registers: the pass
// towards higher x adds what it reaches to the seeds of the pass towards lower x, which fills the same runs as two passes from
// the same seeds.  Otherwise it works on T in LDS word by word: the pass towards higher x leaves the seeds and what they
// reached in T, the pass towards lower x starts from that.
template <int BLOCK, class R>
__device__ __forceinline__ bool fill_band(R rs, const unsigned long long *A, unsigned long long *T, int nrows, int *changed,
                                          unsigned long long *carry) {
    if constexpr (R::FIXED) static_assert(R::ROWW * FILL_SEG <= BLOCK, "one lane per word column and row segment");
    const int tid = threadIdx.x;
    bool any = false;
    for (;;) {
        if (tid == 0) *changed = 0;
        __syncthreads();
        // vertical: down, then up (each ends behind a barrier)
        const bool chd = col_sweep<true>(rs, A, T, nrows, carry);
        const bool chu = col_sweep<false>(rs, A, T, nrows, carry);
        if (chd || chu) *changed = 1;
        // horizontal: one lane per row fills every background run that holds a reached pixel, carrying across words
        for (int y = tid; y < nrows; y += BLOCK) {
            bool ch = false;
            unsigned long long c = 0;
            if constexpr (R::FIXED) {
                constexpr int ROWW = R::ROWW;
                unsigned long long m[ROWW], sd[ROWW];
#pragma unroll
                for (int w = 0; w < ROWW; w++) {
                    m[w] = ~A[y * ROWW + w];
                    sd[w] = T[y * ROWW + w];
                }
#pragma unroll
                for (int w = 0; w < ROWW; w++) {           // towards higher x: m + seeds ripples through each seeded run
                    const unsigned long long s1 = sd[w] | (c & m[w] & 1ull);
                    const unsigned long long t = m[w] + s1;
                    sd[w] = ((t ^ m[w]) | s1) & m[w];       // the seeds and what they reached: a superset of sd[w]
                    c = t < m[w] ? 1ull : 0ull;           // carried out of bit 63: the run goes on in the next word
                }
                c = 0;
#pragma unroll
                for (int w = ROWW - 1; w >= 0; w--) {      // towards lower x: the same on bit-reversed words
                    const unsigned long long rm = __builtin_bitreverse64(m[w]);
                    const unsigned long long s1 = __builtin_bitreverse64(sd[w]) | (c & rm & 1ull);
                    const unsigned long long t = rm + s1;
                    const unsigned long long nw = __builtin_bitreverse64(((t ^ rm) | s1) & rm);
                    c = t < rm ? 1ull : 0ull;
                    if (nw != T[y * ROWW + w]) {
                        T[y * ROWW + w] = nw;
                        ch = true;
                    }
                }
            } else {
                const int roww = rs.roww();
                const unsigned long long *a = A + y * roww;
                unsigned long long *t = T + y * roww;
                for (int w = 0; w < roww; w++) {           // towards higher x
                    const unsigned long long m = ~a[w], sd = t[w];
                    const unsigned long long s1 = sd | (c & m & 1ull);
                    const unsigned long long r = m + s1;
                    const unsigned long long nw = ((r ^ m) | s1) & m;     // a superset of sd
                    c = r < m ? 1ull : 0ull;
                    if (nw != sd) {
                        t[w] = nw;
                        ch = true;
                    }
                }
                c = 0;
                for (int w = roww - 1; w >= 0; w--) {      // towards lower x
                    const unsigned long long rm = __builtin_bitreverse64(~a[w]), sd = t[w];
                    const unsigned long long s1 = __builtin_bitreverse64(sd) | (c & rm & 1ull);
                    const unsigned long long r = rm + s1;
                    const unsigned long long nw = __builtin_bitreverse64(((r ^ rm) | s1) & rm);
                    c = r < rm ? 1ull : 0ull;
                    if (nw != sd) {
                        t[w] = nw;
                        ch = true;
                    }
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

// The banded post kernels' body (mog_post.hip states the three stages), by all BLOCK threads of the workgroup of one (frame,
// stream) pair on a frame of shape `rs`.  bits: raw masks [F][S][roww mh]; filled_bits: the filled masks, same layout (T while the
// fill runs); plane: the mask after the morphology, same layout; labels [F][S][lh][lw]; rows: band height, >= 1; mode, ncover:
// MogLabelArgs.  smem: the workgroup's dynamic LDS, band_lds_bytes(64 roww, mh, rows).
template <int BLOCK, class R>
__device__ __forceinline__ void post_banded(R rs, uint8_t *smem, const unsigned long long *__restrict__ bits,
                                            unsigned long long *filled_bits, unsigned long long *plane, uint8_t *__restrict__ labels,
                                            const int32_t *__restrict__ nvalid, int S, int rows, int mode, int ncover) {
    const int roww = rs.roww(), mw = rs.mw(), mh = rs.mh();
    const int nword = roww * mh, lw = (mw + 7) / 8, nlab = lw * ((mh + 7) / 8);
    const unsigned long long tail = rs.tail();
    // the layout band_lds_bytes sizes: flags ([0] fill loop, [1] a visit's seeds, [2] the sweep), carries, two windows
    int *flags = reinterpret_cast<int *>(smem);
    unsigned long long *carry = reinterpret_cast<unsigned long long *>(smem + BAND_FLAG_BYTES);
    unsigned long long *P = reinterpret_cast<unsigned long long *>(smem + BAND_FLAG_BYTES + band_carry_bytes(roww));
    const int fs = blockIdx.x;
    const int f = fs / S, s = fs % S;
    if (f >= nvalid[s]) return;
    const int tid = threadIdx.x;
    const unsigned long long *src = bits + (size_t)fs * nword;
    unsigned long long *Ag = plane + (size_t)fs * nword, *Tg = filled_bits + (size_t)fs * nword;
    const int nb = (mh + rows - 1) / rows;

    // 1. morphology: close 4x4, open 6x6 on the band and its halo, clipped to the frame
    for (int b = 0; b < nb; b++) {
        const int y0 = b * rows, y1 = y0 + rows < mh ? y0 + rows : mh;
        const int lo = y0 - HALO_UP > 0 ? y0 - HALO_UP : 0, hi = y1 + HALO_DOWN < mh ? y1 + HALO_DOWN : mh;
        const int n = hi - lo;
        unsigned long long *X = P, *Y = P + n * roww;
        for (int i = tid; i < n * roww; i += BLOCK) X[i] = src[lo * roww + i];
        __syncthreads();
        morph_band<BLOCK>(rs, X, Y, n);
        for (int i = tid; i < (y1 - y0) * roww; i += BLOCK) {
            const int gi = y0 * roww + i;
            const unsigned long long a = X[(y0 - lo) * roww + i] & (gi % roww == roww - 1 ? tail : ~0ull);
            Ag[gi] = a;
            Tg[gi] = ~a & edge_seed(rs, gi / roww, gi % roww);
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
            unsigned long long st = 0, sb = 0;
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
            unsigned long long *A = P, *T = P + n * roww;
            for (int i = tid; i < n * roww; i += BLOCK) {
                A[i] = Ag[y0 * roww + i] | (i % roww == roww - 1 ? ~tail : 0ull);   // beyond the image is wall
                T[i] = Tg[y0 * roww + i];
            }
            __syncthreads();
            if (tid < roww) {
                T[tid] |= st;
                T[(n - 1) * roww + tid] |= sb;
            }
            const bool grew = fill_band<BLOCK>(rs, A, T, n, &flags[0], carry);   // (starts and ends with a barrier)
            if (seeded || grew) {
                for (int i = tid; i < n * roww; i += BLOCK) Tg[y0 * roww + i] = T[i];
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
        for (int i = tid; i < nlab; i += BLOCK) lab[i] = label_bit(Tg, i / lw, i % lw, roww);
    } else {
        cover_labels<BLOCK>(Tg, lab, mw, mh, roww, mode, ncover);
    }
    __syncthreads();
    for (int i = tid; i < nword; i += BLOCK) Tg[i] = ~Tg[i] & (i % roww == roww - 1 ? tail : ~0ull);
}

}  // namespace mogdev

// ------------------------------------------------------------------------------------------------ host side
// Geom at run time: what the host derives from a labeller's working size.
struct MogDims {
    int mw, mh;
    constexpr size_t npix() const { return (size_t)mw * mh; }
    constexpr size_t nword() const { return npix() / 64; }
    constexpr int lw() const { return (mw + 7) / 8; }
    constexpr int lh() const { return (mh + 7) / 8; }
    constexpr size_t nlab() const { return (size_t)lw() * lh(); }
    constexpr size_t off_v() const { return (size_t)mogdev::NMIX * npix() * 4; }
    constexpr size_t off_m() const { return 2 * off_v(); }
    constexpr size_t off_n() const { return 5 * off_v(); }
    constexpr size_t state_bytes() const { return off_n() + npix(); }
};
template <class G>
constexpr bool mog_dims_match() {
    constexpr MogDims d{G::MW, G::MH};
    return d.npix() == G::NPIX && d.nword() == G::NWORD && d.lw() == G::LW && d.lh() == G::LH && d.nlab() == G::NLAB &&
           G::OFF_W == 0 && d.off_v() == G::OFF_V && d.off_m() == G::OFF_M && d.off_n() == G::OFF_N &&
           d.state_bytes() == G::STATE_BYTES;
}
static_assert(mog_dims_match<mogdev::G320>() && mog_dims_match<mogdev::G640>() && mog_dims_match<mogdev::G960>() &&
                  mog_dims_match<mogdev::G1280>() && mog_dims_match<mogdev::G1920>(),
              "MogDims restates Geom");

// The admitted (source size, grid) pairs: the working size, how the update kernel loads a working pixel, and which forms of
// the post kernel exist there (resident: both planes in LDS; banded) with the one a new labeller starts in.  Where the resident
// form does not exist the update launch's profile scope is mog_band_update.  The
// macroblock grid works at half the source, so 1280x720 is the reference grid's row there and runs the same kernels.
enum { MOG_LOAD_COPY = 0, MOG_LOAD_HALF = 1, MOG_LOAD_PICK = 2 };
struct MogGeomRow {
    int src_w, src_h;
    unsigned grids;                // bit COVAHIP_MOG_GRID_*
    MogDims work;
    int load;
    bool resident, banded, starts_banded;
};
constexpr unsigned MOG_ON_REF = 1u << COVAHIP_MOG_GRID_REFERENCE, MOG_ON_MB = 1u << COVAHIP_MOG_GRID_MACROBLOCK;
constexpr MogGeomRow MOG_GEOMS[] = {
    {640, 360, MOG_ON_REF, {640, 360}, MOG_LOAD_COPY, true, false, false},
    {1280, 720, MOG_ON_REF | MOG_ON_MB, {640, 360}, MOG_LOAD_HALF, true, false, false},
    {1920, 1080, MOG_ON_REF, {640, 360}, MOG_LOAD_PICK, true, false, false},
    {640, 360, MOG_ON_MB, {320, 180}, MOG_LOAD_HALF, true, false, false},
    {1920, 1080, MOG_ON_MB, {960, 540}, MOG_LOAD_HALF, true, true, false},
    {2560, 1440, MOG_ON_MB, {1280, 720}, MOG_LOAD_HALF, false, true, true},
    {3840, 2160, MOG_ON_MB, {1920, 1080}, MOG_LOAD_HALF, false, true, true},
};
inline const MogGeomRow *mog_geom_row(int src_w, int src_h, int grid) {
    for (const MogGeomRow &r : MOG_GEOMS)
        if (r.src_w == src_w && r.src_h == src_h && (r.grids >> grid & 1u)) return &r;
    return nullptr;
}

// f(Geom<MW, MH>{}) for the one of the listed working geometries that is `mw` wide, else COVAHIP_ERR_UNSUPPORTED
template <class... Gs, class F>
int with_geom(int mw, F &&f) {
    int rc = COVAHIP_ERR_UNSUPPORTED;
    (void)((mw == Gs::MW && ((rc = f(Gs{})), true)) || ...);
    return rc;
}

// What an update launch takes behind its frames: the model, the call's tables (par: (alphaT, prune) [F][S]; nvalid [S]), the
// launch's frames f0 .. f0 + nf of the call, and the call's raw planes.  All device memory.  shadows: COVAHIP_MOG_SHADOWS_* of
// the call; other than _OFF the launch goes to the kernels' SHADOW instances (mog_shadow.hip), which read tau and write
// `shadow`, the call's shadow planes.
struct MogUpdateArgs {
    uint8_t *state;
    const float2 *par;
    const int32_t *nvalid;
    int f0, nf, S;
    float Tb;
    unsigned long long *bits;
    int shadows = COVAHIP_MOG_SHADOWS_OFF;
    float tau = 0.5f;
    unsigned long long *shadow = nullptr;
};
// How a post launch takes its labels (include/covahip.h, "MoG labels", step 6): mode COVAHIP_MOG_LABELS_*, and with _COVER
// ncover in 1 .. 64.  Arguments of the post kernels, the same for the whole launch.
struct MogLabelArgs {
    int mode = COVAHIP_MOG_LABELS_CORNER, ncover = 1;
};
inline mogdev::MogShadowDev mog_shadow_dev(const MogUpdateArgs &a) {
    return {a.shadow, a.tau, a.shadows == COVAHIP_MOG_SHADOWS_DROP};
}
// One kernel launch on ctx->stream under a profile scope
template <class K, class... Args>
int mog_launch(covahip_ctx *ctx, const char *scope, K kernel, dim3 grid, int block, size_t lds, Args... args) {
    {
        ProfScope ps(ctx, scope);
        kernel<<<grid, block, lds, ctx->stream>>>(args...);
    }
    COVAHIP_CHECK_HIP(ctx, hipGetLastError());
    return COVAHIP_OK;
}
// One update launch of geometry G: every update kernel takes (frames, src, the fields of MogUpdateArgs with the shadow test's as
// a MogShadowDev), where src is a BGR24 frame's bytes or a covahip_mog_yuv_src
template <class G, class K, class Src>
int mog_launch_update(covahip_ctx *ctx, const char *scope, K kernel, const uint8_t *frames, const Src &src, const MogUpdateArgs &a) {
    return mog_launch(ctx, scope, kernel, dim3(G::NPIX / mogdev::UPD_BLOCK, a.S), mogdev::UPD_BLOCK, 0, frames, src, a.state, a.par,
                      a.nvalid, a.f0, a.nf, a.S, a.Tb, a.bits, mog_shadow_dev(a));
}

// The post kernels (mog_post.hip).  Pointers are device memory, the layouts those of the kernels above; the launches go to
// ctx->stream and return without waiting.
// The resident form at working width `mw` (640, 960 or 320): both planes in LDS.
int covahip_mog_grid_post(covahip_ctx *ctx, int mw, const unsigned long long *bits, unsigned long long *filled_bits,
                          uint8_t *labels, const int32_t *nvalid, int S, size_t FS, MogLabelArgs la);
// The banded form.  Of the table at working width `mw`: 1280 and 1920, whose planes do not fit LDS, and 960 (for comparison
// with the resident one).  With `any` the general kernel: the macroblock grid at any working size mw x mh, 128 <= mw, mh <= 2048,
// as arguments of the kernel; rows of the planes and of the model then lie at a pitch of mog_any_pitch(mw) pixels, so the sizes
// of a labeller's buffers are those of MogDims{mog_any_pitch(mw), mh}.  plane: one more plane per (frame, stream), FS * NWORD
// words, for the mask after the morphology; rows: the band height, 16 .. mh, with mogdev::band_lds_bytes (at the pitch) within
// COVAHIP_MOG_BAND_LDS_MAX (else COVAHIP_ERR_UNSUPPORTED).
constexpr size_t COVAHIP_MOG_BAND_LDS_MAX = 160 * 1024 - 64;
constexpr int mog_any_pitch(int mw) { return (mw + 63) / 64 * 64; }
int covahip_mog_band_post(covahip_ctx *ctx, bool any, int mw, int mh, const unsigned long long *bits, unsigned long long *filled_bits,
                          unsigned long long *plane, uint8_t *labels, const int32_t *nvalid, int S, size_t FS, int rows,
                          MogLabelArgs la);
