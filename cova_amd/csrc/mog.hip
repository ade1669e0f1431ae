// MoG label generation (utils/generate-mog.py of the reference): per-pixel MOG2 background subtraction at 640x360, then
// close 4x4, open 6x6, hole fill and the ::8 subsample to the 45x80 labels `tfrecordsink gt=` reads.  The arithmetic is
// stated in include/covahip.h ("MoG labels"); tests/mog_ref.py is its numpy float32 restatement and the kernels match it bit
// for bit.
//
//   k_mog_update  one lane per working-size pixel and stream.  The five modes (weight, variance, mean) are read once per call
//                 into registers, every frame of the call is applied to them, and they are written back once.  The source is
//                 resized while it is read (copy, 2x2 mean or centre pick).  The foreground of a wave's 64 pixels (a row is
//                 exactly ten waves wide) is one __ballot word: a frame's raw mask is 3,600 words, 28.8 KB.
//   k_mog_post    one workgroup per (stream, frame): the bit plane in LDS, separable morphology on 64-bit words with shifts,
//                 hole fill by seeding the background on the frame edge and propagating it (column sweeps + word-carry run
//                 fill along rows) until a pass changes nothing, then the subsample.
//
// No contraction in this file: every product and sum is rounded on its own, as the x86 builds of OpenCV compute it.  The
// f32 divisions go through double: the f64 quotient is correctly rounded and 53 >= 2 * 24 + 2 bits, so rounding it to f32
// gives the correctly rounded f32 quotient (double rounding is innocuous for division at that width); unlike the f32 divide
// expansion this needs no f32 fused multiply-add, so the update kernel's ISA has none at all (DESIGN.md checks it).
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "covahip.h"
#include "covahip_dev.h"
#include "internal.h"

namespace {

constexpr int MW = 640, MH = 360;              // working size
constexpr int NPIX = MW * MH;                  // 230,400 pixels
constexpr int ROWW = MW / 64;                  // 64-bit words per row
constexpr int NWORD = NPIX / 64;               // 3,600 words per frame
constexpr int LW = 80, LH = 45, NLAB = LW * LH;
constexpr int NMIX = 5;
constexpr int UPD_BLOCK = 256;
constexpr int POST_BLOCK = 256;
static_assert(NPIX % UPD_BLOCK == 0 && MW % 64 == 0 && NLAB == NWORD, "geometry");

// state of one stream, structure of arrays: W[5][P], V[5][P], M[5][3][P] (f32), nmodes[P] (u8)
constexpr size_t OFF_W = 0, OFF_V = (size_t)NMIX * NPIX * 4, OFF_M = (size_t)2 * NMIX * NPIX * 4;
constexpr size_t OFF_N = (size_t)5 * NMIX * NPIX * 4;
constexpr size_t STATE_BYTES = OFF_N + NPIX;
// device budget for host frames staged per update launch (covahip_dev_mog_set_stage_budget changes it per labeller)
constexpr size_t STAGE_BUDGET = (size_t)1 << 30;

constexpr float TB = 0.9f, TG = 9.0f, VAR_INIT = 15.0f, VAR_MIN = 4.0f, VAR_MAX = 75.0f, FCT = 0.05f;

// correctly rounded a / b through an f64 quotient (see the head of the file).  The empty asm keeps the optimiser from folding
// the widened division back into the f32 one, whose expansion uses f32 fused multiply-adds.
__device__ __forceinline__ float div_rn(float a, float b) {
    double da = a, db = b;
    asm("" : "+v"(da), "+v"(db));
    return (float)(da / db);
}

struct Px { float c0, c1, c2; };

// source pixel(s) of working pixel (x, y) of one frame, resized as cv.resize INTER_LINEAR does for the three sizes
template <int SRC>
__device__ __forceinline__ Px load_px(const uint8_t *__restrict__ fr, int x, int y) {
    if constexpr (SRC == 0) {
        const uint8_t *q = fr + ((size_t)y * 640 + x) * 3;
        return {(float)q[0], (float)q[1], (float)q[2]};
    } else if constexpr (SRC == 1) {
        const uint8_t *a = fr + ((size_t)(2 * y) * 1280 + 2 * x) * 3;
        const uint8_t *b = a + 1280 * 3;
        unsigned s0 = ((unsigned)a[0] + a[3] + b[0] + b[3] + 2) >> 2;
        unsigned s1 = ((unsigned)a[1] + a[4] + b[1] + b[4] + 2) >> 2;
        unsigned s2 = ((unsigned)a[2] + a[5] + b[2] + b[5] + 2) >> 2;
        return {(float)s0, (float)s1, (float)s2};
    } else {
        const uint8_t *q = fr + ((size_t)(3 * y + 1) * 1920 + 3 * x + 1) * 3;
        return {(float)q[0], (float)q[1], (float)q[2]};
    }
}

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

// frames: this launch's first frame, [nf][S][src]; par: (alphaT, prune) [F][S] of the call; bits: raw masks [F][S][3600]
template <int SRC>
__global__ __launch_bounds__(UPD_BLOCK) void k_mog_update(const uint8_t *__restrict__ frames, size_t src_bytes, uint8_t *__restrict__ state,
                                                          const float2 *__restrict__ par, const int32_t *__restrict__ nvalid, int f0,
                                                          int nf, int S, float Tb, unsigned long long *__restrict__ bits) {
    const int s = blockIdx.y;
    int fend = nvalid[s] - f0;
    fend = fend < nf ? fend : nf;
    if (fend <= 0) return;                     // the same for the whole block
    const int p = blockIdx.x * UPD_BLOCK + threadIdx.x;
    const int x = p % MW, y = p / MW;
    uint8_t *st = state + (size_t)s * STATE_BYTES;
    const float *gW = reinterpret_cast<const float *>(st + OFF_W);
    const float *gV = reinterpret_cast<const float *>(st + OFF_V);
    const float *gM = reinterpret_cast<const float *>(st + OFF_M);
    float W[NMIX], V[NMIX], M[NMIX][3];
#pragma unroll
    for (int k = 0; k < NMIX; k++) {
        W[k] = gW[(size_t)k * NPIX + p];
        V[k] = gV[(size_t)k * NPIX + p];
#pragma unroll
        for (int c = 0; c < 3; c++) M[k][c] = gM[(size_t)(k * 3 + c) * NPIX + p];
    }
    int nm = st[OFF_N + p];
    const size_t fstride = (size_t)S * src_bytes;
    const uint8_t *fr = frames + (size_t)s * src_bytes;
    Px cur = load_px<SRC>(fr, x, y);
    for (int f = 0; f < fend; f++) {
        Px nxt = cur;
        if (f + 1 < fend) nxt = load_px<SRC>(fr + (size_t)(f + 1) * fstride, x, y);   // next frame's pixel in flight
        const float2 pr = par[(size_t)(f0 + f) * S + s];
        const bool fg = mog2_pixel(W, V, M, nm, cur, pr.x, pr.y, Tb);
        const unsigned long long word = __ballot(fg);
        if ((threadIdx.x & 63) == 0) bits[((size_t)(f0 + f) * S + s) * NWORD + p / 64] = word;
        cur = nxt;
    }
    float *oW = reinterpret_cast<float *>(st + OFF_W);
    float *oV = reinterpret_cast<float *>(st + OFF_V);
    float *oM = reinterpret_cast<float *>(st + OFF_M);
#pragma unroll
    for (int k = 0; k < NMIX; k++) {
        oW[(size_t)k * NPIX + p] = W[k];
        oV[(size_t)k * NPIX + p] = V[k];
#pragma unroll
        for (int c = 0; c < 3; c++) oM[(size_t)(k * 3 + c) * NPIX + p] = M[k][c];
    }
    st[OFF_N + p] = (uint8_t)nm;
}

// ------------------------------------------------------------------------------------------------ post kernel
// Bit x of word w of a row is pixel 64 w + x.  A k x k window at x covers x - k/2 .. x + k - 1 - k/2 (OpenCV's anchor, the same
// offsets for dilate and erode); outside the image is 0 for dilate and 1 for erode.
template <bool DIL, int K>
__device__ __forceinline__ void hpass(const unsigned long long *in, unsigned long long *out) {
    constexpr int A = K / 2, B = K - 1 - K / 2;
    constexpr unsigned long long NEU = DIL ? 0ull : ~0ull;
    for (int i = threadIdx.x; i < NWORD; i += POST_BLOCK) {
        const int w = i % ROWW;
        const unsigned long long c = in[i];
        const unsigned long long pv = w > 0 ? in[i - 1] : NEU;
        const unsigned long long nx = w < ROWW - 1 ? in[i + 1] : NEU;
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

template <bool DIL, int K>
__device__ __forceinline__ void vpass(const unsigned long long *in, unsigned long long *out) {
    constexpr int A = K / 2, B = K - 1 - K / 2;
    constexpr unsigned long long NEU = DIL ? 0ull : ~0ull;
    for (int i = threadIdx.x; i < NWORD; i += POST_BLOCK) {
        const int y = i / ROWW;
        unsigned long long r = in[i];
#pragma unroll
        for (int d = -A; d <= B; d++) {
            if (d == 0) continue;
            const unsigned long long v = (y + d >= 0 && y + d < MH) ? in[i + d * ROWW] : NEU;
            r = DIL ? (r | v) : (r & v);
        }
        out[i] = r;
    }
}

// bits: raw masks [F][S][3600]; filled_bits: the filled masks, same layout; labels [F][S][45][80]
__global__ __launch_bounds__(POST_BLOCK) void k_mog_post(const unsigned long long *__restrict__ bits,
                                                         unsigned long long *__restrict__ filled_bits, uint8_t *__restrict__ labels,
                                                         const int32_t *__restrict__ nvalid, int S) {
    __shared__ unsigned long long A[NWORD], T[NWORD];
    __shared__ int changed;
    const int fs = blockIdx.x;
    const int f = fs / S, s = fs % S;
    if (f >= nvalid[s]) return;
    const int tid = threadIdx.x;
    const unsigned long long *src = bits + (size_t)fs * NWORD;
    for (int i = tid; i < NWORD; i += POST_BLOCK) A[i] = src[i];
    __syncthreads();
    // close 4x4, open 6x6 (separable)
    hpass<true, 4>(A, T);
    __syncthreads();
    vpass<true, 4>(T, A);
    __syncthreads();
    hpass<false, 4>(A, T);
    __syncthreads();
    vpass<false, 4>(T, A);
    __syncthreads();
    hpass<false, 6>(A, T);
    __syncthreads();
    vpass<false, 6>(T, A);
    __syncthreads();
    hpass<true, 6>(A, T);
    __syncthreads();
    vpass<true, 6>(T, A);
    __syncthreads();
    // hole fill: T = background reached from the frame edge through 4-connected background (~A)
    for (int i = tid; i < NWORD; i += POST_BLOCK) {
        const int y = i / ROWW, w = i % ROWW;
        unsigned long long edge = (y == 0 || y == MH - 1) ? ~0ull : 0ull;
        if (w == 0) edge |= 1ull;
        if (w == ROWW - 1) edge |= 1ull << 63;
        T[i] = ~A[i] & edge;
    }
    for (;;) {
        if (tid == 0) changed = 0;
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
            if (ch) changed = 1;
        }
        __syncthreads();
        // horizontal: one lane per row fills every background run that holds a reached pixel, carrying across words
        for (int y = tid; y < MH; y += POST_BLOCK) {
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
            if (ch) changed = 1;
        }
        __syncthreads();
        const int again = changed;
        __syncthreads();
        if (!again) break;
    }
    unsigned long long *dst = filled_bits + (size_t)fs * NWORD;
    uint8_t *lab = labels + (size_t)fs * NLAB;
    for (int i = tid; i < NWORD; i += POST_BLOCK) {
        dst[i] = ~T[i];
        const int r = i / LW, c = i % LW;              // label (r, c) = filled pixel (8 c, 8 r)
        lab[i] = (uint8_t)((~T[8 * r * ROWW + c / 8] >> (8 * (c % 8))) & 1ull);
    }
}

int src_kind(int w, int h) {
    if (w == 640 && h == 360) return 0;
    if (w == 1280 && h == 720) return 1;
    if (w == 1920 && h == 1080) return 2;
    return -1;
}

}  // namespace

struct covahip_mog {
    covahip_ctx *ctx = nullptr;
    covahip_mog_cfg cfg{};
    int kind = 0;
    size_t src_bytes = 0;
    std::vector<int64_t> n;        // frames each stream has seen
    uint8_t *state = nullptr;      // [S][STATE_BYTES]
    void *bits = nullptr, *filled = nullptr, *d_frames = nullptr, *d_labels = nullptr, *d_par = nullptr;
    size_t bits_bytes = 0, filled_bytes = 0, frames_bytes = 0, labels_bytes = 0, par_bytes = 0;
    void *h_par = nullptr;         // pinned: (alphaT, prune) [F][S], then n_valid [S]
    size_t h_par_bytes = 0;
    int last_frames = 0;
    size_t stage_budget = STAGE_BUDGET;   // bytes of host frames staged per update launch
};

namespace {

void free_mog(covahip_mog *m) {
    for (void *p : {(void *)m->state, m->bits, m->filled, m->d_frames, m->d_labels, m->d_par})
        if (p) hipFree(p);
    if (m->h_par) hipHostFree(m->h_par);
    delete m;
}

int launch_update(covahip_mog *m, const uint8_t *d_frames, int f0, int nf, int S, const float2 *d_par, const int32_t *d_nv) {
    covahip_ctx *ctx = m->ctx;
    const dim3 grid(NPIX / UPD_BLOCK, S);
    auto *bits = static_cast<unsigned long long *>(m->bits);
    {
        ProfScope ps(ctx, "mog_update");
        if (m->kind == 0)
            k_mog_update<0><<<grid, UPD_BLOCK, 0, ctx->stream>>>(d_frames, m->src_bytes, m->state, d_par, d_nv, f0, nf, S,
                                                                 m->cfg.var_threshold, bits);
        else if (m->kind == 1)
            k_mog_update<1><<<grid, UPD_BLOCK, 0, ctx->stream>>>(d_frames, m->src_bytes, m->state, d_par, d_nv, f0, nf, S,
                                                                 m->cfg.var_threshold, bits);
        else
            k_mog_update<2><<<grid, UPD_BLOCK, 0, ctx->stream>>>(d_frames, m->src_bytes, m->state, d_par, d_nv, f0, nf, S,
                                                                 m->cfg.var_threshold, bits);
    }
    COVAHIP_CHECK_HIP(ctx, hipGetLastError());
    return COVAHIP_OK;
}

}  // namespace

extern "C" {

void covahip_mog_default_cfg(covahip_mog_cfg *cfg) {
    if (!cfg) return;
    cfg->src_w = 1280;
    cfg->src_h = 720;
    cfg->n_streams = 1;
    cfg->history = 9000;
    cfg->var_threshold = 32.f;
}

int covahip_mog_create(covahip_ctx *ctx, const covahip_mog_cfg *cfg, covahip_mog **out) {
    if (out) *out = nullptr;
    if (!ctx || !cfg || !out) return COVAHIP_ERR_INVALID_ARG;
    if (cfg->n_streams < 1 || cfg->n_streams > COVAHIP_MOG_MAX_STREAMS || cfg->history < 1 || !std::isfinite(cfg->var_threshold) ||
        !(cfg->var_threshold > 0.f))
        return COVAHIP_ERR_INVALID_ARG;
    const int kind = src_kind(cfg->src_w, cfg->src_h);
    if (kind < 0) return COVAHIP_ERR_UNSUPPORTED;
    COVAHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = covahip_primary_op(ctx)) return rc;
    covahip_mog *m = new covahip_mog();
    m->ctx = ctx;
    m->cfg = *cfg;
    m->kind = kind;
    m->src_bytes = (size_t)cfg->src_w * cfg->src_h * 3;
    m->n.assign(cfg->n_streams, 0);
    const size_t sb = STATE_BYTES * cfg->n_streams;
    hipError_t e = hipMalloc(&m->state, sb);
    if (e == hipSuccess) e = hipMemsetAsync(m->state, 0, sb, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        ctx->last_hip_error = std::string("covahip_mog_create: ") + hipGetErrorString(e);
        free_mog(m);
        return COVAHIP_ERR_HIP;
    }
    *out = m;
    return COVAHIP_OK;
}

int covahip_mog_apply(covahip_mog *m, const uint8_t *frames, int n_frames, const int32_t *n_valid, uint8_t *labels, int mem_kind) {
    if (!m || !frames || !labels || n_frames < 1) return COVAHIP_ERR_INVALID_ARG;
    if (mem_kind != COVAHIP_MEM_HOST && mem_kind != COVAHIP_MEM_DEVICE) return COVAHIP_ERR_INVALID_ARG;
    const int S = m->cfg.n_streams;
    std::vector<int32_t> nv(S, n_frames);
    if (n_valid)
        for (int s = 0; s < S; s++) {
            if (n_valid[s] < 0 || n_valid[s] > n_frames) return COVAHIP_ERR_INVALID_ARG;
            nv[s] = n_valid[s];
        }
    covahip_ctx *ctx = m->ctx;
    COVAHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = covahip_primary_op(ctx)) return rc;
    const size_t FS = (size_t)n_frames * S;
    // per-stream, per-frame learning rates, in double as generate-mog.py's OpenCV computes them
    const size_t par_bytes = FS * sizeof(float2) + S * sizeof(int32_t);
    if (m->h_par_bytes < par_bytes) {
        if (m->h_par) COVAHIP_CHECK_HIP(ctx, hipHostFree(m->h_par));
        m->h_par = nullptr;
        m->h_par_bytes = 0;
        COVAHIP_CHECK_HIP(ctx, hipHostMalloc(&m->h_par, par_bytes));
        m->h_par_bytes = par_bytes;
    }
    float2 *hp = static_cast<float2 *>(m->h_par);
    for (int f = 0; f < n_frames; f++)
        for (int s = 0; s < S; s++) {
            const int64_t k = m->n[s] + f + 1;
            const int64_t den = 2 * k < m->cfg.history ? 2 * k : m->cfg.history;
            const double lr = 1.0 / (double)den;
            hp[(size_t)f * S + s] = make_float2((float)lr, (float)(-lr * (double)FCT));
        }
    std::memcpy(hp + FS, nv.data(), S * sizeof(int32_t));
    if (int rc = covahip_ensure_buffer(ctx, &m->d_par, &m->par_bytes, par_bytes)) return rc;
    if (int rc = covahip_ensure_buffer(ctx, &m->bits, &m->bits_bytes, FS * NWORD * 8)) return rc;
    if (int rc = covahip_ensure_buffer(ctx, &m->filled, &m->filled_bytes, FS * NWORD * 8)) return rc;
    COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(m->d_par, hp, par_bytes, hipMemcpyHostToDevice, ctx->stream));
    const float2 *d_par = static_cast<const float2 *>(m->d_par);
    const int32_t *d_nv = reinterpret_cast<const int32_t *>(d_par + FS);
    uint8_t *d_labels = labels;
    if (mem_kind == COVAHIP_MEM_DEVICE) {
        if (int rc = launch_update(m, frames, 0, n_frames, S, d_par, d_nv)) return rc;
    } else {
        // host frames: staged in launches of as many frames as fit the budget (the model is read and written once per launch)
        const size_t step = (size_t)S * m->src_bytes;
        const int per = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_frames, m->stage_budget / step));
        if (int rc = covahip_ensure_buffer(ctx, &m->d_frames, &m->frames_bytes, (size_t)per * step)) return rc;
        for (int f0 = 0; f0 < n_frames; f0 += per) {
            const int nf = std::min(per, n_frames - f0);
            COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(m->d_frames, frames + (size_t)f0 * step, (size_t)nf * step, hipMemcpyHostToDevice,
                                                  ctx->stream));
            if (int rc = launch_update(m, static_cast<const uint8_t *>(m->d_frames), f0, nf, S, d_par, d_nv)) return rc;
        }
        if (int rc = covahip_ensure_buffer(ctx, &m->d_labels, &m->labels_bytes, FS * NLAB)) return rc;
        d_labels = static_cast<uint8_t *>(m->d_labels);
        // labels of frames past n_valid stay as the caller has them
        COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(d_labels, labels, FS * NLAB, hipMemcpyHostToDevice, ctx->stream));
    }
    {
        ProfScope ps(ctx, "mog_post");
        k_mog_post<<<dim3((unsigned)FS), POST_BLOCK, 0, ctx->stream>>>(static_cast<const unsigned long long *>(m->bits),
                                                                       static_cast<unsigned long long *>(m->filled), d_labels, d_nv, S);
    }
    COVAHIP_CHECK_HIP(ctx, hipGetLastError());
    if (mem_kind == COVAHIP_MEM_HOST)
        COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(labels, d_labels, FS * NLAB, hipMemcpyDeviceToHost, ctx->stream));
    COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int s = 0; s < S; s++) m->n[s] += nv[s];
    m->last_frames = n_frames;
    return COVAHIP_OK;
}

int covahip_mog_reset(covahip_mog *m, int stream) {
    if (!m || stream < 0 || stream >= m->cfg.n_streams) return COVAHIP_ERR_INVALID_ARG;
    covahip_ctx *ctx = m->ctx;
    COVAHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = covahip_primary_op(ctx)) return rc;
    COVAHIP_CHECK_HIP(ctx, hipMemsetAsync(m->state + (size_t)stream * STATE_BYTES, 0, STATE_BYTES, ctx->stream));
    m->n[stream] = 0;
    return COVAHIP_OK;
}

void covahip_mog_destroy(covahip_mog *m) {
    if (!m) return;
    hipSetDevice(m->ctx->device);
    covahip_sync_all(m->ctx);
    free_mog(m);
}

int covahip_dev_mog_masks(covahip_mog *m, uint8_t *raw, uint8_t *filled, size_t cap, int *n_frames) {
    if (!m || !n_frames) return COVAHIP_ERR_INVALID_ARG;
    *n_frames = m->last_frames;
    const size_t FS = (size_t)m->last_frames * m->cfg.n_streams;
    if ((raw || filled) && cap < FS * NPIX) return COVAHIP_ERR_OVERFLOW;
    covahip_ctx *ctx = m->ctx;
    COVAHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = covahip_primary_op(ctx)) return rc;
    std::vector<unsigned long long> w(FS * NWORD);
    for (int which = 0; which < 2; which++) {
        uint8_t *out = which ? filled : raw;
        if (!out || !FS) continue;
        COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(w.data(), which ? m->filled : m->bits, FS * NWORD * 8, hipMemcpyDeviceToHost, ctx->stream));
        COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        const uint8_t one = which ? 1 : 255;
        for (size_t i = 0; i < FS * NWORD; i++)
            for (int b = 0; b < 64; b++) out[i * 64 + b] = (w[i] >> b) & 1ull ? one : 0;
    }
    return COVAHIP_OK;
}

int covahip_dev_mog_set_stage_budget(covahip_mog *m, size_t bytes) {
    if (!m) return COVAHIP_ERR_INVALID_ARG;
    m->stage_budget = bytes ? bytes : STAGE_BUDGET;
    return COVAHIP_OK;
}

int covahip_dev_mog_state(covahip_mog *m, int stream, float *W, float *V, float *M, uint8_t *nmodes, int64_t *n) {
    if (!m || stream < 0 || stream >= m->cfg.n_streams) return COVAHIP_ERR_INVALID_ARG;
    covahip_ctx *ctx = m->ctx;
    COVAHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = covahip_primary_op(ctx)) return rc;
    const uint8_t *st = m->state + (size_t)stream * STATE_BYTES;
    const struct { void *dst; size_t off, bytes; } parts[] = {{W, OFF_W, (size_t)NMIX * NPIX * 4},
                                                              {V, OFF_V, (size_t)NMIX * NPIX * 4},
                                                              {M, OFF_M, (size_t)NMIX * 3 * NPIX * 4},
                                                              {nmodes, OFF_N, (size_t)NPIX}};
    for (const auto &pt : parts)
        if (pt.dst) COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(pt.dst, st + pt.off, pt.bytes, hipMemcpyDeviceToHost, ctx->stream));
    COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (n) *n = m->n[stream];
    return COVAHIP_OK;
}

}  // extern "C"
