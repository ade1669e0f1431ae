// MoG label generation (utils/generate-mog.py of the reference): per-pixel MOG2 background subtraction on a working image, then
// close 4x4, open 6x6, hole fill and the ::8 subsample to the labels `tfrecordsink gt=` reads.  The arithmetic is stated in
// include/covahip.h ("MoG labels"); tests/mog_ref.py is its numpy float32 restatement and the kernels match it bit for bit.
// This file has the C-ABI and the host logic and no kernel: the geometries (the reference grid, every source resized to
// 640x360 and 45x80 labels; the macroblock grid, half-resolution working image; covahip_mog_create_any, the macroblock grid at any
// even source size), the checks and the staging of covahip_mog_apply and covahip_mog_apply_yuv (NV12 / I420 surfaces at the
// caller's pitch, offsets and strides), and which kernels a call launches.  The update kernels are templates of mog_update.h,
// instantiated in mog_update.hip and, for a call with shadow detection on (covahip_mog_set_shadows), in mog_shadow.hip, which
// also has the kernel behind covahip_mog_shadow_counts; the post kernels are mog_post.hip's.  All of them run the device code of
// mog_dev.h.  The model as an object is here too: the state blob (covahip_mog_save_state / _load_state, host code around the
// pitched copy of a model), the per-stream frozen flag (a call then launches the update kernels' frozen instances of
// mog_frozen.hip on the frozen streams and the learning ones on the rest) and covahip_mog_background, whose kernel is
// mog_frozen.hip's.
//
// No contraction in this file (see mog_dev.h); the arithmetic on the host, the learning rates, is in double.
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
#include "mog_dev.h"
#include "mog_update.h"

namespace {

using namespace mogdev;
static_assert(G640::LW == COVAHIP_MOG_LABEL_W && G640::LH == COVAHIP_MOG_LABEL_H, "the reference grid's geometry");
// device budget for host frames staged per update launch (covahip_dev_mog_set_stage_budget changes it per labeller)
constexpr size_t STAGE_BUDGET = (size_t)1 << 30;

// the highest band of the banded post kernel at working width mw: band_lds_bytes is linear in the staged rows (a window of 0
// rows is its fixed part, of 1 row one row more), and a band stages HALO_UP + HALO_DOWN rows beside its own
int band_max_rows(int mw) {
    const size_t fixed = band_lds_bytes(mw, 0, 0), per_row = band_lds_bytes(mw, 1, 1) - fixed;
    return (int)((COVAHIP_MOG_BAND_LDS_MAX - fixed) / per_row) - (HALO_UP + HALO_DOWN);
}

// the automatic band plan: as few bands as fit, of equal height
void band_plan(int mw, int mh, int *rows, int *bands) {
    const int mx = std::min(band_max_rows(mw), mh);
    *bands = (mh + mx - 1) / mx;
    *rows = (mh + *bands - 1) / *bands;
}

}  // namespace

struct covahip_mog {
    covahip_ctx *ctx = nullptr;
    covahip_mog_cfg cfg{};
    const MogGeomRow *row = nullptr;   // the (source size, grid) row of MOG_GEOMS, or &own
    MogGeomRow own{};              // covahip_mog_create_any: this labeller's geometry, banded only, run by the general kernels
    bool any = false;
    MogDims alloc{};               // what the planes and the model are sized and laid out by: row->work, or with `any` its rows at
                                   // the pitch of mog_any_pitch
    bool banded = false;           // the banded post kernel, where the row has it
    int band_rows = 0;             // its band height; 0 = the automatic plan
    MogLabelArgs labels;           // covahip_mog_set_labels: how every post launch takes its labels
    int shadows = COVAHIP_MOG_SHADOWS_OFF;     // covahip_mog_set_shadows: every later apply call runs in this mode, with this tau
    float tau = 0.5f;
    int last_shadows = COVAHIP_MOG_SHADOWS_OFF;    // the mode the call behind m->bits ran in: whether m->shadow belongs to it
    std::vector<int32_t> last_nv;  // and its n_valid
    void *shadow = nullptr;        // the call's shadow planes, as bits; allocated by the first call that leaves OFF
    void *d_counts = nullptr;      // covahip_mog_shadow_counts: (shadow, foreground) u32 [F][S][2]
    size_t shadow_bytes = 0, counts_bytes = 0;
    size_t src_bytes = 0;
    std::vector<int64_t> n;        // frames each stream has learned from
    std::vector<uint8_t> frozen;   // covahip_mog_set_frozen, per stream: its frames are classified and the model stays
    void *d_bg = nullptr;          // covahip_mog_background to host memory: the image(s) on the device
    size_t bg_bytes = 0;
    uint8_t *state = nullptr;      // [S][state_bytes]
    void *bits = nullptr, *filled = nullptr, *d_frames = nullptr, *d_labels = nullptr, *d_par = nullptr;
    void *plane = nullptr;         // banded post: the mask after the morphology, as bits
    size_t bits_bytes = 0, filled_bytes = 0, frames_bytes = 0, labels_bytes = 0, par_bytes = 0, plane_bytes = 0;
    void *h_par = nullptr;         // pinned: (alphaT, prune) [F][S], then n_valid [S]
    size_t h_par_bytes = 0;
    int last_frames = 0;
    size_t stage_budget = STAGE_BUDGET;   // bytes of host frames staged per update launch
};

namespace {

void free_mog(covahip_mog *m) {
    for (void *p : {(void *)m->state, m->bits, m->filled, m->plane, m->d_frames, m->d_labels, m->d_par, m->shadow, m->d_counts, m->d_bg})
        if (p) hipFree(p);
    if (m->h_par) hipHostFree(m->h_par);
    delete m;
}

// A checked covahip_mog_yuv: the surface as the update kernels take it, and the bytes lo .. lo + ext of a frame that
// hold its planes' rows (what a call from host memory stages per frame and stream).
struct YuvPlan {
    int format = 0;
    covahip_mog_yuv_src src{};
    size_t lo = 0, ext = 0;
};

// one update launch on device frames: BGR24 (yuv == nullptr) or the surfaces of `yuv`'s format as `src` describes them
// in its learning or its frozen instance; a.nvalid says which streams the launch has
int launch_update(covahip_mog *m, const YuvPlan *yuv, const uint8_t *d_frames, const covahip_mog_yuv_src &src, const MogUpdateArgs &a,
                  bool frozen) {
    if (yuv && yuv->format != COVAHIP_MOG_FMT_NV12 && yuv->format != COVAHIP_MOG_FMT_I420) return COVAHIP_ERR_INVALID_ARG;
    const MogDims &w = m->row->work;
    const MogRoute route{m->any, yuv ? yuv->format : 0, m->row->load, w.mw, w.mh, m->row->resident};
    if (a.shadows == COVAHIP_MOG_SHADOWS_OFF)
        return frozen ? mog_launch_route<false, true>(m->ctx, route, d_frames, m->src_bytes, src, a)
                      : mog_launch_route<false, false>(m->ctx, route, d_frames, m->src_bytes, src, a);
    if (!a.shadow) return COVAHIP_ERR_INVALID_ARG;
    return frozen ? mog_launch_route<true, true>(m->ctx, route, d_frames, m->src_bytes, src, a)
                  : mog_launch_route<true, false>(m->ctx, route, d_frames, m->src_bytes, src, a);
}

// The update launch(es) of frames a.f0 .. a.f0 + a.nf of a call: the learning instance on the streams that learn and the frozen
// one on the rest, each with the n_valid table that has 0 for the other's streams (the kernels skip those block-wise).  A
// labeller with no frozen stream launches what it always has.
int launch_updates(covahip_mog *m, const YuvPlan *yuv, const uint8_t *d_frames, const covahip_mog_yuv_src &src, MogUpdateArgs a,
                   const int32_t *d_nv_learn, const int32_t *d_nv_frozen) {
    if (d_nv_learn) {
        a.nvalid = d_nv_learn;
        if (int rc = launch_update(m, yuv, d_frames, src, a, false)) return rc;
    }
    if (d_nv_frozen) {
        a.nvalid = d_nv_frozen;
        if (int rc = launch_update(m, yuv, d_frames, src, a, true)) return rc;
    }
    return COVAHIP_OK;
}

// the post launch on the call's raw planes (m->bits): filled planes and labels of FS (frame, stream) pairs
int launch_post(covahip_mog *m, uint8_t *d_labels, const int32_t *d_nv, int S, size_t FS) {
    covahip_ctx *ctx = m->ctx;
    auto *bits = static_cast<const unsigned long long *>(m->bits);
    auto *filled = static_cast<unsigned long long *>(m->filled);
    if (m->banded) {
        if (int rc = covahip_ensure_buffer(ctx, &m->plane, &m->plane_bytes, FS * m->alloc.nword() * 8)) return rc;
        int rows = m->band_rows, bands = 0;
        if (!rows) band_plan(m->alloc.mw, m->alloc.mh, &rows, &bands);
        return covahip_mog_band_post(ctx, m->any, m->row->work.mw, m->row->work.mh, bits, filled, static_cast<unsigned long long *>(m->plane),
                                     d_labels, d_nv, S, FS, rows, m->labels);
    }
    return covahip_mog_grid_post(ctx, m->row->work.mw, bits, filled, d_labels, d_nv, S, FS, m->labels);
}

bool cfg_ok(const covahip_mog_cfg *cfg) {
    return cfg->n_streams >= 1 && cfg->n_streams <= COVAHIP_MOG_MAX_STREAMS && cfg->history >= 1 && std::isfinite(cfg->var_threshold) &&
           cfg->var_threshold > 0.f;
}

// the labeller of a checked cfg: on `row` of MOG_GEOMS, or (row == nullptr) the general kernels at half the source
int create_mog(covahip_ctx *ctx, const covahip_mog_cfg *cfg, const MogGeomRow *row, covahip_mog **out) {
    COVAHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = covahip_primary_op(ctx)) return rc;
    covahip_mog *m = new covahip_mog();
    m->ctx = ctx;
    m->cfg = *cfg;
    if (row) {
        m->row = row;
        m->alloc = row->work;
    } else {
        const MogDims work{cfg->src_w / 2, cfg->src_h / 2};
        m->own = MogGeomRow{cfg->src_w, cfg->src_h, MOG_ON_MB, work, MOG_LOAD_HALF, false, true, true};
        m->row = &m->own;
        m->any = true;
        m->alloc = MogDims{mog_any_pitch(work.mw), work.mh};
    }
    m->banded = m->row->starts_banded;
    m->src_bytes = (size_t)cfg->src_w * cfg->src_h * 3;
    m->n.assign(cfg->n_streams, 0);
    m->frozen.assign(cfg->n_streams, 0);
    const size_t sb = m->alloc.state_bytes() * cfg->n_streams;
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

// One stream's model between the device (rows at the pitch d.mw) and host arrays whose rows are dense, [work_h][work_w]: W, V
// f32 [5][..], M f32 [5][3][..], nmodes u8 [..]; a NULL array is skipped.  to_host: the direction.  The copies go to ctx->stream;
// the caller waits.  A padded row's lanes at x >= work_w are neither read nor written.
int copy_model(covahip_mog *m, int stream, void *W, void *V, void *M, void *nmodes, bool to_host) {
    covahip_ctx *ctx = m->ctx;
    const MogDims &d = m->alloc;
    uint8_t *st = m->state + (size_t)stream * d.state_bytes();
    // elem: bytes per pixel and array
    const struct { void *host; size_t off, end, elem; } parts[] = {{W, 0, d.off_v(), 4},
                                                                   {V, d.off_v(), d.off_m(), 4},
                                                                   {M, d.off_m(), d.off_n(), 4},
                                                                   {nmodes, d.off_n(), d.state_bytes(), 1}};
    const size_t mw = m->row->work.mw;
    const hipMemcpyKind kind = to_host ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice;
    for (const auto &pt : parts) {
        if (!pt.host) continue;
        uint8_t *dev = st + pt.off;
        const size_t dpitch = d.mw * pt.elem, hpitch = mw * pt.elem, rows = (pt.end - pt.off) / dpitch;
        if (d.mw == (int)mw)
            COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(to_host ? pt.host : (void *)dev, to_host ? (const void *)dev : pt.host, pt.end - pt.off, kind,
                                                  ctx->stream));
        else if (to_host)
            COVAHIP_CHECK_HIP(ctx, hipMemcpy2DAsync(pt.host, hpitch, dev, dpitch, hpitch, rows, kind, ctx->stream));
        else
            COVAHIP_CHECK_HIP(ctx, hipMemcpy2DAsync(dev, dpitch, pt.host, hpitch, hpitch, rows, kind, ctx->stream));
    }
    return COVAHIP_OK;
}

// the state blob of include/covahip.h ("MoG labels", model state): a header of 64 bytes, 101 bytes per working pixel, the CRC
constexpr uint32_t B_MAGIC = 0x4D485643, B_VERSION = 1;       // "CVHM"
constexpr size_t B_HEADER = 64;
constexpr size_t blob_bytes(size_t npix) { return B_HEADER + 101 * npix + 4; }
template <class T>
void put(uint8_t *p, size_t off, T v) {
    std::memcpy(p + off, &v, sizeof(T));
}
template <class T>
T get(const uint8_t *p, size_t off) {
    T v;
    std::memcpy(&v, p + off, sizeof(T));
    return v;
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
    return covahip_mog_create_grid(ctx, cfg, COVAHIP_MOG_GRID_REFERENCE, out);
}

int covahip_mog_create_grid(covahip_ctx *ctx, const covahip_mog_cfg *cfg, int grid, covahip_mog **out) {
    if (out) *out = nullptr;
    if (!ctx || !cfg || !out) return COVAHIP_ERR_INVALID_ARG;
    if (grid != COVAHIP_MOG_GRID_REFERENCE && grid != COVAHIP_MOG_GRID_MACROBLOCK) return COVAHIP_ERR_INVALID_ARG;
    if (!cfg_ok(cfg)) return COVAHIP_ERR_INVALID_ARG;
    const MogGeomRow *row = mog_geom_row(cfg->src_w, cfg->src_h, grid);
    if (!row) return COVAHIP_ERR_UNSUPPORTED;
    return create_mog(ctx, cfg, row, out);
}

int covahip_mog_create_any(covahip_ctx *ctx, const covahip_mog_cfg *cfg, covahip_mog **out) {
    if (out) *out = nullptr;
    if (!ctx || !cfg || !out) return COVAHIP_ERR_INVALID_ARG;
    if (!cfg_ok(cfg)) return COVAHIP_ERR_INVALID_ARG;
    for (const int v : {cfg->src_w, cfg->src_h})
        if (v % 2 || v < COVAHIP_MOG_ANY_MIN || v > COVAHIP_MOG_ANY_MAX) return COVAHIP_ERR_UNSUPPORTED;
    return create_mog(ctx, cfg, nullptr, out);
}

}  // extern "C"

namespace {

// One call of either entry: frames are BGR24 [n_frames][S][src] (yuv == nullptr) or the surfaces `yuv` describes from `frames`.
int apply_frames(covahip_mog *m, const uint8_t *frames, const YuvPlan *yuv, int n_frames, const int32_t *n_valid, uint8_t *labels,
                 int mem_kind) {
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
    const size_t NWORD = m->alloc.nword(), NLAB = m->row->work.nlab();   // this labeller's geometry
    // per-stream, per-frame learning rates, in double as generate-mog.py's OpenCV computes them
    // (behind them n_valid [S], and where a stream is frozen the two launches' tables: n_valid of the learning streams with 0
    // for the frozen ones, and the reverse)
    const int n_frozen = (int)std::count(m->frozen.begin(), m->frozen.end(), 1);
    const size_t par_bytes = FS * sizeof(float2) + (n_frozen ? 3 : 1) * S * sizeof(int32_t);
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
    int32_t *hnv = reinterpret_cast<int32_t *>(hp + FS);
    std::memcpy(hnv, nv.data(), S * sizeof(int32_t));
    if (n_frozen)
        for (int s = 0; s < S; s++) {
            hnv[S + s] = m->frozen[s] ? 0 : nv[s];
            hnv[2 * S + s] = m->frozen[s] ? nv[s] : 0;
        }
    if (int rc = covahip_ensure_buffer(ctx, &m->d_par, &m->par_bytes, par_bytes)) return rc;
    if (int rc = covahip_ensure_buffer(ctx, &m->bits, &m->bits_bytes, FS * NWORD * 8)) return rc;
    if (int rc = covahip_ensure_buffer(ctx, &m->filled, &m->filled_bytes, FS * NWORD * 8)) return rc;
    COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(m->d_par, hp, par_bytes, hipMemcpyHostToDevice, ctx->stream));
    const float2 *d_par = static_cast<const float2 *>(m->d_par);
    const int32_t *d_nv = reinterpret_cast<const int32_t *>(d_par + FS);
    const int32_t *d_nv_learn = !n_frozen ? d_nv : (n_frozen < S ? d_nv + S : nullptr), *d_nv_frozen = n_frozen ? d_nv + 2 * S : nullptr;
    MogUpdateArgs a{m->state, d_par, d_nv, 0, n_frames, S, m->cfg.var_threshold, static_cast<unsigned long long *>(m->bits)};
    if (m->shadows != COVAHIP_MOG_SHADOWS_OFF) {
        if (int rc = covahip_ensure_buffer(ctx, &m->shadow, &m->shadow_bytes, FS * NWORD * 8)) return rc;
        a.shadows = m->shadows;
        a.tau = m->tau;
        a.shadow = static_cast<unsigned long long *>(m->shadow);
    }
    covahip_mog_yuv_src src = yuv ? yuv->src : covahip_mog_yuv_src{};
    uint8_t *d_labels = labels;
    if (mem_kind == COVAHIP_MEM_DEVICE) {
        if (int rc = launch_updates(m, yuv, frames, src, a, d_nv_learn, d_nv_frozen)) return rc;
    } else {
        // host memory: staged in launches of as many frames as fit the budget (the model is read and written once per launch).
        // Per (frame, stream) the extent lo .. lo + ext of the frame (a BGR24 frame: all of it) is staged, densely and
        // frame-major, so a kernel on surfaces sees the caller's plane offsets less lo and the caller's pitches; nothing outside
        // an extent is read.  Frames that lie so already (BGR24; covahip_mog_yuv_tight's layout) are one copy per launch.
        const size_t lo = yuv ? yuv->lo : 0, ext = yuv ? yuv->ext : m->src_bytes, slot = yuv ? (ext + 15) & ~(size_t)15 : ext;
        const bool dense = !yuv || ((size_t)src.stream_stride == ext && (size_t)src.frame_stride == (size_t)S * ext);
        const size_t step = (size_t)S * (dense ? ext : slot);   // staged bytes per frame of the call
        const long long h_frame = dense ? (long long)step : src.frame_stride, h_stream = src.stream_stride;
        const int per = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_frames, m->stage_budget / step));
        if (int rc = covahip_ensure_buffer(ctx, &m->d_frames, &m->frames_bytes, (size_t)per * step)) return rc;
        uint8_t *d = static_cast<uint8_t *>(m->d_frames);
        for (int p = 0; p < 3; p++) src.off[p] -= (long long)lo;
        if (!dense) src.stream_stride = (long long)slot, src.frame_stride = (long long)step;
        for (a.f0 = 0; a.f0 < n_frames; a.f0 += per) {
            a.nf = std::min(per, n_frames - a.f0);
            const uint8_t *h0 = frames + lo + (long long)a.f0 * h_frame;
            if (dense) {
                COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(d, h0, (size_t)a.nf * step, hipMemcpyHostToDevice, ctx->stream));
            } else {
                for (int f = 0; f < a.nf; f++)
                    for (int s = 0; s < S; s++) {
                        if (a.f0 + f >= nv[s]) continue;   // frames past n_valid are not read at all
                        COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(d + (size_t)f * step + (size_t)s * slot, h0 + f * h_frame + s * h_stream, ext,
                                                              hipMemcpyHostToDevice, ctx->stream));
                    }
            }
            if (int rc = launch_updates(m, yuv, d, src, a, d_nv_learn, d_nv_frozen)) return rc;
        }
        if (int rc = covahip_ensure_buffer(ctx, &m->d_labels, &m->labels_bytes, FS * NLAB)) return rc;
        d_labels = static_cast<uint8_t *>(m->d_labels);
        // labels of frames past n_valid stay as the caller has them
        COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(d_labels, labels, FS * NLAB, hipMemcpyHostToDevice, ctx->stream));
    }
    if (int rc = launch_post(m, d_labels, d_nv, S, FS)) return rc;
    if (mem_kind == COVAHIP_MEM_HOST)
        COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(labels, d_labels, FS * NLAB, hipMemcpyDeviceToHost, ctx->stream));
    COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int s = 0; s < S; s++)
        if (!m->frozen[s]) m->n[s] += nv[s];
    m->last_frames = n_frames;
    m->last_shadows = a.shadows;
    m->last_nv = nv;
    return COVAHIP_OK;
}

}  // namespace

extern "C" {

int covahip_mog_apply(covahip_mog *m, const uint8_t *frames, int n_frames, const int32_t *n_valid, uint8_t *labels, int mem_kind) {
    return apply_frames(m, frames, nullptr, n_frames, n_valid, labels, mem_kind);
}

int covahip_mog_yuv_tight(const covahip_mog *m, int format, int range, covahip_mog_yuv *out) {
    if (!m || !out) return COVAHIP_ERR_INVALID_ARG;
    if (format != COVAHIP_MOG_FMT_NV12 && format != COVAHIP_MOG_FMT_I420) return COVAHIP_ERR_INVALID_ARG;
    if (range != COVAHIP_MOG_RANGE_LIMITED && range != COVAHIP_MOG_RANGE_FULL) return COVAHIP_ERR_INVALID_ARG;
    const int64_t w = m->cfg.src_w, h = m->cfg.src_h;
    std::memset(out, 0, sizeof(*out));
    out->format = format;
    out->range = range;
    out->offset[1] = w * h;
    out->pitch[0] = w;
    if (format == COVAHIP_MOG_FMT_NV12) {
        out->pitch[1] = w;
    } else {
        out->offset[2] = w * h + w * h / 4;
        out->pitch[1] = out->pitch[2] = w / 2;
    }
    out->stream_stride = w * h * 3 / 2;
    out->frame_stride = out->stream_stride * m->cfg.n_streams;
    return COVAHIP_OK;
}

int covahip_mog_apply_yuv(covahip_mog *m, const covahip_mog_yuv *lay, const uint8_t *base, int n_frames, const int32_t *n_valid,
                          uint8_t *labels, int mem_kind) {
    if (!m || !lay || !base || !labels) return COVAHIP_ERR_INVALID_ARG;
    const bool nv12 = lay->format == COVAHIP_MOG_FMT_NV12;
    if (!nv12 && lay->format != COVAHIP_MOG_FMT_I420) return COVAHIP_ERR_INVALID_ARG;
    if (lay->range != COVAHIP_MOG_RANGE_LIMITED && lay->range != COVAHIP_MOG_RANGE_FULL) return COVAHIP_ERR_INVALID_ARG;
    const int64_t w = m->cfg.src_w, h = m->cfg.src_h;
    const int planes = nv12 ? 2 : 3;
    const int64_t row_bytes[3] = {w, nv12 ? w : w / 2, w / 2}, rows[3] = {h, h / 2, h / 2};
    if ((reinterpret_cast<uintptr_t>(base) & 1) || lay->frame_stride < 0 || lay->stream_stride < 0 ||
        ((lay->frame_stride | lay->stream_stride) & 1))
        return COVAHIP_ERR_INVALID_ARG;
    YuvPlan plan{};
    int64_t lo = INT64_MAX, hi = 0;
    for (int p = 0; p < planes; p++) {
        // (an any-size labeller takes I420's U and V at odd offsets and pitches: they are loaded byte by byte, and where
        // src_w / 2 is odd a tight frame has them so)
        const bool odd_ok = m->any && !nv12 && p > 0;
        if (lay->offset[p] < 0 || lay->pitch[p] < row_bytes[p] || (!odd_ok && ((lay->offset[p] | lay->pitch[p]) & 1)))
            return COVAHIP_ERR_INVALID_ARG;
        lo = std::min(lo, lay->offset[p]);
        hi = std::max(hi, lay->offset[p] + (rows[p] - 1) * lay->pitch[p] + row_bytes[p]);
        plan.src.off[p] = lay->offset[p];
        plan.src.pitch[p] = lay->pitch[p];
    }
    plan.format = lay->format;
    lo -= lo & 1;                  // (staged Y rows keep their even addresses where an odd chroma offset is the lowest)
    plan.lo = (size_t)lo;
    plan.ext = (size_t)(hi - lo);
    plan.src.frame_stride = lay->frame_stride;
    plan.src.stream_stride = lay->stream_stride;
    const bool full = lay->range == COVAHIP_MOG_RANGE_FULL;
    plan.src.ysub = full ? 0 : 16;
    plan.src.ymul = full ? 1 << 20 : 1220542;
    plan.src.bu = full ? 1858077 : 2116026;
    plan.src.gv = full ? 748826 : 852492;
    plan.src.gu = full ? 360853 : 409993;
    plan.src.rv = full ? 1470104 : 1673527;
    return apply_frames(m, base, &plan, n_frames, n_valid, labels, mem_kind);
}

int covahip_mog_reset(covahip_mog *m, int stream) {
    if (!m || stream < 0 || stream >= m->cfg.n_streams) return COVAHIP_ERR_INVALID_ARG;
    covahip_ctx *ctx = m->ctx;
    COVAHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = covahip_primary_op(ctx)) return rc;
    COVAHIP_CHECK_HIP(ctx, hipMemsetAsync(m->state + (size_t)stream * m->alloc.state_bytes(), 0, m->alloc.state_bytes(), ctx->stream));
    m->n[stream] = 0;
    return COVAHIP_OK;
}

int covahip_mog_set_labels(covahip_mog *m, int mode, int min_cover) {
    if (!m) return COVAHIP_ERR_INVALID_ARG;
    if (mode != COVAHIP_MOG_LABELS_CORNER && mode != COVAHIP_MOG_LABELS_COVER && mode != COVAHIP_MOG_LABELS_COUNT)
        return COVAHIP_ERR_INVALID_ARG;
    if (mode == COVAHIP_MOG_LABELS_COVER) {
        if (min_cover < 1 || min_cover > 64) return COVAHIP_ERR_INVALID_ARG;
        m->labels.ncover = min_cover;          // (read in COVER mode only: the other modes keep the last one)
    }
    m->labels.mode = mode;
    return COVAHIP_OK;
}

int covahip_mog_get_labels(const covahip_mog *m, int *mode, int *min_cover) {
    if (!m) return COVAHIP_ERR_INVALID_ARG;
    if (mode) *mode = m->labels.mode;
    if (min_cover) *min_cover = m->labels.ncover;
    return COVAHIP_OK;
}

int covahip_mog_set_shadows(covahip_mog *m, int mode, float tau) {
    if (!m) return COVAHIP_ERR_INVALID_ARG;
    if (mode != COVAHIP_MOG_SHADOWS_OFF && mode != COVAHIP_MOG_SHADOWS_DROP && mode != COVAHIP_MOG_SHADOWS_KEEP)
        return COVAHIP_ERR_INVALID_ARG;
    if (mode != COVAHIP_MOG_SHADOWS_OFF) {
        if (!std::isfinite(tau) || !(tau > 0.f) || tau > 1.f) return COVAHIP_ERR_INVALID_ARG;
        m->tau = tau;                          // (read when the test runs: OFF keeps the last one)
    }
    m->shadows = mode;
    return COVAHIP_OK;
}

int covahip_mog_get_shadows(const covahip_mog *m, int *mode, float *tau) {
    if (!m) return COVAHIP_ERR_INVALID_ARG;
    if (mode) *mode = m->shadows;
    if (tau) *tau = m->tau;
    return COVAHIP_OK;
}

int covahip_mog_shadow_counts(covahip_mog *m, uint32_t *shadow, uint32_t *foreground, size_t cap, int *n_frames) {
    if (!m) return COVAHIP_ERR_INVALID_ARG;
    if (n_frames) *n_frames = m->last_frames;
    const int S = m->cfg.n_streams;
    const size_t FS = (size_t)m->last_frames * S;
    if ((shadow || foreground) && cap < FS) return COVAHIP_ERR_OVERFLOW;
    if (!(shadow || foreground) || !FS) return COVAHIP_OK;
    covahip_ctx *ctx = m->ctx;
    COVAHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = covahip_primary_op(ctx)) return rc;
    if (int rc = covahip_ensure_buffer(ctx, &m->d_counts, &m->counts_bytes, FS * 2 * sizeof(uint32_t))) return rc;
    const bool on = m->last_shadows != COVAHIP_MOG_SHADOWS_OFF;
    if (int rc = covahip_mog_counts(ctx, static_cast<const unsigned long long *>(m->bits),
                                    on ? static_cast<const unsigned long long *>(m->shadow) : nullptr, m->alloc.nword(), FS,
                                    static_cast<uint32_t *>(m->d_counts)))
        return rc;
    std::vector<uint32_t> c(FS * 2);
    COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(c.data(), m->d_counts, FS * 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < FS; i++) {
        const bool valid = (int)(i / S) < m->last_nv[i % S];   // (the planes of frames past n_valid were never written)
        if (shadow) shadow[i] = valid ? c[2 * i] : 0;
        if (foreground) foreground[i] = valid ? c[2 * i + 1] : 0;
    }
    return COVAHIP_OK;
}

int covahip_mog_dims(const covahip_mog *m, int32_t *work_w, int32_t *work_h, int32_t *label_w, int32_t *label_h) {
    if (!m) return COVAHIP_ERR_INVALID_ARG;
    if (work_w) *work_w = m->row->work.mw;
    if (work_h) *work_h = m->row->work.mh;
    if (label_w) *label_w = m->row->work.lw();
    if (label_h) *label_h = m->row->work.lh();
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
    const size_t NPIX = m->row->work.npix(), NWORD = m->alloc.nword();
    const size_t mw = m->row->work.mw, roww = m->alloc.mw / 64, NROW = FS * m->alloc.mh;   // a plane row: mw pixels of roww words
    if ((raw || filled) && cap < FS * NPIX) return COVAHIP_ERR_OVERFLOW;
    covahip_ctx *ctx = m->ctx;
    COVAHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = covahip_primary_op(ctx)) return rc;
    std::vector<unsigned long long> w(FS * NWORD), sh;
    if (raw && FS && m->last_shadows != COVAHIP_MOG_SHADOWS_OFF) {     // the call's shadow planes: 127 wherever a bit is set
        sh.resize(FS * NWORD);
        COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(sh.data(), m->shadow, FS * NWORD * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    for (int which = 0; which < 2; which++) {
        uint8_t *out = which ? filled : raw;
        if (!out || !FS) continue;
        COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(w.data(), which ? m->filled : m->bits, FS * NWORD * 8, hipMemcpyDeviceToHost, ctx->stream));
        COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        const uint8_t one = which ? 1 : 255;
        for (size_t r = 0; r < NROW; r++)
            for (size_t x = 0; x < mw; x++) out[r * mw + x] = (w[r * roww + x / 64] >> (x % 64)) & 1ull ? one : 0;
        if (!which && !sh.empty())
            for (size_t r = 0; r < NROW; r++)
                for (size_t x = 0; x < mw; x++)
                    if ((sh[r * roww + x / 64] >> (x % 64)) & 1ull) out[r * mw + x] = 127;
    }
    return COVAHIP_OK;
}

int covahip_dev_mog_set_stage_budget(covahip_mog *m, size_t bytes) {
    if (!m) return COVAHIP_ERR_INVALID_ARG;
    m->stage_budget = bytes ? bytes : STAGE_BUDGET;
    return COVAHIP_OK;
}

int covahip_dev_mog_post_masks(covahip_mog *m, const uint8_t *raw, int n_frames, uint8_t *labels) {
    if (!m || !raw || !labels || n_frames < 1) return COVAHIP_ERR_INVALID_ARG;
    covahip_ctx *ctx = m->ctx;
    COVAHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = covahip_primary_op(ctx)) return rc;
    const int S = m->cfg.n_streams;
    const size_t FS = (size_t)n_frames * S, NWORD = m->alloc.nword(), NLAB = m->row->work.nlab();
    const size_t mw = m->row->work.mw, roww = m->alloc.mw / 64, NROW = FS * m->alloc.mh;
    std::vector<unsigned long long> w(FS * NWORD, 0ull);       // (the bits beyond a row's mw pixels stay 0)
    for (size_t r = 0; r < NROW; r++)
        for (size_t x = 0; x < mw; x++) w[r * roww + x / 64] |= (unsigned long long)(raw[r * mw + x] != 0) << (x % 64);
    const std::vector<int32_t> nv(S, n_frames);
    if (int rc = covahip_ensure_buffer(ctx, &m->d_par, &m->par_bytes, S * sizeof(int32_t))) return rc;
    if (int rc = covahip_ensure_buffer(ctx, &m->bits, &m->bits_bytes, FS * NWORD * 8)) return rc;
    if (int rc = covahip_ensure_buffer(ctx, &m->filled, &m->filled_bytes, FS * NWORD * 8)) return rc;
    if (int rc = covahip_ensure_buffer(ctx, &m->d_labels, &m->labels_bytes, FS * NLAB)) return rc;
    COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(m->d_par, nv.data(), S * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(m->bits, w.data(), FS * NWORD * 8, hipMemcpyHostToDevice, ctx->stream));
    if (int rc = launch_post(m, static_cast<uint8_t *>(m->d_labels), static_cast<const int32_t *>(m->d_par), S, FS)) return rc;
    COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(labels, m->d_labels, FS * NLAB, hipMemcpyDeviceToHost, ctx->stream));
    COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    m->last_frames = n_frames;
    m->last_shadows = COVAHIP_MOG_SHADOWS_OFF;     // these planes are the caller's: no shadow plane goes with them
    m->last_nv = nv;
    return COVAHIP_OK;
}

int covahip_dev_mog_set_post_form(covahip_mog *m, int banded, int band_rows) {
    if (!m || (banded != 0 && banded != 1)) return COVAHIP_ERR_INVALID_ARG;
    if (banded ? !m->row->banded : !m->row->resident || band_rows != 0) return COVAHIP_ERR_INVALID_ARG;
    if (banded && band_rows != 0 &&
        (band_rows < 16 || band_rows > m->alloc.mh || band_lds_bytes(m->alloc.mw, m->alloc.mh, band_rows) > COVAHIP_MOG_BAND_LDS_MAX))
        return COVAHIP_ERR_INVALID_ARG;
    m->banded = banded != 0;
    m->band_rows = band_rows;
    return COVAHIP_OK;
}

int covahip_dev_mog_band_plan(int work_w, int work_h, int *rows, int *bands, size_t *lds_bytes) {
    if (work_w < 64 || work_w % 64 || work_h < 16 || band_max_rows(work_w) < 16) return COVAHIP_ERR_INVALID_ARG;
    int r = 0, b = 0;
    band_plan(work_w, work_h, &r, &b);
    if (rows) *rows = r;
    if (bands) *bands = b;
    if (lds_bytes) *lds_bytes = band_lds_bytes(work_w, work_h, r);
    return COVAHIP_OK;
}

int covahip_dev_mog_state(covahip_mog *m, int stream, float *W, float *V, float *M, uint8_t *nmodes, int64_t *n) {
    if (!m || stream < 0 || stream >= m->cfg.n_streams) return COVAHIP_ERR_INVALID_ARG;
    covahip_ctx *ctx = m->ctx;
    COVAHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = covahip_primary_op(ctx)) return rc;
    if (int rc = copy_model(m, stream, W, V, M, nmodes, true)) return rc;
    COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (n) *n = m->n[stream];
    return COVAHIP_OK;
}

int covahip_mog_state_size(const covahip_mog *m, size_t *n) {
    if (!m || !n) return COVAHIP_ERR_INVALID_ARG;
    *n = blob_bytes(m->row->work.npix());
    return COVAHIP_OK;
}

int covahip_mog_save_state(covahip_mog *m, int stream, void *buf, size_t cap, size_t *n) {
    if (!m || !n || stream < 0 || stream >= m->cfg.n_streams) return COVAHIP_ERR_INVALID_ARG;
    const size_t P = m->row->work.npix(), need = blob_bytes(P);
    *n = need;
    if (!buf || cap < need) return COVAHIP_ERR_OVERFLOW;
    covahip_ctx *ctx = m->ctx;
    COVAHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = covahip_primary_op(ctx)) return rc;
    uint8_t *p = static_cast<uint8_t *>(buf);
    std::memset(p, 0, B_HEADER);
    put<uint32_t>(p, 0, B_MAGIC);
    put<uint32_t>(p, 4, B_VERSION);
    put<int32_t>(p, 8, m->row->work.mw);
    put<int32_t>(p, 12, m->row->work.mh);
    put<int32_t>(p, 16, m->cfg.history);
    put<float>(p, 20, m->cfg.var_threshold);
    put<int64_t>(p, 24, m->n[stream]);
    uint8_t *q = p + B_HEADER;                                 // W, V, M, nmodes, dense
    if (int rc = copy_model(m, stream, q, q + 20 * P, q + 40 * P, q + 100 * P, true)) return rc;
    COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    put<uint32_t>(p, need - 4, covahip_crc32c(p, need - 4));
    return COVAHIP_OK;
}

int covahip_mog_load_state(covahip_mog *m, int stream, const void *buf, size_t n) {
    if (!m || !buf || stream < 0 || stream >= m->cfg.n_streams) return COVAHIP_ERR_INVALID_ARG;
    const uint8_t *p = static_cast<const uint8_t *>(buf);
    if (n < B_HEADER + 4 || get<uint32_t>(p, 0) != B_MAGIC || get<uint32_t>(p, 4) != B_VERSION) return COVAHIP_ERR_BAD_DATA;
    const int32_t bw = get<int32_t>(p, 8), bh = get<int32_t>(p, 12);
    if (bw < 1 || bh < 1 || bw > COVAHIP_MOG_ANY_MAX || bh > COVAHIP_MOG_ANY_MAX) return COVAHIP_ERR_BAD_DATA;
    const size_t P = (size_t)bw * bh;
    if (n != blob_bytes(P)) return COVAHIP_ERR_BAD_DATA;
    if (get<uint32_t>(p, n - 4) != covahip_crc32c(p, n - 4)) return COVAHIP_ERR_BAD_DATA;
    const int64_t frames = get<int64_t>(p, 24);
    if (frames < 0) return COVAHIP_ERR_BAD_DATA;
    const uint8_t *q = p + B_HEADER;
    for (size_t i = 0; i < P; i++)
        if (q[100 * P + i] > NMIX) return COVAHIP_ERR_BAD_DATA;
    if (bw != m->row->work.mw || bh != m->row->work.mh) return COVAHIP_ERR_INVALID_ARG;
    covahip_ctx *ctx = m->ctx;
    COVAHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = covahip_primary_op(ctx)) return rc;
    uint8_t *w = const_cast<uint8_t *>(q);                     // (copy_model only reads it in this direction)
    if (int rc = copy_model(m, stream, w, w + 20 * P, w + 40 * P, w + 100 * P, false)) return rc;
    COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    m->n[stream] = frames;
    return COVAHIP_OK;
}

int covahip_mog_set_frozen(covahip_mog *m, int stream, int frozen) {
    if (!m || stream < -1 || stream >= m->cfg.n_streams || (frozen != 0 && frozen != 1)) return COVAHIP_ERR_INVALID_ARG;
    for (int s = 0; s < m->cfg.n_streams; s++)
        if (stream < 0 || s == stream) m->frozen[s] = (uint8_t)frozen;
    return COVAHIP_OK;
}

int covahip_mog_get_frozen(const covahip_mog *m, int stream, int *frozen) {
    if (!m || !frozen || stream < 0 || stream >= m->cfg.n_streams) return COVAHIP_ERR_INVALID_ARG;
    *frozen = m->frozen[stream];
    return COVAHIP_OK;
}

int covahip_mog_background(covahip_mog *m, int stream, uint8_t *bgr, size_t cap, int mem_kind) {
    if (!m || stream < -1 || stream >= m->cfg.n_streams) return COVAHIP_ERR_INVALID_ARG;
    if (mem_kind != COVAHIP_MEM_HOST && mem_kind != COVAHIP_MEM_DEVICE) return COVAHIP_ERR_INVALID_ARG;
    const int ns = stream < 0 ? m->cfg.n_streams : 1, s0 = stream < 0 ? 0 : stream;
    const size_t need = (size_t)ns * m->row->work.npix() * 3;
    if (!bgr || cap < need) return COVAHIP_ERR_OVERFLOW;
    covahip_ctx *ctx = m->ctx;
    COVAHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = covahip_primary_op(ctx)) return rc;
    uint8_t *d_out = bgr;
    if (mem_kind == COVAHIP_MEM_HOST) {
        if (int rc = covahip_ensure_buffer(ctx, &m->d_bg, &m->bg_bytes, need)) return rc;
        d_out = static_cast<uint8_t *>(m->d_bg);
    }
    const size_t sb = m->alloc.state_bytes();
    if (int rc = covahip_mog_background_launch(ctx, m->state + (size_t)s0 * sb, sb, m->alloc.mw, m->row->work.mw, m->row->work.mh, ns, d_out))
        return rc;
    if (mem_kind == COVAHIP_MEM_HOST) COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(bgr, d_out, need, hipMemcpyDeviceToHost, ctx->stream));
    COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return COVAHIP_OK;
}

}  // extern "C"
