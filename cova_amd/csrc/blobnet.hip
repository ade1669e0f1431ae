// BlobNet model state: weight blob validation, geometry (pad / crop rules), HBM
// workspace, and the C-ABI entry points covahip_blobnet_* / covahip_filter_forward.
//
// Geometry follows utils/model/encoder.py:58-80 (level i -> ceil(H/2) x ceil(W/2), zero
// row on top / zero column on the left when the pre-pool size is odd) and
// utils/model/decoder.py:43-59 (convT output 2*in+2, crop ceil(p/2) top/left).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "blobnet.h"
#include "covahip_dev.h"

static void free_model(covahip_ctx *ctx, covahip_blobnet *m) {
    if (!m) return;
    blobnet_release_mfma(ctx, m);
    if (m->d_post) hipFree(m->d_post);
    for (BnWorkspace &ws : m->ws) {
        for (int i = 0; i <= BN_LEVELS; i++)
            if (ws.act[i]) hipFree(ws.act[i]);
        for (int j = 0; j < BN_LEVELS; j++)
            if (ws.dact[j]) hipFree(ws.dact[j]);
        if (ws.pbuf) hipFree(ws.pbuf);
        if (ws.part) hipFree(ws.part);
        if (ws.planes) hipFree(ws.planes);
        ws.index.release();
        ws.models.release();
        ws.areas.release();
    }
    delete m;
}

void covahip_blobnet_destroy(covahip_ctx *ctx) {
    if (!ctx->blobnet) return;
    hipSetDevice(ctx->device);
    covahip_sync_all(ctx);
    covahip_monitor_close(ctx, true);   // an attached monitor counts THIS model's batches: it goes with it
    free_model(ctx, ctx->blobnet);
    ctx->blobnet = nullptr;
}

int covahip_blobnet_geometry(covahip_ctx *ctx, int *h, int *w) {
    if (!ctx->blobnet) return COVAHIP_ERR_NOT_LOADED;
    *h = ctx->blobnet->H;
    *w = ctx->blobnet->W;
    return COVAHIP_OK;
}

// Model sets: every id of a call names a model of the set.
static int check_model_ids(const covahip_blobnet *m, const uint8_t *model_ids, int batch) {
    if (model_ids)
        for (int b = 0; b < batch; b++)
            if (model_ids[b] >= m->n_models) return COVAHIP_ERR_INVALID_ARG;
    return COVAHIP_OK;
}

// The model ids of a call (host array, one per stack; null: model 0) -> in.  A batch of ONE model runs the single-model kernels on
// that model's weights (in.model); a mixed batch gets its ids per stack and per carrier frame uploaded to the lane's workspace
// (in.model_ids, in.frame_models; ids equal to the resident ones are not uploaded again).  table: the stack -> frame table of a
// carrier-frame call, null for the stacked entry (stack b = frames 4b .. 4b+3).  Level 0 runs once per carrier frame, so a frame
// that stacks of two models read is an error; a frame no stack reads runs under model 0.
static int resolve_models(covahip_ctx *ctx, covahip_blobnet *m, BnWorkspace &ws, const uint8_t *model_ids, int batch,
                          const int32_t *table, int n_frames, BnInput &in) {
    in.model = 0;
    in.model_ids = nullptr;
    in.frame_models = nullptr;
    in.h_model_ids = nullptr;
    if (!model_ids) return COVAHIP_OK;
    if (int rc = check_model_ids(m, model_ids, batch)) return rc;
    bool uniform = true;
    for (int b = 1; b < batch && uniform; b++) uniform = model_ids[b] == model_ids[0];
    if (uniform) {
        in.model = model_ids[0];
        return COVAHIP_OK;
    }
    std::vector<uint8_t> ids((size_t)batch + n_frames, 0);
    std::vector<uint8_t> seen((size_t)n_frames, 0);
    std::copy(model_ids, model_ids + batch, ids.begin());
    for (int b = 0; b < batch; b++)
        for (int t = 0; t < BN_T; t++) {
            const int f = table ? table[(size_t)b * BN_T + t] : b * BN_T + t;
            uint8_t &fm = ids[(size_t)batch + f];
            if (seen[f] && fm != model_ids[b]) return COVAHIP_ERR_INVALID_ARG;
            seen[f] = 1;
            fm = model_ids[b];
        }
    if (int rc = ws.models.reserve(ctx, (size_t)m->max_batch * (1 + BN_T))) return rc;
    if (int rc = ws.models.upload(ctx, ids.data(), ids.size(), &in.model_ids)) return rc;
    in.frame_models = in.model_ids + batch;
    in.h_model_ids = model_ids;
    return COVAHIP_OK;
}

// The stacks' area thresholds for the stand-alone bboxcc behind a forward (covahip_blobnet_set_area: the model's own when it has
// one, else the call's), on the device: *d_out.  Null while no model has one: the scalar form runs.  Uploaded like the model ids:
// from a pinned copy, on the lane's stream, and not at all when they equal the resident ones.
static int resolve_areas(covahip_ctx *ctx, covahip_blobnet *m, BnWorkspace &ws, const BnInput &in, int batch, int area_thresh,
                         const int32_t **d_out) {
    *d_out = nullptr;
    if (!m->area_on) return COVAHIP_OK;
    std::vector<int32_t> eff((size_t)batch);
    for (int b = 0; b < batch; b++) {
        const int32_t a = m->post_area[in.h_model_ids ? in.h_model_ids[b] : in.model];
        eff[b] = a >= 1 ? a : area_thresh;
    }
    if (int rc = ws.areas.reserve(ctx, (size_t)m->max_batch)) return rc;
    return ws.areas.upload(ctx, eff.data(), eff.size(), d_out);
}

// BlobNet forward (+ optionally bboxcc) on device pointers, asynchronous on the ctx stream.
static int ensure_pbuf(covahip_ctx *ctx, covahip_blobnet *m, BnWorkspace &ws, int n_frames);
static int filter_dev(covahip_ctx *ctx, BnInput &in, int batch, float *d_logits, uint8_t *d_mask,
                      bool with_cc, int area_thresh, covahip_box *d_boxes, int32_t *d_counts, int max_boxes,
                      const uint8_t *model_ids = nullptr) {
    covahip_blobnet *m = ctx->blobnet;
    if (!m) return COVAHIP_ERR_NOT_LOADED;
    if (batch > m->max_batch) return COVAHIP_ERR_INVALID_ARG;
    if (batch == 0) return COVAHIP_OK;
    if (in.stack) {   // the stacked tensor is batch * T carrier frames (blobnet_mfma.hip)
        int rc = resolve_models(ctx, m, m->ws[ctx->cur_lane], model_ids, batch, nullptr, batch * BN_T, in);
        if (rc) return rc;
        rc = ensure_pbuf(ctx, m, m->ws[ctx->cur_lane], batch * BN_T);
        if (rc) return rc;
    }
    BnCcTail tail{area_thresh, max_boxes, d_boxes, d_counts};
    bool cc_done = false;
    int rc = blobnet_forward_mfma(ctx, m, m->ws[ctx->cur_lane], in, batch, d_logits, d_mask, with_cc ? &tail : nullptr, &cc_done);
    if (rc) return rc;
    // the fused decoder tail normally runs bboxcc itself; the separate kernel is the fallback for
    // geometries whose frame does not fit its LDS plan -- with the stacks' own area thresholds where models have them
    if (with_cc && !cc_done) {
        const int32_t *d_areas = nullptr;
        rc = resolve_areas(ctx, m, m->ws[ctx->cur_lane], in, batch, area_thresh, &d_areas);
        if (rc) return rc;
        rc = covahip_bboxcc_launch(ctx, d_mask, batch, m->H, m->W, area_thresh, d_boxes, d_counts, max_boxes, d_areas);
    }
    return rc;
}

// Carrier-frame input: validates the stack -> frame table on the host (an index outside the frame array would be an
// out-of-bounds read on the GPU) and uploads it.  stack_index == nullptr: one stream in order.  A table equal to the
// one resident in this lane's workspace is not uploaded again.
static int prepare_frames(covahip_ctx *ctx, covahip_blobnet *m, BnWorkspace &ws, const uint8_t *d_frames, int n_frames,
                          const int32_t *stack_index, int batch, BnInput &in, const uint8_t *model_ids = nullptr) {
    if (n_frames < BN_T || n_frames > BN_T * m->max_batch) return COVAHIP_ERR_INVALID_ARG;
    if (!stack_index && batch != n_frames - (BN_T - 1)) return COVAHIP_ERR_INVALID_ARG;
    std::vector<int32_t> table((size_t)batch * BN_T);
    for (int b = 0; b < batch; b++)
        for (int t = 0; t < BN_T; t++) {
            const int32_t f = stack_index ? stack_index[b * BN_T + t] : b + (BN_T - 1) - t;
            if (f < 0 || f >= n_frames) return COVAHIP_ERR_INVALID_ARG;
            table[(size_t)b * BN_T + t] = f;
        }
    // model ids per stack and per frame (a frame shared across models is rejected here, before anything is uploaded or launched)
    if (int rc = resolve_models(ctx, m, ws, model_ids, batch, table.data(), n_frames, in)) return rc;
    // small batches: the table travels in the level-1 kernel's arguments (blobnet_mfma.hip); the device copy below is for
    // larger ones and for the round-1..3 level-1 kernel
    const bool by_value = batch <= BN_KTAB_STACKS && n_frames <= 65535 && bn_level1_on_enc1(ctx, m);
    in.frames = d_frames;
    in.n_frames = n_frames;
    if (by_value) {
        ws.kept_table = std::move(table);
        in.h_index = ws.kept_table.data();
    } else {
        if (n_frames != ws.index_frames) ws.index.invalidate();
        if (int rc = ws.index.reserve(ctx, (size_t)m->max_batch * BN_T)) return rc;
        if (int rc = ws.index.upload(ctx, table.data(), table.size(), &in.index)) return rc;
        ws.index_frames = n_frames;
    }
    return ensure_pbuf(ctx, m, ws, n_frames);
}

// The tensor P of pooled level-0 values, one slice per carrier frame (the stacked entry has batch * T of them).
static int ensure_pbuf(covahip_ctx *ctx, covahip_blobnet *m, BnWorkspace &ws, int n_frames) {
    if (ws.pbuf_frames < (size_t)n_frames) {
        // grown in whole steps; the pad row / column of P (odd grids) is zeroed here and never written
        const size_t want = std::min((size_t)BN_T * m->max_batch, std::max((size_t)n_frames, 2 * ws.pbuf_frames));
        const size_t bytes = want * m->lv[1].H * m->lv[1].W * m->enc_c[1] * sizeof(__half);
        if (ws.pbuf) {
            COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
            COVAHIP_CHECK_HIP(ctx, hipFree(ws.pbuf));
            ws.pbuf = nullptr;
            ws.pbuf_frames = 0;
        }
        COVAHIP_CHECK_HIP(ctx, hipMalloc((void **)&ws.pbuf, bytes));
        COVAHIP_CHECK_HIP(ctx, hipMemsetAsync(ws.pbuf, 0, bytes, ctx->stream));
        ws.pbuf_frames = want;
    }
    return COVAHIP_OK;
}

int covahip_blobnet_forward_dev(covahip_ctx *ctx, const uint8_t *d_stack, int batch, float *d_logits,
                                uint8_t *d_mask, const uint8_t *model_ids) {
    BnInput in;
    in.stack = d_stack;
    return filter_dev(ctx, in, batch, d_logits, d_mask, false, 0, nullptr, nullptr, 0, model_ids);
}

// HBM workspace of one lane: activations stay resident; pad rows/columns are zeroed once here and never written
// afterwards.  (The memsets go to the stream of the caller's choice: ctx->stream.)
static int alloc_workspace(covahip_ctx *ctx, covahip_blobnet *m, BnWorkspace &ws) {
    if (ws.ready) return COVAHIP_OK;
    for (int i = 1; i <= BN_LEVELS; i++) {
        const size_t tt = (i == BN_LEVELS) ? 1 : BN_T;
        const size_t n = (size_t)m->max_batch * tt * m->lv[i].H * m->lv[i].W * m->enc_c[i];
        COVAHIP_CHECK_HIP(ctx, hipMalloc((void **)&ws.act[i], n * sizeof(__half)));
        COVAHIP_CHECK_HIP(ctx, hipMemsetAsync(ws.act[i], 0, n * sizeof(__half), ctx->stream));
    }
    for (int j = 0; j < BN_LEVELS - 1; j++) {
        const BnLevelGeom out = m->lv[BN_LEVELS - 1 - j];
        const size_t n = (size_t)m->max_batch * out.H * out.W * m->dec_co[j];
        COVAHIP_CHECK_HIP(ctx, hipMalloc((void **)&ws.dact[j], n * sizeof(__half)));
    }
    COVAHIP_CHECK_HIP(ctx, hipMalloc((void **)&ws.part, (size_t)m->max_batch * (m->lv[1].H + 1) * (m->lv[1].W + 1) * 4 * sizeof(float)));
    COVAHIP_CHECK_HIP(ctx, hipMalloc((void **)&ws.planes, (size_t)m->max_batch * (2 * ((m->H + 1) / 2) + 2) * 16));
    ws.ready = true;
    return COVAHIP_OK;
}

int covahip_blobnet_grow_lanes(covahip_ctx *ctx, int n_lanes) {
    covahip_blobnet *m = ctx->blobnet;
    if (!m) return COVAHIP_OK;
    for (int k = 0; k < n_lanes && k < COVAHIP_MAX_LANES; k++) {
        const int rc = alloc_workspace(ctx, m, m->ws[k]);
        if (rc) return rc;
    }
    COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return COVAHIP_OK;
}

// Geometry, HBM workspace and prepared weights of a model.  Every limit of the kernels is checked here (a
// planning-only pass of the forward for batch 1 and max_batch), so an unsupported grid fails at load time.
static int build_model(covahip_ctx *ctx, covahip_blobnet *m, const float *const *h_w, int n_models, int h_mb, int w_mb, int max_batch) {
    m->H = h_mb;
    m->W = w_mb;
    m->max_batch = max_batch;
    m->lv[0] = {h_mb, w_mb};
    for (int i = 0; i < BN_LEVELS; i++) m->lv[i + 1] = {(m->lv[i].H + 1) / 2, (m->lv[i].W + 1) / 2};
    for (int j = 0; j < BN_LEVELS; j++) {
        const BnLevelGeom in = m->lv[BN_LEVELS - j], out = m->lv[BN_LEVELS - 1 - j];
        const int ph = 2 * in.H + 2 - out.H, pw = 2 * in.W + 2 - out.W;
        if (ph < 0 || pw < 0) return COVAHIP_ERR_UNSUPPORTED;  // decoder.py zero-pad branch: never at these sizes
        m->dec_cy[j] = ph / 2 + ph % 2;
        m->dec_cx[j] = pw / 2 + pw % 2;
    }
    // algorithmic MACs per frame (conv + convT(full, uncropped as Keras computes it) + tmix + final)
    int64_t macs = 0;
    for (int i = 0; i < BN_LEVELS; i++) {
        macs += (int64_t)BN_T * m->lv[i].H * m->lv[i].W * 9 * m->enc_c[i] * m->enc_c[i + 1];
        macs += (int64_t)m->lv[i + 1].H * m->lv[i + 1].W * m->enc_c[i + 1] * 32;
    }
    for (int j = 0; j < BN_LEVELS; j++) {
        const BnLevelGeom in = m->lv[BN_LEVELS - j];
        macs += (int64_t)in.H * in.W * 16 * m->dec_ci[j] * m->dec_co[j];
    }
    macs += (int64_t)h_mb * w_mb * 16;
    m->macs_per_frame = macs;

    for (int k = 0; k < ctx->n_lanes; k++) {
        const int rc = alloc_workspace(ctx, m, m->ws[k]);
        if (rc) return rc;
    }
    int rc = blobnet_prepare_mfma(ctx, m, h_w, n_models);
    if (rc) return rc;
    m->post_thr.assign(n_models, 0.f);   // per-model post-processing: the defaults
    m->post_keep.assign(n_models, {});
    m->post_area.assign(n_models, 0);
    BnInput plan;   // planning only, both input forms, smallest and largest batch (a set: also the mixed-batch kernels)
    plan.dry = true;
    for (int pass = 0; pass < (n_models > 1 ? 8 : 4) && !rc; pass++) {
        const int b = (pass & 1) ? max_batch : 1;
        plan.n_frames = (pass & 2) ? b + BN_T - 1 : 0;   // both entry points
        plan.mixed = (pass & 4) != 0;
        rc = blobnet_forward_mfma(ctx, m, m->ws[0], plan, b, nullptr, nullptr, nullptr, nullptr);
    }
    return rc;
}

extern "C" {

int covahip_blobnet_load(covahip_ctx *ctx, const void *weights, size_t weights_bytes, int h_mb, int w_mb, int t,
                         int max_batch) {
    if (!ctx || !weights) return COVAHIP_ERR_INVALID_ARG;
    if (t == BN_T && h_mb >= 16 && w_mb >= 16 && h_mb <= 1024 && w_mb <= 1024 && max_batch > 0 && !bn_check_blob(weights, weights_bytes))
        return COVAHIP_ERR_BAD_WEIGHTS;   // a bad blob alone leaves the model loaded before in place
    return covahip_blobnet_load_set(ctx, 1, &weights, &weights_bytes, h_mb, w_mb, t, max_batch);
}

int covahip_blobnet_load_set(covahip_ctx *ctx, int n_models, const void *const *weights, const size_t *weights_bytes, int h_mb,
                             int w_mb, int t, int max_batch) {
    if (!ctx || !weights || !weights_bytes || h_mb <= 0 || w_mb <= 0 || max_batch <= 0) return COVAHIP_ERR_INVALID_ARG;
    if (n_models < 1 || n_models > COVAHIP_MAX_MODELS) return COVAHIP_ERR_INVALID_ARG;
    for (int k = 0; k < n_models; k++)
        if (!weights[k]) return COVAHIP_ERR_INVALID_ARG;
    if (t != BN_T) return COVAHIP_ERR_UNSUPPORTED;
    if (h_mb < 16 || w_mb < 16 || h_mb > 1024 || w_mb > 1024) return COVAHIP_ERR_UNSUPPORTED;
    std::vector<const float *> h_w(n_models);
    bool bad = false;
    for (int k = 0; k < n_models; k++) bad = bad || !(h_w[k] = bn_check_blob(weights[k], weights_bytes[k]));

    COVAHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    covahip_blobnet_destroy(ctx);
    if (bad) return COVAHIP_ERR_BAD_WEIGHTS;   // (whatever the ctx held is gone: the same rule as a failed build below)
    // The model is built on the side and attached to the ctx only when every step succeeded: a failed
    // load leaves the ctx without a model (COVAHIP_ERR_NOT_LOADED afterwards), never with half of one.
    covahip_blobnet *m = new covahip_blobnet();
    int rc = build_model(ctx, m, h_w.data(), n_models, h_mb, w_mb, max_batch);
    if (rc == COVAHIP_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = COVAHIP_ERR_HIP;
    if (rc) {
        hipStreamSynchronize(ctx->stream);
        (void)hipGetLastError();
        free_model(ctx, m);
        return rc;
    }
    ctx->blobnet = m;
    return COVAHIP_OK;
}

int covahip_blobnet_num_models(covahip_ctx *ctx, int *n_models) {
    if (!ctx || !n_models) return COVAHIP_ERR_INVALID_ARG;
    if (!ctx->blobnet) return COVAHIP_ERR_NOT_LOADED;
    *n_models = ctx->blobnet->n_models;
    return COVAHIP_OK;
}

// Per-model post-processing (covahip.h).  The device tables are one allocation, made at the first non-default setting and
// rewritten whole by every later call: the ctx is drained first, so nothing in flight reads them.
//   fp32 threshold [n_models] | i32 area threshold [n_models] | keep bytes u8 [n_models][H][W] |
//   keep planes u32 [n_models][H][E lo, E hi, O lo, O hi]
// A plane holds the even (E) or odd (O) pixels of a row, pixel 2k (2k + 1) at bit k: bboxcc's planes (bboxcc_wave.h), which
// dec3cc_rows_mfma ballots its logits into.  That kernel takes rows of at most 128 pixels; the planes of a wider grid are not read.
static int upload_post(covahip_ctx *ctx, covahip_blobnet *m) {
    const size_t hw = (size_t)m->H * m->W, n = (size_t)m->n_models;
    if (!m->d_post) {
        m->post_keep_stride = (hw + 15) & ~(size_t)15;
        m->post_planes_stride = (size_t)m->H * 16;
        m->post_area_off = n * sizeof(float);
        m->post_keep_off = align256(m->post_area_off + n * sizeof(int32_t));
        m->post_planes_off = align256(m->post_keep_off + n * m->post_keep_stride);
        m->post_bytes = m->post_planes_off + n * m->post_planes_stride;
        COVAHIP_CHECK_HIP(ctx, hipMalloc(&m->d_post, m->post_bytes));
    }
    std::vector<uint8_t> host(m->post_bytes, 0);
    std::memcpy(host.data(), m->post_thr.data(), n * sizeof(float));
    std::memcpy(host.data() + m->post_area_off, m->post_area.data(), n * sizeof(int32_t));
    for (size_t k = 0; k < n; k++) {
        uint8_t *kb = host.data() + m->post_keep_off + k * m->post_keep_stride;
        uint32_t *kp = reinterpret_cast<uint32_t *>(host.data() + m->post_planes_off + k * m->post_planes_stride);
        const std::vector<uint8_t> &keep = m->post_keep[k];
        for (int y = 0; y < m->H; y++)
            for (int x = 0; x < m->W; x++) {
                const bool on = keep.empty() || keep[(size_t)y * m->W + x];
                kb[(size_t)y * m->W + x] = on ? 1 : 0;
                if (on && x < 128) kp[y * 4 + 2 * (x & 1) + (x >> 6)] |= 1u << ((x >> 1) & 31);
            }
    }
    COVAHIP_CHECK_HIP(ctx, hipMemcpy(m->d_post, host.data(), host.size(), hipMemcpyHostToDevice));
    return COVAHIP_OK;
}

// The host settings changed (the ctx is drained): the tables follow, and the forward runs the POST = true kernels while any model
// has a setting that is not the default -- a threshold, a keep map or an area threshold.
static int commit_post(covahip_ctx *ctx, covahip_blobnet *m) {
    bool on = false, area = false;
    for (int k = 0; k < m->n_models; k++) {
        area = area || m->post_area[k] >= 1;
        on = on || m->post_thr[k] != 0.f || !m->post_keep[k].empty() || m->post_area[k] >= 1;
    }
    if (on || m->d_post) {
        if (int rc = upload_post(ctx, m)) {   // (an allocation or a copy failed: the model falls back to the defaults rather than to half a table)
            m->post_thr.assign(m->n_models, 0.f);
            m->post_keep.assign(m->n_models, {});
            m->post_area.assign(m->n_models, 0);
            m->post_on = m->area_on = false;
            return rc;
        }
    }
    m->post_on = on;
    m->area_on = area;
    return COVAHIP_OK;
}

int covahip_blobnet_set_post(covahip_ctx *ctx, int model, const covahip_blobnet_post *post) {
    if (!ctx) return COVAHIP_ERR_INVALID_ARG;
    covahip_blobnet *m = ctx->blobnet;
    if (!m) return COVAHIP_ERR_NOT_LOADED;
    if (model < 0 || model >= m->n_models) return COVAHIP_ERR_INVALID_ARG;
    if (post && !std::isfinite(post->logit_thresh)) return COVAHIP_ERR_INVALID_ARG;
    COVAHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = covahip_sync_all(ctx)) return rc;   // batches in flight keep the settings they were submitted with
    const size_t hw = (size_t)m->H * m->W;
    m->post_thr[model] = post ? post->logit_thresh : 0.f;
    m->post_keep[model].clear();
    if (post && post->keep) {
        m->post_keep[model].resize(hw);
        for (size_t i = 0; i < hw; i++) m->post_keep[model][i] = post->keep[i] ? 1 : 0;
    }
    return commit_post(ctx, m);
}

// Per-model area threshold of bboxcc (covahip.h): the same tables, the same ordering rule, a setting of its own.
int covahip_blobnet_set_area(covahip_ctx *ctx, int model, int area_thresh) {
    if (!ctx) return COVAHIP_ERR_INVALID_ARG;
    covahip_blobnet *m = ctx->blobnet;
    if (!m) return COVAHIP_ERR_NOT_LOADED;
    if (model < 0 || model >= m->n_models || area_thresh < 0) return COVAHIP_ERR_INVALID_ARG;
    COVAHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = covahip_sync_all(ctx)) return rc;   // batches in flight keep the settings they were submitted with
    m->post_area[model] = area_thresh;
    return commit_post(ctx, m);
}

int covahip_blobnet_get_area(covahip_ctx *ctx, int model, int *area_thresh) {
    if (!ctx || !area_thresh) return COVAHIP_ERR_INVALID_ARG;
    covahip_blobnet *m = ctx->blobnet;
    if (!m) return COVAHIP_ERR_NOT_LOADED;
    if (model < 0 || model >= m->n_models) return COVAHIP_ERR_INVALID_ARG;
    *area_thresh = m->post_area[model];
    return COVAHIP_OK;
}

int covahip_blobnet_get_post(covahip_ctx *ctx, int model, float *logit_thresh, uint8_t *keep_or_null, int *has_keep) {
    if (!ctx) return COVAHIP_ERR_INVALID_ARG;
    covahip_blobnet *m = ctx->blobnet;
    if (!m) return COVAHIP_ERR_NOT_LOADED;
    if (model < 0 || model >= m->n_models) return COVAHIP_ERR_INVALID_ARG;
    const std::vector<uint8_t> &keep = m->post_keep[model];
    if (logit_thresh) *logit_thresh = m->post_thr[model];
    if (has_keep) *has_keep = keep.empty() ? 0 : 1;
    if (keep_or_null) {
        const size_t hw = (size_t)m->H * m->W;
        if (keep.empty()) std::memset(keep_or_null, 1, hw);
        else std::memcpy(keep_or_null, keep.data(), hw);
    }
    return COVAHIP_OK;
}

int covahip_blobnet_macs_per_frame(covahip_ctx *ctx, int64_t *macs) {
    if (!ctx || !macs) return COVAHIP_ERR_INVALID_ARG;
    if (!ctx->blobnet) return COVAHIP_ERR_NOT_LOADED;
    *macs = ctx->blobnet->macs_per_frame;
    return COVAHIP_OK;
}

int covahip_blobnet_set_enc_plan(covahip_ctx *ctx, int level, int nbands, int nbuf) {
    if (!ctx || level < 1 || level > 3 || nbands < 0 || nbands > 64 || (nbands && nbuf != 1 && nbuf != 2)) return COVAHIP_ERR_INVALID_ARG;
    ctx->enc_plan[level].nbands = nbands;
    ctx->enc_plan[level].nbuf = nbands ? nbuf : 0;
    return COVAHIP_OK;
}

int covahip_blobnet_set_impl(covahip_ctx *ctx, int impl) {
    if (!ctx || !ctx->blobnet) return COVAHIP_ERR_NOT_LOADED;
    if (impl != 1 && (impl < 4 || impl > 12)) return COVAHIP_ERR_INVALID_ARG;
    ctx->blobnet->fuse_dec = impl != 4;
    ctx->blobnet->enc1_tile16 = impl != 5;
    ctx->blobnet->enc_rowtiles = impl != 6;
    ctx->blobnet->fuse_enc23 = impl == 7 ? 0 : impl == 8 ? 2 : 1;
    ctx->blobnet->tail_part = impl != 9;
    ctx->blobnet->tail_rows = impl != 10;
    ctx->blobnet->tail_in_dec012 = impl == 11 ? 2 : impl == 12 ? 0 : 1;
    return COVAHIP_OK;
}

// The hot path on device pointers, on ctx->stream with the current lane's workspace (the caller has placed the call).
static int filter_placed(covahip_ctx *ctx, covahip_blobnet *m, const uint8_t *d_src, int n_frames, const int32_t *stack_index,
                         int batch, int area_thresh, covahip_box *d_boxes, int32_t *d_counts, int max_boxes, float *d_logits,
                         uint8_t *d_mask, bool packed = false, const uint8_t *model_ids = nullptr) {
    if (!d_mask) {
        CtxLane &l = ctx->lane();
        int rc = covahip_ensure_buffer(ctx, &l.cc_scratch, &l.cc_scratch_bytes, (size_t)batch * m->H * m->W);
        if (rc) return rc;
        d_mask = (uint8_t *)l.cc_scratch;
    }
    BnInput in;
    if (n_frames > 0) {
        int rc = prepare_frames(ctx, m, m->ws[ctx->cur_lane], d_src, n_frames, stack_index, batch, in, model_ids);
        if (rc) return rc;
        in.packed = packed;
    } else {
        in.stack = d_src;
    }
    int rc = filter_dev(ctx, in, batch, d_logits, d_mask, true, area_thresh, d_boxes, d_counts, max_boxes, n_frames > 0 ? nullptr : model_ids);
    // the serving monitor (monitor.hip): the batch's mask, counts and boxes are on the device and this is the stream that wrote them
    if (rc == COVAHIP_OK && batch > 0 && ctx->mon && ctx->mon->attached && !ctx->mon_suspended)
        rc = covahip_monitor_hook(ctx, d_mask, d_counts, d_boxes, max_boxes, model_ids, batch, &in);
    return rc;
}

// Shared body of covahip_filter_forward / covahip_filter_forward_frames: `src` is the stacked tensor (n_frames == 0)
// or the carrier frames.
static int filter_any(covahip_ctx *ctx, const uint8_t *src, int n_frames, const int32_t *stack_index, int batch,
                      int area_thresh, covahip_box *boxes, int32_t *counts, int max_boxes, float *logits, uint8_t *mask,
                      int mem_kind, const uint8_t *model_ids = nullptr) {
    if (!ctx || batch < 0 || max_boxes < 0 || n_frames < 0) return COVAHIP_ERR_INVALID_ARG;
    covahip_blobnet *m = ctx->blobnet;
    if (!m) return COVAHIP_ERR_NOT_LOADED;
    if (batch == 0) return COVAHIP_OK;
    if (!src || !counts || (!boxes && max_boxes > 0) || batch > m->max_batch) return COVAHIP_ERR_INVALID_ARG;
    if (int rc = check_model_ids(m, model_ids, batch)) return rc;
    COVAHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const bool by_frames = n_frames > 0;
    const size_t hw = (size_t)m->H * m->W;
    const size_t in_bytes = by_frames ? (size_t)n_frames * hw * 4 : (size_t)batch * BN_T * hw * 4;
    const size_t mask_bytes = (size_t)batch * hw;
    const size_t logit_bytes = mask_bytes * sizeof(float);
    const size_t box_bytes = (size_t)batch * max_boxes * sizeof(covahip_box);
    const size_t cnt_bytes = (size_t)batch * sizeof(int32_t);
    if (mem_kind != COVAHIP_MEM_DEVICE && mem_kind != COVAHIP_MEM_HOST) return COVAHIP_ERR_INVALID_ARG;

    // device pointers: the call goes to the next lane (internal.h, CtxLane) and overlaps the calls before it; host pointers:
    // synchronous, on the primary stream, behind everything in flight
    if (mem_kind == COVAHIP_MEM_DEVICE) {
        LaneScope lane(ctx);
        if (!lane.ok()) return COVAHIP_ERR_HIP;
        return filter_placed(ctx, m, src, n_frames, stack_index, batch, area_thresh, boxes, counts, max_boxes, logits, mask, false, model_ids);
    }
    if (int rc = covahip_primary_op(ctx)) return rc;
    const uint8_t *d_src = src;
    int rc = covahip_ensure_buffer(ctx, &ctx->stage_in, &ctx->stage_in_bytes, in_bytes);
    if (rc) return rc;
    rc = covahip_ensure_buffer(ctx, &ctx->stage_out, &ctx->stage_out_bytes,
                               align256(mask_bytes) + align256(logit_bytes) + align256(box_bytes) + align256(cnt_bytes));
    if (rc) return rc;
    uint8_t *base = (uint8_t *)ctx->stage_out;
    uint8_t *d_mask = base;
    float *d_logits = logits ? (float *)(base + align256(mask_bytes)) : nullptr;
    covahip_box *d_boxes = (covahip_box *)(base + align256(mask_bytes) + align256(logit_bytes));
    int32_t *d_counts = (int32_t *)(base + align256(mask_bytes) + align256(logit_bytes) + align256(box_bytes));
    COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(ctx->stage_in, src, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    d_src = (const uint8_t *)ctx->stage_in;
    rc = filter_placed(ctx, m, d_src, n_frames, stack_index, batch, area_thresh, d_boxes, d_counts, max_boxes, d_logits, d_mask, false,
                       model_ids);
    if (rc) return rc;
    if (logits) COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(logits, d_logits, logit_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (mask) COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(mask, d_mask, mask_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (box_bytes) COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(boxes, d_boxes, box_bytes, hipMemcpyDeviceToHost, ctx->stream));
    COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(counts, d_counts, cnt_bytes, hipMemcpyDeviceToHost, ctx->stream));
    COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return COVAHIP_OK;
}

int covahip_filter_forward(covahip_ctx *ctx, const uint8_t *rgba_stack, int batch, int area_thresh,
                           covahip_box *boxes, int32_t *counts, int max_boxes, float *logits, uint8_t *mask,
                           int mem_kind) {
    return filter_any(ctx, rgba_stack, 0, nullptr, batch, area_thresh, boxes, counts, max_boxes, logits, mask, mem_kind);
}

int covahip_filter_forward_m(covahip_ctx *ctx, const uint8_t *rgba_stack, const uint8_t *model_ids, int batch, int area_thresh,
                             covahip_box *boxes, int32_t *counts, int max_boxes, float *logits, uint8_t *mask, int mem_kind) {
    return filter_any(ctx, rgba_stack, 0, nullptr, batch, area_thresh, boxes, counts, max_boxes, logits, mask, mem_kind, model_ids);
}

int covahip_filter_forward_frames(covahip_ctx *ctx, const uint8_t *frames, int n_frames, const int32_t *stack_index,
                                  int batch, int area_thresh, covahip_box *boxes, int32_t *counts, int max_boxes,
                                  float *logits, uint8_t *mask, int mem_kind) {
    if (n_frames <= 0) return COVAHIP_ERR_INVALID_ARG;
    return filter_any(ctx, frames, n_frames, stack_index, batch, area_thresh, boxes, counts, max_boxes, logits, mask, mem_kind);
}

int covahip_filter_forward_frames_m(covahip_ctx *ctx, const uint8_t *frames, int n_frames, const int32_t *stack_index,
                                    const uint8_t *model_ids, int batch, int area_thresh, covahip_box *boxes, int32_t *counts,
                                    int max_boxes, float *logits, uint8_t *mask, int mem_kind) {
    if (n_frames <= 0) return COVAHIP_ERR_INVALID_ARG;
    return filter_any(ctx, frames, n_frames, stack_index, batch, area_thresh, boxes, counts, max_boxes, logits, mask, mem_kind,
                      model_ids);
}

int covahip_filter_forward_frames_packed(covahip_ctx *ctx, const uint16_t *d_records, int n_frames, const int32_t *stack_index,
                                         int batch, int area_thresh, covahip_box *d_boxes, int32_t *d_counts, int max_boxes,
                                         float *d_logits, uint8_t *d_mask) {
    return covahip_filter_forward_frames_packed_m(ctx, d_records, n_frames, stack_index, nullptr, batch, area_thresh, d_boxes,
                                                  d_counts, max_boxes, d_logits, d_mask);
}

int covahip_filter_forward_frames_packed_m(covahip_ctx *ctx, const uint16_t *d_records, int n_frames, const int32_t *stack_index,
                                           const uint8_t *model_ids, int batch, int area_thresh, covahip_box *d_boxes,
                                           int32_t *d_counts, int max_boxes, float *d_logits, uint8_t *d_mask) {
    if (!ctx || batch < 0 || max_boxes < 0 || n_frames <= 0) return COVAHIP_ERR_INVALID_ARG;
    covahip_blobnet *m = ctx->blobnet;
    if (!m) return COVAHIP_ERR_NOT_LOADED;
    if (batch == 0) return COVAHIP_OK;
    if (!d_records || !d_counts || (!d_boxes && max_boxes > 0) || batch > m->max_batch) return COVAHIP_ERR_INVALID_ARG;
    if (int rc = check_model_ids(m, model_ids, batch)) return rc;
    COVAHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    LaneScope lane(ctx);
    if (!lane.ok()) return COVAHIP_ERR_HIP;
    return filter_placed(ctx, m, reinterpret_cast<const uint8_t *>(d_records), n_frames, stack_index, batch, area_thresh, d_boxes, d_counts,
                         max_boxes, d_logits, d_mask, true, model_ids);
}

int covahip_dev_blobnet_tail_form(covahip_ctx *ctx, int *form) {
    if (!ctx || !form) return COVAHIP_ERR_INVALID_ARG;
    *form = ctx->tail_form;
    return COVAHIP_OK;
}

int covahip_dev_blobnet_tail_in_dec012(covahip_ctx *ctx, int *in_dec012) {
    if (!ctx || !in_dec012) return COVAHIP_ERR_INVALID_ARG;
    *in_dec012 = ctx->tail_in_dec012;
    return COVAHIP_OK;
}

// Developer read-back (include/covahip_dev.h): one activation buffer of lane 0's workspace, for stage-by-stage tests.
int covahip_dev_blobnet_buffer(covahip_ctx *ctx, int which, int index, void **dptr, size_t *bytes, int32_t dims[5]) {
    if (!ctx || !dptr || !bytes || !dims) return COVAHIP_ERR_INVALID_ARG;
    covahip_blobnet *m = ctx->blobnet;
    if (!m) return COVAHIP_ERR_NOT_LOADED;
    const BnWorkspace &ws = m->ws[0];
    int64_t d[5] = {0, 0, 0, 0, 0};
    size_t elem = sizeof(__half);
    void *p = nullptr;
    if (which == 0 && index == 0) {          // P: [frames][H_1][W_1][16]
        p = ws.pbuf;
        d[0] = (int64_t)ws.pbuf_frames; d[1] = m->lv[1].H; d[2] = m->lv[1].W; d[3] = m->enc_c[1];
    } else if (which == 1 && index >= 1 && index <= BN_LEVELS) {   // act[i]: [B][T][H_i][W_i][C_i], act[4]: [B][H_4][W_4][128]
        p = ws.act[index];
        const BnLevelGeom g = m->lv[index];
        if (index < BN_LEVELS) { d[0] = m->max_batch; d[1] = BN_T; d[2] = g.H; d[3] = g.W; d[4] = m->enc_c[index]; }
        else { d[0] = m->max_batch; d[1] = g.H; d[2] = g.W; d[3] = m->enc_c[index]; }
    } else if (which == 2 && index >= 0 && index < BN_LEVELS - 1) {   // dact[j]: [B][Hd][Wd][Cout_j]
        p = ws.dact[index];
        const BnLevelGeom g = m->lv[BN_LEVELS - 1 - index];
        d[0] = m->max_batch; d[1] = g.H; d[2] = g.W; d[3] = m->dec_co[index];
    } else if (which == 3 && index == 0) {   // part: fp32 [B][H_1 + 1][W_1 + 1][4]
        p = ws.part;
        elem = sizeof(float);
        d[0] = m->max_batch; d[1] = m->lv[1].H + 1; d[2] = m->lv[1].W + 1; d[3] = 4;
    } else {
        return COVAHIP_ERR_INVALID_ARG;
    }
    size_t n = p ? elem : 0;
    for (int k = 0; k < 5; k++) {
        dims[k] = p ? (int32_t)d[k] : 0;
        if (d[k]) n *= (size_t)d[k];
    }
    *dptr = p;
    *bytes = n;
    return COVAHIP_OK;
}

// Developer probe (include/covahip_dev.h): the same carrier-frame step `iters` times as stream launches and as launches of ONE
// captured HIP graph of it -- what the gaps between the six launches of a step cost on their own.
int covahip_dev_graph_probe(covahip_ctx *ctx, const uint8_t *d_frames, int n_frames, const int32_t *stack_index, int batch,
                            int area_thresh, covahip_box *d_boxes, int32_t *d_counts, int max_boxes, uint8_t *d_mask, int iters,
                            float *ms_direct, float *ms_graph) {
    if (!ctx || !ctx->blobnet || !ms_direct || !ms_graph || iters < 1) return COVAHIP_ERR_INVALID_ARG;
    covahip_blobnet *m = ctx->blobnet;
    COVAHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = covahip_primary_op(ctx)) return rc;
    // a captured step must not contain the standalone bboxcc launches: their alternating counter sets are chosen at capture time,
    // a replay would keep adding to ONE set -- the probe is for the fused tail only
    if (!m->fuse_tail) return COVAHIP_ERR_UNSUPPORTED;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    int rc = COVAHIP_OK;
    // every exit goes through `done`: events, graph and exec are destroyed, and a capture that was begun is always ended
    auto hip_ok = [&](hipError_t e, const char *what) {
        if (e == hipSuccess || rc) return e == hipSuccess;
        ctx->last_hip_error = std::string(what) + ": " + hipGetErrorString(e);
        rc = COVAHIP_ERR_HIP;
        return false;
    };
    auto run = [&](int n) {
        for (int i = 0; i < n && !rc; i++)
            rc = filter_placed(ctx, m, d_frames, n_frames, stack_index, batch, area_thresh, d_boxes, d_counts, max_boxes, nullptr, d_mask);
    };
    bool capturing = false;
    const bool was_suspended = ctx->mon_suspended;
    ctx->mon_suspended = true;   // the probe's steps are not served batches, and a counted launch must not be captured
    do {
        if (!hip_ok(hipEventCreate(&e0), "hipEventCreate") || !hip_ok(hipEventCreate(&e1), "hipEventCreate")) break;
        run(3);
        if (rc || !hip_ok(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize")) break;
        if (!hip_ok(hipEventRecord(e0, ctx->stream), "hipEventRecord")) break;
        run(iters);
        if (rc || !hip_ok(hipEventRecord(e1, ctx->stream), "hipEventRecord") || !hip_ok(hipEventSynchronize(e1), "hipEventSynchronize") ||
            !hip_ok(hipEventElapsedTime(ms_direct, e0, e1), "hipEventElapsedTime"))
            break;
        if (!hip_ok(hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeRelaxed), "hipStreamBeginCapture")) break;
        capturing = true;
        run(1);
        capturing = false;
        const hipError_t ee = hipStreamEndCapture(ctx->stream, &graph);   // always: the stream must leave capture mode
        if (rc || !hip_ok(ee, "hipStreamEndCapture")) break;
        if (!hip_ok(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0), "hipGraphInstantiate")) break;
        for (int i = 0; i < 3 && !rc; i++) hip_ok(hipGraphLaunch(exec, ctx->stream), "hipGraphLaunch");
        if (rc || !hip_ok(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize") || !hip_ok(hipEventRecord(e0, ctx->stream), "hipEventRecord")) break;
        for (int i = 0; i < iters && !rc; i++) hip_ok(hipGraphLaunch(exec, ctx->stream), "hipGraphLaunch");
        if (rc || !hip_ok(hipEventRecord(e1, ctx->stream), "hipEventRecord") || !hip_ok(hipEventSynchronize(e1), "hipEventSynchronize")) break;
        hip_ok(hipEventElapsedTime(ms_graph, e0, e1), "hipEventElapsedTime");
    } while (false);
    ctx->mon_suspended = was_suspended;
    if (capturing) (void)hipStreamEndCapture(ctx->stream, &graph);
    if (exec) (void)hipGraphExecDestroy(exec);
    if (graph) (void)hipGraphDestroy(graph);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return rc;
}

int covahip_blobnet_forward(covahip_ctx *ctx, const uint8_t *rgba_stack, int batch, float *logits, uint8_t *mask,
                            int mem_kind) {
    return covahip_blobnet_forward_m(ctx, rgba_stack, nullptr, batch, logits, mask, mem_kind);
}

int covahip_blobnet_forward_m(covahip_ctx *ctx, const uint8_t *rgba_stack, const uint8_t *model_ids, int batch, float *logits,
                              uint8_t *mask, int mem_kind) {
    if (!ctx || batch < 0) return COVAHIP_ERR_INVALID_ARG;
    covahip_blobnet *m = ctx->blobnet;
    if (!m) return COVAHIP_ERR_NOT_LOADED;
    if (batch == 0) return COVAHIP_OK;
    if (!rgba_stack || batch > m->max_batch) return COVAHIP_ERR_INVALID_ARG;
    if (int rc = check_model_ids(m, model_ids, batch)) return rc;
    COVAHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int prc = covahip_primary_op(ctx)) return prc;   // BlobNet alone runs on the primary stream (lane 0's workspace)
    if (mem_kind == COVAHIP_MEM_DEVICE) return covahip_blobnet_forward_dev(ctx, rgba_stack, batch, logits, mask, model_ids);
    if (mem_kind != COVAHIP_MEM_HOST) return COVAHIP_ERR_INVALID_ARG;
    const size_t hw = (size_t)m->H * m->W;
    const size_t in_bytes = (size_t)batch * BN_T * hw * 4;
    const size_t mask_bytes = (size_t)batch * hw;
    const size_t logit_bytes = mask_bytes * sizeof(float);
    int rc = covahip_ensure_buffer(ctx, &ctx->stage_in, &ctx->stage_in_bytes, in_bytes);
    if (rc) return rc;
    rc = covahip_ensure_buffer(ctx, &ctx->stage_out, &ctx->stage_out_bytes, align256(mask_bytes) + align256(logit_bytes));
    if (rc) return rc;
    uint8_t *d_mask = (uint8_t *)ctx->stage_out;
    float *d_logits = (float *)((uint8_t *)ctx->stage_out + align256(mask_bytes));
    COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(ctx->stage_in, rgba_stack, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    rc = covahip_blobnet_forward_dev(ctx, (const uint8_t *)ctx->stage_in, batch, logits ? d_logits : nullptr,
                                     mask ? d_mask : nullptr, model_ids);
    if (rc) return rc;
    if (logits) COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(logits, d_logits, logit_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (mask) COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(mask, d_mask, mask_bytes, hipMemcpyDeviceToHost, ctx->stream));
    COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return COVAHIP_OK;
}

}  // extern "C"
