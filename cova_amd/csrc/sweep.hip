// covahip_post_sweep (include/covahip.h, "Calibration"): score logits against labels at T mask thresholds x A area thresholds
// in one pass -- pixel tp / fp / fn per threshold, and per cell the boxes serving would emit, how many of them hit a labelled
// object and how many labelled objects they find.  Everything is an integer count, so the result is exact.
//
// Per chunk of samples, on the primary stream:
//   1. sweep_masks   reads every logit and label byte once and writes the T masks of each sample plus the scored label mask
//                    as u8 frames ([chunk][T] prediction frames, then [chunk] label frames); pixel counts by ballot + popcount
//                    into LDS counters, one 64-bit atomic per workgroup, threshold and counter at the end;
//   2. covahip_bboxcc_launch twice: the chunk * T prediction frames at area_thresh[0], the chunk label frames at gt_area_thresh;
//   3. sweep_match   one wave per (sample, threshold): the hit rule between the frame's boxes and the sample's label boxes, per
//                    area threshold a ballot count and one atomic per cell.
// DESIGN.md section 4 "Calibration" has the rules, the chunk budget and the cost.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "internal.h"

namespace {

constexpr int SW_MAX_T = 64, SW_MAX_A = 16;
constexpr int SW_THREADS = 256;
// Scratch of one chunk (mask frames, their boxes and counts) stays within this budget; see DESIGN.md.
constexpr size_t SW_BUDGET = (size_t)128 << 20;

// device accumulators, i64 each, zeroed per call and summed over the call's chunks
enum { ACC_MASK = 0, ACC_TP = SW_MAX_T, ACC_TRUNC = 2 * SW_MAX_T, ACC_GT_PX = 3 * SW_MAX_T, ACC_GT_OBJ, ACC_GT_TRUNC,
       ACC_CELLS = 3 * SW_MAX_T + 4, ACC_WORDS = ACC_CELLS + SW_MAX_T * SW_MAX_A * 3 };

struct SwThresh { float v[SW_MAX_T]; };
struct SwAreas  { int32_t v[SW_MAX_A]; };   // entries past n_area: INT_MAX (no box reaches it)

__device__ __forceinline__ void add64(unsigned long long *p, unsigned long long v) {
    if (v) atomicAdd(p, v);
}

// One item = V consecutive macroblocks of one sample (V divides h * w, so an item never straddles two samples).
// pred: [n_samples][T][hw], gtm: [n_samples][hw].  keep may be nullptr.
template <int V>
__global__ __launch_bounds__(SW_THREADS) void sweep_masks(const float *__restrict__ logits, const uint8_t *__restrict__ gt,
                                                          const uint8_t *__restrict__ keep, int n_items, int hw, int T,
                                                          SwThresh th, uint8_t *__restrict__ pred, uint8_t *__restrict__ gtm,
                                                          unsigned long long *__restrict__ acc) {
    __shared__ unsigned int cnt[2 * SW_MAX_T + 1];   // [t]: |mask_t|, [T_MAX + t]: |mask_t & gt'|, [2 T_MAX]: |gt'|
    for (int i = threadIdx.x; i < 2 * SW_MAX_T + 1; i += SW_THREADS) cnt[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (int base = blockIdx.x * SW_THREADS; base < n_items; base += gridDim.x * SW_THREADS) {   // (uniform per workgroup)
        const int item = base + threadIdx.x;
        const bool valid = item < n_items;
        float x[V];
        bool g[V], k[V];
        size_t s = 0, p = 0;
        if (valid) {
            const size_t px = (size_t)item * V;
            s = px / hw;
            p = px - s * hw;
            if constexpr (V == 4) {
                const float4 q = *reinterpret_cast<const float4 *>(logits + px);
                const uint32_t gb = *reinterpret_cast<const uint32_t *>(gt + px);
                const uint32_t kb = keep ? *reinterpret_cast<const uint32_t *>(keep + p) : 0x01010101u;
                x[0] = q.x, x[1] = q.y, x[2] = q.z, x[3] = q.w;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    k[j] = ((kb >> (8 * j)) & 0xFF) != 0;
                    g[j] = ((gb >> (8 * j)) & 0xFF) != 0 && k[j];
                }
            } else {
                x[0] = logits[px];
                k[0] = keep ? keep[p] != 0 : true;
                g[0] = gt[px] != 0 && k[0];
            }
        } else {
#pragma unroll
            for (int j = 0; j < V; j++) x[j] = 0.f, g[j] = false, k[j] = false;   // k false: no mask bit, no count
        }
        // the scored label mask and its pixel count
        unsigned int ng = 0;
#pragma unroll
        for (int j = 0; j < V; j++) ng += __popcll(__ballot(g[j]));
        if (lane == 0 && ng) atomicAdd(&cnt[2 * SW_MAX_T], ng);
        if (valid) {
            if constexpr (V == 4)
                *reinterpret_cast<uint32_t *>(gtm + s * hw + p) = (uint32_t)g[0] | (uint32_t)g[1] << 8 | (uint32_t)g[2] << 16 | (uint32_t)g[3] << 24;
            else
                gtm[s * hw + p] = g[0];
        }
        uint8_t *const out = pred + (s * T) * hw + p;
        for (int t = 0; t < T; t++) {
            const float thr = th.v[t];
            bool m[V];
            unsigned int nm = 0, ntp = 0;
#pragma unroll
            for (int j = 0; j < V; j++) {
                m[j] = x[j] > thr && k[j];   // NaN compares false: background
                nm += __popcll(__ballot(m[j]));
                ntp += __popcll(__ballot(m[j] && g[j]));
            }
            if (lane == 0) {
                if (nm) atomicAdd(&cnt[t], nm);
                if (ntp) atomicAdd(&cnt[SW_MAX_T + t], ntp);
            }
            if (valid) {
                if constexpr (V == 4)
                    *reinterpret_cast<uint32_t *>(out + (size_t)t * hw) = (uint32_t)m[0] | (uint32_t)m[1] << 8 | (uint32_t)m[2] << 16 | (uint32_t)m[3] << 24;
                else
                    out[(size_t)t * hw] = m[0];
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * SW_MAX_T + 1; i += SW_THREADS) {
        const int t = i & (SW_MAX_T - 1);
        if (i == 2 * SW_MAX_T) add64(acc + ACC_GT_PX, cnt[i]);
        else if (t < T) add64(acc + (i < SW_MAX_T ? ACC_MASK : ACC_TP) + t, cnt[i]);
    }
}

__device__ __forceinline__ bool boxes_hit(const covahip_box &p, const covahip_box &g, long long num, long long den) {
    const int iw = min(p.left + p.width, g.left + g.width) - max(p.left, g.left);
    const int ih = min(p.top + p.height, g.top + g.height) - max(p.top, g.top);
    if (iw <= 0 || ih <= 0) return false;
    const long long inter = (long long)iw * ih;
    const long long uni = (long long)p.width * p.height + (long long)g.width * g.height - inter;
    return inter * den >= num * uni;
}

// One wave per prediction frame f = sample * T + t.  pboxes [n_frames][max_boxes], pcounts [n_frames]: regionprops at
// area_thresh[0]; gboxes [n_samples][max_boxes], gcounts [n_samples]: the label objects.  Counts above max_boxes are clamped.
constexpr int SM_WAVES = 4;
__global__ __launch_bounds__(SM_WAVES * 64) void sweep_match(const covahip_box *__restrict__ pboxes, const int32_t *__restrict__ pcounts,
                                                             const covahip_box *__restrict__ gboxes, const int32_t *__restrict__ gcounts,
                                                             int n_frames, int T, int A, SwAreas ar, int max_boxes, int iou_num,
                                                             int iou_den, unsigned long long *__restrict__ acc) {
    const int lane = threadIdx.x & 63;
    const int f = blockIdx.x * SM_WAVES + (threadIdx.x >> 6);
    if (f >= n_frames) return;   // (whole waves leave: no barrier in this kernel)
    const int s = f / T, t = f - s * T;
    const int pc = pcounts[f], gc = gcounts[s];
    const int np = min(pc, max_boxes), ng = min(gc, max_boxes);
    const covahip_box *const P = pboxes + (size_t)f * max_boxes, *const G = gboxes + (size_t)s * max_boxes;
    if (lane == 0) {
        if (pc > max_boxes) atomicAdd(acc + ACC_TRUNC + t, 1ull);
        if (t == 0) {   // the sample's label side, once
            add64(acc + ACC_GT_OBJ, (unsigned long long)ng);
            if (gc > max_boxes) atomicAdd(acc + ACC_GT_TRUNC, 1ull);
        }
    }
    const long long num = iou_num, den = iou_den;
    unsigned int n_pred[SW_MAX_A], n_true[SW_MAX_A], n_found[SW_MAX_A];   // wave-uniform
#pragma unroll
    for (int a = 0; a < SW_MAX_A; a++) n_pred[a] = n_true[a] = n_found[a] = 0;
    // lanes stride over the predictions: does p hit any label box?  (does not depend on the area threshold)
    for (int b = 0; b < np; b += 64) {
        const int i = b + lane;
        bool hit = false;
        int area = -1;
        if (i < np) {
            const covahip_box p = P[i];
            area = p.area_px;
            for (int j = 0; j < ng && !hit; j++) hit = boxes_hit(p, G[j], num, den);
        }
        const unsigned long long hm = __ballot(hit);
#pragma unroll
        for (int a = 0; a < SW_MAX_A; a++) {
            const unsigned long long in = __ballot(area >= ar.v[a]);
            n_pred[a] += __popcll(in);
            n_true[a] += __popcll(in & hm);
        }
    }
    // lanes stride over the label boxes: the largest area_px among the predictions that hit g decides up to which area
    // threshold g is found (P[t][a] is P[t][0] with the boxes of area_px < area_thresh[a] dropped)
    for (int b = 0; b < ng; b += 64) {
        const int j = b + lane;
        int best = -1;
        if (j < ng) {
            const covahip_box g = G[j];
            for (int i = 0; i < np; i++) {
                const covahip_box p = P[i];
                if (p.area_px > best && boxes_hit(p, g, num, den)) best = p.area_px;
            }
        }
#pragma unroll
        for (int a = 0; a < SW_MAX_A; a++) n_found[a] += __popcll(__ballot(best >= ar.v[a]));
    }
    unsigned int v0 = 0, v1 = 0, v2 = 0;
#pragma unroll
    for (int a = 0; a < SW_MAX_A; a++)
        if (lane == a) v0 = n_pred[a], v1 = n_true[a], v2 = n_found[a];
    if (lane < A) {
        unsigned long long *cell = acc + ACC_CELLS + ((size_t)t * SW_MAX_A + lane) * 3;
        add64(cell + 0, v0);
        add64(cell + 1, v1);
        add64(cell + 2, v2);
    }
}


}  // namespace

extern "C" int covahip_post_sweep(covahip_ctx *ctx, const covahip_sweep_cfg *cfg, const float *logits, const uint8_t *gt, int n,
                                  int mem_kind, int64_t *pixel, covahip_sweep_cell *cells, int64_t *truncated,
                                  covahip_sweep_result *out) {
    // ---- every argument check, on the host, before the ctx or the GPU is touched
    if (!ctx || !cfg || !pixel || !cells || !truncated || !out) return COVAHIP_ERR_INVALID_ARG;
    if (n < 0 || (n > 0 && (!logits || !gt))) return COVAHIP_ERR_INVALID_ARG;
    if (mem_kind != COVAHIP_MEM_HOST && mem_kind != COVAHIP_MEM_DEVICE) return COVAHIP_ERR_INVALID_ARG;
    if (cfg->h <= 0 || cfg->w <= 0) return COVAHIP_ERR_INVALID_ARG;
    if (cfg->n_thresh < 1 || cfg->n_thresh > SW_MAX_T || !cfg->logit_thresh) return COVAHIP_ERR_INVALID_ARG;
    if (cfg->n_area < 1 || cfg->n_area > SW_MAX_A || !cfg->area_thresh) return COVAHIP_ERR_INVALID_ARG;
    if (!covahip_thresholds_ok(cfg->logit_thresh, cfg->n_thresh)) return COVAHIP_ERR_INVALID_ARG;
    for (int a = 0; a < cfg->n_area; a++)
        if (cfg->area_thresh[a] < 1 || (a && cfg->area_thresh[a] <= cfg->area_thresh[a - 1])) return COVAHIP_ERR_INVALID_ARG;
    if (cfg->gt_area_thresh < 1 || cfg->iou_num < 1 || cfg->iou_num > cfg->iou_den) return COVAHIP_ERR_INVALID_ARG;
    if (cfg->max_boxes < 1 || cfg->max_boxes > 1024 || cfg->chunk < 0) return COVAHIP_ERR_INVALID_ARG;
    // covahip_bboxcc's limit; the height bound keeps one sample's frames within 32-bit item counts
    if (cfg->w > 256 || cfg->h > 16384) return COVAHIP_ERR_UNSUPPORTED;

    const int T = cfg->n_thresh, A = cfg->n_area, max_boxes = cfg->max_boxes;
    const size_t hw = (size_t)cfg->h * cfg->w;
    std::memset(pixel, 0, sizeof(int64_t) * 3 * T);
    std::memset(cells, 0, sizeof(covahip_sweep_cell) * (size_t)T * A);
    std::memset(truncated, 0, sizeof(int64_t) * T);
    std::memset(out, 0, sizeof(*out));
    if (n == 0) return COVAHIP_OK;

    // ---- chunk: the library's choice keeps one chunk's scratch within SW_BUDGET (at least one sample)
    const size_t per_sample = (size_t)(T + 1) * (hw + (size_t)max_boxes * sizeof(covahip_box) + sizeof(int32_t));
    int chunk = cfg->chunk > 0 ? cfg->chunk : (int)std::max<size_t>(1, SW_BUDGET / per_sample);
    chunk = std::min(chunk, n);
    // prediction frames of a chunk are indexed with 32 bits (frame count, item count)
    chunk = (int)std::min<size_t>((size_t)chunk, std::max<size_t>(1, (size_t)INT_MAX / ((size_t)(T + 1) * hw)));

    COVAHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int prc = covahip_primary_op(ctx)) return prc;   // on the primary stream, behind all lanes

    // scratch: [accumulators][keep map][prediction frames][label frames][prediction boxes][label boxes][counts]
    const size_t off_keep = align256(ACC_WORDS * sizeof(uint64_t));
    const size_t off_pred = off_keep + align256(hw);
    const size_t off_gtm = off_pred + align256((size_t)chunk * T * hw);
    const size_t off_pbox = off_gtm + align256((size_t)chunk * hw);
    const size_t off_gbox = off_pbox + align256((size_t)chunk * T * max_boxes * sizeof(covahip_box));
    const size_t off_pcnt = off_gbox + align256((size_t)chunk * max_boxes * sizeof(covahip_box));
    const size_t off_gcnt = off_pcnt + align256((size_t)chunk * T * sizeof(int32_t));
    const size_t total = off_gcnt + align256((size_t)chunk * sizeof(int32_t));
    int rc = covahip_ensure_buffer(ctx, &ctx->sweep_buf, &ctx->sweep_bytes, total);
    if (rc) return rc;
    uint8_t *const base = (uint8_t *)ctx->sweep_buf;
    unsigned long long *const d_acc = (unsigned long long *)base;
    uint8_t *const d_keep = cfg->keep ? base + off_keep : nullptr;
    uint8_t *const d_pred = base + off_pred, *const d_gtm = base + off_gtm;
    covahip_box *const d_pbox = (covahip_box *)(base + off_pbox), *const d_gbox = (covahip_box *)(base + off_gbox);
    int32_t *const d_pcnt = (int32_t *)(base + off_pcnt), *const d_gcnt = (int32_t *)(base + off_gcnt);

    COVAHIP_CHECK_HIP(ctx, hipMemsetAsync(d_acc, 0, ACC_WORDS * sizeof(uint64_t), ctx->stream));
    if (d_keep) COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(d_keep, cfg->keep, hw, hipMemcpyHostToDevice, ctx->stream));

    const float *d_logits = logits;
    const uint8_t *d_gt = gt;
    if (mem_kind == COVAHIP_MEM_HOST) {   // a chunk's inputs are staged: [logits f32][labels u8]
        rc = covahip_ensure_buffer(ctx, &ctx->stage_in, &ctx->stage_in_bytes, (size_t)chunk * hw * 5);
        if (rc) return rc;
    }
    SwThresh th;
    SwAreas ar;
    for (int t = 0; t < SW_MAX_T; t++) th.v[t] = t < T ? cfg->logit_thresh[t] : 0.f;
    for (int a = 0; a < SW_MAX_A; a++) ar.v[a] = a < A ? cfg->area_thresh[a] : INT_MAX;
    const int num_cu = std::max(1, ctx->props.multiProcessorCount);

    for (int s0 = 0; s0 < n; s0 += chunk) {
        const int c = std::min(chunk, n - s0);
        if (mem_kind == COVAHIP_MEM_HOST) {
            float *sl = (float *)ctx->stage_in;
            uint8_t *sg = (uint8_t *)ctx->stage_in + (size_t)chunk * hw * 4;
            COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(sl, logits + (size_t)s0 * hw, (size_t)c * hw * 4, hipMemcpyHostToDevice, ctx->stream));
            COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(sg, gt + (size_t)s0 * hw, (size_t)c * hw, hipMemcpyHostToDevice, ctx->stream));
            d_logits = sl;
            d_gt = sg;
        } else {
            d_logits = logits + (size_t)s0 * hw;
            d_gt = gt + (size_t)s0 * hw;
        }
        // four macroblocks per work item where every frame and pointer is aligned for it, else one
        const bool vec = (hw & 3) == 0 && (reinterpret_cast<uintptr_t>(d_logits) & 15) == 0 && (reinterpret_cast<uintptr_t>(d_gt) & 3) == 0;
        const int n_items = (int)((size_t)c * hw / (vec ? 4 : 1));
        const int grid = std::min((n_items + SW_THREADS - 1) / SW_THREADS, 8 * num_cu);
        {
            ProfScope ps(ctx, "sweep_masks");
            if (vec)
                hipLaunchKernelGGL(sweep_masks<4>, dim3(grid), dim3(SW_THREADS), 0, ctx->stream, d_logits, d_gt, (const uint8_t *)d_keep,
                                   n_items, (int)hw, T, th, d_pred, d_gtm, d_acc);
            else
                hipLaunchKernelGGL(sweep_masks<1>, dim3(grid), dim3(SW_THREADS), 0, ctx->stream, d_logits, d_gt, (const uint8_t *)d_keep,
                                   n_items, (int)hw, T, th, d_pred, d_gtm, d_acc);
            COVAHIP_CHECK_HIP(ctx, hipGetLastError());
        }
        rc = covahip_bboxcc_launch(ctx, d_pred, c * T, cfg->h, cfg->w, cfg->area_thresh[0], d_pbox, d_pcnt, max_boxes);
        if (rc) return rc;
        rc = covahip_bboxcc_launch(ctx, d_gtm, c, cfg->h, cfg->w, cfg->gt_area_thresh, d_gbox, d_gcnt, max_boxes);
        if (rc) return rc;
        {
            ProfScope ps(ctx, "sweep_match");
            hipLaunchKernelGGL(sweep_match, dim3((c * T + SM_WAVES - 1) / SM_WAVES), dim3(SM_WAVES * 64), 0, ctx->stream,
                               (const covahip_box *)d_pbox, (const int32_t *)d_pcnt, (const covahip_box *)d_gbox,
                               (const int32_t *)d_gcnt, c * T, T, A, ar, max_boxes, cfg->iou_num, cfg->iou_den, d_acc);
            COVAHIP_CHECK_HIP(ctx, hipGetLastError());
        }
    }
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "accumulators are 64-bit");
    int64_t *h_acc = new int64_t[ACC_WORDS];
    hipError_t e = hipMemcpyAsync(h_acc, d_acc, ACC_WORDS * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        delete[] h_acc;
        ctx->last_hip_error = std::string("covahip_post_sweep: ") + hipGetErrorString(e);
        return COVAHIP_ERR_HIP;
    }
    for (int t = 0; t < T; t++) {
        const int64_t tp = h_acc[ACC_TP + t];
        pixel[3 * t + 0] = tp;
        pixel[3 * t + 1] = h_acc[ACC_MASK + t] - tp;
        pixel[3 * t + 2] = h_acc[ACC_GT_PX] - tp;
        truncated[t] = h_acc[ACC_TRUNC + t];
        for (int a = 0; a < A; a++) {
            const int64_t *cell = h_acc + ACC_CELLS + ((size_t)t * SW_MAX_A + a) * 3;
            cells[(size_t)t * A + a] = covahip_sweep_cell{cell[0], cell[1], cell[2]};
        }
    }
    out->samples = n;
    out->gt_objects = h_acc[ACC_GT_OBJ];
    out->gt_truncated = h_acc[ACC_GT_TRUNC];
    delete[] h_acc;
    return COVAHIP_OK;
}
