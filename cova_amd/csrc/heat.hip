// covahip_post_heat_* (include/covahip.h, "Ignore region from heat"): per macroblock, per mask threshold and over all samples of
// a begin ... end bracket, how often the logits fire (logit > thresh[t]), how often the labels do (gt != 0) and how often both.
// covahip_post_sweep's expression without a keep map; integer counts, exact, additive over the add calls.
//
// heat_hist: a workgroup owns a tile of HT_P consecutive macroblocks and a slice of the call's samples; thread p owns
// macroblock p of the tile.  Per sample it loads one logit and one label byte (coalesced across the tile), counts the
// thresholds the logit exceeds (k, thresholds by value in scalar registers) and bumps ONE bin of its own column of an LDS
// histogram hist[k][p]: the bank is p mod 64 whatever k is, so a wave's 64 bumps never conflict and need no atomic.  A bin is
// one 32-bit word, samples in the low half and labelled samples in the high half (a slice has at most HT_SLICE_MAX samples,
// so neither half overflows).  When the slice is done a suffix sum over k turns the column into fire[t] and both[t], and each
// non-zero count goes to the ctx's table with one global atomic.  DESIGN.md section 4 "Ignore region from heat".
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "internal.h"

namespace {

constexpr int HT_MAX_T = 64;
constexpr int HT_P = 256;               // macroblocks per tile = threads per workgroup
constexpr int HT_SLICE_MAX = 32768;     // samples per workgroup: both halves of a bin stay below 2^16
constexpr int HT_LAUNCH_MAX = 1 << 30;  // samples per launch: at most 32,768 slices
constexpr int HT_MIN_SLICE = 8;         // fewer samples than this do not pay for a slice's flush
constexpr size_t HT_STAGE = (size_t)64 << 20;   // host samples are staged in pieces of at most this many bytes

template <int TB> struct HtThresh { float v[TB]; };   // entries past T: +inf, which no logit exceeds

// table: u32 [T fire planes][T both planes][1 label plane], each hw words
template <int TB>
__global__ __launch_bounds__(HT_P) void heat_hist(const float *__restrict__ logits, const uint8_t *__restrict__ gt, int n, int hw,
                                                  int T, int per_slice, HtThresh<TB> th, unsigned int *__restrict__ table) {
    __shared__ unsigned int hist[(TB + 1) * HT_P];
    const int p = threadIdx.x;
#pragma unroll
    for (int k = 0; k <= TB; k++) hist[k * HT_P + p] = 0;   // a thread touches its own column only: no barrier anywhere
    const int mb = blockIdx.x * HT_P + p;
    if (mb >= hw) return;
    const int s0 = blockIdx.y * per_slice, s1 = min(n, s0 + per_slice);
    const float *lp = logits + (size_t)s0 * hw + mb;
    const uint8_t *gp = gt + (size_t)s0 * hw + mb;
    int s = s0;
    for (; s + 4 <= s1; s += 4) {   // four samples' loads in flight
        float x[4];
        unsigned int g[4];
#pragma unroll
        for (int j = 0; j < 4; j++) x[j] = lp[(size_t)j * hw], g[j] = gp[(size_t)j * hw];
        lp += (size_t)4 * hw;
        gp += (size_t)4 * hw;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            int k = 0;
#pragma unroll
            for (int t = 0; t < TB; t++) k += x[j] > th.v[t];   // NaN compares false: background
            hist[k * HT_P + p] += 1u + (g[j] ? 0x10000u : 0u);
        }
    }
    for (; s < s1; s++) {
        const float x = *lp;
        const unsigned int g = *gp;
        lp += hw;
        gp += hw;
        int k = 0;
#pragma unroll
        for (int t = 0; t < TB; t++) k += x > th.v[t];
        hist[k * HT_P + p] += 1u + (g ? 0x10000u : 0u);
    }
    // the thresholds are ascending, so logit > thresh[t] exactly when k > t: fire[t] = sum of the bins above t
    unsigned int run = 0;
    for (int k = T; k >= 1; k--) {
        run += hist[k * HT_P + p];
        const unsigned int fire = run & 0xFFFFu, both = run >> 16;
        if (fire) atomicAdd(table + (size_t)(k - 1) * hw + mb, fire);
        if (both) atomicAdd(table + (size_t)(T + k - 1) * hw + mb, both);
    }
    run += hist[p];
    if (run >> 16) atomicAdd(table + (size_t)2 * T * hw + mb, run >> 16);
}

template <int TB>
void launch(covahip_ctx *ctx, const float *d_logits, const uint8_t *d_gt, int n, int hw, int T, const float *thresh, dim3 grid,
            int per_slice, unsigned int *table) {
    HtThresh<TB> th;
    for (int t = 0; t < TB; t++) th.v[t] = t < T ? thresh[t] : INFINITY;
    hipLaunchKernelGGL(heat_hist<TB>, grid, dim3(HT_P), 0, ctx->stream, d_logits, d_gt, n, hw, T, per_slice, th, table);
}

// one launch over n device-resident samples
int heat_launch(covahip_ctx *ctx, const float *d_logits, const uint8_t *d_gt, int n) {
    const int hw = ctx->heat_h * ctx->heat_w, T = ctx->heat_T;
    const int tiles = (hw + HT_P - 1) / HT_P;
    const int num_cu = std::max(1, ctx->props.multiProcessorCount);
    // slices: enough workgroups for every CU, no slice shorter than HT_MIN_SLICE or longer than HT_SLICE_MAX samples
    int slices = std::min((num_cu + tiles - 1) / tiles, (n + HT_MIN_SLICE - 1) / HT_MIN_SLICE);
    slices = std::max(slices, (n + HT_SLICE_MAX - 1) / HT_SLICE_MAX);
    const int per_slice = (n + slices - 1) / slices;
    slices = (n + per_slice - 1) / per_slice;
    const dim3 grid(tiles, slices);
    unsigned int *table = (unsigned int *)ctx->heat_buf;
    ProfScope ps(ctx, "heat_hist");
    if (T <= 16) launch<16>(ctx, d_logits, d_gt, n, hw, T, ctx->heat_thresh, grid, per_slice, table);
    else if (T <= 32) launch<32>(ctx, d_logits, d_gt, n, hw, T, ctx->heat_thresh, grid, per_slice, table);
    else launch<64>(ctx, d_logits, d_gt, n, hw, T, ctx->heat_thresh, grid, per_slice, table);
    COVAHIP_CHECK_HIP(ctx, hipGetLastError());
    return COVAHIP_OK;
}

}  // namespace

extern "C" int covahip_post_heat_begin(covahip_ctx *ctx, const covahip_heat_cfg *cfg) {
    if (!ctx || !cfg || !cfg->logit_thresh) return COVAHIP_ERR_INVALID_ARG;
    if (cfg->h < 1 || cfg->w < 1 || cfg->n_thresh < 1 || cfg->n_thresh > HT_MAX_T) return COVAHIP_ERR_INVALID_ARG;
    if (!covahip_thresholds_ok(cfg->logit_thresh, cfg->n_thresh)) return COVAHIP_ERR_INVALID_ARG;
    // a launch indexes macroblocks and tiles with 32 bits, and a grid's second dimension is at most 65,535 slices
    if ((int64_t)cfg->h * cfg->w > (int64_t)1 << 24) return COVAHIP_ERR_UNSUPPORTED;

    ctx->heat_open = false;   // a heat that was open is dropped, whatever happens below
    COVAHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int prc = covahip_primary_op(ctx)) return prc;
    const size_t words = ((size_t)2 * cfg->n_thresh + 1) * cfg->h * cfg->w;
    if (int rc = covahip_ensure_buffer(ctx, &ctx->heat_buf, &ctx->heat_bytes, words * sizeof(uint32_t))) return rc;
    COVAHIP_CHECK_HIP(ctx, hipMemsetAsync(ctx->heat_buf, 0, words * sizeof(uint32_t), ctx->stream));
    ctx->heat_h = cfg->h;
    ctx->heat_w = cfg->w;
    ctx->heat_T = cfg->n_thresh;
    std::memcpy(ctx->heat_thresh, cfg->logit_thresh, sizeof(float) * cfg->n_thresh);
    ctx->heat_samples = 0;
    ctx->heat_open = true;
    return COVAHIP_OK;
}

extern "C" int covahip_post_heat_add(covahip_ctx *ctx, const float *logits, const uint8_t *gt, int n, int mem_kind) {
    if (!ctx || !ctx->heat_open) return COVAHIP_ERR_INVALID_ARG;
    if (n < 0 || (n > 0 && (!logits || !gt))) return COVAHIP_ERR_INVALID_ARG;
    if (mem_kind != COVAHIP_MEM_HOST && mem_kind != COVAHIP_MEM_DEVICE) return COVAHIP_ERR_INVALID_ARG;
    if (ctx->heat_samples + n > INT32_MAX) return COVAHIP_ERR_INVALID_ARG;   // the device counters are 32-bit
    if (n == 0) return COVAHIP_OK;

    COVAHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int prc = covahip_primary_op(ctx)) return prc;   // on the primary stream, behind all lanes
    const size_t hw = (size_t)ctx->heat_h * ctx->heat_w;
    if (mem_kind == COVAHIP_MEM_DEVICE) {
        for (int s0 = 0; s0 < n; s0 += HT_LAUNCH_MAX)   // (a launch's slices fit a grid dimension)
            if (int rc = heat_launch(ctx, logits + (size_t)s0 * hw, gt + (size_t)s0 * hw, std::min(HT_LAUNCH_MAX, n - s0))) return rc;
    } else {   // staged in pieces: [logits f32][labels u8]
        const size_t stage = ctx->heat_stage ? ctx->heat_stage : HT_STAGE;
        const int piece = (int)std::min<size_t>((size_t)n, std::max<size_t>(1, stage / (hw * 5)));
        if (int rc = covahip_ensure_buffer(ctx, &ctx->stage_in, &ctx->stage_in_bytes, (size_t)piece * hw * 5)) return rc;
        float *sl = (float *)ctx->stage_in;
        uint8_t *sg = (uint8_t *)ctx->stage_in + (size_t)piece * hw * 4;
        for (int s0 = 0; s0 < n; s0 += piece) {
            const int c = std::min(piece, n - s0);
            COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(sl, logits + (size_t)s0 * hw, (size_t)c * hw * 4, hipMemcpyHostToDevice, ctx->stream));
            COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(sg, gt + (size_t)s0 * hw, (size_t)c * hw, hipMemcpyHostToDevice, ctx->stream));
            if (int rc = heat_launch(ctx, sl, sg, c)) return rc;
        }
    }
    COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the caller's next forward may overwrite the logits
    ctx->heat_samples += n;
    return COVAHIP_OK;
}

extern "C" int covahip_post_heat_end(covahip_ctx *ctx, int64_t *fire, int64_t *both, int64_t *gt_fire, int64_t *samples) {
    if (!ctx || !ctx->heat_open) return COVAHIP_ERR_INVALID_ARG;
    ctx->heat_open = false;
    const size_t hw = (size_t)ctx->heat_h * ctx->heat_w, T = ctx->heat_T;
    if (samples) *samples = ctx->heat_samples;
    if (!fire && !both && !gt_fire) return COVAHIP_OK;
    COVAHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int prc = covahip_primary_op(ctx)) return prc;
    std::vector<uint32_t> host((2 * T + 1) * hw);
    COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(host.data(), ctx->heat_buf, host.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (fire) std::copy(host.begin(), host.begin() + T * hw, fire);
    if (both) std::copy(host.begin() + T * hw, host.begin() + 2 * T * hw, both);
    if (gt_fire) std::copy(host.begin() + 2 * T * hw, host.end(), gt_fire);
    return COVAHIP_OK;
}

extern "C" int covahip_dev_heat_set_stage(covahip_ctx *ctx, size_t bytes) {
    if (!ctx) return COVAHIP_ERR_INVALID_ARG;
    ctx->heat_stage = bytes;
    return COVAHIP_OK;
}
