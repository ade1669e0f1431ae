// covahip_monitor_* (include/covahip.h, "Serving monitor"): per model of a set, how often each macroblock of the served mask fires,
// how many boxes a frame emits and how large they are.  Integer counts, exact, additive over batches, 64-bit on the device.
//
// monitor_count, one launch per counted batch on the stream that ran the batch.  The host groups the batch's samples by model
// (a stable counting sort of the host model ids) and cuts every model's segment into slices; the order and the slices reach the
// kernel by value (batches of at most MON_KTAB samples), from a per-lane device table (larger ones), or not at all (a batch of
// one model: the slices are ranges of the call's own order).
//   * mask workgroups, one wave each, own (a tile of MON_TILE consecutive macroblocks, one slice): lane l loads macroblocks
//     4 l .. 4 l + 3 of the tile as ONE 32-bit word per sample, normalises the bytes to 0 / 1 and adds the word to a register
//     whose four byte lanes are four counters; every 255 samples the byte lanes spill into four 32-bit counters.  At the end of
//     the slice the 4 x 64 counts go through LDS so that lane l holds macroblocks l, l + 64, l + 128, l + 192, and every
//     wave-level 64-bit atomic covers contiguous bytes of fire[model].  A mask pointer that is not 4-byte aligned, or a grid of
//     h * w % 4 != 0, takes the byte form (WORDS = false): lane l loads macroblocks l + 64 j directly.
//   * box workgroups, one per slice, behind them in the same grid: 64 samples at a time, lane l reads counts[] of its sample;
//     a wave scan of min(count, max_boxes) numbers the written boxes of the 64 frames, the lanes stride over them and bump a
//     16-bin LDS histogram of floor(log2(area_px)); then at most 16 + 4 global atomics.
// DESIGN.md section 4 "Serving monitor".
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "blobnet.h"
#include "covahip_dev.h"
#include "internal.h"
#include "monitor_tab.h"

namespace {

constexpr int MON_TILE = 256;            // macroblocks per mask workgroup: 64 lanes x 4 bytes
constexpr int MON_MIN_SLICE = 16;        // fewer samples than this do not pay for a slice's flush
constexpr int MON_CHUNK = 16384;         // samples per launch of a stand-alone add
constexpr int MON_SPILL = 255;           // samples a packed byte lane takes
constexpr size_t MON_STAGE = (size_t)64 << 20;   // host samples are staged in pieces of at most this many bytes
constexpr int MON_BINS = COVAHIP_MONITOR_AREA_BINS;

// every non-zero byte of v -> 1 (bit 0 of a byte ends up as the OR of its eight bits; what the shifts drag in from the byte above
// never reaches bit 0)
__device__ inline uint32_t mon_norm(uint32_t v) {
    v |= v >> 4;
    v |= v >> 2;
    v |= v >> 1;
    return v & 0x01010101u;
}

// tab: the monitor's counters (CovahipMonitor::d_tab); M models, hw macroblocks, tiles = ceil(hw / MON_TILE), S slices
template <bool WORDS, class TAB>
__global__ __launch_bounds__(64) void monitor_count(const uint8_t *__restrict__ mask, const int32_t *__restrict__ counts,
                                                    const covahip_box *__restrict__ boxes, int n, int hw, int max_boxes, int M,
                                                    int tiles, int S, TAB t, unsigned long long *__restrict__ tab) {
    __shared__ uint32_t lds[MON_TILE];
    __shared__ long long pre[65];
    __shared__ int smp[64];
    const int lane = threadIdx.x;
    const int nmask = tiles * S;
    if ((int)blockIdx.x < nmask) {
        const int tile = blockIdx.x % tiles, s = blockIdx.x / tiles;
        int m, i0, i1;
        mon_slice(t, s, S, n, m, i0, i1);
        unsigned long long *fire = tab + (size_t)M * (4 + MON_BINS) + (size_t)m * hw;
        const int mb0 = tile * MON_TILE;
        uint32_t wide[4] = {0, 0, 0, 0};
        if (WORDS) {
            const int hw4 = hw >> 2, w0 = tile * (MON_TILE / 4) + lane;
            const bool valid = w0 < hw4;
            const uint32_t *mw = reinterpret_cast<const uint32_t *>(mask) + (valid ? w0 : 0);
            for (int c0 = i0; c0 < i1; c0 += MON_SPILL) {   // no byte lane passes 255 within a block
                const int c1 = min(i1, c0 + MON_SPILL);
                uint32_t p = 0;
                int i = c0;
                for (; i + 8 <= c1; i += 8) {   // eight samples' loads in flight
                    uint32_t v[8];
#pragma unroll
                    for (int j = 0; j < 8; j++) v[j] = valid ? mw[(size_t)mon_sample(t, S, i + j) * hw4] : 0u;
#pragma unroll
                    for (int j = 0; j < 8; j++) p += mon_norm(v[j]);
                }
                for (; i < c1; i++) p += mon_norm(valid ? mw[(size_t)mon_sample(t, S, i) * hw4] : 0u);
#pragma unroll
                for (int k = 0; k < 4; k++) wide[k] += (p >> (8 * k)) & 0xFFu;
            }
            // lane l holds macroblocks 4 l + k; through LDS to macroblocks l + 64 j, so that a wave's atomic is contiguous
#pragma unroll
            for (int k = 0; k < 4; k++) lds[4 * lane + k] = wide[k];
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 4; j++) wide[j] = lds[lane + 64 * j];
        } else {
            bool valid[4];
            const uint8_t *mp[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                valid[j] = mb0 + lane + 64 * j < hw;
                mp[j] = mask + (valid[j] ? mb0 + lane + 64 * j : 0);
            }
            for (int i = i0; i < i1; i++) {
                const size_t off = (size_t)mon_sample(t, S, i) * hw;
#pragma unroll
                for (int j = 0; j < 4; j++) wide[j] += valid[j] && mp[j][off] != 0;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int mb = mb0 + lane + 64 * j;
            if (mb < hw && wide[j]) atomicAdd(fire + mb, (unsigned long long)wide[j]);
        }
        return;
    }
    // ---- box statistics of slice s
    const int s = blockIdx.x - nmask;
    int m, i0, i1;
    mon_slice(t, s, S, n, m, i0, i1);
    if (lane < MON_BINS) lds[lane] = 0;
    __syncthreads();
    long long nbox = 0;
    int with = 0, trunc = 0;
    for (int base = i0; base < i1; base += 64) {
        const int i = base + lane;
        int b = 0, c = 0;
        if (i < i1) {
            b = mon_sample(t, S, i);
            c = counts[b];
            nbox += c;
            with += c > 0;
            trunc += c > max_boxes;
        }
        long long x = max(0, min(c, max_boxes));   // the boxes of this lane's frame that were written
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long y = __shfl_up(x, o, 64);
            if (lane >= o) x += y;
        }
        pre[lane + 1] = x;
        if (lane == 0) pre[0] = 0;
        smp[lane] = b;
        __syncthreads();
        const long long total = pre[64];
        for (long long q = lane; q < total; q += 64) {
            int lo = 0, hi = 63;   // the frame of box q: the last lane whose boxes start at or before q
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (pre[mid] <= q) lo = mid;
                else hi = mid - 1;
            }
            const int a = boxes[(size_t)smp[lo] * max_boxes + (size_t)(q - pre[lo])].area_px;
            const int bin = a < 2 ? 0 : min(MON_BINS - 1, 31 - __clz(a));
            atomicAdd(&lds[bin], 1u);
        }
        __syncthreads();
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        nbox += __shfl_xor(nbox, o, 64);
        with += __shfl_xor(with, o, 64);
        trunc += __shfl_xor(trunc, o, 64);
    }
    if (lane == 0) {
        if (i1 > i0) atomicAdd(tab + m, (unsigned long long)(i1 - i0));
        if (nbox) atomicAdd(tab + M + m, (unsigned long long)nbox);
        if (with) atomicAdd(tab + 2 * (size_t)M + m, (unsigned long long)with);
        if (trunc) atomicAdd(tab + 3 * (size_t)M + m, (unsigned long long)trunc);
    }
    if (lane < MON_BINS && lds[lane]) atomicAdd(tab + 4 * (size_t)M + (size_t)m * MON_BINS + lane, (unsigned long long)lds[lane]);
}

template <class TAB>
void launch(covahip_ctx *ctx, const CovahipMonitor *mon, bool words, const uint8_t *d_mask, const int32_t *d_counts,
            const covahip_box *d_boxes, int n, int max_boxes, int tiles, int S, const TAB &t) {
    const int hw = mon->h * mon->w;
    const dim3 grid((unsigned)(tiles * S + S));
    if (words)
        hipLaunchKernelGGL((monitor_count<true, TAB>), grid, dim3(64), 0, ctx->stream, d_mask, d_counts, d_boxes, n, hw, max_boxes,
                           mon->n_models, tiles, S, t, mon->d_tab);
    else
        hipLaunchKernelGGL((monitor_count<false, TAB>), grid, dim3(64), 0, ctx->stream, d_mask, d_counts, d_boxes, n, hw, max_boxes,
                           mon->n_models, tiles, S, t, mon->d_tab);
}

// One launch over n device-resident samples on ctx->stream, by the batch's plan.
int count_batch(covahip_ctx *ctx, CovahipMonitor *mon, const MonPlan &plan, const uint8_t *d_mask, const int32_t *d_counts,
                const covahip_box *d_boxes, int max_boxes, int n) {
    const int hw = mon->h * mon->w;
    const int tiles = (hw + MON_TILE - 1) / MON_TILE;
    const bool words = hw % 4 == 0 && (reinterpret_cast<uintptr_t>(d_mask) & 3) == 0;
    ProfScope ps(ctx, "monitor_count");
    if (plan.kind == MonPlan::UNIFORM) launch(ctx, mon, words, d_mask, d_counts, d_boxes, n, max_boxes, tiles, plan.S, plan.u);
    else if (plan.kind == MonPlan::BY_VALUE) launch(ctx, mon, words, d_mask, d_counts, d_boxes, n, max_boxes, tiles, plan.S, plan.v);
    else launch(ctx, mon, words, d_mask, d_counts, d_boxes, n, max_boxes, tiles, plan.S, plan.p);
    COVAHIP_CHECK_HIP(ctx, hipGetLastError());
    return COVAHIP_OK;
}

int mon_tiles(const CovahipMonitor *mon) { return (mon->h * mon->w + MON_TILE - 1) / MON_TILE; }

void free_monitor(CovahipMonitor *mon) {
    if (!mon) return;
    if (mon->d_tab) hipFree(mon->d_tab);
    covahip_monitor_free_inputs(mon);
    for (MonTable &tb : mon->lane) tb.release();
    delete mon;
}

}  // namespace

// n <= tb.cap / 3 when the batch is mixed and larger than MON_KTAB (the callers see to it).
int covahip_monitor_plan(covahip_ctx *ctx, MonTable &tb, int tiles, int per_cu, int min_slice, const uint8_t *model_ids, int n,
                         MonPlan *plan) {
    const int num_cu = std::max(1, ctx->props.multiProcessorCount);
    // slices: enough workgroups for every CU, none shorter than min_slice samples (or the developer's length)
    const int want = (num_cu * per_cu + tiles - 1) / tiles;
    const int per = ctx->mon_slice > 0 ? ctx->mon_slice : std::max(min_slice, (n + want - 1) / want);
    bool uniform = true;
    if (model_ids)
        for (int b = 1; b < n && uniform; b++) uniform = model_ids[b] == model_ids[0];
    if (uniform) {
        const int S = (n + per - 1) / per;
        plan->kind = MonPlan::UNIFORM;
        plan->u = MonUniform{model_ids ? model_ids[0] : 0, (n + S - 1) / S};
        plan->S = (n + plan->u.per_slice - 1) / plan->u.per_slice;
        return COVAHIP_OK;
    }
    // stable counting sort of the samples by model, each model's segment cut into slices of near-equal length
    int seg[COVAHIP_MAX_MODELS + 1] = {};
    for (int b = 0; b < n; b++) seg[model_ids[b] + 1]++;
    for (int k = 0; k < COVAHIP_MAX_MODELS; k++) seg[k + 1] += seg[k];
    std::vector<int32_t> starts, models;
    for (int k = 0; k < COVAHIP_MAX_MODELS; k++) {
        const int len = seg[k + 1] - seg[k];
        if (!len) continue;
        const int parts = (len + per - 1) / per;
        for (int q = 0; q < parts; q++) {
            starts.push_back(seg[k] + (int)((int64_t)len * q / parts));
            models.push_back(k);
        }
    }
    const int S = (int)starts.size();
    plan->S = S;
    if (n <= MON_KTAB) {
        MonByValue &t = plan->v;
        std::memset(&t, 0, sizeof(t));
        int at[COVAHIP_MAX_MODELS];
        std::copy(seg, seg + COVAHIP_MAX_MODELS, at);
        for (int b = 0; b < n; b++) t.order[at[model_ids[b]]++] = (uint8_t)b;
        for (int s = 0; s < S; s++) t.start[s] = (uint8_t)starts[s], t.model[s] = (uint8_t)models[s];
        plan->kind = MonPlan::BY_VALUE;
        return COVAHIP_OK;
    }
    std::vector<int32_t> table((size_t)2 * S + n);
    std::copy(starts.begin(), starts.end(), table.begin());
    std::copy(models.begin(), models.end(), table.begin() + S);
    {
        int at[COVAHIP_MAX_MODELS];
        std::copy(seg, seg + COVAHIP_MAX_MODELS, at);
        for (int b = 0; b < n; b++) table[(size_t)2 * S + at[model_ids[b]]++] = b;
    }
    const int32_t *d_table = nullptr;   // (a counted batch never allocates: a table beyond what begin reserved is refused)
    if (int rc = tb.upload(ctx, table.data(), table.size(), &d_table)) return rc;
    plan->kind = MonPlan::BY_PTR;
    plan->p = MonByPtr{d_table};
    return COVAHIP_OK;
}

int covahip_monitor_hook(covahip_ctx *ctx, const uint8_t *d_mask, const int32_t *d_counts, const covahip_box *d_boxes, int max_boxes,
                         const uint8_t *model_ids, int batch, const BnInput *in) {
    CovahipMonitor *mon = ctx->mon;
    const bool counted = mon->batches_seen % mon->every == 0;
    if (counted) {
        MonPlan plan;
        if (int rc = covahip_monitor_plan(ctx, mon->lane[ctx->cur_lane], mon_tiles(mon), 1, MON_MIN_SLICE, model_ids, batch, &plan)) return rc;
        if (int rc = count_batch(ctx, mon, plan, d_mask, d_counts, d_boxes, max_boxes, batch)) return rc;
        // the batch's inputs (input_stats.hip) behind it on the same stream; a plan that lies in the lane's table is shared
        if (mon->d_in && in)
            if (int rc = covahip_monitor_hook_inputs(ctx, mon, plan, model_ids, *in, batch)) return rc;
    }
    mon->batches_seen++;
    mon->batches_counted += counted;
    return COVAHIP_OK;
}

void covahip_monitor_close(covahip_ctx *ctx, bool attached_only) {
    if (!ctx->mon || (attached_only && !ctx->mon->attached)) return;
    covahip_sync_all(ctx);
    free_monitor(ctx->mon);
    ctx->mon = nullptr;
}

extern "C" {

int covahip_monitor_begin(covahip_ctx *ctx, const covahip_monitor_cfg *cfg) {
    if (!ctx || !cfg) return COVAHIP_ERR_INVALID_ARG;
    if (cfg->h < 1 || cfg->w < 1 || cfg->n_models < 1 || cfg->n_models > COVAHIP_MAX_MODELS) return COVAHIP_ERR_INVALID_ARG;
    if (cfg->attach != 0 && cfg->attach != 1) return COVAHIP_ERR_INVALID_ARG;
    if (cfg->attach ? cfg->every < 1 : cfg->max_boxes < 0) return COVAHIP_ERR_INVALID_ARG;
    // a launch indexes macroblocks with 32 bits
    if ((int64_t)cfg->h * cfg->w > (int64_t)1 << 24) return COVAHIP_ERR_UNSUPPORTED;
    size_t tab_ints = (size_t)3 * MON_CHUNK;
    if (cfg->attach) {
        const covahip_blobnet *m = ctx->blobnet;
        if (!m) return COVAHIP_ERR_NOT_LOADED;
        if (m->H != cfg->h || m->W != cfg->w || m->n_models != cfg->n_models) return COVAHIP_ERR_INVALID_ARG;
        tab_ints = (size_t)3 * m->max_batch;
    }
    COVAHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = covahip_sync_all(ctx)) return rc;
    // built on the side: a failed begin leaves an open monitor as it was
    CovahipMonitor *mon = new CovahipMonitor();
    mon->h = cfg->h;
    mon->w = cfg->w;
    mon->n_models = cfg->n_models;
    mon->max_boxes = cfg->attach ? 0 : cfg->max_boxes;
    mon->every = cfg->attach ? cfg->every : 1;
    mon->attached = cfg->attach != 0;
    mon->words = (size_t)cfg->n_models * (4 + MON_BINS + (size_t)cfg->h * cfg->w);
    bool ok = hipMalloc((void **)&mon->d_tab, mon->words * sizeof(unsigned long long)) == hipSuccess &&
              hipMemsetAsync(mon->d_tab, 0, mon->words * sizeof(unsigned long long), ctx->primary) == hipSuccess &&
              hipStreamSynchronize(ctx->primary) == hipSuccess;
    for (int k = 0; k < (cfg->attach ? COVAHIP_MAX_LANES : 1) && ok; k++) ok = mon->lane[k].reserve(ctx, tab_ints) == COVAHIP_OK;
    if (!ok) {
        ctx->last_hip_error = "covahip_monitor_begin: allocation failed";
        (void)hipGetLastError();
        free_monitor(mon);
        return COVAHIP_ERR_HIP;
    }
    free_monitor(ctx->mon);   // (the ctx is drained: nothing in flight adds to it)
    ctx->mon = mon;
    return COVAHIP_OK;
}

int covahip_monitor_add(covahip_ctx *ctx, const uint8_t *mask, const int32_t *counts, const covahip_box *boxes, const uint8_t *model_ids,
                        int n, int mem_kind) {
    if (!ctx || !ctx->mon || ctx->mon->attached) return COVAHIP_ERR_INVALID_ARG;
    CovahipMonitor *mon = ctx->mon;
    if (n < 0 || (n > 0 && (!mask || !counts || (!boxes && mon->max_boxes > 0)))) return COVAHIP_ERR_INVALID_ARG;
    if (mem_kind != COVAHIP_MEM_HOST && mem_kind != COVAHIP_MEM_DEVICE) return COVAHIP_ERR_INVALID_ARG;
    if (model_ids)
        for (int b = 0; b < n; b++)
            if (model_ids[b] >= mon->n_models) return COVAHIP_ERR_INVALID_ARG;
    if (n == 0) return COVAHIP_OK;

    COVAHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int prc = covahip_primary_op(ctx)) return prc;   // on the primary stream, behind all lanes
    const size_t hw = (size_t)mon->h * mon->w, mb = (size_t)mon->max_boxes;
    if (mem_kind == COVAHIP_MEM_DEVICE) {
        for (int s0 = 0; s0 < n; s0 += MON_CHUNK) {
            const int c = std::min(MON_CHUNK, n - s0);
            MonPlan plan;
            if (int rc = covahip_monitor_plan(ctx, mon->lane[0], mon_tiles(mon), 1, MON_MIN_SLICE, model_ids ? model_ids + s0 : nullptr, c, &plan)) return rc;
            if (int rc = count_batch(ctx, mon, plan, mask + (size_t)s0 * hw, counts + s0, boxes ? boxes + (size_t)s0 * mb : nullptr,
                                     mon->max_boxes, c))
                return rc;
        }
    } else {   // staged in pieces: [mask][counts][boxes]
        const size_t per_sample = hw + sizeof(int32_t) + mb * sizeof(covahip_box);
        const int piece = (int)std::min<size_t>(std::min(n, MON_CHUNK), std::max<size_t>(1, MON_STAGE / per_sample));
        const size_t o_cnt = align256((size_t)piece * hw), o_box = o_cnt + align256((size_t)piece * sizeof(int32_t));
        if (int rc = covahip_ensure_buffer(ctx, &ctx->stage_in, &ctx->stage_in_bytes, o_box + align256((size_t)piece * mb * sizeof(covahip_box))))
            return rc;
        uint8_t *sm = (uint8_t *)ctx->stage_in;
        int32_t *sc = (int32_t *)(sm + o_cnt);
        covahip_box *sb = (covahip_box *)(sm + o_box);
        for (int s0 = 0; s0 < n; s0 += piece) {
            const int c = std::min(piece, n - s0);
            COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(sm, mask + (size_t)s0 * hw, (size_t)c * hw, hipMemcpyHostToDevice, ctx->stream));
            COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(sc, counts + s0, (size_t)c * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
            if (mb) COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(sb, boxes + (size_t)s0 * mb, (size_t)c * mb * sizeof(covahip_box), hipMemcpyHostToDevice, ctx->stream));
            MonPlan plan;
            if (int rc = covahip_monitor_plan(ctx, mon->lane[0], mon_tiles(mon), 1, MON_MIN_SLICE, model_ids ? model_ids + s0 : nullptr, c, &plan)) return rc;
            if (int rc = count_batch(ctx, mon, plan, sm, sc, sb, mon->max_boxes, c)) return rc;
        }
    }
    COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the caller may overwrite its arrays
    return COVAHIP_OK;
}

int covahip_monitor_read(covahip_ctx *ctx, int reset, int64_t *frames, int64_t *fire, int64_t *boxes, int64_t *frames_with_boxes,
                         int64_t *truncated, int64_t *area_hist, int64_t *batches_seen, int64_t *batches_counted) {
    if (!ctx || !ctx->mon) return COVAHIP_ERR_INVALID_ARG;
    CovahipMonitor *mon = ctx->mon;
    COVAHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = covahip_sync_all(ctx)) return rc;   // everything in flight on all lanes has been counted
    if (int prc = covahip_primary_op(ctx)) return prc;
    const size_t M = mon->n_models;
    const bool any = frames || fire || boxes || frames_with_boxes || truncated || area_hist;
    if (any) {
        // the scalars and the histogram are M * 20 words in front of the fire planes: fetched always, the planes when wanted
        const size_t words = fire ? mon->words : M * (4 + MON_BINS);
        std::vector<int64_t> host(words);
        COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(host.data(), mon->d_tab, words * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
        COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (frames) std::copy(host.begin(), host.begin() + M, frames);
        if (boxes) std::copy(host.begin() + M, host.begin() + 2 * M, boxes);
        if (frames_with_boxes) std::copy(host.begin() + 2 * M, host.begin() + 3 * M, frames_with_boxes);
        if (truncated) std::copy(host.begin() + 3 * M, host.begin() + 4 * M, truncated);
        if (area_hist) std::copy(host.begin() + 4 * M, host.begin() + M * (4 + MON_BINS), area_hist);
        if (fire) std::copy(host.begin() + M * (4 + MON_BINS), host.end(), fire);
    }
    if (batches_seen) *batches_seen = mon->batches_seen;
    if (batches_counted) *batches_counted = mon->batches_counted;
    if (reset) {
        COVAHIP_CHECK_HIP(ctx, hipMemsetAsync(mon->d_tab, 0, mon->words * sizeof(unsigned long long), ctx->stream));
        if (mon->d_in) COVAHIP_CHECK_HIP(ctx, hipMemsetAsync(mon->d_in, 0, mon->in_words * sizeof(unsigned long long), ctx->stream));
        COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        mon->batches_seen = mon->batches_counted = 0;
    }
    return COVAHIP_OK;
}

int covahip_monitor_end(covahip_ctx *ctx) {
    if (!ctx || !ctx->mon) return COVAHIP_ERR_INVALID_ARG;
    COVAHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    covahip_monitor_close(ctx, false);
    return COVAHIP_OK;
}

// Developer switch (include/covahip_dev.h): samples per slice of the monitor kernel, 0 = automatic.
int covahip_dev_monitor_slice(covahip_ctx *ctx, int samples) {
    if (!ctx || samples < 0) return COVAHIP_ERR_INVALID_ARG;
    ctx->mon_slice = samples;
    return COVAHIP_OK;
}

}  // extern "C"
