// Device-resident training data (include/covahip.h, "Training data"): the frames of any number of recordings as two-byte
// records (covahip_carrier_pack's packing) with their label bytes, and the launch that builds a training step's stacks and labels
// from a table of frame indices, mirrored where a sample asks for it, straight into the trainer's staging.  The label mass of
// the resident frames is served from here too (covahip_train_data_label_mass); its kernel lives in label_mass.hip.  So are the
// label-alignment counts of a recording (covahip_train_data_align); their kernel lives in train_align.hip.
//
// Storage: rec u16 [capacity][h][w], gt u8 [capacity][h][w]; every element offset is 64-bit (a 16x16 set of 8.5 M frames is 4.4 GB
// of records).  A frame of an odd h * w starts on an odd element, so the read side relies on 2-byte alignment only.
#include <algorithm>
#include <cstring>
#include <vector>

#include "internal.h"
#include "monitor_tab.h"

namespace {

constexpr int TT = 4;                         // slices of a stack
constexpr int BLK = 256;
constexpr int GATHER_MAX = 65535;             // samples per launch: the grid's y extent
constexpr size_t STAGE_BYTES = 32u << 20;     // host appends and host-bound gathers move through a staging area of this size
constexpr unsigned PACK_BLOCKS_MAX = 1u << 18;

// u8 [n_mb][4] -> min(type, 6) | min(mv_x, 6) << 3 | min(mv_y, 6) << 6, one macroblock per thread and round of the grid.
// WORDS: the source is 4-byte aligned and read a record at a time; otherwise byte by byte.
template <bool WORDS>
__global__ void k_pack_records(const uint8_t *__restrict__ frames, uint16_t *__restrict__ rec, int64_t n_mb) {
    const int64_t stride = (int64_t)gridDim.x * BLK;
    for (int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x; i < n_mb; i += stride) {
        uint32_t t, x, y;
        if (WORDS) {
            const uint32_t v = reinterpret_cast<const uint32_t *>(frames)[i];
            t = v & 0xFFu, x = (v >> 8) & 0xFFu, y = (v >> 16) & 0xFFu;
        } else {
            t = frames[4 * i], x = frames[4 * i + 1], y = frames[4 * i + 2];
        }
        rec[i] = (uint16_t)(min(t, 6u) | (min(x, 6u) << 3) | (min(y, 6u) << 6));
    }
}

// One workgroup row per output sample (blockIdx.y), one thread per macroblock of the grid: the thread at (y, x) reads the four
// records and the label at (y', x') and stores four bytes per slice at (y, x), so a wave's stores are contiguous whatever the
// mirror; a mirrored row is read back to front inside the same cache lines.
__global__ void k_gather(const uint16_t *__restrict__ rec, const uint8_t *__restrict__ gt, const covahip_train_sample *__restrict__ tab,
                         uint32_t *__restrict__ stack, uint8_t *__restrict__ lab, int h, int w) {
    const int hw = h * w;
    const int pos = (int)(blockIdx.x * BLK + threadIdx.x);
    if (pos >= hw) return;
    const covahip_train_sample s = tab[blockIdx.y];
    const int y = pos / w, x = pos - y * w;
    const int ys = (s.flags & 2u) ? h - 1 - y : y, xs = (s.flags & 1u) ? w - 1 - x : x;
    const int src = ys * w + xs;
    uint32_t *out = stack + (int64_t)blockIdx.y * TT * hw + pos;
#pragma unroll
    for (int t = 0; t < TT; t++) {
        const uint32_t r = rec[(int64_t)s.frame[t] * hw + src];
        out[(int64_t)t * hw] = (r & 7u) | ((r >> 3) & 7u) << 8 | ((r >> 6) & 7u) << 16;
    }
    lab[(int64_t)blockIdx.y * hw + pos] = gt[(int64_t)s.label * hw + src];
}

}  // namespace

struct covahip_train_data {
    covahip_ctx *ctx = nullptr;
    int h = 0, w = 0;
    int64_t capacity = 0, frames = 0;
    uint16_t *rec = nullptr;
    uint8_t *gt = nullptr;
    covahip_train_sample *d_tab = nullptr, *h_tab = nullptr;   // the table of one launch sequence; h_: pinned
    int tab_cap = 0;
    void *stage = nullptr;                                      // device staging of a host-bound gather
    size_t stage_bytes = 0;
    std::vector<uint16_t> pack;                                 // host staging of a host append
    size_t stage_budget = STAGE_BYTES;                          // covahip_dev_train_data_set_stage changes it per set
    ResidentTable<uint32_t> keep_bits;                          // label mass: the call's keep map, a bit per macroblock; reserved on first use
    // record statistics: i64 [4 + 512 + 16 + hw] as one model of the input monitor | hist_set [512] | the launch pair's per-frame
    // partials u64 [IN_CHUNK][2] (zero between calls); one allocation, on first use
    unsigned long long *stats = nullptr;
};

namespace {

int enter(covahip_ctx *ctx) {
    COVAHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    return covahip_primary_op(ctx);
}

void free_data(covahip_train_data *d) {
    if (d->rec) hipFree(d->rec);
    if (d->gt) hipFree(d->gt);
    if (d->d_tab) hipFree(d->d_tab);
    if (d->h_tab) hipHostFree(d->h_tab);
    if (d->stage) hipFree(d->stage);
    if (d->stats) hipFree(d->stats);
    d->keep_bits.release();
    delete d;
}

}  // namespace

int covahip_train_data_check(const covahip_train_data *d, const covahip_ctx *ctx, int h, int w, const covahip_train_sample *s,
                             int64_t n) {
    if (!d || !s || n < 0 || (ctx && d->ctx != ctx) || d->h != h || d->w != w) return COVAHIP_ERR_INVALID_ARG;
    for (int64_t i = 0; i < n; i++) {
        if (s[i].flags & ~3u) return COVAHIP_ERR_INVALID_ARG;
        if (s[i].label < 0 || s[i].label >= d->frames) return COVAHIP_ERR_INVALID_ARG;
        for (int t = 0; t < TT; t++)
            if (s[i].frame[t] < 0 || s[i].frame[t] >= d->frames) return COVAHIP_ERR_INVALID_ARG;
    }
    return COVAHIP_OK;
}

int covahip_train_data_table(covahip_train_data *d, int n, covahip_train_sample **tab) {
    covahip_ctx *ctx = d->ctx;
    if (n > d->tab_cap) {
        COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));   // nothing in flight reads the old table
        if (d->d_tab) hipFree(d->d_tab);
        if (d->h_tab) hipHostFree(d->h_tab);
        d->d_tab = d->h_tab = nullptr;
        d->tab_cap = 0;
        const int cap = std::max(n, 256);
        COVAHIP_CHECK_HIP(ctx, hipMalloc(reinterpret_cast<void **>(&d->d_tab), (size_t)cap * sizeof(covahip_train_sample)));
        COVAHIP_CHECK_HIP(ctx, hipHostMalloc(reinterpret_cast<void **>(&d->h_tab), (size_t)cap * sizeof(covahip_train_sample)));
        d->tab_cap = cap;
    }
    *tab = d->h_tab;
    return COVAHIP_OK;
}

int covahip_train_data_launch(covahip_train_data *d, int n, uint8_t *d_stack, uint8_t *d_gt) {
    covahip_ctx *ctx = d->ctx;
    if (n <= 0 || n > d->tab_cap) return COVAHIP_ERR_INVALID_ARG;
    const hipStream_t s = ctx->stream;
    const size_t hw = (size_t)d->h * d->w;
    COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(d->d_tab, d->h_tab, (size_t)n * sizeof(covahip_train_sample), hipMemcpyHostToDevice, s));
    for (int at = 0; at < n; at += GATHER_MAX) {
        const int m = std::min(GATHER_MAX, n - at);
        ProfScope prof(ctx, "train_data_gather");
        k_gather<<<dim3((unsigned)((hw + BLK - 1) / BLK), (unsigned)m), BLK, 0, s>>>(
            d->rec, d->gt, d->d_tab + at, reinterpret_cast<uint32_t *>(d_stack + (size_t)at * TT * hw * 4), d_gt + (size_t)at * hw, d->h, d->w);
        COVAHIP_CHECK_HIP(ctx, hipGetLastError());
    }
    return COVAHIP_OK;
}

extern "C" {

int covahip_train_data_create(covahip_ctx *ctx, int h_mb, int w_mb, int64_t capacity_frames, covahip_train_data **out) {
    if (out) *out = nullptr;
    if (!ctx || !out || h_mb < 16 || w_mb < 16 || h_mb > 1024 || w_mb > 1024 || capacity_frames < 1 || capacity_frames > INT32_MAX)
        return COVAHIP_ERR_INVALID_ARG;
    if (int rc = enter(ctx)) return rc;
    covahip_train_data *d = new covahip_train_data();
    d->ctx = ctx;
    d->h = h_mb;
    d->w = w_mb;
    d->capacity = capacity_frames;
    const size_t n_mb = (size_t)capacity_frames * h_mb * w_mb;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&d->rec), n_mb * sizeof(uint16_t));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&d->gt), n_mb);
    if (e != hipSuccess) {
        ctx->last_hip_error = std::string("covahip_train_data_create: ") + hipGetErrorString(e);
        (void)hipGetLastError();
        free_data(d);
        return COVAHIP_ERR_HIP;
    }
    *out = d;
    return COVAHIP_OK;
}

int covahip_train_data_append(covahip_train_data *d, const uint8_t *frames, const uint8_t *gt, int n, int mem_kind, int64_t *first_index) {
    if (!d || !frames || !gt || n < 1 || (mem_kind != COVAHIP_MEM_HOST && mem_kind != COVAHIP_MEM_DEVICE)) return COVAHIP_ERR_INVALID_ARG;
    if ((int64_t)n > d->capacity - d->frames) return COVAHIP_ERR_OVERFLOW;
    covahip_ctx *ctx = d->ctx;
    if (int rc = enter(ctx)) return rc;
    const hipStream_t s = ctx->stream;
    const size_t hw = (size_t)d->h * d->w, at = (size_t)d->frames * hw, n_mb = (size_t)n * hw;
    if (mem_kind == COVAHIP_MEM_DEVICE) {
        const unsigned blocks = (unsigned)std::min<size_t>((n_mb + BLK - 1) / BLK, PACK_BLOCKS_MAX);
        ProfScope prof(ctx, "train_data_pack");
        if ((reinterpret_cast<uintptr_t>(frames) & 3u) == 0)
            k_pack_records<true><<<blocks, BLK, 0, s>>>(frames, d->rec + at, (int64_t)n_mb);
        else
            k_pack_records<false><<<blocks, BLK, 0, s>>>(frames, d->rec + at, (int64_t)n_mb);
        COVAHIP_CHECK_HIP(ctx, hipGetLastError());
        COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(d->gt + at, gt, n_mb, hipMemcpyDeviceToDevice, s));
    } else {   // packed on the host: two bytes per macroblock cross the bus
        const size_t chunk = std::min(n_mb, std::max<size_t>(1, d->stage_budget / sizeof(uint16_t)));
        if (d->pack.size() < chunk) d->pack.resize(chunk);
        for (size_t o = 0; o < n_mb; o += chunk) {
            const size_t m = std::min(chunk, n_mb - o);
            covahip_carrier_pack(frames + 4 * o, m, d->pack.data());
            COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(d->rec + at + o, d->pack.data(), m * sizeof(uint16_t), hipMemcpyHostToDevice, s));
            COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));   // the staging is packed again by the next round
        }
        COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(d->gt + at, gt, n_mb, hipMemcpyHostToDevice, s));
    }
    COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
    if (first_index) *first_index = d->frames;
    d->frames += n;
    return COVAHIP_OK;
}

int covahip_train_data_frames(const covahip_train_data *d, int64_t *n) {
    if (!d || !n) return COVAHIP_ERR_INVALID_ARG;
    *n = d->frames;
    return COVAHIP_OK;
}

int covahip_train_data_gather(covahip_train_data *d, const covahip_train_sample *samples, int n, uint8_t *stack, uint8_t *gt, int mem_kind) {
    if (!d || !samples || !stack || !gt || n < 1 || (mem_kind != COVAHIP_MEM_HOST && mem_kind != COVAHIP_MEM_DEVICE))
        return COVAHIP_ERR_INVALID_ARG;
    const bool host = mem_kind == COVAHIP_MEM_HOST;
    if (!host && (reinterpret_cast<uintptr_t>(stack) & 3u)) return COVAHIP_ERR_INVALID_ARG;   // the launch stores whole records
    if (int rc = covahip_train_data_check(d, nullptr, d->h, d->w, samples, n)) return rc;
    covahip_ctx *ctx = d->ctx;
    if (int rc = enter(ctx)) return rc;
    const hipStream_t s = ctx->stream;
    const size_t hw = (size_t)d->h * d->w, stack_b = TT * hw * 4, per = stack_b + hw;
    // a launch's samples: what the grid takes, and for host output what the staging holds
    const size_t fit = host ? std::max<size_t>(1, std::min<size_t>(d->stage_budget / per, GATHER_MAX)) : (size_t)GATHER_MAX;
    const int chunk = (int)std::min<size_t>((size_t)n, fit);
    if (host)
        if (int rc = covahip_ensure_buffer(ctx, &d->stage, &d->stage_bytes, (size_t)chunk * per)) return rc;
    for (int at = 0; at < n; at += chunk) {
        const int m = std::min(chunk, n - at);
        covahip_train_sample *tab = nullptr;
        if (int rc = covahip_train_data_table(d, m, &tab)) return rc;
        std::memcpy(tab, samples + at, (size_t)m * sizeof(covahip_train_sample));
        uint8_t *o_stack = host ? static_cast<uint8_t *>(d->stage) : stack + (size_t)at * stack_b;
        uint8_t *o_gt = host ? static_cast<uint8_t *>(d->stage) + (size_t)chunk * stack_b : gt + (size_t)at * hw;
        if (int rc = covahip_train_data_launch(d, m, o_stack, o_gt)) return rc;
        if (host) {
            COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(stack + (size_t)at * stack_b, o_stack, (size_t)m * stack_b, hipMemcpyDeviceToHost, s));
            COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(gt + (size_t)at * hw, o_gt, (size_t)m * hw, hipMemcpyDeviceToHost, s));
        }
        COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));   // the table and the staging are reused by the next chunk
    }
    return COVAHIP_OK;
}

int covahip_train_data_label_mass(covahip_train_data *d, int64_t first, int64_t n, const uint8_t *keep_or_null, uint32_t *mass,
                                  int mem_kind) {
    if (!d || !mass || n < 1 || first < 0 || (mem_kind != COVAHIP_MEM_HOST && mem_kind != COVAHIP_MEM_DEVICE))
        return COVAHIP_ERR_INVALID_ARG;
    if (n > d->frames || first > d->frames - n) return COVAHIP_ERR_INVALID_ARG;
    const bool host = mem_kind == COVAHIP_MEM_HOST;
    if (!host && (reinterpret_cast<uintptr_t>(mass) & 3u)) return COVAHIP_ERR_INVALID_ARG;   // the launch stores whole counts
    const int hw = d->h * d->w;
    const size_t nw = ((size_t)hw + 31) / 32;
    std::vector<uint32_t> bits;
    if (keep_or_null) {
        bits.assign(nw, 0u);
        bool any = false;
        for (int i = 0; i < hw; i++)
            if (keep_or_null[i]) bits[(size_t)i >> 5] |= 1u << (i & 31), any = true;
        if (!any) return COVAHIP_ERR_INVALID_ARG;   // nothing would count
    }
    covahip_ctx *ctx = d->ctx;
    if (int rc = enter(ctx)) return rc;
    const hipStream_t s = ctx->stream;
    const uint32_t *d_bits = nullptr;
    if (keep_or_null) {
        if (int rc = d->keep_bits.reserve(ctx, nw)) return rc;
        if (int rc = d->keep_bits.upload(ctx, bits.data(), nw, &d_bits)) return rc;
    }
    // a launch sequence's frames: all of them, or for host output what the staging holds
    const int64_t chunk = host ? std::min<int64_t>(n, (int64_t)std::max<size_t>(1, d->stage_budget / sizeof(uint32_t))) : n;
    if (host)
        if (int rc = covahip_ensure_buffer(ctx, &d->stage, &d->stage_bytes, (size_t)chunk * sizeof(uint32_t))) return rc;
    for (int64_t at = 0; at < n; at += chunk) {
        const int64_t m = std::min(chunk, n - at);
        uint32_t *out = host ? static_cast<uint32_t *>(d->stage) : mass + at;
        if (int rc = covahip_label_mass_launch(ctx, d->gt, d_bits, out, first + at, m, hw)) return rc;
        if (host) {
            COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(mass + at, out, (size_t)m * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));   // the staging is written again by the next chunk
        }
    }
    COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
    return COVAHIP_OK;
}

int covahip_train_data_record_stats(covahip_train_data *d, int64_t first, int64_t n, const covahip_record_stats *out) {
    if (!d || !out || n < 1 || first < 0) return COVAHIP_ERR_INVALID_ARG;
    if (n > d->frames || first > d->frames - n) return COVAHIP_ERR_INVALID_ARG;
    covahip_ctx *ctx = d->ctx;
    if (int rc = enter(ctx)) return rc;
    const hipStream_t s = ctx->stream;
    const int hw = d->h * d->w;
    const size_t words = covahip_input_words((size_t)hw), counts = words + IN_HIST;
    const size_t total = counts + (size_t)IN_CHUNK * 2;
    if (!d->stats) {
        COVAHIP_CHECK_HIP(ctx, hipMalloc(reinterpret_cast<void **>(&d->stats), total * sizeof(unsigned long long)));
        COVAHIP_CHECK_HIP(ctx, hipMemsetAsync(d->stats, 0, total * sizeof(unsigned long long), s));
    } else {   // the partials too: an earlier call that failed between its two launches may have left some
        COVAHIP_CHECK_HIP(ctx, hipMemsetAsync(d->stats, 0, total * sizeof(unsigned long long), s));
    }
    MonTable none;   // (a one-model plan uploads nothing)
    for (int64_t at = 0; at < n; at += IN_CHUNK) {
        const int c = (int)std::min<int64_t>(IN_CHUNK, n - at);
        MonPlan plan;
        if (int rc = covahip_input_plan(ctx, none, hw, nullptr, c, &plan)) return rc;
        InJob j;
        j.src = reinterpret_cast<const uint8_t *>(d->rec);
        j.packed = true;
        j.stride = (size_t)hw * sizeof(uint16_t);
        j.frames.off = (int)(first + at);
        j.labels = d->gt;
        j.tab = d->stats;
        j.model_stride = words;
        j.set_hist = d->stats + words;
        j.scratch = d->stats + counts;
        j.hw = hw;
        if (int rc = covahip_input_count(ctx, j, plan, c)) return rc;
    }
    std::vector<int64_t> host(counts);
    COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(host.data(), d->stats, counts * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
    const int64_t *t = host.data();
    if (out->frames) *out->frames = t[0];
    if (out->still_frames) *out->still_frames = t[1];
    if (out->intra_frames) *out->intra_frames = t[2];
    if (out->hist) std::copy(t + IN_HEAD, t + IN_HEAD + IN_HIST, out->hist);
    if (out->move_hist) std::copy(t + IN_HEAD + IN_HIST, t + IN_HEAD + IN_HIST + IN_MOVE_BINS, out->move_hist);
    if (out->moving) std::copy(t + IN_HEAD + IN_HIST + IN_MOVE_BINS, t + words, out->moving);
    if (out->hist_set) std::copy(t + words, t + counts, out->hist_set);
    if (out->set_total) {
        int64_t sum = 0;
        for (size_t k = words; k < counts; k++) sum += t[k];
        *out->set_total = sum;
    }
    return COVAHIP_OK;
}

int covahip_train_data_align(covahip_train_data *d, int64_t first, int64_t n, const covahip_align_cfg *cfg, uint32_t *both,
                             uint32_t *mov, uint32_t *lab, int mem_kind) {
    if (!d || !cfg || !both || !mov || !lab || n < 1 || first < 0 || (mem_kind != COVAHIP_MEM_HOST && mem_kind != COVAHIP_MEM_DEVICE))
        return COVAHIP_ERR_INVALID_ARG;
    if (n > d->frames || first > d->frames - n) return COVAHIP_ERR_INVALID_ARG;
    if (cfg->max_shift < 0 || cfg->max_shift > 32 || cfg->min_mv < 0 || cfg->min_mv > 6 || (cfg->class_mask & ~0x7Fu)) return COVAHIP_ERR_INVALID_ARG;
    if (cfg->min_mv == 0 && cfg->class_mask == 0) return COVAHIP_ERR_INVALID_ARG;   // nothing can move
    const bool host = mem_kind == COVAHIP_MEM_HOST;
    if (!host && ((reinterpret_cast<uintptr_t>(both) | reinterpret_cast<uintptr_t>(mov) | reinterpret_cast<uintptr_t>(lab)) & 3u))
        return COVAHIP_ERR_INVALID_ARG;                                              // the launch stores whole counts
    const int hw = d->h * d->w, S = cfg->max_shift;
    const size_t nw = ((size_t)hw + 31) / 32, W = 2 * (size_t)S + 1;
    std::vector<uint32_t> bits;
    if (cfg->keep) {
        bits.assign(nw, 0u);
        bool any = false;
        for (int i = 0; i < hw; i++)
            if (cfg->keep[i]) bits[(size_t)i >> 5] |= 1u << (i & 31), any = true;
        if (!any) return COVAHIP_ERR_INVALID_ARG;   // nothing would count
    }
    uint64_t lut = 0;                                // bit (mv_x | mv_y << 3): max(mv_x, mv_y) >= min_mv
    for (int y = 0; y < 8 && cfg->min_mv; y++)
        for (int x = 0; x < 8; x++)
            if (std::max(x, y) >= cfg->min_mv) lut |= (uint64_t)1 << (x | y << 3);
    covahip_ctx *ctx = d->ctx;
    if (int rc = enter(ctx)) return rc;
    const hipStream_t s = ctx->stream;
    const uint32_t *d_bits = nullptr;
    if (cfg->keep) {
        if (int rc = d->keep_bits.reserve(ctx, nw)) return rc;
        if (int rc = d->keep_bits.upload(ctx, bits.data(), nw, &d_bits)) return rc;
    }
    // a launch's frames: all of them, or for host outputs what the staging holds of the three tables
    const size_t per = (W + 2) * sizeof(uint32_t);
    const int64_t chunk = host ? std::min<int64_t>(n, (int64_t)std::max<size_t>(1, d->stage_budget / per)) : n;
    if (host)
        if (int rc = covahip_ensure_buffer(ctx, &d->stage, &d->stage_bytes, (size_t)chunk * per)) return rc;
    uint32_t *st = static_cast<uint32_t *>(d->stage);
    for (int64_t at = 0; at < n; at += chunk) {
        const int64_t m = std::min(chunk, n - at);
        uint32_t *o_both = host ? st : both + (size_t)at * W, *o_mov = host ? st + (size_t)chunk * W : mov + at;
        uint32_t *o_lab = host ? st + (size_t)chunk * (W + 1) : lab + at;
        if (int rc = covahip_align_launch(ctx, d->rec, d->gt, d->capacity, d_bits, lut, cfg->class_mask, S, first, n, at, m, hw, o_both,
                                          o_mov, o_lab))
            return rc;
        if (host) {
            COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(both + (size_t)at * W, o_both, (size_t)m * W * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(mov + at, o_mov, (size_t)m * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(lab + at, o_lab, (size_t)m * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));   // the staging is written again by the next chunk
        }
    }
    COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
    return COVAHIP_OK;
}

void covahip_train_data_destroy(covahip_train_data *d) {
    if (!d) return;
    hipSetDevice(d->ctx->device);
    covahip_sync_all(d->ctx);
    free_data(d);
}

int covahip_dev_train_data_set_stage(covahip_train_data *d, size_t bytes) {
    if (!d) return COVAHIP_ERR_INVALID_ARG;
    d->stage_budget = bytes ? bytes : STAGE_BYTES;
    return COVAHIP_OK;
}

}  // extern "C"
