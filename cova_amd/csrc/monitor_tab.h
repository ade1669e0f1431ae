// The order / slice table of a counted batch, shared by the serving monitor's kernels (monitor.hip: monitor_count; input_stats.hip:
// input_count, input_finish).  The host groups the batch's samples by model (a stable counting sort of the host model ids) and
// cuts every model's segment into slices; the order and the slices reach a kernel by value (batches of at most MON_KTAB
// samples), from a per-lane device table (larger ones), or not at all (a batch of one model: the slices are ranges of the call's
// own order).  A slice s of S covers positions [i0, i1) of the order; position i is sample `mon_sample(t, S, i)`.
#pragma once
#include <cstdint>

#include "internal.h"

constexpr int MON_KTAB = 256;            // samples whose order / slice table travels in the kernel arguments

struct MonUniform {   // one model: slices are ranges of the call's own order
    int model, per_slice;
};
struct MonByValue {   // <= MON_KTAB samples: start[s] is slice s's first position (the next slice's start, or n, ends it)
    uint8_t order[MON_KTAB], start[MON_KTAB], model[MON_KTAB];
};
struct MonByPtr {     // i32 [S starts][S models][n order] on the device
    const int32_t *tab;
};
__device__ inline void mon_slice(const MonUniform &t, int s, int S, int n, int &m, int &i0, int &i1) {
    m = t.model;
    i0 = s * t.per_slice;
    i1 = min(n, i0 + t.per_slice);
}
__device__ inline int mon_sample(const MonUniform &, int, int i) { return i; }
__device__ inline void mon_slice(const MonByValue &t, int s, int S, int n, int &m, int &i0, int &i1) {
    m = t.model[s];
    i0 = t.start[s];
    i1 = s + 1 < S ? (int)t.start[s + 1] : n;
}
__device__ inline int mon_sample(const MonByValue &t, int, int i) { return t.order[i]; }
__device__ inline void mon_slice(const MonByPtr &t, int s, int S, int n, int &m, int &i0, int &i1) {
    m = t.tab[S + s];
    i0 = t.tab[s];
    i1 = s + 1 < S ? t.tab[s + 1] : n;
}
__device__ inline int mon_sample(const MonByPtr &t, int S, int i) { return t.tab[2 * S + i]; }

// One batch's table in the form it travels in; built on the host by covahip_monitor_plan (monitor.hip).
struct MonPlan {
    enum Kind { UNIFORM, BY_VALUE, BY_PTR } kind = UNIFORM;
    int S = 0;   // slices
    MonUniform u{};
    MonByValue v{};
    MonByPtr p{};
};
// The plan of n samples (model_ids: host u8 [n] or null = model 0; every id is below COVAHIP_MAX_MODELS) for a kernel whose
// workgroups own (one of `tiles` tiles, one slice): enough slices for per_cu workgroups on every CU, none shorter than min_slice
// samples (covahip_dev_monitor_slice overrides the length).  tb: the table buffers of the lane (or of the primary stream) a mixed batch larger than MON_KTAB is uploaded
// through, on ctx->stream; nothing is allocated (a table beyond what tb has reserved is refused).
int covahip_monitor_plan(covahip_ctx *ctx, MonTable &tb, int tiles, int per_cu, int min_slice, const uint8_t *model_ids, int n,
                         MonPlan *plan);

// input_stats.hip: the input statistics (include/covahip.h, "Input monitor") of n samples in two launches on ctx->stream.
// Sample b's frame is frame f(b) of `src`: val[b] (by_value), d_idx[b * idx_stride] (d_idx != null) or b + off, `stride` bytes
// apart; a frame is u8 [hw][4] or, packed, u16 [hw], at any alignment.  labels (packed, one-model plans only): u8 frames of hw
// bytes with the same index, whose non-zero bytes select the records of set_hist.
// tab: i64 words of model m at tab + m * model_stride: in_frames, still_frames, intra_frames, (spare) | hist [512] |
// move_hist [16] | moving [hw]; set_hist: i64 [512] or null.  scratch: u64 [n][2], all zero before and after the call.
struct InFrames {
    const int32_t *d_idx = nullptr;
    int idx_stride = 1, off = 0, by_value = 0;
    uint16_t val[MON_KTAB] = {};
};
struct InJob {
    const uint8_t *src = nullptr;
    bool packed = false;
    size_t stride = 0;
    InFrames frames;
    const uint8_t *labels = nullptr;
    unsigned long long *tab = nullptr, *set_hist = nullptr, *scratch = nullptr;
    size_t model_stride = 0;
    int hw = 0;
};
constexpr int IN_CHUNK = 16384;   // samples per launch pair of a stand-alone add and of the training-data form: what a scratch holds
constexpr int IN_HEAD = 4, IN_HIST = 512, IN_MOVE_BINS = 16;
constexpr size_t covahip_input_words(size_t hw) { return IN_HEAD + IN_HIST + IN_MOVE_BINS + hw; }
int covahip_input_count(covahip_ctx *ctx, const InJob &job, const MonPlan &plan, int n);
// the plan input_count wants of n samples on a grid of hw macroblocks (tb as above)
int covahip_input_plan(covahip_ctx *ctx, MonTable &tb, int hw, const uint8_t *model_ids, int n, MonPlan *plan);
