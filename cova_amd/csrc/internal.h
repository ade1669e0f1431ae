// Internal declarations shared by the translation units of libcovahip.so.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "covahip.h"

struct covahip_blobnet;  // blobnet.hip
struct covahip_ctx;

// x rounded up to the 256-byte step of sub-buffers carved from one allocation
constexpr size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// A list of mask thresholds as covahip_post_sweep and covahip_post_heat_begin take it: finite and strictly ascending.
inline bool covahip_thresholds_ok(const float *v, int n) {
    for (int t = 0; t < n; t++)
        if (!std::isfinite(v[t]) || (t && !(v[t] > v[t - 1]))) return false;
    return true;
}

// A small host table that kernels read from device memory: uploaded from a pinned copy on ctx->stream, and not at all while the
// contents a call asks for are the resident ones.  One stream per table (a lane's, or the primary one).  The owner states the
// capacity policy: reserve() is the only member that allocates, upload() refuses what does not fit.  (Members: below the ctx.)
template <typename T>
struct ResidentTable {
    T *dev = nullptr;
    T *pinned = nullptr;         // host copy the device copy is uploaded from
    size_t cap = 0;              // capacity of both, in elements
    hipEvent_t ev = nullptr;     // behind the last upload: once it has passed, the pinned copy is free again
    bool recorded = false;       // `ev` was ever recorded
    std::vector<T> resident;     // what `dev` holds; empty: nothing a call could ask for

    // Room for n elements.  Storage that is replaced may still be read by kernels on ctx->stream: that stream is drained first,
    // and nothing is resident afterwards.
    int reserve(covahip_ctx *ctx, size_t n);
    // src[0 .. n) on the device: *d_out = dev.  Resident contents cost no HIP call; n > cap is COVAHIP_ERR_INVALID_ARG.
    int upload(covahip_ctx *ctx, const T *src, size_t n, const T **d_out);
    void invalidate() { resident.clear(); }   // the next upload copies whatever it is given
    void release();                           // frees everything (nothing in flight reads the device copy any more)
};

// Lanes: batches in flight on one GPU.  Every launch of the hot path has a fixed cost (weights into registers, the first
// band's DMA, the slowest workgroup's tail) during which most of the chip idles; at b = 256 that is a third of a step.
// The reference keeps its GPU busy the same way -- sixteen BlobNet engines with their own batches on one GPU
// (experiment/cova/config.yaml:33-34, pipeline/cova/pipeline.py:139-181).  A ctx therefore owns `n_lanes` HIP streams,
// each with its own activation workspace and bboxcc scratch; consecutive covahip_filter_forward(_frames) calls on device
// pointers go to consecutive lanes and overlap.  Ordering rules (LaneScope / covahip_primary_op, ctx.hip):
//   * a call placed on a lane is ordered behind everything enqueued on the ctx's primary stream before it;
//   * every other entry point (timers, sync, copies, stand-alone bboxcc / blobnet calls) first makes the primary stream
//     wait for all lanes, so it observes every earlier filter call;
//   * two filter calls with nothing in between are NOT ordered with each other: they must not share output buffers.
// n_lanes = 1: everything runs on the primary stream, in call order.
constexpr int COVAHIP_MAX_LANES = 4;
struct CtxLane {
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;     // recorded behind the last call placed on this lane
    bool pending = false;          // `done` has not been joined into the primary stream yet
    uint64_t seen_seq = 0;         // state of the primary stream this lane is ordered behind (covahip_ctx::primary_seq)
    // bboxcc scratch of the fused path (mask when the caller wants none), overflow list of the wave kernel (count + frame
    // indices), state slab of frames too large for LDS (one per resident workgroup)
    void *cc_scratch = nullptr;
    size_t cc_scratch_bytes = 0;
    void *cc_ovf = nullptr;
    size_t cc_ovf_bytes = 0;
    void *cc_slab = nullptr;
    size_t cc_slab_bytes = 0;
    // overflow counters of the last completed large-batch bboxcc call on this lane: pinned, device-visible words
    // {overflowed pass 1, overflowed pass 2, sampled frames with 128 < runs <= 192 / <= 256 / more, batch, capacity of pass 1}
    // written by the call's last kernel (no copy, no event); bboxcc.hip adapts the next call's plan to them
    int32_t *cc_stat = nullptr;
    int32_t *cc_stat_ring = nullptr;
    unsigned cc_stat_turn = 0;           // which of the two device counter sets the next call uses
    bool cc_second_skipped = false;      // the last call ran without the second-chance pass
    int cc_stat_batch = 0, cc_stat_cap = 0;
    int cc_first_cap = 0;                // first-pass capacity the statistics last decided on (0: none yet)
};

// covahip_monitor_* (monitor.hip): the open serving monitor of a ctx.  Everything a counted batch touches is allocated by begin.
using MonTable = ResidentTable<int32_t>;   // order / slice table of a mixed batch too large for the kernel arguments; reserved by begin
struct CovahipMonitor {
    int h = 0, w = 0, n_models = 0, max_boxes = 0, every = 1;
    bool attached = false;
    // i64 counters on the device: frames [M] | boxes [M] | frames_with_boxes [M] | truncated [M] | area_hist [M][16] | fire [M][h][w]
    unsigned long long *d_tab = nullptr;
    size_t words = 0;
    int64_t batches_seen = 0, batches_counted = 0;
    MonTable lane[COVAHIP_MAX_LANES];   // attached: one per lane (lane 0's also serves the primary stream); stand-alone: [0] only
    // covahip_monitor_set_inputs (input_stats.hip), null / empty while the input statistics are off.  i64 words per model:
    // in_frames, still_frames, intra_frames, (spare) | hist [512] | move_hist [16] | moving [h][w]
    unsigned long long *d_in = nullptr;
    size_t in_words = 0;
    // per-frame partials of a batch in flight, u64 [samples][2] per lane as `lane`, zero between batches
    unsigned long long *in_scratch[COVAHIP_MAX_LANES] = {};
    int in_samples = 0;          // samples a scratch holds
    MonTable in_frames;          // stand-alone: a call's host frame list beyond what travels in the kernel arguments
};

struct covahip_ctx {
    int device = 0;
    hipStream_t primary = nullptr;   // the ctx's own stream
    hipStream_t stream = nullptr;    // where launches go NOW: `primary`, or the current lane's stream inside a LaneScope
    CtxLane lanes[COVAHIP_MAX_LANES];
    int n_lanes = 1, next_lane = 0, cur_lane = 0;   // one lane unless the caller opts in (covahip_ctx_set_lanes)
    bool in_lane = false;
    uint64_t primary_seq = 1;        // bumped by every operation enqueued on the primary stream
    hipEvent_t ev_fork = nullptr;
    std::string last_hip_error;
    hipDeviceProp_t props{};
    // timers
    hipEvent_t t_start[16]{};
    hipEvent_t t_stop[16]{};
    // per-kernel profiling
    bool profile = false;
    std::string profile_filter;
    struct ProfEntry {
        std::string name;
        hipEvent_t a, b;
    };
    std::vector<ProfEntry> prof_pending;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_pool;
    std::map<std::string, std::pair<double, int64_t>> prof_acc;
    // staging buffers for host-pointer calls
    void *stage_in = nullptr;
    size_t stage_in_bytes = 0;
    void *stage_out = nullptr;
    size_t stage_out_bytes = 0;
    void *pinned = nullptr;
    size_t pinned_bytes = 0;
    void *sweep_buf = nullptr;   // covahip_post_sweep: accumulators, keep map, one chunk's mask frames, boxes and counts
    size_t sweep_bytes = 0;
    ResidentTable<int32_t> cc_area;   // covahip_bboxcc_v: the call's per-frame area thresholds, on the primary stream; grows to the batch
    int cc_wave_cap = 0;       // bboxcc wave kernel: developer override of its run capacity
    int tail_in_dec012 = 0;    // the last forward ran the last decoder block inside dec012_mfma (covahip_dev_blobnet_tail_in_dec012)
    int tail_form = 0;         // which kernel ran the last decoder block of the last forward (covahip_dev_blobnet_tail_form)
    CtxLane &lane() { return lanes[cur_lane]; }
    struct { int nbands, nbuf; } enc_plan[4] = {};   // developer override of the encoder band plan per level (0 = automatic)
    covahip_blobnet *blobnet = nullptr;
    // covahip_post_heat_*: the open heat's counters, u32 [2 T + 1][h][w] (fire planes, both planes, the label plane)
    void *heat_buf = nullptr;
    size_t heat_bytes = 0;
    bool heat_open = false;
    int heat_h = 0, heat_w = 0, heat_T = 0;
    float heat_thresh[64] = {};
    int64_t heat_samples = 0;
    size_t heat_stage = 0;   // bytes of host samples staged per piece; 0: heat.hip's default (covahip_dev_heat_set_stage)
    // covahip_monitor_*: the open monitor (null: none), the developer override of its slice length (0 = automatic), and whether
    // filter steps bypass it (covahip_dev_graph_probe: a captured step must not carry a counted launch into its replays)
    CovahipMonitor *mon = nullptr;
    int mon_slice = 0;
    int in_flush = 0;   // samples between two flushes of the input kernel's workgroup counters; 0: its default (covahip_dev_input_flush)
    bool mon_suspended = false;
};

#define COVAHIP_CHECK_HIP(ctx, expr)                                                        \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) {                                                             \
            (ctx)->last_hip_error = std::string(#expr) + ": " + hipGetErrorString(_e);      \
            return COVAHIP_ERR_HIP;                                                         \
        }                                                                                   \
    } while (0)

template <typename T>
int ResidentTable<T>::reserve(covahip_ctx *ctx, size_t n) {
    if (n <= cap) return COVAHIP_OK;
    if (dev || pinned) {
        COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        hipFree(dev);
        hipHostFree(pinned);
        dev = pinned = nullptr;
        cap = 0;
        resident.clear();
    }
    if (!ev) COVAHIP_CHECK_HIP(ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    COVAHIP_CHECK_HIP(ctx, hipMalloc((void **)&dev, n * sizeof(T)));
    COVAHIP_CHECK_HIP(ctx, hipHostMalloc((void **)&pinned, n * sizeof(T), hipHostMallocDefault));
    cap = n;
    return COVAHIP_OK;
}

template <typename T>
int ResidentTable<T>::upload(covahip_ctx *ctx, const T *src, size_t n, const T **d_out) {
    *d_out = dev;
    if (n > cap) return COVAHIP_ERR_INVALID_ARG;
    if (n && resident.size() == n && std::equal(src, src + n, resident.begin())) return COVAHIP_OK;
    if (recorded) COVAHIP_CHECK_HIP(ctx, hipEventSynchronize(ev));   // the pinned copy is free again
    std::copy(src, src + n, pinned);
    COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(dev, pinned, n * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    resident.clear();   // (should the record fail, the device copy is no longer what it was)
    COVAHIP_CHECK_HIP(ctx, hipEventRecord(ev, ctx->stream));
    recorded = true;
    resident.assign(src, src + n);
    return COVAHIP_OK;
}

template <typename T>
void ResidentTable<T>::release() {
    if (dev) hipFree(dev);
    if (pinned) hipHostFree(pinned);
    if (ev) hipEventDestroy(ev);
    *this = ResidentTable<T>();
}

// Opens a kernel's dynamic LDS above the 64 KiB every kernel has (ctx.hip): sets the function's limit to `limit` bytes unless a
// limit of at least `lds` was set for this (device, function) before.  The attribute is sticky, so a launch path calls this
// with the launch's `lds` every time and pays a cache look-up.
int covahip_open_lds(covahip_ctx *ctx, const void *fn, size_t lds, size_t limit);
template <typename K>
int covahip_open_lds(covahip_ctx *ctx, K kernel, size_t lds, size_t limit) {
    return lds <= 64 * 1024 ? COVAHIP_OK : covahip_open_lds(ctx, reinterpret_cast<const void *>(kernel), lds, limit);
}

// RAII-less helpers: bracket a kernel launch with events when profiling is on.
struct ProfScope {
    covahip_ctx *ctx;
    int idx = -1;
    ProfScope(covahip_ctx *c, const char *name);
    ~ProfScope();
};

int covahip_ensure_buffer(covahip_ctx *ctx, void **buf, size_t *cur, size_t need);

// Places what follows on the next lane (see CtxLane above); re-entrant (an inner scope is a no-op).  `ok()` is false when a
// HIP call of the fork failed (ctx->last_hip_error says which).
struct LaneScope {
    covahip_ctx *ctx;
    bool owner = false, failed = false;
    explicit LaneScope(covahip_ctx *c);
    ~LaneScope();
    bool ok() const { return !failed; }
};
// Before anything is enqueued on the primary stream: the primary stream waits for every lane's last call.
int covahip_primary_op(covahip_ctx *ctx);
// Blocks until every lane and the primary stream have drained.
int covahip_sync_all(covahip_ctx *ctx);

// hostlib.cpp: CRC-32C (Castagnoli, reflected) of n bytes, the TFRecord checksum before masking
uint32_t covahip_crc32c(const uint8_t *p, size_t n);

// bboxcc.hip
// d_area: optional device array i32 [batch], frame b's own area threshold (null: area_thresh for every frame)
int covahip_bboxcc_launch(covahip_ctx *ctx, const uint8_t *d_mask, int batch, int h, int w, int area_thresh,
                          covahip_box *d_boxes, int32_t *d_counts, int max_boxes, const int32_t *d_area = nullptr);

// monitor.hip
// The hook at the end of a filter step that succeeded, on ctx->stream (the lane that ran the batch): sees the batch and, every
// `every`-th time, counts it with one launch.  Only called while an attached monitor is open and not suspended.
// in: the batch's input as the forward took it (blobnet.h), for the input statistics; null: the inputs are not counted.
struct BnInput;
int covahip_monitor_hook(covahip_ctx *ctx, const uint8_t *d_mask, const int32_t *d_counts, const covahip_box *d_boxes, int max_boxes,
                         const uint8_t *model_ids, int batch, const BnInput *in = nullptr);
// input_stats.hip: the counted batch's inputs by the batch's plan (monitor_tab.h), on ctx->stream; frees what set_inputs allocated
struct MonPlan;
int covahip_monitor_hook_inputs(covahip_ctx *ctx, CovahipMonitor *mon, const MonPlan &plan, const uint8_t *model_ids, const BnInput &in,
                                int batch);
void covahip_monitor_free_inputs(CovahipMonitor *mon);
void covahip_monitor_close(covahip_ctx *ctx, bool attached_only);   // drains the ctx and frees the monitor (if any)

// train_data.hip: what the trainer's data entry points (train.hip) need of a covahip_train_data
// Host check of n samples against the data set, the caller's ctx (null: any) and geometry: COVAHIP_OK or COVAHIP_ERR_INVALID_ARG.
int covahip_train_data_check(const covahip_train_data *d, const covahip_ctx *ctx, int h, int w, const covahip_train_sample *s,
                             int64_t n);
// The data set's pinned sample table, grown to n entries: the caller writes the samples of one launch there, in output order ...
int covahip_train_data_table(covahip_train_data *d, int n, covahip_train_sample **tab);
// ... and this uploads the first n and builds their stacks u8 [n][4h][w][4] and labels u8 [n][h][w] in device memory, on the ctx's
// stream.  The table is free again once the stream has passed the launch.
int covahip_train_data_launch(covahip_train_data *d, int n, uint8_t *d_stack, uint8_t *d_gt);

// label_mass.hip: d_mass[i] = the label mass of frame first + i of d_gt u8 [..][hw] for i in [0, n), n >= 1, in one launch on the
// ctx's stream.  d_bits: the keep map as a bit per macroblock, u32 [(hw + 31) / 32] (bit p & 31 of word p >> 5), or null: the
// form that reads none.
int covahip_label_mass_launch(covahip_ctx *ctx, const uint8_t *d_gt, const uint32_t *d_bits, uint32_t *d_mass, int64_t first,
                              int64_t n, int hw);

// train_align.hip: the alignment counts (covahip_train_data_align) of frames [at, at + m) of the recording [first, first + n) of
// d_rec u16 / d_gt u8 [capacity][hw], in one launch on the ctx's stream: d_both u32 [m][2 S + 1], d_mov and d_lab u32 [m].
// lut: bit (mv_x | mv_y << 3) = a record with these vectors moves; cmask: bit c = class c moves; d_bits as for the label mass.
int covahip_align_launch(covahip_ctx *ctx, const uint16_t *d_rec, const uint8_t *d_gt, int64_t capacity, const uint32_t *d_bits,
                         uint64_t lut, uint32_t cmask, int S, int64_t first, int64_t n, int64_t at, int64_t m, int hw,
                         uint32_t *d_both, uint32_t *d_mov, uint32_t *d_lab);

// blobnet.hip
void covahip_blobnet_destroy(covahip_ctx *ctx);
int covahip_blobnet_forward_dev(covahip_ctx *ctx, const uint8_t *d_stack, int batch, float *d_logits,
                                uint8_t *d_mask, const uint8_t *model_ids = nullptr);
int covahip_blobnet_geometry(covahip_ctx *ctx, int *h, int *w);
int covahip_blobnet_grow_lanes(covahip_ctx *ctx, int n_lanes);   // workspaces of lanes [0, n_lanes) of the loaded model
