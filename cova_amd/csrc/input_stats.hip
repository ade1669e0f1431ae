// Input statistics (include/covahip.h, "Input monitor"): what records a camera sends.  Per model of a monitor (covahip_monitor_
// set_inputs / add_inputs / read_inputs, and behind every counted batch of an attached monitor) or per call over resident
// training frames (covahip_train_data_record_stats, train_data.hip): a 512-bin histogram of the packed records, how often each
// macroblock moves, and per frame whether it is still, all intra, and how many macroblocks move.  Integer counts, exact, additive
// over batches, 64-bit on the device.
//
// Two launches per batch on the stream that ran it, by the batch's order / slice plan (monitor_tab.h: the one monitor_count ran by).
//   * input_count: a workgroup of IN_BLK lanes owns (a tile of IN_TILE consecutive macroblocks, one slice of samples of one
//     model).  Lane l takes macroblocks 8 l .. 8 l + 7 of the tile: one 16-byte load per sample for packed records, two for the
//     decoder's four bytes, eight label bytes in one load where there are labels (AL = 2: the source and the frame stride are on
//     16-byte boundaries); a record at a time where they are only on a record's boundary, and for the last lanes of a frame
//     (AL = 1: a training set of an odd h * w, a caller's pointer off 16 bytes); bytes off a record's boundary (AL = 0).
//       - Real records are almost all zero (2.6 % of a P picture's macroblocks move): a zero record bumps a REGISTER of its lane
//         and never reaches LDS; only non-zero records go through LDS atomics into the workgroup's 512 bins.  The registers are
//         reduced in the wave and added to bin 0 when the workgroup flushes.
//       - moving[p]: eight registers per lane, one per macroblock, across the slice's samples (monitor_count's tile x slice shape).
//       - per frame: (non-zero, moving, intra) of a lane's eight macroblocks packed as 10-bit fields of one word, summed over the
//         wave by shuffles (a wave has 512 macroblocks: no field passes 512), summed over the workgroup's waves through LDS once
//         per IN_GROUP samples, and added to the frame's partials in the batch's scratch, u64 {non-zero << 32 | moving} and
//         u64 {intra}: at most two atomics per workgroup and sample, none where its macroblocks are all skip.  (Two per WAVE put the
//         16 waves of a 68x120 frame on the same two words; what that cost was not established: DESIGN.md, "What was tried".)
//       - Counter widths.  Every workgroup counter is 32-bit.  Between two flushes a workgroup sees at most `flush` samples of
//         IN_TILE macroblocks, so no bin, no bin-0 register sum and no moving register passes flush * IN_TILE <= 2^20 * 2^11 = 2^31.
//         The workgroup flushes every `flush` samples and at the end of its slice: the moving registers through LDS, so that lane l
//         holds macroblocks l + 256 j and a wave's 64-bit atomics cover contiguous words; the bins, lane l bins l and l + 256.
//         flush is IN_FLUSH unless the developer sets it (covahip_dev_input_flush).
//   * input_finish: one wave per slice reads the partials of its samples, decides still / all intra / the move_hist bin, ZEROES the
//     partials (the scratch is zero between batches: no memset launch) and adds at most 3 + 16 words to the model's table.
// One workgroup per frame (no scratch, no second launch) was the alternative for small grids; it leaves moving[] to one global
// atomic per moving macroblock and sample, which is what uniform contents make of every macroblock.  DESIGN.md section 4, "Input monitor".
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "blobnet.h"
#include "covahip_dev.h"
#include "internal.h"
#include "monitor_tab.h"

namespace {

using ull = unsigned long long;
constexpr int IN_BLK = 256;
constexpr int IN_PER = 8;                       // macroblocks of a lane
constexpr int IN_TILE = IN_BLK * IN_PER;        // macroblocks of a workgroup
constexpr int IN_GROUP = 4;                     // samples between two sums of the per-frame partials over the workgroup
constexpr int IN_FLUSH = 1 << 20;               // samples between two flushes: IN_FLUSH * IN_TILE = 2^31 < 2^32
constexpr int IN_WGS_PER_CU = 4;                // workgroups the slicing aims at per CU
constexpr int IN_MIN_SLICE = 4;                 // fewer samples than this do not pay for a slice's flush
constexpr size_t IN_STAGE = (size_t)64 << 20;   // host frames are staged in pieces of at most this many bytes
constexpr int IN_O_HIST = IN_HEAD, IN_O_MOVE = IN_HEAD + IN_HIST, IN_O_MOVING = IN_HEAD + IN_HIST + IN_MOVE_BINS;

__device__ inline int in_frame(const InFrames &f, int b) {
    return f.by_value ? (int)f.val[b] : f.d_idx ? f.d_idx[(size_t)b * f.idx_stride] : b + f.off;
}
// the record of a macroblock's four bytes (byte 3 ignored): every field clipped at 6, as covahip_carrier_pack keeps it
__device__ inline uint32_t in_rec(uint32_t b0, uint32_t b1, uint32_t b2) { return min(b0, 6u) | min(b1, 6u) << 3 | min(b2, 6u) << 6; }
__device__ inline uint32_t in_rec(uint32_t v) { return in_rec(v & 255u, (v >> 8) & 255u, (v >> 16) & 255u); }

// tab / model_stride / set_hist / scratch: monitor_tab.h, InJob.  tiles = ceil(hw / IN_TILE); S slices; grid: tiles * S.
template <bool PACKED, int AL, bool LABELS, class TAB>
__global__ __launch_bounds__(IN_BLK) void input_count(const uint8_t *__restrict__ src, size_t stride, InFrames fr,
                                                      const uint8_t *__restrict__ labels, int n, int hw, int tiles, int S,
                                                      int flush, TAB t, ull *__restrict__ tab, size_t model_stride,
                                                      ull *__restrict__ set_hist, ull *__restrict__ scratch) {
    __shared__ uint32_t hist[IN_HIST];
    __shared__ uint32_t hset[LABELS ? IN_HIST : 1];
    __shared__ uint32_t mv[IN_TILE];
    __shared__ uint32_t part[2][IN_GROUP][IN_BLK / 64];
    int par = 0;
    const int tid = threadIdx.x;
    const int tile = blockIdx.x % tiles, s = blockIdx.x / tiles;
    int m, i0, i1;
    mon_slice(t, s, S, n, m, i0, i1);
    ull *mt = tab + (size_t)m * model_stride;
    const int p0 = tile * IN_TILE + tid * IN_PER;          // this lane's first macroblock
    const int cnt = max(0, min(IN_PER, hw - p0));          // and how many of its eight the frame has
    for (int k = tid; k < IN_HIST; k += IN_BLK) {
        hist[k] = 0;
        if (LABELS) hset[k] = 0;
    }
    __syncthreads();
    uint32_t moving[IN_PER] = {};
    uint32_t zeros = 0, zeros_set = 0;
    int since = 0;
    const bool whole = AL == 2 && cnt == IN_PER;               // this lane reads its eight macroblocks in whole loads
    for (int g0 = i0; g0 < i1; g0 += IN_GROUP) {           // a group: the samples between two workgroup sums of the partials
#pragma unroll
        for (int u = 0; u < IN_GROUP; u++) {
            const int i = g0 + u;
            if (i >= i1) break;                            // (uniform over the workgroup)
            const int f = in_frame(fr, mon_sample(t, S, i));
            const uint8_t *fp = src + (size_t)f * stride;
            uint32_t r[IN_PER];
            uint32_t lab = 0;                              // bit k: macroblock k's label is set
            if (whole) {
                const uint4 *q = reinterpret_cast<const uint4 *>(fp + (size_t)p0 * (PACKED ? 2 : 4));
                if (PACKED) {
                    const uint4 v = q[0];
                    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int j = 0; j < IN_PER; j++) r[j] = (w[j >> 1] >> (16 * (j & 1))) & 511u;
                } else {
                    const uint4 v = q[0], v2 = q[1];
                    const uint32_t w[8] = {v.x, v.y, v.z, v.w, v2.x, v2.y, v2.z, v2.w};
#pragma unroll
                    for (int j = 0; j < IN_PER; j++) r[j] = in_rec(w[j]);
                }
                if (LABELS) {
                    const uint2 g = *reinterpret_cast<const uint2 *>(labels + (size_t)f * hw + p0);
                    const uint32_t w[2] = {g.x, g.y};
#pragma unroll
                    for (int j = 0; j < IN_PER; j++) lab |= (uint32_t)(((w[j >> 2] >> (8 * (j & 3))) & 255u) != 0) << j;
                }
            } else {
#pragma unroll
                for (int k = 0; k < IN_PER; k++) {
                    r[k] = 0;
                    if (k < cnt) {
                        const size_t p = (size_t)(p0 + k);
                        if (PACKED) r[k] = (AL ? (uint32_t)reinterpret_cast<const uint16_t *>(fp)[p] : (uint32_t)fp[2 * p] | (uint32_t)fp[2 * p + 1] << 8) & 511u;
                        else r[k] = AL ? in_rec(reinterpret_cast<const uint32_t *>(fp)[p]) : in_rec(fp[4 * p], fp[4 * p + 1], fp[4 * p + 2]);
                        if (LABELS) lab |= (uint32_t)(labels[(size_t)f * hw + p] != 0) << k;
                    }
                }
            }
            uint32_t nz = 0, nm = 0, ni = 0;
#pragma unroll
            for (int k = 0; k < IN_PER; k++) {
                if (k < cnt) {
                    const uint32_t x = r[k];
                    if (x) {
                        atomicAdd(&hist[x], 1u);
                        nz++;
                    } else {
                        zeros++;
                    }
                    const uint32_t mk = (x & 0x1F8u) != 0;
                    moving[k] += mk;
                    nm += mk;
                    ni += (x & 7u) >= 5u;
                    if (LABELS && (lab >> k & 1u)) {
                        if (x) atomicAdd(&hset[x], 1u);
                        else zeros_set++;
                    }
                }
            }
            // the frame's partials: three 10-bit fields, at most 8 a lane and 512 a wave; lane 0 leaves the wave's for the workgroup
            uint32_t pk = nz | nm << 10 | ni << 20;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) pk += __shfl_xor(pk, o, 64);
            if ((tid & 63) == 0) part[par][u][tid >> 6] = pk;
            if (++since == flush || i + 1 == i1) {         // (uniform over the workgroup)
                since = 0;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    zeros += __shfl_xor(zeros, o, 64);
                    if (LABELS) zeros_set += __shfl_xor(zeros_set, o, 64);
                }
                if ((tid & 63) == 0) {
                    if (zeros) atomicAdd(&hist[0], zeros);
                    if (LABELS && zeros_set) atomicAdd(&hset[0], zeros_set);
                }
                zeros = zeros_set = 0;
#pragma unroll
                for (int k = 0; k < IN_PER; k++) {
                    mv[tid * IN_PER + k] = moving[k];
                    moving[k] = 0;
                }
                __syncthreads();
#pragma unroll
                for (int j = 0; j < IN_PER; j++) {
                    const int q = tid + IN_BLK * j, mb = tile * IN_TILE + q;
                    const uint32_t v = mv[q];
                    if (mb < hw && v) atomicAdd(mt + IN_O_MOVING + mb, (ull)v);
                }
                for (int k = tid; k < IN_HIST; k += IN_BLK) {
                    const uint32_t v = hist[k];
                    if (v) atomicAdd(mt + IN_O_HIST + k, (ull)v);
                    hist[k] = 0;
                    if (LABELS) {
                        const uint32_t w = hset[k];
                        if (w) atomicAdd(set_hist + k, (ull)w);
                        hset[k] = 0;
                    }
                }
                __syncthreads();
            }
        }
        // one lane per sample of the group adds the workgroup's partials to the frame's: same-address atomics are what the L2
        // serialises, so a frame gets two per workgroup instead of two per wave.  `part` alternates between two buffers, so one
        // barrier per group orders both its writes against these reads and these reads against the writes two groups on.
        __syncthreads();
        if (tid < IN_GROUP && g0 + tid < i1) {
            uint32_t wz = 0, wm = 0, wi = 0;
#pragma unroll
            for (int v = 0; v < IN_BLK / 64; v++) {
                const uint32_t pk = part[par][tid][v];
                wz += pk & 1023u, wm += (pk >> 10) & 1023u, wi += pk >> 20;
            }
            const size_t b = (size_t)mon_sample(t, S, g0 + tid);
            if (wz | wm) atomicAdd(scratch + 2 * b, (ull)wz << 32 | wm);
            if (wi) atomicAdd(scratch + 2 * b + 1, (ull)wi);
        }
        par ^= 1;
    }
}

// grid: S workgroups of one wave
template <class TAB>
__global__ __launch_bounds__(64) void input_finish(int n, int hw, int S, TAB t, ull *__restrict__ tab, size_t model_stride,
                                                   ull *__restrict__ scratch) {
    __shared__ uint32_t mh[IN_MOVE_BINS];
    const int lane = threadIdx.x, s = blockIdx.x;
    int m, i0, i1;
    mon_slice(t, s, S, n, m, i0, i1);
    ull *mt = tab + (size_t)m * model_stride;
    if (lane < IN_MOVE_BINS) mh[lane] = 0;
    __syncthreads();
    int still = 0, intra = 0;
    for (int i = i0 + lane; i < i1; i += 64) {
        const size_t b = (size_t)mon_sample(t, S, i);
        const ull a = scratch[2 * b], c = scratch[2 * b + 1];
        scratch[2 * b] = 0;
        scratch[2 * b + 1] = 0;
        const uint32_t nz = (uint32_t)(a >> 32), nm = (uint32_t)a;
        still += nz == 0;
        intra += c == (ull)hw;
        atomicAdd(&mh[nm == 0 ? 0 : min(IN_MOVE_BINS - 1, 32 - __clz(nm))], 1u);   // 1 + floor(log2 nm)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        still += __shfl_xor(still, o, 64);
        intra += __shfl_xor(intra, o, 64);
    }
    __syncthreads();
    if (lane == 0) {
        if (i1 > i0) atomicAdd(mt + 0, (ull)(i1 - i0));
        if (still) atomicAdd(mt + 1, (ull)still);
        if (intra) atomicAdd(mt + 2, (ull)intra);
    }
    if (lane < IN_MOVE_BINS && mh[lane]) atomicAdd(mt + IN_O_MOVE + lane, (ull)mh[lane]);
}

template <bool PACKED, int AL, bool LABELS, class TAB>
void launch_count(covahip_ctx *ctx, const InJob &j, int n, int tiles, int S, int flush, const TAB &t) {
    hipLaunchKernelGGL((input_count<PACKED, AL, LABELS, TAB>), dim3((unsigned)(tiles * S)), dim3(IN_BLK), 0, ctx->stream, j.src,
                       j.stride, j.frames, j.labels, n, j.hw, tiles, S, flush, t, j.tab, j.model_stride, j.set_hist, j.scratch);
}
template <bool PACKED, bool LABELS, class TAB>
void launch_al(covahip_ctx *ctx, const InJob &j, int al, int n, int tiles, int S, int flush, const TAB &t) {
    if (al == 2) launch_count<PACKED, 2, LABELS>(ctx, j, n, tiles, S, flush, t);
    else if (al == 1) launch_count<PACKED, 1, LABELS>(ctx, j, n, tiles, S, flush, t);
    else launch_count<PACKED, 0, LABELS>(ctx, j, n, tiles, S, flush, t);
}
template <class TAB>
int launch_both(covahip_ctx *ctx, const InJob &j, int n, int S, const TAB &t) {
    const int tiles = (j.hw + IN_TILE - 1) / IN_TILE;
    const int flush = ctx->in_flush > 0 ? ctx->in_flush : IN_FLUSH;
    // how every frame of the source may be read: 2 = 16 bytes at a time (a lane whose eight macroblocks end behind the frame reads
    // records), 1 = a record at a time (4-byte records on a 4-byte boundary, 2-byte records on a 2-byte boundary), 0 = bytes
    const uintptr_t at = reinterpret_cast<uintptr_t>(j.src), rec = j.packed ? 2 : 4;
    int al = at % rec || j.stride % rec ? 0 : at % 16 || j.stride % 16 ? 1 : 2;
    if (al == 2 && j.labels && ((reinterpret_cast<uintptr_t>(j.labels) & 7) || j.hw % 8)) al = 1;   // (eight label bytes in one load)
    {
        ProfScope ps(ctx, "input_count");
        if (j.labels) launch_al<true, true>(ctx, j, al, n, tiles, S, flush, t);
        else if (j.packed) launch_al<true, false>(ctx, j, al, n, tiles, S, flush, t);
        else launch_al<false, false>(ctx, j, al, n, tiles, S, flush, t);
        COVAHIP_CHECK_HIP(ctx, hipGetLastError());
    }
    ProfScope ps(ctx, "input_finish");
    hipLaunchKernelGGL((input_finish<TAB>), dim3((unsigned)S), dim3(64), 0, ctx->stream, n, j.hw, S, t, j.tab, j.model_stride, j.scratch);
    COVAHIP_CHECK_HIP(ctx, hipGetLastError());
    return COVAHIP_OK;
}

// n device-resident samples of a stand-alone monitor, in launch pairs of at most IN_CHUNK, on the primary stream.  Sample b's frame:
// frames[b] (host, validated) or b + off.
int count_device(covahip_ctx *ctx, CovahipMonitor *mon, const uint8_t *d_src, bool packed, size_t stride, const int32_t *frames, int off,
                 const uint8_t *model_ids, int n) {
    const int hw = mon->h * mon->w;
    for (int s0 = 0; s0 < n; s0 += IN_CHUNK) {
        const int c = std::min(IN_CHUNK, n - s0);
        MonPlan plan;
        if (int rc = covahip_input_plan(ctx, mon->lane[0], hw, model_ids ? model_ids + s0 : nullptr, c, &plan)) return rc;
        InJob j;
        j.src = d_src;
        j.packed = packed;
        j.stride = stride;
        j.hw = hw;
        j.tab = mon->d_in;
        j.model_stride = covahip_input_words((size_t)hw);
        j.scratch = mon->in_scratch[0];
        if (!frames) {
            j.frames.off = off + s0;
        } else {
            const int32_t *f = frames + s0;
            if (c <= MON_KTAB && *std::max_element(f, f + c) <= 65535) {
                j.frames.by_value = 1;
                for (int b = 0; b < c; b++) j.frames.val[b] = (uint16_t)f[b];
            } else if (int rc = mon->in_frames.upload(ctx, f, (size_t)c, &j.frames.d_idx)) {
                return rc;
            }
        }
        if (int rc = covahip_input_count(ctx, j, plan, c)) return rc;
    }
    return COVAHIP_OK;
}

}  // namespace

int covahip_input_plan(covahip_ctx *ctx, MonTable &tb, int hw, const uint8_t *model_ids, int n, MonPlan *plan) {
    return covahip_monitor_plan(ctx, tb, (hw + IN_TILE - 1) / IN_TILE, IN_WGS_PER_CU, IN_MIN_SLICE, model_ids, n, plan);
}

int covahip_input_count(covahip_ctx *ctx, const InJob &job, const MonPlan &plan, int n) {
    if (job.labels && (!job.packed || plan.kind != MonPlan::UNIFORM)) return COVAHIP_ERR_INVALID_ARG;
    const int rc = plan.kind == MonPlan::UNIFORM    ? launch_both(ctx, job, n, plan.S, plan.u)
                   : plan.kind == MonPlan::BY_VALUE ? launch_both(ctx, job, n, plan.S, plan.v)
                                                    : launch_both(ctx, job, n, plan.S, plan.p);
    // only input_finish leaves the partials zero: where a launch of the pair failed, the next batch must not inherit them
    if (rc) (void)hipMemsetAsync(job.scratch, 0, (size_t)n * 2 * sizeof(ull), ctx->stream);
    return rc;
}

int covahip_monitor_hook_inputs(covahip_ctx *ctx, CovahipMonitor *mon, const MonPlan &mon_plan, const uint8_t *model_ids,
                                const BnInput &in, int batch) {
    if (batch > mon->in_samples) return COVAHIP_ERR_INVALID_ARG;   // (set_inputs reserved the loaded model's max_batch)
    const int hw = mon->h * mon->w;
    // monitor_count's plan where it lies in the lane's table (a mixed batch beyond MON_KTAB: nothing more is uploaded), else a
    // plan of the input kernel's own, which costs the host a counting sort and travels in the arguments
    MonPlan plan = mon_plan;
    if (mon_plan.kind != MonPlan::BY_PTR)
        if (int rc = covahip_input_plan(ctx, mon->lane[ctx->cur_lane], hw, model_ids, batch, &plan)) return rc;
    InJob j;
    j.hw = hw;
    j.tab = mon->d_in;
    j.model_stride = covahip_input_words((size_t)hw);
    j.scratch = mon->in_scratch[ctx->cur_lane];
    if (in.stack) {   // the counted frame of stack b is its row block 0
        j.src = in.stack;
        j.stride = (size_t)BN_T * hw * 4;
    } else {
        j.src = in.frames;
        j.packed = in.packed;
        j.stride = (size_t)hw * (in.packed ? 2 : 4);
        if (in.h_index) {   // the table travelled by value: so does the frame list, from the same host copy
            j.frames.by_value = 1;
            for (int b = 0; b < batch; b++) j.frames.val[b] = (uint16_t)in.h_index[(size_t)b * BN_T];
        } else {
            j.frames.d_idx = in.index;
            j.frames.idx_stride = BN_T;
        }
    }
    return covahip_input_count(ctx, j, plan, batch);
}

void covahip_monitor_free_inputs(CovahipMonitor *mon) {
    if (mon->d_in) hipFree(mon->d_in);
    mon->d_in = nullptr;
    mon->in_words = 0;
    for (ull *&p : mon->in_scratch) {
        if (p) hipFree(p);
        p = nullptr;
    }
    mon->in_samples = 0;
    mon->in_frames.release();
}

extern "C" {

int covahip_monitor_set_inputs(covahip_ctx *ctx, int on) {
    if (!ctx || !ctx->mon || (on != 0 && on != 1)) return COVAHIP_ERR_INVALID_ARG;
    CovahipMonitor *mon = ctx->mon;
    if (mon->attached && !ctx->blobnet) return COVAHIP_ERR_NOT_LOADED;
    COVAHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = covahip_sync_all(ctx)) return rc;   // nothing in flight adds to the tables
    if ((mon->d_in != nullptr) == (on != 0)) return COVAHIP_OK;
    if (!on) {
        covahip_monitor_free_inputs(mon);
        return COVAHIP_OK;
    }
    const size_t words = (size_t)mon->n_models * covahip_input_words((size_t)mon->h * mon->w);
    const int samples = mon->attached ? ctx->blobnet->max_batch : IN_CHUNK;
    const size_t sbytes = (size_t)samples * 2 * sizeof(ull);
    bool ok = hipMalloc((void **)&mon->d_in, words * sizeof(ull)) == hipSuccess &&
              hipMemsetAsync(mon->d_in, 0, words * sizeof(ull), ctx->primary) == hipSuccess;
    for (int k = 0; k < (mon->attached ? COVAHIP_MAX_LANES : 1) && ok; k++)
        ok = hipMalloc((void **)&mon->in_scratch[k], sbytes) == hipSuccess &&
             hipMemsetAsync(mon->in_scratch[k], 0, sbytes, ctx->primary) == hipSuccess;
    ok = ok && hipStreamSynchronize(ctx->primary) == hipSuccess;
    if (ok && !mon->attached) ok = mon->in_frames.reserve(ctx, IN_CHUNK) == COVAHIP_OK;
    if (!ok) {
        ctx->last_hip_error = "covahip_monitor_set_inputs: allocation failed";
        (void)hipGetLastError();
        covahip_monitor_free_inputs(mon);
        return COVAHIP_ERR_HIP;
    }
    mon->in_words = words;
    mon->in_samples = samples;
    return COVAHIP_OK;
}

int covahip_monitor_get_inputs(covahip_ctx *ctx, int *on) {
    if (!ctx || !ctx->mon || !on) return COVAHIP_ERR_INVALID_ARG;
    *on = ctx->mon->d_in != nullptr;
    return COVAHIP_OK;
}

int covahip_monitor_add_inputs(covahip_ctx *ctx, const void *src, int form, int n_frames, const int32_t *stack_index, int batch,
                               const uint8_t *model_ids, int mem_kind) {
    if (!ctx || !ctx->mon || ctx->mon->attached || !ctx->mon->d_in) return COVAHIP_ERR_INVALID_ARG;
    CovahipMonitor *mon = ctx->mon;
    if (form != COVAHIP_INPUT_STACKED && form != COVAHIP_INPUT_FRAMES && form != COVAHIP_INPUT_PACKED) return COVAHIP_ERR_INVALID_ARG;
    if (batch < 0 || (batch > 0 && !src)) return COVAHIP_ERR_INVALID_ARG;
    if (mem_kind != COVAHIP_MEM_HOST && mem_kind != COVAHIP_MEM_DEVICE) return COVAHIP_ERR_INVALID_ARG;
    if (model_ids)
        for (int b = 0; b < batch; b++)
            if (model_ids[b] >= mon->n_models) return COVAHIP_ERR_INVALID_ARG;
    if (batch == 0) return COVAHIP_OK;
    const bool stacked = form == COVAHIP_INPUT_STACKED, packed = form == COVAHIP_INPUT_PACKED;
    std::vector<int32_t> frames;   // the counted frame of every stack: the newest slice
    if (!stacked) {
        if (n_frames < BN_T) return COVAHIP_ERR_INVALID_ARG;
        if (!stack_index && batch != n_frames - (BN_T - 1)) return COVAHIP_ERR_INVALID_ARG;
        frames.resize((size_t)batch);
        for (int b = 0; b < batch; b++)
            for (int t = 0; t < BN_T; t++) {
                const int32_t f = stack_index ? stack_index[(size_t)b * BN_T + t] : b + (BN_T - 1) - t;
                if (f < 0 || f >= n_frames) return COVAHIP_ERR_INVALID_ARG;
                if (t == 0) frames[b] = f;
            }
    }
    COVAHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int prc = covahip_primary_op(ctx)) return prc;   // on the primary stream, behind all lanes
    const size_t hw = (size_t)mon->h * mon->w;
    const size_t fbytes = hw * (packed ? 2 : 4);
    const uint8_t *p = static_cast<const uint8_t *>(src);
    if (mem_kind == COVAHIP_MEM_DEVICE) {
        int rc;
        if (stacked) rc = count_device(ctx, mon, p, false, BN_T * fbytes, nullptr, 0, model_ids, batch);
        else if (!stack_index) rc = count_device(ctx, mon, p, packed, fbytes, nullptr, BN_T - 1, model_ids, batch);
        else rc = count_device(ctx, mon, p, packed, fbytes, frames.data(), 0, model_ids, batch);
        if (rc) return rc;
    } else if (stacked) {   // staged in pieces of whole samples, row block 0 of every stack only
        const int piece = (int)std::min<size_t>((size_t)batch, std::max<size_t>(1, IN_STAGE / fbytes));
        if (int rc = covahip_ensure_buffer(ctx, &ctx->stage_in, &ctx->stage_in_bytes, (size_t)piece * fbytes)) return rc;
        for (int s0 = 0; s0 < batch; s0 += piece) {
            const int c = std::min(piece, batch - s0);
            COVAHIP_CHECK_HIP(ctx, hipMemcpy2DAsync(ctx->stage_in, fbytes, p + (size_t)s0 * BN_T * fbytes, BN_T * fbytes, fbytes, (size_t)c,
                                                    hipMemcpyHostToDevice, ctx->stream));
            if (int rc = count_device(ctx, mon, (const uint8_t *)ctx->stage_in, false, fbytes, nullptr, 0, model_ids ? model_ids + s0 : nullptr, c))
                return rc;
            COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the staging is written again by the next piece
        }
    } else {   // staged in pieces of whole frames; a piece counts the stacks whose newest slice lies in it
        const int piece = (int)std::min<size_t>((size_t)n_frames, std::max<size_t>(1, IN_STAGE / fbytes));
        if (int rc = covahip_ensure_buffer(ctx, &ctx->stage_in, &ctx->stage_in_bytes, (size_t)piece * fbytes)) return rc;
        std::vector<int32_t> sel;
        std::vector<uint8_t> ids;
        for (int f0 = 0; f0 < n_frames; f0 += piece) {
            const int f1 = std::min(n_frames, f0 + piece);
            sel.clear();
            ids.clear();
            for (int b = 0; b < batch; b++)
                if (frames[b] >= f0 && frames[b] < f1) {
                    sel.push_back(frames[b] - f0);
                    if (model_ids) ids.push_back(model_ids[b]);
                }
            if (sel.empty()) continue;
            COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(ctx->stage_in, p + (size_t)f0 * fbytes, (size_t)(f1 - f0) * fbytes, hipMemcpyHostToDevice, ctx->stream));
            if (int rc = count_device(ctx, mon, (const uint8_t *)ctx->stage_in, packed, fbytes, sel.data(), 0, model_ids ? ids.data() : nullptr,
                                      (int)sel.size()))
                return rc;
            COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        }
    }
    COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the caller may overwrite its arrays
    return COVAHIP_OK;
}

int covahip_monitor_read_inputs(covahip_ctx *ctx, int reset, int64_t *in_frames, int64_t *hist, int64_t *moving, int64_t *still_frames,
                                int64_t *intra_frames, int64_t *move_hist) {
    if (!ctx || !ctx->mon || !ctx->mon->d_in) return COVAHIP_ERR_INVALID_ARG;
    CovahipMonitor *mon = ctx->mon;
    COVAHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = covahip_sync_all(ctx)) return rc;   // everything in flight on all lanes has been counted
    if (int prc = covahip_primary_op(ctx)) return prc;
    const size_t M = mon->n_models, hw = (size_t)mon->h * mon->w, per = covahip_input_words(hw);
    if (in_frames || hist || moving || still_frames || intra_frames || move_hist) {
        std::vector<int64_t> host(mon->in_words);
        COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(host.data(), mon->d_in, mon->in_words * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
        COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (size_t m = 0; m < M; m++) {
            const int64_t *t = host.data() + m * per;
            if (in_frames) in_frames[m] = t[0];
            if (still_frames) still_frames[m] = t[1];
            if (intra_frames) intra_frames[m] = t[2];
            if (hist) std::copy(t + IN_O_HIST, t + IN_O_HIST + IN_HIST, hist + m * IN_HIST);
            if (move_hist) std::copy(t + IN_O_MOVE, t + IN_O_MOVE + IN_MOVE_BINS, move_hist + m * IN_MOVE_BINS);
            if (moving) std::copy(t + IN_O_MOVING, t + IN_O_MOVING + hw, moving + m * hw);
        }
    }
    if (reset) {
        COVAHIP_CHECK_HIP(ctx, hipMemsetAsync(mon->d_in, 0, mon->in_words * sizeof(ull), ctx->stream));
        COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return COVAHIP_OK;
}

// Developer switch (include/covahip_dev.h): samples between two flushes of input_count's workgroup counters, 0 = the default.
int covahip_dev_input_flush(covahip_ctx *ctx, int samples) {
    if (!ctx || samples < 0 || samples > IN_FLUSH) return COVAHIP_ERR_INVALID_ARG;
    ctx->in_flush = samples;
    return COVAHIP_OK;
}

}  // extern "C"
