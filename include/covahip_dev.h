/*
 * covahip_dev.h -- developer switches of libcovahip.so.  NOT part of the drop-in boundary
 * (include/covahip.h): used by tools/ and tests/ only, may change or disappear between builds.
 */
#ifndef COVAHIP_DEV_H
#define COVAHIP_DEV_H

#include "covahip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Kernel chain of the loaded model: 1 = default, 4 = decoder blocks 0..2 as three launches instead of one (the form
 * before the fused decoder; measured slower on MI355X, kept because it is the fallback for grids whose three decoder
 * tiles do not fit in LDS together, and tests compare the two bit for bit).  (2 and 3 were single-launch forms of encoder
 * levels 0 + 1, measured slower and removed in round 3; DESIGN.md has their numbers.)  5 = encoder level 1 on the
 * round-1..3 kernel (32x32x16 products, swizzled LDS band, LDS-DMA) instead of enc1_mfma (16x16x32 products, affine band,
 * round 4): the fallback for grids wider than enc1_mfma's fixed LDS row, and the A/B partner.  6 = encoder levels 2 and 3
 * on the general tiles (eight consecutive windows of a band) instead of the row-aligned ones (eight windows of one window
 * row, fragment addresses from per-kernel lane constants; round 4), which are the default where the geometry suits them. */
int covahip_blobnet_set_impl(covahip_ctx *ctx, int impl);

/* bboxcc kernel choice: cap > 0 = run capacity of the wave-per-frame kernel's first pass (frames with more runs get a
 * second chance at four times the capacity, then the workgroup kernel), cap < 0 = workgroup-per-frame kernel only,
 * 0 = automatic (default: 128; 192, 256 or 512 when more than a quarter of the previous call's frames on the lane had more
 * than 128, 192 or 256 runs, counted on one frame in sixteen). */
int covahip_bboxcc_set_wave_cap(covahip_ctx *ctx, int cap);
/* Overflow statistics of the last large-batch covahip_bboxcc call (device pointers): out4 = {batch, frames that overflowed
 * pass 1, frames that overflowed pass 2 too, capacity of pass 1}; batch = 0 when that call ran a kernel that cannot
 * overflow.  When that call ran no second-chance pass (skipped because the call before it had no overflow, or not planned
 * because four waves at four times the capacity do not fit LDS), pass 3 labelled every frame that overflowed pass 1, and
 * those count as having overflowed pass 2 too: out4[2] = out4[1].  Synchronises the ctx.  (tools/bboxcc_sweep.py) */
int covahip_dev_bboxcc_overflow(covahip_ctx *ctx, int32_t *out4);

/* Encoder band plan of level 1..3 (tools/plan_sweep.sh): nbands bands of pool-window rows per frame, nbuf = 1 or 2 LDS
 * buffers (2 = the next band is requested while this one is computed; measured no faster).  nbands = 0
 * restores the automatic plan.  A plan that does not fit in LDS makes the next forward call return
 * COVAHIP_ERR_UNSUPPORTED. */
int covahip_blobnet_set_enc_plan(covahip_ctx *ctx, int level, int nbands, int nbuf);

/* Device pointer, byte size and dims of one activation buffer of lane 0's BlobNet workspace (the buffers the primary-stream calls
 * write; layouts: BnWorkspace in cova_amd/csrc/blobnet.h): which = 0 P (pooled level 0 per carrier frame, index 0), 1 act[index]
 * (1..4), 2 dact[index] (0..2), 3 part (fp32 partial logits, index 0).  dims: up to 5, unused = 0; a buffer not allocated yet
 * gives a null pointer, 0 bytes and all-zero dims.  No synchronisation: the caller reads it after the forward it inspects has
 * finished.  (tests/test_gpu_stages.py) */
int covahip_dev_blobnet_buffer(covahip_ctx *ctx, int which, int index, void **dptr, size_t *bytes, int32_t dims[5]);

/* Shader clock (MHz) the chip holds right now: one wave runs a dependent chain for about busy_us microseconds on a stream
 * of its own -- beside whatever the ctx has in flight -- and brackets it with s_memtime / s_memrealtime
 * (MI355X_MICROARCH.md, DVFS give-back).  bench.py prints it so that step times of different boxes can be compared. */
int covahip_dev_clock_mhz(covahip_ctx *ctx, int busy_us, float *mhz);

/* The same carrier-frame step (device pointers, one lane) `iters` times as stream launches and as launches of ONE captured HIP
 * graph of it: total milliseconds of each.  Synchronises the ctx.  (tools/graph_probe.py) */
int covahip_dev_graph_probe(covahip_ctx *ctx, const uint8_t *d_frames, int n_frames, const int32_t *stack_index, int batch,
                            int area_thresh, covahip_box *d_boxes, int32_t *d_counts, int max_boxes, uint8_t *d_mask, int iters,
                            float *ms_direct, float *ms_graph);

/* Which kernel ran the last decoder block of the ctx's last BlobNet forward (the launch names of the profile do not tell the
 * fused forms apart): ALONE = dec_mfma<.., FINAL> (no bboxcc in the launch), ROWS = dec3cc_rows_mfma, BANDS + 2 * WV + PART =
 * dec3cc_mfma<WV, PART> (WV: the run-based bboxcc body, PART: partial logits instead of the skip tensor).  0: no forward yet. */
#define COVAHIP_DEV_TAIL_ALONE 1
#define COVAHIP_DEV_TAIL_ROWS 2
#define COVAHIP_DEV_TAIL_BANDS 4
int covahip_dev_blobnet_tail_form(covahip_ctx *ctx, int *form);
/* Whether the ctx's last BlobNet forward ran the last decoder block INSIDE the decoder launch (dec012_mfma ending in bboxcc's
 * parity planes, "dec3_bboxcc_fused" then being bboxcc alone on those planes: cc_planes) -- 1 -- or as a launch of its own -- 0.
 * tail_form reads ROWS in both cases: it is the row tail's text that runs.  covahip_blobnet_set_impl 11 takes that form wherever
 * its geometry allows it (single model, no per-model post-processing), 12 never; the default takes it when the batch fills the
 * chip and the call does not ask for the logits. */
int covahip_dev_blobnet_tail_in_dec012(covahip_ctx *ctx, int *in_dec012);

/* What covahip_pipe_create's hardware-queue probe decided (pipe.hip, round 6): how many of the ctx's ACTIVE lanes share a hardware
 * queue with the pipe's upload stream / with its result stream.  0 / <= 1 with up to three lanes on the default four queues. */
struct covahip_pipe;
int covahip_dev_pipe_queue_plan(struct covahip_pipe *pipe, int *lanes_on_upload_queue, int *lanes_on_result_queue);

/* MoG labels (covahip_mog_apply) of the last call, expanded from its bit planes: raw = the MOG2 mask (0 / 255) and filled = the
 * mask after close, open and hole fill (0 / 1), each u8 [n_frames][n_streams][work_h][work_w] of the labeller's own working size
 * (covahip_mog_dims; 360 x 640 on the reference grid) (either may be NULL; cap = bytes of each; COVAHIP_ERR_OVERFLOW when too small).  *n_frames = that call's n_frames.  Frames past a stream's n_valid hold nothing
 * meaningful.  Where that call ran with shadow detection on (covahip_mog_set_shadows, a mode other than COVAHIP_MOG_SHADOWS_OFF)
 * raw is OpenCV's three-valued mask, 0 / 127 / 255 with 127 = shadow, in _DROP and in _KEEP mode alike; filled is 0 / 1 as ever.
 * (tests/test_gpu_mog.py, tests/test_gpu_mog_shadow.py) */
struct covahip_mog;
int covahip_dev_mog_masks(struct covahip_mog *m, uint8_t *raw, uint8_t *filled, size_t cap, int *n_frames);
/* One stream's model: W f32 [5][P], V f32 [5][P], M f32 [5][3][P], nmodes u8 [P] and n (frames seen), P = work_w * work_h of
 * the labeller (covahip_mog_dims; 230400 on the reference grid); any pointer may be NULL. */
int covahip_dev_mog_state(struct covahip_mog *m, int stream, float *W, float *V, float *M, uint8_t *nmodes, int64_t *n);
/* Device bytes of host frames that covahip_mog_apply (COVAHIP_MEM_HOST) stages per update launch; 0 restores the default of
 * 1 GiB.  A call whose frames exceed it runs as several update launches of whole frame-steps (one frame of every stream), at
 * least one per launch; the results do not depend on it.  (tests/test_gpu_mog_branches.py) */
int covahip_dev_mog_set_stage_budget(struct covahip_mog *m, size_t bytes);
/* The labeller's post launch (close, open, hole fill, labels) on given masks instead of MOG2's: raw u8
 * [n_frames][n_streams][work_h][work_w], non-zero = foreground, is packed into bit planes on the host and uploaded as the call's
 * raw planes; labels u8 [n_frames][n_streams][label_h][label_w] (host memory) come back, and covahip_dev_mog_masks then reads the
 * raw / filled masks of this call.  The model and the frame counts are untouched.  Works for every labeller, in the label mode
 * of covahip_mog_set_labels.  (tests/test_gpu_mog_band.py, tests/test_gpu_mog_cover.py) */
int covahip_dev_mog_post_masks(struct covahip_mog *m, const uint8_t *raw, int n_frames, uint8_t *labels);
/* Which post kernel a macroblock-grid labeller runs.  banded = 1: the banded kernel of mog_band.hip, which labellers of
 * 2560x1440 and 3840x2160 sources always run and a 1920x1080 one (960x540 working) runs only through this switch, to be compared
 * with its resident kernel on the same planes; band_rows = 0 is the automatic plan (covahip_dev_mog_band_plan), otherwise the band
 * height, 16 .. work_h, whose staged window must fit LDS.  banded = 0 (band_rows = 0): the resident kernel.
 * COVAHIP_ERR_INVALID_ARG outside those ranges, for banded = 0 on a labeller that has no resident kernel and for banded = 1 on
 * one that has no banded kernel (the reference grid, 320x180).  The results do not depend on it.  A labeller of
 * covahip_mog_create_any has the banded form only (mog_any.hip), with the window's rows at work_w rounded up to 64.  These
 * entries, covahip_dev_mog_masks and covahip_dev_mog_state take such a labeller too, and give and take masks and model in the
 * working image's own [work_h][work_w] order whatever pitch the device uses. */
int covahip_dev_mog_set_post_form(struct covahip_mog *m, int banded, int band_rows);
/* The automatic band plan of a working size (a multiple of 64 wide): `bands` bands of `rows` rows (the last may be shorter), as
 * few as fit, and the dynamic LDS of the launch: two planes of min(rows + 16, work_h) rows, 16 bytes of flags and 256 bytes per 64 columns for the column sweep, at most
 * 160 KiB - 64 B.  Any pointer may be NULL.  Pure host code: no GPU call. */
int covahip_dev_mog_band_plan(int work_w, int work_h, int *rows, int *bands, size_t *lds_bytes);

/* Serving monitor (covahip_monitor_*): samples per slice of its kernel; 0 restores the automatic choice (enough workgroups for
 * every CU, at least 16 samples).  The counts do not depend on it; a slice longer than 255 samples makes the kernel's packed
 * byte counters spill, which the automatic choice reaches only with batches of thousands.  (tests/test_gpu_monitor.py) */
int covahip_dev_monitor_slice(covahip_ctx *ctx, int samples);
/* Input monitor (covahip_monitor_set_inputs, covahip_train_data_record_stats): its kernel runs by the slices of
 * covahip_dev_monitor_slice and flushes a workgroup's 32-bit counters into the 64-bit tables every `samples` samples of a slice
 * and at the slice's end; 0 restores the default of 2^20 (times the 2,048 macroblocks of a workgroup: 2^31, no counter wraps),
 * which no batch reaches.  COVAHIP_ERR_INVALID_ARG outside 0 .. 2^20.  The counts do not depend on it.
 * (tests/test_gpu_monitor_inputs.py) */
int covahip_dev_input_flush(covahip_ctx *ctx, int samples);

/* Device bytes of host samples (4 bytes of logit and 1 label byte per macroblock) that covahip_post_heat_add (COVAHIP_MEM_HOST)
 * stages per piece; 0 restores the default of 64 MiB.  A call whose samples exceed it is uploaded and counted in several pieces
 * of whole samples, at least one per piece.  Host-only: no kernel changes and the tables do not depend on it; device-memory calls
 * ignore it.  (tests/test_gpu_heat.py) */
int covahip_dev_heat_set_stage(covahip_ctx *ctx, size_t bytes);
/* Bytes of the staging that a training-data set's host traffic moves through; 0 restores the default of 32 MiB.  A host
 * covahip_train_data_append packs and uploads its frames in rounds of bytes / 2 macroblocks (at least one; a round may end in the
 * middle of a frame), and a host-bound covahip_train_data_gather runs one launch per as many samples as fit (at least one).
 * Host-only: no kernel changes and the results do not depend on it; device-memory calls ignore it.
 * (tests/test_gpu_train_data.py) */
struct covahip_train_data;
int covahip_dev_train_data_set_stage(struct covahip_train_data *data, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* COVAHIP_DEV_H */
