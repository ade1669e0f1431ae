/*
 * covahip.h -- C-ABI of libcovahip.so, the MI355X (gfx950) compressed-domain filter
 * stage for CoVA.
 *
 * This is the drop-in boundary: every entry point replaces one piece of arithmetic
 * or host state that a CoVA GStreamer element performs today, and is what that
 * element's FFI (Rust `extern "C"` / C++ direct call) would bind.  The shape follows
 * the reference's own C-ABI precedent, cova-rs/nvdsbbox/nvdsbbox.h:7-14 (opaque
 * handle, plain scalars, caller-owned byte buffers, integer status).
 *
 *   - no C++/HIP/torch types in any signature: plain pointers, sizes, ints
 *   - every function returns a covahip_status (0 = OK) unless noted
 *   - no exceptions or unwinding cross the boundary, no global state
 *   - one covahip_ctx per GPU per thread of use; host objects (stack / sort /
 *     gopfilter) are one per stream, like the element instances they back
 *   - pointers tagged "dev" must be device memory of the ctx's GPU (from
 *     covahip_malloc or any HIP allocation of the same process); "host" pointers
 *     are ordinary memory.  mem_kind says which one a dual-use pointer is.
 *
 * Reference paths below are relative to /root/reference.
 */
#ifndef COVAHIP_H
#define COVAHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ status */
typedef enum covahip_status {
    COVAHIP_OK = 0,
    COVAHIP_ERR_INVALID_ARG = 1,
    COVAHIP_ERR_NO_DEVICE = 2,      /* no HIP device / HIP runtime failure at init      */
    COVAHIP_ERR_HIP = 3,            /* a HIP call failed; see covahip_last_hip_error    */
    COVAHIP_ERR_NOT_LOADED = 4,     /* BlobNet weights not loaded                       */
    COVAHIP_ERR_UNSUPPORTED = 5,    /* geometry outside what the kernels are built for  */
    COVAHIP_ERR_BAD_WEIGHTS = 6,    /* weight blob header / size mismatch               */
    COVAHIP_ERR_OVERFLOW = 7,       /* caller buffer too small                          */
    COVAHIP_ERR_BAD_DATA = 8        /* malformed bincode input                          */
} covahip_status;

const char *covahip_strerror(int status);
/* "covahip <version> gfx950 ..." -- static string */
const char *covahip_version(void);

enum { COVAHIP_MEM_HOST = 0, COVAHIP_MEM_DEVICE = 1 };
/* Alignment of DEVICE pointers (host pointers are copied into the library's own staging and may have any alignment).  Every
 * entry below says which of two things holds for each of its device pointers:
 *   "any alignment": the library looks at the address, runs a narrower kernel form where the wide one does not apply, and
 *       gives the same results (tests offset each such pointer by single bytes);
 *   "aligned to N": the kernels load or store N bytes at a time through the pointer and there is NO check and no other form;
 *       what covahip_malloc returns (256-byte aligned) always qualifies, an address inside such an allocation must be a
 *       multiple of N.
 * Pointers to f32, i32 and covahip_box always need their natural 4-byte alignment; that is not repeated per entry.
 * ("Host-side choices of kernel form and chunking", lists the branches and the tests that run them.) */

/* ------------------------------------------------------------ GPU context */
typedef struct covahip_ctx covahip_ctx;

int covahip_device_count(int *count);
/* PCI address ("0000:c1:00.0") of HIP device `device_id` into out (>= 13 bytes): what a host process needs to find the
 * device's NUMA node (/sys/bus/pci/devices/<address>/numa_node, local_cpulist) and pin its per-stream threads next to the GPU
 * it feeds -- one process per GPU, as the reference runs one pipeline per GoP range (gst-gopsplit/gstgopsplit.cpp:556-603). */
int covahip_device_pci_bus_id(int device_id, char *out, int out_len);
/* Creates a context on GPU `device_id` with its own HIP stream.
 * (The reference pins its engines with gpu-id, config/blobnet/amsterdam_b128.txt:6,
 *  gst-plugins/gst-maskcopy/gstmaskcopy.cpp:247.) */
int covahip_ctx_create(int device_id, covahip_ctx **out);
void covahip_ctx_destroy(covahip_ctx *ctx);
/* Blocks until everything the ctx has enqueued (all lanes, see below) is done. */
int covahip_ctx_sync(covahip_ctx *ctx);
/* Lanes = batches in flight.  The reference keeps one GPU busy with sixteen BlobNet engines, each with a batch of its own
 * (experiment/cova/config.yaml:33-34 num_mask / mask_batch_size, pipeline/cova/pipeline.py:139-181); here a ctx owns
 * n_lanes HIP streams with an activation workspace each, and consecutive covahip_filter_forward /
 * covahip_filter_forward_frames calls on DEVICE pointers (and consecutive covahip_pipe_submit calls) go to consecutive
 * lanes, so the launches of batch k+1 fill the ramps and tails of batch k's.  Rules:
 *   - such a call sees everything enqueued on the ctx before it (copies, memsets, timers);
 *   - every other entry point (covahip_ctx_sync, timers, copies, covahip_bboxcc, covahip_blobnet_forward, host-pointer
 *     calls) waits for / is ordered behind all lanes;
 *   - two device-pointer filter calls with nothing in between may run concurrently: give them separate output buffers
 *     (inputs may be shared) or call covahip_ctx_sync between them.
 * n_lanes in [1, 4]; DEFAULT 1 = strictly in call order on one stream, no hidden concurrency (the boundary the reference's
 * own FFI has, cova-rs/nvdsbbox/nvdsbbox.h:7-14).  A caller that owns one set of output buffers per batch in flight opts in
 * with covahip_ctx_set_lanes(ctx, n), n = 2 or 3: the blobnetfilter element, tools/pipe_bench and bench.py do (covahip_pipe_* slots own
 * their buffers).  Workspace per lane at 68x120, max_batch 256: about 150 MB.  Drains the ctx first. */
int covahip_ctx_set_lanes(covahip_ctx *ctx, int n_lanes);
int covahip_ctx_get_lanes(covahip_ctx *ctx, int *n_lanes);
/* Text of the last failing HIP call on this ctx ("" if none). */
const char *covahip_last_hip_error(covahip_ctx *ctx);
/* Device properties the bench reports: name (<=255 chars), CU count, HBM bytes. */
int covahip_device_info(covahip_ctx *ctx, char *name, size_t name_cap, int *num_cu, size_t *hbm_bytes);

/* Device memory helpers so a host language needs no HIP binding of its own. */
int covahip_malloc(covahip_ctx *ctx, size_t bytes, void **dev_ptr);
int covahip_free(covahip_ctx *ctx, void *dev_ptr);
int covahip_memcpy_h2d(covahip_ctx *ctx, void *dev_dst, const void *host_src, size_t bytes);
int covahip_memcpy_d2h(covahip_ctx *ctx, void *host_dst, const void *dev_src, size_t bytes);
int covahip_memset(covahip_ctx *ctx, void *dev_ptr, int value, size_t bytes);

/* HIP-event timing on the ctx's stream (bench.py's timed region and per-kernel
 * roofline numbers).  slot in [0, 16). */
int covahip_timer_start(covahip_ctx *ctx, int slot);
int covahip_timer_stop(covahip_ctx *ctx, int slot);
/* Synchronises on the stop event and returns elapsed milliseconds. */
int covahip_timer_elapsed_ms(covahip_ctx *ctx, int slot, float *ms);

/* Per-kernel profiling: when enabled every kernel launch of blobnet/bboxcc calls is
 * bracketed by HIP events on the ctx stream; covahip_profile_read then reports the
 * accumulated time and launch count per kernel name. */
int covahip_profile_enable(covahip_ctx *ctx, int on);
/* Restricts the event bracketing to one kernel name (NULL or "" = all kernels), so a
 * timed region can carry the two events of its dominant kernel only. */
int covahip_profile_filter(covahip_ctx *ctx, const char *kernel_name);
int covahip_profile_reset(covahip_ctx *ctx);
/* Fills up to cap entries; *n gets the number of distinct kernels seen. */
typedef struct covahip_kernel_time {
    char name[48];
    double total_ms;
    int64_t launches;
} covahip_kernel_time;
int covahip_profile_read(covahip_ctx *ctx, covahip_kernel_time *out, int cap, int *n);

/* ------------------------------------------------------------------ BlobNet
 * Replaces the nvinfer/TensorRT BlobNet engine and its pre/post-processing:
 *   config/blobnet/amsterdam_b128.txt:1-28 (engine, net-scale-factor 1, RGB planar,
 *   segmentation threshold 0.5), model/tasks.py:34-55 (fp16 engine, explicit batch),
 *   utils/model/{blobnet,encoder,decoder,pointwise,preprocessing}.py (the graph), gst-plugins/gst-maskcopy/gstmaskcopy.cpp:226-230
 *   (class_map + 1 -> GRAY8 {0,1} mask).
 *
 * weights: blob in the format of cova_amd/weights.py (64-byte header + fp32 payload).
 * h_mb x w_mb: macroblock grid (e.g. 68x120 for 1080p, 45x80 for 720p); t must be 4.
 * max_batch sizes the activation workspace held in HBM by the ctx.
 * Limits of the kernels, all checked HERE (COVAHIP_ERR_UNSUPPORTED), never at forward time:
 *   16 <= h_mb <= 1024; 16 <= w_mb <= 252, a multiple of 4 (the first level reads 16-byte groups of four
 *   macroblocks).  The width limit is the LDS of a CU: a band of one pool-window row of every level must fit its
 *   kernel's share of it, and level 1's is the first that does not (its 126 columns at w_mb = 252 fill the 64 KB
 *   tile of its workgroup).  A 4K grid (135x240) loads; no height up to 1024 is refused.  The limit does not
 *   depend on max_batch (tests/test_gpu_geometry_edges.py probes the range and runs its edges).
 * A ctx holds ONE model or ONE model set (covahip_blobnet_load_set): loading again replaces it.
 * A failed load leaves the ctx without a model (later calls return COVAHIP_ERR_NOT_LOADED).  A malformed blob
 * (COVAHIP_ERR_BAD_WEIGHTS) is rejected before anything changes: the model loaded before stays.  */
int covahip_blobnet_load(covahip_ctx *ctx, const void *weights, size_t weights_bytes, int h_mb, int w_mb,
                         int t, int max_batch);
/* Model sets: one ctx holds K models of ONE geometry and max_batch (e.g. one BlobNet per camera), and every stack of a
 * batch names its model, so streams of different models share one batch and one launch of each kernel.
 *   1 <= n_models <= COVAHIP_MAX_MODELS; weights[k] / weights_bytes[k]: model k's blob (format as above).
 *   Replaces whatever the ctx held.  All or nothing: one malformed blob is COVAHIP_ERR_BAD_WEIGHTS and, like any
 *   other failure here, leaves the ctx with no model.
 *   covahip_blobnet_load is a set of one.  The forward entries without _m run every stack on model 0.
 * The _m entries below take model_ids: a HOST array u8 [batch], the model of output stack b (like stack_index, read
 * during the call); NULL = model 0 everywhere.  An id >= n_models is COVAHIP_ERR_INVALID_ARG.  A stack's result is
 * the result of a ctx loaded with its model alone, bit for bit.
 * Carrier-frame entries: level 0 runs ONCE per carrier frame, so a frame has exactly one model: a frame that stacks
 * of two different models reference is COVAHIP_ERR_INVALID_ARG (checked on the host with stack_index).  Frames no
 * stack references may run under any model; nothing of them is visible.                                          */
#define COVAHIP_MAX_MODELS 256
int covahip_blobnet_load_set(covahip_ctx *ctx, int n_models, const void *const *weights, const size_t *weights_bytes,
                             int h_mb, int w_mb, int t, int max_batch);
/* Models of the loaded set (1 after covahip_blobnet_load). */
int covahip_blobnet_num_models(covahip_ctx *ctx, int *n_models);
/* rgba_stack: u8 [batch][t*h_mb][w_mb][4] -- metapreprocess output (row block k =
 *   frame i-k; byte 0/1/2 = mb_type/mv_x/mv_y, byte 3 ignored).
 * logits (may be NULL): f32 [batch][h_mb][w_mb] pre-sigmoid output.
 * mask   (may be NULL): u8  [batch][h_mb][w_mb], 1 where sigmoid(logit) > 0.5.
 * mem_kind applies to all three pointers.  Asynchronous for device pointers (use
 * covahip_ctx_sync); synchronous for host pointers.
 * Device pointers: rgba_stack aligned to 16 (four macroblocks a load; w_mb is a multiple of 4, so every row is); mask any
 * alignment (off a 4-byte boundary it is stored byte by byte); logits natural.        */
int covahip_blobnet_forward(covahip_ctx *ctx, const uint8_t *rgba_stack, int batch, float *logits,
                            uint8_t *mask, int mem_kind);
/* covahip_blobnet_forward with a model per stack (model_ids: see covahip_blobnet_load_set). */
int covahip_blobnet_forward_m(covahip_ctx *ctx, const uint8_t *rgba_stack, const uint8_t *model_ids, int batch,
                              float *logits, uint8_t *mask, int mem_kind);
/* Per-model post-processing: what turns a stack's logits into its mask.  For a stack b that runs on model m
 *     mask[b, y, x] = (logit[b, y, x] > logit_thresh[m]) && keep[m][y, x]
 * and the boxes are regionprops of THAT mask.  The logits output is not affected.  The reference carries the threshold
 * per engine (segmentation-threshold in the files of config/blobnet); keep is the ignore region of a camera (a burned-in
 * clock, a neighbouring road).  Both are applied inside the kernel that makes the mask: no launch is added, and while
 * every model of the set has the defaults (threshold 0, keep everything) the forward runs the very kernels it ran
 * before this call existed.
 * The settings live in the ctx, per model of the loaded set (model 0 after covahip_blobnet_load), and apply to every
 * entry that produces a mask or boxes from a model: covahip_blobnet_forward[_m], covahip_filter_forward[_m], the
 * _frames / _frames_m / _frames_packed[_m] entries and covahip_pipe_submit.  covahip_bboxcc has no model and is not
 * affected.  covahip_blobnet_load and covahip_blobnet_load_set reset every model to the defaults.
 * covahip_blobnet_set_post waits for everything the ctx has in flight on all lanes, then updates the device tables:
 * batches submitted before the call have the old settings, batches submitted after it the new ones.  Call it under the
 * lock that guards acquire and submit.  post == NULL restores the defaults of that model.  Neither form touches the model's
 * area threshold (covahip_blobnet_set_area below): the two settings are independent.
 *   COVAHIP_ERR_INVALID_ARG: NULL ctx, model outside the set, NaN or infinite threshold (nothing changes);
 *   COVAHIP_ERR_NOT_LOADED: no model loaded.                                                                        */
typedef struct covahip_blobnet_post {
    float logit_thresh;     /* mask where logit > logit_thresh; 0 = the reference's p > 0.5; must be finite */
    const uint8_t *keep;    /* HOST u8 [h_mb][w_mb], non-zero = this macroblock may be foreground; NULL = all */
} covahip_blobnet_post;
int covahip_blobnet_set_post(covahip_ctx *ctx, int model, const covahip_blobnet_post *post /* NULL = defaults */);
/* The settings of a model.  logit_thresh, keep_or_null (u8 [h_mb][w_mb], written as 0 / 1; all 1 without a keep map)
 * and has_keep (1 when a keep map is set) may each be NULL.                                                         */
int covahip_blobnet_get_post(covahip_ctx *ctx, int model, float *logit_thresh, uint8_t *keep_or_null, int *has_keep);
/* Per-model area threshold: the cc-threshold of bboxcc, which the reference carries per bboxcc element, i.e. per stream
 * (cova-rs/gst-plugins/src/bboxcc, experiment/cova/config.yaml:59).  A model m of the loaded set has area[m]: 0 (the default)
 * = unset, >= 1 = a threshold in macroblocks.  For a stack b that runs on model m
 *     eff(b)    = area[m] >= 1 ? area[m] : the call's area_thresh
 *     boxes[b]  = regionprops(mask[b], eff(b))     -- covahip_bboxcc semantics: 8-connected, OpenCV label order, area_px >= eff(b)
 *     counts[b] = components that pass; the first min(count, max_boxes) are written
 * byte for byte what the stack gives in a batch of its own with the scalar area_thresh = eff(b).  Logits and masks are not
 * affected.  This is the P[t][a] of covahip_post_sweep: the number calibration prints is the number serving applies.
 * It applies wherever a model produces boxes: covahip_filter_forward[_m], covahip_filter_forward_frames[_m],
 * covahip_filter_forward_frames_packed[_m] and covahip_pipe_submit (the entries without _m run model 0 and use area[0]);
 * covahip_blobnet_forward* makes no boxes and covahip_bboxcc has no model.  The threshold travels with the stack's other settings
 * into the kernel that runs bboxcc: no launch, no copy and no synchronisation is added to a step, and while every model is unset
 * (and has the defaults of covahip_blobnet_set_post) the forward runs the very kernels it ran before.
 * Ordering and locking are those of covahip_blobnet_set_post: it waits for everything in flight on all lanes; batches
 * submitted before the call see the old value, batches after it the new one.  covahip_blobnet_load[_set] reset every model to
 * unset.  The two settings are independent: covahip_blobnet_set_post (post == NULL included) does not touch area[m], and
 * covahip_blobnet_set_area does not touch the threshold or the keep map.
 *   COVAHIP_ERR_INVALID_ARG: NULL ctx, model outside the set, negative value (nothing changes);
 *   COVAHIP_ERR_NOT_LOADED: no model loaded.                                                                        */
int covahip_blobnet_set_area(covahip_ctx *ctx, int model, int area_thresh /* 0 = unset */);
int covahip_blobnet_get_area(covahip_ctx *ctx, int model, int *area_thresh);
/* Calibration: which logit_thresh (covahip_blobnet_set_post) and which area threshold (the cc-threshold of bboxcc / cova) to
 * set for a camera.  covahip_post_sweep scores logits against labels (the MoG labels of a held-out set) at n_thresh mask
 * thresholds x n_area area thresholds in one pass on the GPU: pixel counts per threshold, and per cell the boxes serving would
 * emit, how many of them hit a labelled object and how many labelled objects they find.  It has no model: it scores whatever
 * forward produced the logits (python -m cova_amd.calibrate feeds it the deployed fp16 path).  Every quantity is an integer
 * count, so the result is exact.  Rules:
 *   keep'[y,x] = keep ? keep[y,x] != 0 : 1
 *   mask_t     = (logit > logit_thresh[t]) & keep'     -- the expression of covahip_blobnet_set_post; NaN is background
 *   gt'        = (gt != 0) & keep'                     -- a labelled object inside the ignore region is neither a miss nor a hit
 *   pixel[t]   = tp |mask_t & gt'|, fp |mask_t & ~gt'|, fn |~mask_t & gt'|, over all samples
 *   G          = regionprops(gt', gt_area_thresh), P[t][a] = regionprops(mask_t, area_thresh[a]): covahip_bboxcc semantics
 *                (8-connected components in OpenCV label order, area_px >= the threshold).  regionprops(mask, a) is
 *                regionprops(mask, area_thresh[0]) with the boxes of area_px < a dropped, order kept: one labelling per
 *                (sample, threshold) serves every area.  Only the first max_boxes boxes of a frame take part -- of that
 *                labelling at area_thresh[0] for predictions, of G for labels; a frame with more is counted in truncated[t] /
 *                gt_truncated, and the boxes beyond are as if they did not exist (gt_objects counts the label boxes that take part).
 *   hit(p, g)  = inter > 0 && inter * iou_den >= iou_num * (area_box(p) + area_box(g) - inter), in 64-bit integers, with
 *                area_box = width * height of the box and inter the area of the boxes' intersection
 *   cells[t][a]: pred = |P[t][a]|, pred_true = the p in P[t][a] that hit some g in G, gt_found = the g in G that hit some p in
 *                P[t][a]; gt_objects = sum |G|.  There is no assignment, so there are no ties to break.
 *   Additivity: the counts of n samples equal the sums of the counts of any partition of them into calls, and do not depend on
 *   chunk.
 * Errors, all checked on the host before the GPU is touched: COVAHIP_ERR_INVALID_ARG for a NULL pointer (keep may be NULL;
 * logits / gt may be NULL when n == 0), a non-finite or not strictly ascending list, a count outside its range, iou_num < 1 or
 * > iou_den, h or w < 1, n < 0, chunk < 0, another mem_kind; COVAHIP_ERR_UNSUPPORTED for w > 256 (covahip_bboxcc's limit) or
 * h > 16384.  n == 0 is COVAHIP_OK with zeros.
 * Runs on the primary stream behind all lanes, like stand-alone covahip_bboxcc; its scratch belongs to the ctx.  It changes no
 * model, no setting and no result of any forward. */
typedef struct covahip_sweep_cfg {
    int32_t h, w;                    /* grid; the limits of covahip_bboxcc (w <= 256) */
    int32_t n_thresh;                /* 1..64 */
    const float *logit_thresh;       /* HOST [n_thresh], finite, strictly ascending */
    int32_t n_area;                  /* 1..16 */
    const int32_t *area_thresh;      /* HOST [n_area], >= 1, strictly ascending: cc-threshold candidates */
    int32_t gt_area_thresh;          /* >= 1: a label component is an object when it has at least this many macroblocks */
    int32_t iou_num, iou_den;        /* 1 <= iou_num <= iou_den: the hit rule's IoU as an exact fraction */
    int32_t max_boxes;               /* 1..1024 boxes kept per frame (see "truncated") */
    const uint8_t *keep;             /* HOST u8 [h][w], non-zero = scored; NULL = all (set_post's keep map) */
    int32_t chunk;                   /* samples per internal pass; 0 = chosen by the library */
} covahip_sweep_cfg;
typedef struct covahip_sweep_cell { int64_t pred, pred_true, gt_found; } covahip_sweep_cell;
typedef struct covahip_sweep_result {
    int64_t samples, gt_objects, gt_truncated;   /* gt_truncated: samples whose label had more than max_boxes objects */
} covahip_sweep_result;
/* logits f32 [n][h][w], gt u8 [n][h][w] (mem_kind applies to both; outputs are HOST).  Device pointers: gt any alignment, logits
 * natural (with h * w a multiple of 4, logits on a 16-byte and gt on a 4-byte boundary the masks are made four macroblocks per
 * work item, otherwise one: same counts).  pixel: i64 [n_thresh][3] = tp, fp, fn;
 * cells: [n_thresh][n_area]; truncated: i64 [n_thresh] = frames (sample, threshold) with more than max_boxes components.
 * Synchronous.  Outputs are OVERWRITTEN with this call's counts; the caller adds calls up. */
int covahip_post_sweep(covahip_ctx *ctx, const covahip_sweep_cfg *cfg, const float *logits, const uint8_t *gt, int n,
                       int mem_kind, int64_t *pixel, covahip_sweep_cell *cells, int64_t *truncated, covahip_sweep_result *out);
/* Ignore region from heat: how often each macroblock fires.  The sweep above cannot see a burned-in clock: MoG marks it in every
 * frame, a model trained on those labels fires there, and its box hits the label box at every threshold.  What gives it away is
 * persistence, so covahip_post_heat_* count per macroblock, per mask threshold and over all samples of a begin ... end bracket
 *   fire[t][y][x]  = the samples with logit > logit_thresh[t]   -- covahip_post_sweep's expression WITHOUT a keep map (the heat
 *                    must show what a keep map would hide); the compare is strict, NaN is background, +inf fires everywhere
 *   both[t][y][x]  = the samples with logit > logit_thresh[t] and gt != 0
 *   gt_fire[y][x]  = the samples with gt != 0
 * so that per macroblock fp = fire - both and fn = gt_fire - both, and the sums over y, x of (both, fire - both, gt_fire - both)
 * are pixel[t] of covahip_post_sweep without keep on the same inputs.  All values are integer counts and exact, and do not
 * depend on how the samples are split over covahip_post_heat_add calls.  python -m cova_amd.calibrate --auto-ignore turns the
 * table into the camera's ignore rectangles ("Ignore region from heat").
 * The counters (u32) live in the ctx, on the device, between begin and end.  begin zeroes them; a begin while a heat is open
 * starts over.  add runs on the primary stream behind all lanes and is synchronous, like the sweep: when it returns the
 * caller's next forward may overwrite the logits.  end copies the counters out, widens them to i64 and closes the heat; every
 * output pointer may be NULL.  The calls read no model state and write none.
 * Errors, all checked on the host before the GPU is touched: COVAHIP_ERR_INVALID_ARG for a NULL ctx, cfg or list, a non-finite
 * or not strictly ascending list, n_thresh outside 1..64, h or w < 1, n < 0, NULL logits or gt with n > 0, another mem_kind,
 * add or end without begin, more than INT32_MAX samples in one heat; COVAHIP_ERR_UNSUPPORTED for h * w > 2^24.  A failed begin
 * leaves an open heat as it was.  n == 0 is COVAHIP_OK and changes nothing. */
typedef struct covahip_heat_cfg {
    int32_t h, w;                    /* grid */
    int32_t n_thresh;                /* 1..64 */
    const float *logit_thresh;       /* HOST [n_thresh], finite, strictly ascending (copied by begin) */
} covahip_heat_cfg;
int covahip_post_heat_begin(covahip_ctx *ctx, const covahip_heat_cfg *cfg);
/* logits f32 [n][h][w], gt u8 [n][h][w]; mem_kind applies to both.  Device pointers: gt any alignment, logits natural (the kernel
 * loads single values). */
int covahip_post_heat_add(covahip_ctx *ctx, const float *logits, const uint8_t *gt, int n, int mem_kind);
/* HOST outputs: fire, both i64 [n_thresh][h][w]; gt_fire i64 [h][w]; samples: the number of samples added. */
int covahip_post_heat_end(covahip_ctx *ctx, int64_t *fire, int64_t *both, int64_t *gt_fire, int64_t *samples);
/* Serving monitor: how a deployed model behaves, from what every filter step already has on the device -- no decode, no labels.
 * Per model m of a set and over all COUNTED samples b (model m's) since begin or the last reset
 *   frames[m]            += 1
 *   fire[m][y][x]        += mask[b][y][x] != 0       -- the mask AS SERVED (the model's threshold and keep map applied); any
 *                                                       non-zero byte counts once
 *   boxes[m]             += counts[b]                -- the components that pass the stack's effective area threshold
 *   frames_with_boxes[m] += counts[b] > 0
 *   truncated[m]         += counts[b] > max_boxes
 *   area_hist[m][k]      += the boxes i < min(counts[b], max_boxes) with min(15, floor(log2(boxes[b][i].area_px))) == k
 *                           (an area below 2 is bin 0)
 * All values are integer counts and exact; they are additive over batches and depend neither on the lanes nor on how the samples
 * are split over calls.  The counters are 64-bit and live in the ctx, on the device, between begin and end ((20 + h * w) * 8
 * bytes per model: 16.7 MB for 256 models of 68 x 120).  python -m cova_amd.monitor reports them per camera (DESIGN.md section
 * 4, "Serving monitor").
 * attach = 1: the monitor counts the filter batches of THIS ctx's loaded model or set -- every entry that produces boxes from a
 * model: covahip_filter_forward[_m], the _frames[_m] / _frames_packed[_m] entries and covahip_pipe_submit, host or device
 * pointers; covahip_blobnet_forward* makes no boxes and is not counted.  Batch i since begin or the last reset (0-based, in
 * submission order) is counted iff i % every == 0, with one kernel launch behind the batch's own on the lane that ran it: no
 * synchronisation, no allocation.  A failed or empty (batch == 0) call is neither seen nor counted.  max_boxes is the call's.
 * begin needs a loaded model whose grid and number of models equal the cfg (COVAHIP_ERR_INVALID_ARG otherwise,
 * COVAHIP_ERR_NOT_LOADED with nothing loaded); covahip_blobnet_load[_set] and destroying the model close an attached monitor.
 * attach = 0: the monitor is fed by covahip_monitor_add alone (on an attached one add is COVAHIP_ERR_INVALID_ARG) and survives
 * loads.  add runs on the primary stream behind all lanes and is synchronous, like covahip_post_heat_add.  With no monitor open,
 * or one that is not attached, a filter step launches exactly the kernels it launches without this interface.
 * read waits for everything the ctx has in flight on all lanes (like covahip_blobnet_set_post), copies the counters out and, with
 * reset != 0, zeroes the tables and both batch counters; it does not close the monitor.  begin while a monitor is open starts
 * over; a failed begin leaves an open monitor as it was.  end closes it.
 * Errors, all checked on the host before the GPU is touched: COVAHIP_ERR_INVALID_ARG for a NULL ctx or cfg, h or w < 1, n_models
 * outside 1..COVAHIP_MAX_MODELS, attach other than 0 / 1, every < 1 (attached), max_boxes < 0 (stand-alone), n < 0, NULL mask or
 * counts with n > 0, NULL boxes while max_boxes > 0, an id >= n_models, another mem_kind, add, read or end without begin;
 * COVAHIP_ERR_UNSUPPORTED for h * w > 2^24.  n == 0 is COVAHIP_OK and changes nothing. */
typedef struct covahip_monitor_cfg {
    int32_t h, w;        /* grid */
    int32_t n_models;    /* 1..COVAHIP_MAX_MODELS */
    int32_t max_boxes;   /* >= 0: row length of the boxes arrays that will be fed (stand-alone add); ignored when attached */
    int32_t attach;      /* 1: count every `every`-th filter batch of THIS ctx's loaded model / set; 0: fed by covahip_monitor_add only */
    int32_t every;       /* >= 1; attach only: filter batch i since begin (0-based, in submission order) is counted iff i % every == 0 */
} covahip_monitor_cfg;
#define COVAHIP_MONITOR_AREA_BINS 16
struct covahip_box;   /* (bboxcc, below) */
int covahip_monitor_begin(covahip_ctx *ctx, const covahip_monitor_cfg *cfg);
/* mask u8 [n][h][w], counts i32 [n], boxes [n][max_boxes] (mem_kind applies to the three; boxes may be NULL with max_boxes == 0);
 * model_ids: HOST u8 [n], read during the call, or NULL = model 0.  Device pointers: mask any alignment (read a word at a time
 * only when h * w is a multiple of 4 and the pointer is on a 4-byte boundary); counts and boxes natural. */
int covahip_monitor_add(covahip_ctx *ctx, const uint8_t *mask, const int32_t *counts, const struct covahip_box *boxes,
                        const uint8_t *model_ids, int n, int mem_kind);
/* HOST outputs, each may be NULL: frames, boxes, frames_with_boxes, truncated i64 [n_models]; fire i64 [n_models][h][w];
 * area_hist i64 [n_models][16]; batches_seen / batches_counted: attached filter batches since begin or the last reset. */
int covahip_monitor_read(covahip_ctx *ctx, int reset, int64_t *frames, int64_t *fire, int64_t *boxes, int64_t *frames_with_boxes,
                         int64_t *truncated, int64_t *area_hist, int64_t *batches_seen, int64_t *batches_counted);
int covahip_monitor_end(covahip_ctx *ctx);
/* Input monitor: what records a camera SENDS, beside what the model makes of them.  The records are whatever the camera's encoder
 * and the entropy front end make of the scene, and a firmware update, a bitrate cap or a frozen feed changes them without
 * touching the scene or the model.  One set of exact integer statistics over packed records, behind served batches (an attached
 * monitor), on a caller's inputs (covahip_monitor_add_inputs) and over resident training frames
 * (covahip_train_data_record_stats, below).
 * A record is what covahip_carrier_pack keeps of a macroblock's four bytes: c = min(byte0, 6), x = min(byte1, 6),
 * y = min(byte2, 6), r = c | x << 3 | y << 6; byte 3 is ignored.  For data that is already packed r = value & 511: bits 9 and
 * above are ignored and a field of 7 is counted as given.  Per counted frame f of h x w macroblocks p:
 *   bin(p)       = r(p), 0 .. 511
 *   moves(p)     = (r(p) & 0x1F8) != 0          -- either vector field is non-zero
 *   intra(p)     = (r(p) & 7) >= 5
 *   n_move(f)    = #{p : moves(p)}
 *   still(f)     = every r(p) == 0              -- all skip and no vector: a frozen or duplicated picture
 *   all_intra(f) = every intra(p)               -- an I picture; in_frames / intra_frames estimates the GoP length
 * and per model m (the counted frames of model m's stacks), 64-bit counts:
 *   in_frames[m]      += 1
 *   hist[m][bin(p)]   += 1 for every p
 *   moving[m][y][x]   += moves(p)
 *   still_frames[m]   += still(f)
 *   intra_frames[m]   += all_intra(f)
 *   move_hist[m][k]   += 1 with k = 0 when n_move(f) == 0, else k = min(15, 1 + floor(log2 n_move(f)))
 * NO keep map applies to any of them: the network's receptive field reads ignored macroblocks too, and the serving side and the
 * training side must stay comparable.  All counts are exact and additive over calls and batches; they depend neither on the
 * lanes, nor on the slicing, nor on the input form, nor on pointer alignment.
 * Which frame is counted: each stack counts ONE frame for its model, its newest slice.  COVAHIP_INPUT_STACKED, u8
 * [batch][4h][w][4]: row block 0 of stack b.  COVAHIP_INPUT_FRAMES, u8 [n_frames][h][w][4], and COVAHIP_INPUT_PACKED, u16
 * [n_frames][h][w]: frame stack_index ? stack_index[4 b] : b + 3.  A frame that is the newest slice of two stacks is counted
 * twice; sliding windows at gamma 1 count every stream frame once.
 * covahip_monitor_set_inputs(ctx, on), on an open monitor, attached or stand-alone: drains the ctx as begin does and allocates
 * (on = 1) or frees (on = 0) the input tables, (4 + 512 + 16 + h * w) words per model, zeroed; a call that changes nothing keeps
 * the tables.  Off is the default, and with it off everything behaves as without this interface: the kernels a filter step
 * launches and what covahip_monitor_read returns.  begin and end discard the setting with the monitor.
 * Attached, inputs on: every counted filter batch (i % every == 0) also counts its inputs -- the stacked entries, the _frames[_m]
 * and _frames_packed[_m] entries and covahip_pipe_submit -- on the lane that ran the batch, in two launches behind the
 * monitor's own: no synchronisation, no allocation, no upload.
 * covahip_monitor_add_inputs: the stand-alone feed, on the primary stream behind all lanes and synchronous, like
 * covahip_monitor_add.  stack_index: HOST i32 [batch][4] or NULL (one stream in order: batch == n_frames - 3), validated as the
 * _frames entries validate it (every index in [0, n_frames)); n_frames and stack_index are ignored for the stacked form.
 * model_ids: HOST u8 [batch] or NULL = model 0.  Device pointers of any alignment: records are read 16 bytes at a time where the pointer
 * and the frames lie on 16-byte boundaries, a record at a time on a record's boundary (4 bytes, 2 packed) and byte-wise off
 * it; host data is staged in pieces.
 * covahip_monitor_read_inputs: HOST outputs, each may be NULL: in_frames, still_frames, intra_frames i64 [n_models]; hist i64
 * [n_models][512]; moving i64 [n_models][h][w]; move_hist i64 [n_models][16].  Drains like covahip_monitor_read.  reset != 0
 * zeroes the input tables ONLY; covahip_monitor_read(reset = 1) zeroes what it always zeroed and, when they exist, the input
 * tables too.
 * Errors, all checked on the host before the GPU is touched, and a refused call changes nothing: COVAHIP_ERR_INVALID_ARG for a
 * NULL ctx, no open monitor, on other than 0 / 1; for add_inputs also inputs not switched on, an attached monitor, an unknown
 * form or mem_kind, batch < 0, NULL src with batch > 0, an id >= n_models, and for the two frame forms n_frames < 4, a NULL
 * stack_index with batch != n_frames - 3, an index outside [0, n_frames); for read_inputs and get_inputs also inputs not
 * switched on (read) or a NULL `on` (get).  batch == 0 is COVAHIP_OK and changes nothing. */
#define COVAHIP_INPUT_STACKED 0
#define COVAHIP_INPUT_FRAMES 1
#define COVAHIP_INPUT_PACKED 2
#define COVAHIP_INPUT_BINS 512
#define COVAHIP_INPUT_MOVE_BINS 16
int covahip_monitor_set_inputs(covahip_ctx *ctx, int on);
int covahip_monitor_get_inputs(covahip_ctx *ctx, int *on);
int covahip_monitor_add_inputs(covahip_ctx *ctx, const void *src, int form, int n_frames, const int32_t *stack_index, int batch,
                               const uint8_t *model_ids, int mem_kind);
int covahip_monitor_read_inputs(covahip_ctx *ctx, int reset, int64_t *in_frames, int64_t *hist, int64_t *moving,
                                int64_t *still_frames, int64_t *intra_frames, int64_t *move_hist);
/* Algorithmic MACs per frame of the loaded geometry. */
int covahip_blobnet_macs_per_frame(covahip_ctx *ctx, int64_t *macs);
/* ------------------------------------------------------------------- bboxcc
 * Replaces regionprops() (cova-rs/gst-plugins/src/bboxcc/process.rs:5-49): 8-connected
 * components with stats on an h x w u8 mask (non-zero = foreground), components in
 * OpenCV label order, keep pixel-count >= area_thresh.                            */
typedef struct covahip_box {
    int32_t left, top, width, height; /* CC_STAT_LEFT/TOP/WIDTH/HEIGHT */
    int32_t area_px;                  /* CC_STAT_AREA (pixel count)     */
} covahip_box;

/* mask: u8 [batch][h][w]; boxes: [batch][max_boxes]; counts: i32 [batch] = number of
 * components that pass the filter (if > max_boxes only the first max_boxes are
 * written).  mem_kind applies to mask, boxes and counts.
 * Limit (COVAHIP_ERR_UNSUPPORTED): w <= 256.  Frames of up to about 6,400 2x2 blocks (1080p = 68x120, 1440p =
 * 90x160 macroblock grids) keep their union-find in the LDS of one CU; larger ones (a 4K grid is 135x240) run the
 * same algorithm with that state in global memory -- same results, slower.
 * Device pointers: mask any alignment.  The wave-per-frame kernel and the run-based body load 8 mask bytes at a time and are
 * chosen only when the pointer is on an 8-byte boundary and h * w and w are multiples of 8; otherwise the workgroup kernel reads
 * the frame byte by byte -- same boxes, slower.  boxes and counts natural.        */
int covahip_bboxcc(covahip_ctx *ctx, const uint8_t *mask, int batch, int h, int w, int area_thresh,
                   covahip_box *boxes, int32_t *counts, int max_boxes, int mem_kind);
/* covahip_bboxcc with a threshold per frame.  area_thresh: HOST i32 [batch], frame b keeps pixel-count >= area_thresh[b]; read
 * during the call (like model_ids), whatever mem_kind says about the other pointers; NULL is COVAHIP_ERR_INVALID_ARG.  Same
 * limits, same kernel selection; frame b's result is covahip_bboxcc's of that frame alone at area_thresh[b], byte for byte. */
int covahip_bboxcc_v(covahip_ctx *ctx, const uint8_t *mask, int batch, int h, int w, const int32_t *area_thresh,
                     covahip_box *boxes, int32_t *counts, int max_boxes, int mem_kind);

/* Fused hot path = nvinfer(BlobNet) -> maskcopy -> bboxcc for one batch: the mask
 * stays on the GPU.  logits/mask may be NULL.  bboxcc's limit (w <= 256) lies beyond the model's (w_mb <= 252):
 * every grid that loads runs here.
 * Device pointers: rgba_stack aligned to 16, as for covahip_blobnet_forward; mask any alignment (off a 4-byte boundary the fused
 * tail runs its band form, which stores the mask byte by byte, instead of its row form -- same mask, counts and boxes); logits,
 * boxes and counts natural.                                                                         */
int covahip_filter_forward(covahip_ctx *ctx, const uint8_t *rgba_stack, int batch, int area_thresh,
                           covahip_box *boxes, int32_t *counts, int max_boxes, float *logits,
                           uint8_t *mask, int mem_kind);
/* covahip_filter_forward with a model per stack (model_ids: see covahip_blobnet_load_set). */
int covahip_filter_forward_m(covahip_ctx *ctx, const uint8_t *rgba_stack, const uint8_t *model_ids, int batch,
                             int area_thresh, covahip_box *boxes, int32_t *counts, int max_boxes, float *logits,
                             uint8_t *mask, int mem_kind);

/* The same hot path fed with CARRIER frames instead of stacks: metapreprocess' temporal stacking (timestep 4,
 * cova-rs/gst-plugins/src/metapreprocess/imp.rs:288-332) becomes an index gather on the GPU.  With gamma = 1 a
 * carrier frame is a slice of four consecutive stacks; here it crosses PCIe / HBM once and the first encoder
 * level's convolution runs once per carrier frame instead of once per (stack, slice).  Results are bit-identical
 * to covahip_filter_forward on the stacks those indices describe.
 *   frames:      u8 [n_frames][h_mb][w_mb][4], any mix of streams (mem_kind as for the other pointers)
 *   stack_index: HOST i32 [batch][4]: for output b the indices into `frames` of its T = 0 (current), 1, 2, 3
 *                (oldest) slices; NULL = one stream in order (batch == n_frames - 3, output b = frames b+3 .. b)
 *   4 <= n_frames <= 4 * max_batch; an index outside [0, n_frames) is COVAHIP_ERR_INVALID_ARG.
 * Device pointers: frames aligned to 16 (four macroblocks a load); the others as for covahip_filter_forward.     */
int covahip_filter_forward_frames(covahip_ctx *ctx, const uint8_t *frames, int n_frames, const int32_t *stack_index,
                                  int batch, int area_thresh, covahip_box *boxes, int32_t *counts, int max_boxes,
                                  float *logits, uint8_t *mask, int mem_kind);
/* covahip_filter_forward_frames with a model per stack (model_ids: see covahip_blobnet_load_set; one model per frame). */
int covahip_filter_forward_frames_m(covahip_ctx *ctx, const uint8_t *frames, int n_frames, const int32_t *stack_index,
                                    const uint8_t *model_ids, int batch, int area_thresh, covahip_box *boxes,
                                    int32_t *counts, int max_boxes, float *logits, uint8_t *mask, int mem_kind);

/* Pipelined host-buffer form of the carrier-frame hot path, for a caller that batches frames continuously (the
 * batching element gst/gstcova.c `blobnetfilter`; stands where nvstreammux -> nvinfer -> nvstreamdemux -> maskcopy
 * -> bboxcc stand in pipeline/cova/pipeline.py:139-261).  A pipe owns n_slots batches in flight: H2D of batch k+1,
 * the kernels of batch k and D2H of batch k-1 overlap.  (Round 6: the runtime multiplexes its streams onto a few hardware queues and a
 * copy stream that shares one with a lane stalls that lane; covahip_pipe_create therefore measures -- a few milliseconds, the ctx
 * idle -- where candidate streams land for the lane count the ctx has AT THAT MOMENT, uploads on a queue without a lane and sends a
 * batch's results out on the lane that ran it: set the lanes before creating the pipe.)  Per batch:
 *   acquire: a free slot and its PINNED host buffers -- frames u8 [max_frames][h_mb][w_mb][4] and stack_index
 *            i32 [max_batch][4] (see covahip_filter_forward_frames) -- which the caller fills in place;
 *            COVAHIP_ERR_OVERFLOW when every slot is taken (collect one first);
 *   submit:  enqueues copy-in, kernels, on-device compaction of the boxes and copy-out; returns at once;
 *   collect: waits for that slot; counts i32 [batch] (components that pass the filter), offsets i32 [batch + 1] and
 *            boxes [offsets[batch]] = the first min(count, max_boxes) boxes of every frame, packed; mask u8
 *            [batch][h_mb][w_mb] when the pipe was created with want_mask (else NULL);
 *   release: the caller is done with the results, the slot can be acquired again.
 * acquire / submit / collect / release: one thread at a time per pipe and its ctx (the caller's lock).
 * covahip_pipe_wait only blocks until a submitted slot's results have landed in host memory; it may run on
 * another thread, concurrently with acquire / submit of other slots (collect returns at once after it).   */
typedef struct covahip_pipe covahip_pipe;
int covahip_pipe_create(covahip_ctx *ctx, int max_batch, int max_frames, int max_boxes, int n_slots, int want_mask,
                        covahip_pipe **out);
void covahip_pipe_destroy(covahip_pipe *pipe);
/* Before the first acquire: the slots' frame area holds packed records (covahip_carrier_pack), hw * 2 bytes per carrier frame. */
int covahip_pipe_set_packed(covahip_pipe *p, int on);
/* Before the first acquire: covahip_pipe_wait / covahip_pipe_collect SLEEP until a slot's results have landed instead of spinning
 * on the completion signal (the default).  Round 6: as a poll -- hipEventQuery + a 20 us nanosleep -- because the runtime's own
 * blocking wait spins before it parks and, at a batch every 110 - 200 us, never parks (12.5 % of the plugin chain's CPU).  For callers whose host cores are the scarce resource
 * (`blobnetfilter`: its collector thread waits for the GPU most of the time). */
int covahip_pipe_set_blocking_wait(covahip_pipe *p, int on);
int covahip_pipe_acquire(covahip_pipe *pipe, int *slot, uint8_t **frames, int32_t **stack_index);
int covahip_pipe_submit(covahip_pipe *pipe, int slot, int n_frames, int batch, int area_thresh);
/* Model sets (covahip_blobnet_load_set): the PINNED model id array u8 [max_batch] of an ACQUIRED slot, filled in place like
 * stack_index.  acquire zeroes it (every stack on model 0); submit reads the first `batch` ids with the rules of
 * covahip_filter_forward_frames_m (an id >= the set's size, or a frame shared across models, fails the submit). */
int covahip_pipe_model_ids(covahip_pipe *pipe, int slot, uint8_t **model_ids);
/* Gives an ACQUIRED slot back without submitting it (after a failed covahip_pipe_submit, or when the caller shuts down with
 * a partly filled batch). */
int covahip_pipe_abort(covahip_pipe *pipe, int slot);
int covahip_pipe_wait(covahip_pipe *pipe, int slot);
int covahip_pipe_collect(covahip_pipe *pipe, int slot, const int32_t **counts, const int32_t **offsets,
                         const covahip_box **boxes, const uint8_t **mask);
int covahip_pipe_release(covahip_pipe *pipe, int slot);

/* --------------------------------------------------------- Bbox wire format
 * bincode 1.3 (default config) bytes of Vec<Bbox> / Frame as the reference's elements
 * exchange them (cova-rs/bbox/src/bbox.rs:4-14,84-90; cova-rs/bbox/src/lib.rs:8-22).  */
typedef struct covahip_bbox {
    float left, top, width, height, area; /* area = width*height (bbox.rs:23) */
    uint64_t track_id;                    /* valid iff has_track_id           */
    uint64_t timestamp;
    uint32_t class_id;
    float confidence;
    uint8_t has_track_id, has_timestamp, has_class_id, has_confidence;
} covahip_bbox;

/* Bbox::new for each CC box (process.rs:47, bbox.rs:17-29). */
void covahip_boxes_to_bbox(const covahip_box *in, int n, covahip_bbox *out);
/* Returns the encoded size; writes only if it fits in cap (else COVAHIP_ERR_OVERFLOW
 * is reported through *status, which may be NULL). */
size_t covahip_bbox_serialize_vec(const covahip_bbox *boxes, size_t n, uint8_t *out, size_t cap, int *status);
/* Decodes up to cap boxes; *n gets the vector length found in the stream. */
int covahip_bbox_deserialize_vec(const uint8_t *data, size_t len, covahip_bbox *out, size_t cap, size_t *n);
size_t covahip_frame_serialize(uint64_t range_start, uint64_t oldest, const covahip_bbox *boxes, size_t n,
                               uint8_t *out, size_t cap, int *status);
/* Bbox::iou (bbox.rs:39-56). */
float covahip_bbox_iou(const covahip_bbox *a, const covahip_bbox *b);

/* ------------------------------------------------------------ BlobNet training
 * One training step of the reference architecture on the GPU: what utils/train-blobnet.py does with Keras (a BlobNet has to be
 * trained on the front end it runs behind, see the entropy-decode section).  fp32 throughout (master weights, activations,
 * gradients); forward, backward and the optimiser are HIP kernels on the ctx's stream, ordered behind all lanes.
 *
 * Semantics (utils/model/{blobnet,encoder,decoder,pointwise}.py in training mode; layer order, odd-size padding and decoder crop as covahip_blobnet_forward):
 *   - input: the u8 stack of covahip_blobnet_forward, clip(x, 0, 6) / 6 of bytes 0..2;
 *   - encoder level: conv 3x3 + bias -> ReLU -> BatchNorm -> 2x2 max-pool (gradient to the first maximum in row-major window
 *     order) -> zero row on top / column on the left for odd sizes -> PointWiseTN (Conv1D(4) + ReLU -> Dropout -> Conv1D(4) +
 *     ReLU -> Dropout -> + x -> ReLU);
 *   - decoder block: ReLU -> Dropout -> convT 4x4 stride 2 + bias -> crop; blocks 0..2 then BatchNorm -> concat with the t = 0
 *     slice of the matching encoder level; after block 3 the 1x1 conv 16 -> 1 -> sigmoid;
 *   - BatchNorm: batch mean and biased variance over (N, T, H, W), eps bn_eps; moving = m * moving + (1 - m) * batch, the
 *     variance's batch value taken unbiased (n / (n - 1)) as TF's fused kernel and torch do -- the reference does not pin this;
 *   - loss: Jaccard distance per sample, I = sum y*p, S = sum (y + p) over H x W, (1 - (I + s) / (S - I + s)) * s with
 *     s = smooth, averaged over the batch; y = the label byte as a float;
 *   - Adam in the Keras form: var -= lr * sqrt(1 - b2^t) / (1 - b1^t) * m / (sqrt(v) + eps); BN gamma and beta are trained,
 *     the moving statistics are not;
 *   - Dropout: inverted (kept values scaled by 1 / (1 - p)), p = cfg.dropout (0: off).  The mask is a counter-based hash,
 *     no device RNG state, so a step is reproducible:
 *         splitmix64(z): z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB;
 *                        return z ^ z >> 31                                          (all mod 2^64)
 *         key  = splitmix64(seed ^ splitmix64(step << 8 | site))
 *         keep = (splitmix64(key + index) >> 40) >= round(p * 2^24)
 *     step = steps this trainer has taken before (0 for the first); site = 2i / 2i + 1 for the two dropouts of encoder level i,
 *     8 + j for decoder block j; index = the element's NCTHW offset in the dropped tensor: [B][C][T][H][W] of the Conv1D output
 *     (T = its output channel) for the encoder, [B][C_in][H][W] of the block input for the decoder.
 * Geometry: 16 <= h_mb, w_mb <= 1024.  Activation memory is sized for max_batch at creation (about 5 MB per sample at 45x80). */
typedef struct covahip_train covahip_train;
typedef struct covahip_train_cfg {
    int32_t h_mb, w_mb, max_batch;
    float lr, beta1, beta2, eps;    /* Adam (lr: what covahip_train_default_cfg's callers use; each step takes its own) */
    float bn_momentum, bn_eps;
    float dropout, smooth;
    uint64_t seed;                  /* dropout hash */
} covahip_train_cfg;
/* The reference's settings: 45x80, batch 4, lr 1e-3, Adam 0.9 / 0.999 / 1e-7, BN 0.99 / 1e-3, dropout 0.2, smooth 100. */
void covahip_train_default_cfg(covahip_train_cfg *cfg);
/* cvhw: the initial weights, a weight file as covahip_blobnet_load takes it (COVAHIP_ERR_BAD_WEIGHTS otherwise). */
int covahip_train_create(covahip_ctx *ctx, const covahip_train_cfg *cfg, const void *cvhw, size_t cvhw_bytes,
                         covahip_train **out);
/* One step on stack u8 [batch][4*h_mb][w_mb][4] and labels gt u8 [batch][h_mb][w_mb] (mem_kind applies to both), with learning
 * rate lr (the epoch schedule is the caller's).  *loss = the batch's loss before the update.  Synchronous. */
int covahip_train_step(covahip_train *tr, const uint8_t *stack, const uint8_t *gt, int batch, float lr, float *loss, int mem_kind);
/* True positives, false positives, false negatives of the last step's predictions at sigmoid > 0.5. */
int covahip_train_metrics(covahip_train *tr, int64_t tp_fp_fn[3]);
/* The current weights as a weight file (moving statistics in the BN mean / var slots); *n = its size.  COVAHIP_ERR_OVERFLOW
 * when cvhw is NULL or cap < *n. */
int covahip_train_weights(covahip_train *tr, void *cvhw, size_t cap, size_t *n);
/* The last step's gradients, n = 320305 floats in weight-file order; the BN mean / var slots hold the step's batch mean and
 * biased batch variance. */
int covahip_train_grads(covahip_train *tr, float *flat, size_t n);
/* Training sets: one trainer holds K models of ONE geometry and cfg (e.g. one BlobNet per camera, the input of
 * covahip_blobnet_load_set), each with its own weights, Adam moments, BN moving statistics, step counter, dropout seed and, per
 * step, its own batch and learning rate.  A set step takes one step of every model in ONE launch of each kernel: the number of
 * launches does not depend on K, and K small-batch trainings fill the GPU as one large batch would.
 *   1 <= n_models <= COVAHIP_MAX_MODELS; weights[k] / weights_bytes[k]: model k's initial weight file; seeds[k]: its dropout seed
 *   (seeds NULL: cfg->seed for every model).  All or nothing: a bad blob in any slot is COVAHIP_ERR_BAD_WEIGHTS, checked before
 *   anything is allocated.  A set whose totals would pass a 32-bit sample index or a grid extent is COVAHIP_ERR_UNSUPPORTED.
 *   Memory: K * max_batch samples of activations (about 5 MB each at 45x80) plus four parameter-sized buffers (1.3 MB each) per
 *   model.
 * Contract: model k of a set is BIT-IDENTICAL to the same model trained alone.  Its loss, gradients, TP / FP / FN, weights,
 * moving statistics and Adam state after any sequence of set steps equal those of a covahip_train_create trainer with the same
 * initial weights, the same cfg and seed = seeds[k], fed model k's (stack, gt, batch, lr) steps with the set steps in which it
 * had batch 0 left out.  (Every reduction splits by the model's OWN batch, whatever the others take in that step.)
 * covahip_train_create is a set of one; the entries without _m mean model 0.  covahip_train_step on a set of more than one
 * model is COVAHIP_ERR_INVALID_ARG. */
int covahip_train_create_set(covahip_ctx *ctx, const covahip_train_cfg *cfg, int n_models, const void *const *weights,
                             const size_t *weights_bytes, const uint64_t *seeds, covahip_train **out);
int covahip_train_num_models(covahip_train *tr, int *n_models);
/* One step of every model k with batches[k] > 0.  Sample order: PACKED in model order -- stack holds the batches[0] stacks of
 * model 0, then the batches[1] stacks of model 1 and so on (sum of batches stacks in all), gt likewise; mem_kind applies to both.
 * batches / lrs / losses: HOST arrays of n_models entries.  0 <= batches[k] <= max_batch.  A model with batches[k] = 0 sits the
 * step out: NOTHING of it changes (weights, moving statistics, Adam state, step counter, last gradients and metrics) and
 * losses[k] = 0.  All batches 0, a batch above max_batch, a NULL array or a negative / non-finite lr: COVAHIP_ERR_INVALID_ARG.
 * Synchronous. */
int covahip_train_step_set(covahip_train *tr, const uint8_t *stack, const uint8_t *gt, const int32_t *batches, const float *lrs,
                           float *losses, int mem_kind);
/* covahip_train_metrics / _weights / _grads of model `model` (its last step; outside [0, n_models): COVAHIP_ERR_INVALID_ARG). */
int covahip_train_metrics_m(covahip_train *tr, int model, int64_t tp_fp_fn[3]);
int covahip_train_weights_m(covahip_train *tr, int model, void *cvhw, size_t cap, size_t *n);
int covahip_train_grads_m(covahip_train *tr, int model, float *flat, size_t n);
/* Evaluation and resume.
 * Evaluation: the forward of the training step in INFERENCE mode, on samples the caller holds out.  Two differences from the
 * step's forward: BatchNorm normalises with the model's MOVING mean / variance ((x - mean) * (1 / sqrt(var + bn_eps)) * gamma +
 * beta, the expression of the step with the moving values in place of the batch's), and every dropout site is the identity.
 * This is the arithmetic of covahip_blobnet_forward in fp32.  Per-sample loss = the Jaccard distance of the sample as the step
 * forms it (I = sum y*p, S = sum (y + p) over H x W, (1 - (I + s) / (S - I + s)) * s, s = cfg.smooth); the result's loss is the
 * mean of the per-sample values, summed in double on the host in sample order.  Valid before any step: it scores the weights
 * the trainer was created with.
 *   Contract A -- a sample's result depends on the sample and the model only.  Its logits, its sample_loss and its contribution
 *   to TP / FP / FN are BIT-IDENTICAL whatever n, max_batch, the sample's position, mem_kind, and whether the model is evaluated
 *   alone or as model k of a set next to others.  (Nothing in an inference-mode forward couples the samples of a batch.)
 *   Contract B -- evaluation is invisible to training.  It changes no weight, no moving statistic, no Adam moment, no step
 *   counter, and neither covahip_train_grads nor covahip_train_metrics (they keep describing the last TRAINING step).  A
 *   training step after an evaluation is bit-identical to the same step without it. */
typedef struct covahip_train_eval_result {
    double  loss;            /* mean over the samples of the per-sample Jaccard distance (smooth = cfg.smooth) */
    int64_t tp, fp, fn;      /* at sigmoid > 0.5 (logit > 0), summed over the samples                           */
    int64_t samples;
} covahip_train_eval_result;
/* n >= 1 samples, ANY n (the library walks them in chunks of cfg.max_batch): stack u8 [n][4*h_mb][w_mb][4], gt u8 [n][h_mb][w_mb].
 * sample_loss: f32 [n] or NULL.  logits: f32 [n][h_mb][w_mb] or NULL.  mem_kind applies to stack, gt, sample_loss and logits.
 * Synchronous. */
int covahip_train_eval(covahip_train *tr, const uint8_t *stack, const uint8_t *gt, int n,
                       float *sample_loss, float *logits, covahip_train_eval_result *out, int mem_kind);
/* Every model of a set on its own samples in one launch of each kernel per chunk: counts[k] >= 0 samples of model k (HOST array
 * of n_models entries, any size, not all 0), packed in model order as covahip_train_step_set takes them; sample_loss / logits in
 * the same packing; out: HOST [n_models]; a model with counts[k] = 0 gets zeros.  covahip_train_eval on a set of more than one
 * model is COVAHIP_ERR_INVALID_ARG (as covahip_train_step). */
int covahip_train_eval_set(covahip_train *tr, const uint8_t *stack, const uint8_t *gt, const int32_t *counts,
                           float *sample_loss, float *logits, covahip_train_eval_result *out, int mem_kind);
/* Trainer state: everything a training needs to continue, as ONE little-endian blob for the whole trainer (solo or set).
 *   offset  0  u32 magic "CVHS" (0x53485643)     4  u32 version = 1        8  u32 n_models      12  u32 n_params = 320305
 *          16  i32 h_mb    20  i32 w_mb          24  f32 lr, beta1, beta2, eps, bn_momentum, bn_eps, dropout, smooth (the
 *          creating cfg, for information)        56  u64 user_tag (the caller's: an epoch number, say)
 *          64  per model, n_models times: u64 step (steps taken: Adam's t, the dropout hash's step), u64 seed (dropout),
 *              f32 params[n_params] (a weight file's payload, moving statistics included), f32 adam_m[n_params],
 *              f32 adam_v[n_params]
 *          end u32 CRC-32C (Castagnoli, as TFRecord frames use it, unmasked) of every byte before it
 *   Contract C -- exact resume.  Take any trainer after any sequence of steps, save, and load the blob into a trainer created
 *   with the same cfg and n_models from ANY initial weights and seeds.  From then on both trainers are bit-identical: losses,
 *   gradients, metrics, weights, moving statistics, Adam state, for every model, including models that sat steps out.  The
 *   seeds come from the blob.
 * covahip_train_save_state: *n = the blob's size; COVAHIP_ERR_OVERFLOW when buf is NULL or cap < *n (as covahip_train_weights).
 * covahip_train_load_state: all or nothing, validated before anything is copied.  Wrong magic / version / size / CRC:
 * COVAHIP_ERR_BAD_DATA; n_models or n_params not the trainer's: COVAHIP_ERR_INVALID_ARG; the trainer is then untouched.  The
 * geometry and cfg scalars of the header are not compared (the parameters do not depend on them).  After a load
 * covahip_train_grads / _metrics describe no step: zeros.  *user_tag (may be NULL) = the tag given to save. */
int covahip_train_state_size(covahip_train *tr, size_t *n);
int covahip_train_save_state(covahip_train *tr, uint64_t user_tag, void *buf, size_t cap, size_t *n);
int covahip_train_load_state(covahip_train *tr, const void *buf, size_t n, uint64_t *user_tag);
/* Fine-tuning: a training plan says which layer groups a step trains and which BatchNorm layers run in inference mode -- what
 * Keras does with `trainable = False` (the variable is not given to the optimiser; a BatchNormalization layer normalises with
 * its moving statistics and does not update them).  One plan per trainer: in a set it holds for every model, like cfg.
 *   Groups: encoder level i = enc{i}.conv.kernel / .bias, enc{i}.bn.gamma / .beta, enc{i}.tmix.w1 / .w2; decoder block j =
 *   dec{j}.up.kernel / .bias, dec{j}.bn.gamma / .beta, and for j = 3 final.kernel / final.bias.
 *   A FROZEN group: none of its tensors and none of their Adam moments changes in a step, its slots in covahip_train_grads
 *   read 0, and its BatchNorm is in inference mode: the effective bn_inference = given | (frozen_groups & 0x7F).  Gradients
 *   still flow THROUGH it to trainable groups nearer the input.
 *   A BN layer in INFERENCE MODE: forward (x - moving_mean) * (1 / sqrt(moving_var + bn_eps)) * gamma + beta, the expression
 *   of covahip_train_eval; its moving statistics are not updated; backward dx = dy * gamma / sqrt(moving_var + bn_eps), no
 *   batch-mean terms.  Where its group is not frozen gamma and beta are still trained: dgamma = sum dy * xhat, dbeta = sum dy
 *   with xhat formed from the moving statistics.  Its mean / var slots of covahip_train_grads hold the moving values the
 *   forward normalised with.  The convT bias in front of such a layer has a real, non-zero gradient (a batch-mode layer
 *   subtracts the bias again).
 *   Unchanged by any plan: the dropout hash (site, step) -- dropout stays active in frozen groups, this is training mode --,
 *   Adam's t, the loss, TP / FP / FN.
 *   Work follows the plan: no weight gradient is computed for a frozen group, and the backward pass stops where nothing
 *   trainable lies nearer the input (encoder frozen: nothing of the encoder's backward runs).
 * covahip_train_set_plan: takes effect from the next step and may be changed between steps; the default is the empty plan.
 * Bits outside the fields, a NULL argument, or all eight groups frozen: COVAHIP_ERR_INVALID_ARG, the trainer untouched.
 * covahip_train_get_plan: the EFFECTIVE plan (frozen_groups as given, bn_inference with the frozen groups' layers).
 *   Contract D -- the empty plan is no plan.  A trainer that never sets a plan, or sets the empty one, is the trainer described
 *   above, bit for bit: losses, gradients, weights, moving statistics, Adam state.
 *   The other contracts hold under any plan: model k of a set equals the solo trainer with the same plan; evaluation
 *   (Contracts A and B) does not depend on the plan; exact resume (Contract C) holds with the plan set again by the caller, as
 *   the cfg is created again -- the plan is not in the state blob and covahip_train_load_state does not touch it.  A model
 *   that sits a set step out keeps its last gradients, also in slots a newer plan freezes. */
typedef struct covahip_train_plan {
    uint32_t frozen_groups; /* bit i (0..3): encoder level i; bit 4 + j (j = 0..3): decoder block j */
    uint32_t bn_inference;  /* bit i (0..3): enc{i}.bn; bit 4 + j (j = 0..2): dec{j}.bn              */
} covahip_train_plan;
int covahip_train_set_plan(covahip_train *tr, const covahip_train_plan *plan);
int covahip_train_get_plan(covahip_train *tr, covahip_train_plan *plan);
/* Training with a post: the camera's ignore region and mask threshold (covahip_blobnet_set_post, the sidecar of
 * covahip_post_sweep) in the loss and the metrics, so that a model is trained on, and scored as, what serving lets through.
 * Each model of a trainer (solo or set) has its own post: device tables of u8 [K][h_mb * w_mb] keep maps, a threshold and a
 * flag per model, written by covahip_train_set_post only -- no launch is added to a step or an evaluation chunk and nothing is
 * uploaded per step.  For a model WITH a post and keep'[y,x] = keep ? keep[y,x] != 0 : 1:
 *   Loss (the step's, and sample_loss of an evaluation): I = sum over keep' of y*p, S = sum over keep' of (y + p); everything
 *   else as without: (1 - (I + s) / (S - I + s)) * s per sample, the step's loss the mean over the model's batch.
 *   Backward: d loss / d logit = 0 where !keep', elsewhere the expression of a step without a post with the masked I and S.
 *   Nothing downstream changes: the weight-gradient reductions and all other layers run as they are.
 *   Metrics (covahip_train_metrics[_m] and the evaluation result): TP / FP / FN over keep' pixels only, with
 *   pos = logit > logit_thresh -- serving's expression, so NaN counts as background -- and lab = gt != 0.
 *   The threshold affects the counts only, never the loss.
 * A model WITHOUT a post: everything exactly as described above, pos = sigmoid(logit) > 0.5f included.
 * covahip_train_set_post: takes effect from the next step or evaluation; may be set, changed or removed (post == NULL) between
 * steps.  Like the training plan the post is NOT part of the state blob: covahip_train_load_state does not touch it, and a
 * resumed run sets it again.  All errors are checked on the host and leave the trainer untouched: COVAHIP_ERR_INVALID_ARG for a
 * NULL trainer, a model outside the set, a non-finite threshold, or a keep map without a single non-zero byte (there would be
 * nothing to train on).
 * covahip_train_get_post: logit_thresh (0 without a post), keep_or_null (u8 [h_mb][w_mb], written as 0 / 1; all 1 without a
 * keep map or a post) and has_post may each be NULL.
 *   Contract E -- no post is no post.  A trainer that never sets a post, or has removed every one, launches the kernels it
 *   launched before posts existed: it is that trainer, bit for bit.
 *   Contract F -- an all-ones keep map changes no float.  With a post whose keep map is all non-zero or NULL, at any threshold,
 *   losses, gradients, weights, Adam moments, moving statistics, sample_loss and logits are BIT-IDENTICAL to the model without a
 *   post; only the counts follow the threshold.  (An ignored pixel is skipped by a select inside the loops and slabs of the
 *   reductions; their order is the same.)
 *   Contract G -- what is ignored does not exist.  Changing the label bytes at ignored macroblocks to any values changes no
 *   output bit: loss, gradients, weights, counts, sample_loss.
 *   Sets: model k of a set with post k is bit-identical to the solo trainer with that post, and a post on model k changes
 *   nothing of model j.  Models with and without a post share each launch: the masked kernel forms run while any model of the
 *   trainer has a post, and a model without one keeps its expressions through its flag.
 *   Contracts A - D hold with "the model" read as "the model and its post"; a post combines with any training plan. */
int covahip_train_set_post(covahip_train *tr, int model, const covahip_blobnet_post *post /* NULL = no post */);
int covahip_train_get_post(covahip_train *tr, int model, float *logit_thresh, uint8_t *keep_or_null, int *has_post);
/* Training arithmetic: which kernels compute the convolutions of a step and of an evaluation.  Both are fp32 throughout and
 * compute the same sums; they differ in the ORDER of the additions inside a sum, so their results differ in the last bits.
 *   COVAHIP_TRAIN_MATH_EXACT (the default): the plain kernels described above, one thread per output element or per weight.
 *   They are the path pinned against f64 autograd and bit-reproducible against every earlier checkpoint.
 *   COVAHIP_TRAIN_MATH_MATRIX: the 3x3 convolution's forward, data gradient and weight gradient and the transposed
 *   convolution's weight gradient run as implicit GEMMs on the fp32-input matrix instruction (v_mfma_f32_16x16x4_f32: an fmaf
 *   chain in k order, one rounding per product).  Everything else -- the transposed convolution's forward and data gradient,
 *   BatchNorm, pooling, the temporal MLP, dropout, the loss, Adam -- runs the kernels of the exact mode.  No loss scaling, no
 *   other tolerance, no change to the weight file.
 * The guarantees of the trainer hold in either mode, each within its mode: no float atomics, a step is bit-reproducible, batch
 * b of max_batch equals batch b of b, model k of a set equals the solo trainer, a skipped model is not touched, exact resume,
 * frozen groups launch no weight-gradient work.  A matrix-mode run is NOT bit-identical to an exact-mode run.
 * covahip_train_set_math: may be called between steps; applies to all models of a set; synchronous.  Every kernel limit of the
 * matrix mode is checked here by a planning pass over the trainer's geometry at max_batch (COVAHIP_ERR_UNSUPPORTED, the mode
 * unchanged; none of the geometries covahip_train_create admits is refused).  An unknown value is COVAHIP_ERR_INVALID_ARG
 * and changes nothing.  Like the plan and the post the mode is NOT part of the state blob: a checkpoint written in one mode
 * loads in the other, and a resumed run sets the mode again.
 *   Contract H -- exact is what was.  A trainer that never calls covahip_train_set_math, or calls it with
 *   COVAHIP_TRAIN_MATH_EXACT, launches the kernels it launched before the mode existed, with the same arguments. */
enum {
    COVAHIP_TRAIN_MATH_EXACT = 0,
    COVAHIP_TRAIN_MATH_MATRIX = 1
};
int covahip_train_set_math(covahip_train *tr, int math);
int covahip_train_get_math(covahip_train *tr, int *math);
void covahip_train_destroy(covahip_train *tr);

/* ------------------------------------------------------------ Training data
 * A device-resident training data set: the frames of any number of recordings (of any mix of cameras, of ONE geometry) with their
 * labels, and a trainer that takes its batches from it by a table of frame indices.  A stack is four frame indices, as the
 * stack_index of covahip_filter_forward_frames has it, so a recording of F frames holds F - 3 windows (metapreprocess at
 * gamma = 4 emits F / 4 of them), and since bytes 1 and 2 of a record are motion-vector MAGNITUDES a mirrored frame and a
 * time-reversed window are valid records too: no field changes sign.
 *   Storage: records u16 [capacity][h_mb][w_mb], packed exactly as covahip_carrier_pack packs them (everything BlobNet keeps of a
 *   record: the step's first operation is clip(x, 0, 6)), and labels u8 [capacity][h_mb][w_mb], the bytes AS GIVEN -- not reduced
 *   to 0 / 1, the loss reads the byte as a float.  3 bytes per macroblock against 5 of the frames appended; the capacity is fixed at
 *   creation (16 <= h_mb, w_mb <= 1024, 1 <= capacity_frames < 2^31) and all element offsets are 64-bit.
 *   A sample names GLOBAL frame indices of the data set: */
typedef struct covahip_train_data covahip_train_data;
typedef struct covahip_train_sample {   /* 24 bytes */
    int32_t  frame[4];   /* the frames of the T = 0 (current) .. 3 (oldest) slices, as stack_index names them */
    int32_t  label;      /* the frame whose gt labels the sample (frame[0] for a forward window)            */
    uint32_t flags;      /* bit 0 mirror x, bit 1 mirror y; any other bit: COVAHIP_ERR_INVALID_ARG           */
} covahip_train_sample;
/*   The batch a table of n samples describes: stack u8 [n][4 * h_mb][w_mb][4] and labels u8 [n][h_mb][w_mb] with
 *       stack[b][t * h_mb + y][x] = (min(class, 6), min(mv_x, 6), min(mv_y, 6), 0) of frame[t] at (y', x'),
 *       label[b][y][x]           = the gt byte of frame `label` at (y', x'),
 *       x' = w_mb - 1 - x when bit 0 of flags is set, else x;  y' = h_mb - 1 - y when bit 1 is set, else y.
 *   ONE launch builds the stacks and the labels of all n samples (of all models of a set step).
 * Calling rules.  `samples` is always a HOST array.  Every call is synchronous, on the ctx's primary stream, ordered as
 * covahip_train_step is.  Every check runs on the host before anything is launched and a refused call changes nothing:
 * COVAHIP_ERR_INVALID_ARG for a NULL array, an index outside [0, frames), an unknown flag bit, a data set whose geometry (or
 * ctx) is not the trainer's, and what the pointer form of the call refuses (a batch above max_batch among it);
 * COVAHIP_ERR_OVERFLOW for an append past the capacity.
 * covahip_train_data_append: n >= 1 frames u8 [n][h_mb][w_mb][4] (byte 3 is ignored) and gt u8 [n][h_mb][w_mb]; mem_kind applies
 * to both.  Device frames are packed by a kernel; host frames with covahip_carrier_pack, and two bytes per macroblock are
 * uploaded.  *first_index (may be NULL) = the index of the first frame appended: the n frames are [first, first + n).
 * Device pointers: frames and gt any alignment (frames off a 4-byte boundary are read byte by byte).
 * covahip_train_data_gather: the batch itself, for a caller that wants to see it (mem_kind applies to stack and gt).  A DEVICE
 * stack must be 4-byte aligned (the launch stores a record's four bytes at once): COVAHIP_ERR_INVALID_ARG otherwise; a device
 * gt may have any alignment (label bytes are stored one at a time).
 * covahip_train_data_label_mass: how much label each of the frames [first, first + n) carries AS A CAMERA IS SERVED, for a
 * sampler that wants to tell busy frames from quiet ones (utils/data/balance.py's reduce_sum(y) >= threshold) without taking
 * the labels off the device:
 *       mass[i] = the number of macroblocks (y, x) of frame first + i with gt != 0 (the trainer's `lab`) and keep'[y,x],
 *       keep'[y,x] = keep ? keep[y,x] != 0 : 1 (covahip_train_set_post's definition; keep_or_null is a HOST array u8 [h_mb * w_mb]).
 *   Integer counts, exact; for 0 / 1 labels without a keep map the reference's label sum.  A label byte at an ignored macroblock
 *   counts nothing whatever its value (Contract G).  mem_kind applies to `mass` (a DEVICE mass must be 4-byte aligned); one launch
 *   sequence serves any n up to the capacity, and a host mass moves through the data set's staging.
 *   COVAHIP_ERR_INVALID_ARG, checked on the host before anything is launched and with nothing written: a NULL d or mass, n < 1,
 *   first < 0, first + n > frames, an unknown mem_kind, a misaligned device mass, or a keep map without a single non-zero byte
 *   (as covahip_train_set_post refuses it). */
int  covahip_train_data_create(covahip_ctx *ctx, int h_mb, int w_mb, int64_t capacity_frames, covahip_train_data **out);
int  covahip_train_data_append(covahip_train_data *d, const uint8_t *frames, const uint8_t *gt, int n, int mem_kind,
                               int64_t *first_index);
int  covahip_train_data_frames(const covahip_train_data *d, int64_t *n);
int  covahip_train_data_gather(covahip_train_data *d, const covahip_train_sample *samples, int n, uint8_t *stack, uint8_t *gt,
                               int mem_kind);
int  covahip_train_data_label_mass(covahip_train_data *d, int64_t first, int64_t n, const uint8_t *keep_or_null, uint32_t *mass,
                                   int mem_kind);
/* covahip_train_data_record_stats: the input statistics of frames [first, first + n) of the data set, each counted once, as the
 * serving side counts them ("Input monitor" above: the same quantities from the resident packed records, r = record & 511, as
 * one model's; no keep map), so that a recording can be judged before training and compared with a deployed camera.  The
 * training side adds what only it can know, from the label bytes:
 *       hist_set[r(p)] += 1 for every macroblock p of the range whose label byte is non-zero,
 *       set_total       = the number of such macroblocks = the sum of covahip_train_data_label_mass over the same frames
 *                         without a keep map.
 *   `out` holds HOST pointers, each may be NULL.  Every record and label byte is read once per call; any n up to the capacity in
 *   one call.  The calling rules are covahip_train_data_label_mass's.
 *   COVAHIP_ERR_INVALID_ARG, checked on the host before anything is launched and with nothing written: a NULL d or out, n < 1,
 *   first < 0, first + n > frames. */
typedef struct covahip_record_stats {
    int64_t *frames;        /* [1]: n                                            */
    int64_t *hist;          /* [512]                                             */
    int64_t *hist_set;      /* [512]                                             */
    int64_t *set_total;     /* [1]                                               */
    int64_t *moving;        /* [h_mb][w_mb]                                      */
    int64_t *still_frames;  /* [1]                                               */
    int64_t *intra_frames;  /* [1]                                               */
    int64_t *move_hist;     /* [16]                                              */
} covahip_record_stats;
int  covahip_train_data_record_stats(covahip_train_data *d, int64_t first, int64_t n, const covahip_record_stats *out);
/* covahip_train_data_align: whether the labels of ONE recording, frames [first, first + n), stand at the frames of their records.
 * Records come from the entropy front end and labels from a pixel decoder; a frame dropped by either moves every label by a few
 * frames against its record, and nothing else in training shows it.  The counts compare where the records MOVE with where the
 * labels are SET, per frame and per shift s in -S .. S.  The fields of a record are those covahip_carrier_pack stores: class in
 * bits 0-2, mv_x in bits 3-5, mv_y in bits 6-8.
 *       moves_f[p] = keep'[p] and (min_mv > 0 and max(mv_x, mv_y) >= min_mv   or   bit `class` of class_mask) of frame f at p,
 *       set_f[p]   = keep'[p] and gt_f[p] != 0,            keep' as covahip_train_data_label_mass has it;
 *   for i in [0, n), f = first + i, j in [0, 2 S + 1), s = j - S and g = f + s:
 *       both[i][j] = #{p : moves_f[p] and set_g[p]} when first <= g < first + n, else 0 (a shift never reads a neighbouring
 *                    recording),
 *       mov[i]     = #{p : moves_f[p]},        lab[i] = #{p : set_f[p]}  (covahip_train_data_label_mass of the same frame and map).
 *   Sign: s > 0 reads "the label that belongs to record frame f stands at f + s".  Integer counts, exact; a label byte at an
 *   ignored macroblock counts nothing whatever its value (Contract G).  mem_kind applies to the three outputs (DEVICE outputs
 *   4-byte aligned); host outputs move through the data set's staging in chunks of frames.  Every record and label byte is read
 *   once per call, apart from 2 S label frames per 32 frames; the 2 S + 1 shifts are scored on bit planes in LDS.
 *   COVAHIP_ERR_INVALID_ARG, checked on the host before anything is launched and with nothing written: a NULL pointer, n < 1, a
 *   range outside the data set, max_shift outside 0 .. 32, min_mv outside 0 .. 6, a class bit >= 7, min_mv == 0 with
 *   class_mask == 0 (nothing can move), a keep map without a single non-zero byte, an unknown mem_kind, a misaligned device
 *   output. */
typedef struct covahip_align_cfg {
    int32_t  max_shift;   /* S: shifts -S .. S are scored; 0 <= S <= 32                                             */
    int32_t  min_mv;      /* 1 .. 6: a macroblock MOVES when max(mv_x, mv_y) of its packed record >= min_mv; 0: the
                             vectors decide nothing                                                                  */
    uint32_t class_mask;  /* bit c, c in 0 .. 6: a macroblock whose packed class (min(class, 6)) is c moves whatever
                             its vectors say; bits 7.. must be 0                                                     */
    const uint8_t *keep;  /* HOST u8 [h_mb * w_mb] or NULL, covahip_train_set_post's keep' (non-zero = kept)         */
} covahip_align_cfg;
int  covahip_train_data_align(covahip_train_data *d, int64_t first, int64_t n, const covahip_align_cfg *cfg,
                              uint32_t *both /* [n][2S+1] */, uint32_t *mov /* [n] */, uint32_t *lab /* [n] */,
                              int mem_kind);
void covahip_train_data_destroy(covahip_train_data *d);
/* covahip_train_step / _step_set / _eval / _eval_set on samples of a data set: the gather launch writes the batch straight into
 * the trainer's own staging, in the packing the step expects; nothing is copied from the host but the table.  samples: packed in
 * model order (sum of batches / counts entries); eval takes any n, in chunks of max_batch, as covahip_train_eval does; mem_kind
 * of the eval forms applies to sample_loss and logits.
 *   Contract D (data) -- the data forms are BIT-IDENTICAL to their pointer forms on the stacks and labels the samples describe,
 *   the comparison stacks built from the frames AS THEY WERE APPENDED, field values above 6 included (the step clips them as the
 *   packing does): loss, gradients and metrics; weights, moving statistics, Adam state and step counter; logits and sample
 *   losses.  The step itself is unchanged, only the way its staging gets filled is new: contracts A, B and C, the bit-identity
 *   of a set's models, the training plan and the post hold as written. */
int covahip_train_step_data(covahip_train *tr, covahip_train_data *d, const covahip_train_sample *samples, int batch, float lr,
                            float *loss);
int covahip_train_step_set_data(covahip_train *tr, covahip_train_data *d, const covahip_train_sample *samples,
                                const int32_t *batches, const float *lrs, float *losses);
int covahip_train_eval_data(covahip_train *tr, covahip_train_data *d, const covahip_train_sample *samples, int n,
                            float *sample_loss, float *logits, covahip_train_eval_result *out, int mem_kind);
int covahip_train_eval_set_data(covahip_train *tr, covahip_train_data *d, const covahip_train_sample *samples,
                                const int32_t *counts, float *sample_loss, float *logits, covahip_train_eval_result *out,
                                int mem_kind);

/* ------------------------------------------------------------ MoG labels
 * The training labels of the reference's "train from scratch" flow, made on the GPU: what utils/generate-mog.py does with
 * OpenCV to a decoded video, per frame in decode-output order, per video:
 *   1. resize to 640x360 (cv.resize INTER_LINEAR).  Three source sizes, any other is COVAHIP_ERR_UNSUPPORTED:
 *        640x360 copy; 1280x720 (OpenCV's area-fast path at an exact 2x scale) (a + b + c + d + 2) >> 2 per channel over the
 *        2x2 block; 1920x1080 (linear weights (1, 0) at an exact 3x scale) source pixel (3x + 1, 3y + 1);
 *   2. MOG2 of createBackgroundSubtractorMOG2(history, var_threshold, detectShadows = false), apply() with the default
 *      learning rate (below);
 *   3. fg = mask > 0 (with shadows dropped, covahip_mog_set_shadows: fg = mask == 255);
 *   4. close with a 4x4 ones kernel, then open with a 6x6 ones kernel.  OpenCV's anchor k/2, the same offsets for erode and
 *      dilate: the window at x covers x - 2 .. x + 1 (4x4) and x - 3 .. x + 2 (6x6) in both axes; outside the image is 0 for
 *      dilate and 1 for erode;
 *   5. contour fill (findContours RETR_EXTERNAL + drawContours FILLED) as hole filling: foreground 8-connected, background
 *      4-connected, every background 4-component that does not touch the image edge becomes 1;
 *   6. label[i][j] = filled[8i][8j]: 45x80 bytes of 0 / 1 per frame, the file `tfrecordsink gt=` reads (frames one after the
 *      other, as ndarray.tofile writes them).  That is the label mode COVAHIP_MOG_LABELS_CORNER, the default and the
 *      reference's cl_op_fill[::8, ::8]; covahip_mog_set_labels (below) chooses another per labeller.  With F the filled mask
 *      of step 5, mw x mh working pixels, block (i, j) is the pixels y in [8i, min(8i + 8, mh)), x in [8j, min(8j + 8, mw));
 *      `inside` is their number (64, except in a last label row or column that is only started) and `count` how many of them
 *      are 1 in F.  Nothing at x >= mw or y >= mh is counted or inside.
 *        COVAHIP_MOG_LABELS_CORNER  label = F[8i][8j];
 *        COVAHIP_MOG_LABELS_COVER   with min_cover N in 1 .. 64: label = 1 iff 64 * count >= N * inside, else 0.  N = 1: any
 *                                   foreground pixel in the block; N = 32: at least half of what the image holds of the block;
 *                                   N = 64: all of it.  COVER(1) holds every CORNER label, and COVER(N) shrinks as N grows;
 *        COVAHIP_MOG_LABELS_COUNT   label = count, a byte 0 .. 64, > 0 exactly where COVER(1) is 1.  For inspection and for
 *                                   choosing N (tools/label_cover.py): it is not a trainer input.
 *      The opening guarantees an object only a 6x6 square and a corner sits every 8 pixels, so CORNER gives an object narrower
 *      than 8 working pixels a label only where it straddles a corner ("MoG labels by coverage").
 * That is the reference grid (COVAHIP_MOG_GRID_REFERENCE): 45x80 is the macroblock grid of a 1280x720 stream, whatever the
 * source.  The macroblock grid (COVAHIP_MOG_GRID_MACROBLOCK) labels the source's own 16x16 macroblocks; it differs in two steps:
 *   1. the working image is half the source in both axes, by the exact-2x rule above ((a + b + c + d + 2) >> 2 per channel over
 *      the 2x2 block): 1920x1080 -> 960x540, 1280x720 -> 640x360 (the reference grid itself: the same labels, masks and model,
 *      byte for byte), 640x360 -> 320x180, and two sizes that only this grid takes (the reference grid answers
 *      COVAHIP_ERR_UNSUPPORTED): 2560x1440 -> 1280x720 and 3840x2160 -> 1920x1080; any other size is COVAHIP_ERR_UNSUPPORTED;
 *   6. one label for every i, j with 8i < working height and 8j < working width, in the default mode filled[8i][8j], the pixel
 *      at the top-left corner of macroblock (i, j): 68x120 (the last row reads working row 536), 45x80, 23x40 (row 176), 90x160 and 135x240
 *      (a 4K grid; row 1072) bytes per frame.
 * Steps 2 - 5 are the same: the 4x4 / 6x6 kernels stay in working pixels, the same size relative to a macroblock.
 * MOG2 (the CPU path of OpenCV 4.x MOG2Invoker, nmixtures 5).  All values f32 unless noted, every product and sum rounded on
 * its own (no fused multiply-add), divisions correctly rounded:
 *   constants Tb = var_threshold, TB = 0.9, Tg = 9, varInit = 15, varMin = 4, varMax = 75, fCT = 0.05f;
 *   per frame: n += 1 (this stream's frames, from 1); lr = 1.0 / min(2n, history) in double; alphaT = (float)lr;
 *     alpha1 = 1 - alphaT; prune = (float)(-lr * (double)0.05f).  The model starts all zero with nmodes = 0, so frame 1 is
 *     all foreground;
 *   per pixel, data = the three channels as float:
 *     1. fits = false, bg = false, tw = 0;
 *     2. for mode = 0 while mode < nmodes (the bound shrinks when a mode is pruned):
 *          w = alpha1 * W[mode] + prune; swaps = 0;
 *          if !fits: d = M[mode] - data per channel; dist2 = (d0*d0 + d1*d1) + d2*d2;
 *            if tw < TB && dist2 < Tb * V[mode]: bg = true;
 *            if dist2 < Tg * V[mode]: fits = true; w += alphaT; k = alphaT / w; M[mode] -= k * d per channel;
 *              V[mode] = min(max(V + k * (dist2 - V), varMin), varMax);
 *              for i = mode down to 1: stop if w < W[i-1], else swap entries i and i-1 (weight, variance, mean), swaps++;
 *          if w < -prune: w = 0, nmodes--;
 *          W[mode - swaps] = w; tw += w;
 *     3. inv = |tw| > FLT_EPSILON ? 1 / tw : 0; W[i] *= inv for i < nmodes;
 *     4. if !fits: slot m = nmodes == 5 ? 4 : nmodes++; if nmodes == 1: W[m] = 1, else W[m] = alphaT and W[i] *= alpha1 for
 *        i < nmodes - 1; M[m] = data; V[m] = varInit; for i = nmodes - 1 down to 1: stop if alphaT < W[i-1], else swap;
 *     5. mask = bg ? 0 : 255.
 *   2a. The shadow test (covahip_mog_set_shadows below; off by default, and then none of this runs).  It is detectShadowGMM of
 *     OpenCV 4.x bgfg_gaussmix2.cpp, what createBackgroundSubtractorMOG2(.., detectShadows = true) adds, restated: this text is
 *     the contract, and tests/test_mog_shadow_host.py compares it with cv2 wherever cv2 is installed.  Per pixel, after steps
 *     1 - 4 on the UPDATED model (the new mode of step 4, the renormalised weights and the new nmodes included), only where bg
 *     is false.  All values f32, every product and sum rounded on its own, the division correctly rounded; tau is the shadow
 *     threshold:
 *       tw = 0
 *       for mode = 0 .. nmodes - 1:
 *           num = ((0 + data0*M0) + data1*M1) + data2*M2;   den = ((0 + M0*M0) + M1*M1) + M2*M2     (M = M[mode])
 *           if den == 0: not a shadow, stop
 *           if num <= den && num >= tau * den:
 *               a = num / den;  dD_c = a * M_c - data_c;  dist2a = ((0 + dD0*dD0) + dD1*dD1) + dD2*dD2
 *               if dist2a < ((Tb * V[mode]) * a) * a: a shadow, stop
 *           tw += W[mode];  if tw > TB: not a shadow, stop
 *       not a shadow
 *     mask = bg ? 0 : (shadow ? 127 : 255), OpenCV's values.  Two consequences, both checked by the tests:
 *       frame 1: every pixel's only mode is the pixel itself, so num == den, a = 1 and dist2a = 0: every pixel that is not
 *         (0, 0, 0) is a shadow, and a (0, 0, 0) pixel has den == 0 and is 255.  With shadows dropped, frame 1 is therefore
 *         nearly all background, where without the test it is all foreground;
 *       exact edges: after a constant (100, 120, 140) history, (50, 60, 70) is a shadow at tau = 0.5 (num = 22000 = tau * den
 *         exactly); (49, 60, 70) is not.
 * Streams: n_streams independent videos advance in one call, each with its own model and frame count.  Memory: about 23 MB of
 * model per stream (101 bytes per working pixel: 52 MB at 960x540, 93 MB at 1280x720, 209 MB at 1920x1080; many 4K streams can
 * exhaust device memory, and create then answers COVAHIP_ERR_HIP).  Every call is synchronous. */
enum { COVAHIP_MOG_MAX_STREAMS = 1024, COVAHIP_MOG_LABEL_H = 45, COVAHIP_MOG_LABEL_W = 80 };
typedef struct covahip_mog covahip_mog;
typedef struct covahip_mog_cfg {
    int32_t src_w, src_h;       /* 640x360, 1280x720 or 1920x1080 (BGR24, or NV12 / I420 through covahip_mog_apply_yuv); on the
                                 * macroblock grid also 2560x1440 and 3840x2160; covahip_mog_create_any: any even size of
                                 * COVAHIP_MOG_ANY_MIN .. COVAHIP_MOG_ANY_MAX */
    int32_t n_streams;          /* independent videos advanced per call, 1 .. COVAHIP_MOG_MAX_STREAMS */
    int32_t history;            /* 9000 (generate-mog.py); >= 1 */
    float   var_threshold;      /* 32; finite and > 0 */
} covahip_mog_cfg;
/* generate-mog.py's settings: 1280x720 sources, one stream, history 9000, var_threshold 32. */
void covahip_mog_default_cfg(covahip_mog_cfg *cfg);
/* COVAHIP_ERR_UNSUPPORTED for another source size, COVAHIP_ERR_INVALID_ARG for streams, history or var_threshold out of range. */
int  covahip_mog_create(covahip_ctx *ctx, const covahip_mog_cfg *cfg, covahip_mog **out);
/* The same on either label grid; covahip_mog_create is the reference grid.  COVAHIP_ERR_INVALID_ARG for another `grid`,
 * COVAHIP_ERR_UNSUPPORTED for a size the grid does not take (2560x1440 and 3840x2160 are the macroblock grid's alone).  apply,
 * reset and destroy take either kind of labeller; in the comments below 45x80 stands for the labeller's label_h x label_w. */
enum { COVAHIP_MOG_GRID_REFERENCE = 0, COVAHIP_MOG_GRID_MACROBLOCK = 1 };
int  covahip_mog_create_grid(covahip_ctx *ctx, const covahip_mog_cfg *cfg, int grid, covahip_mog **out);
/* The macroblock grid at any source size: src_w and src_h even and within COVAHIP_MOG_ANY_MIN .. COVAHIP_MOG_ANY_MAX (16
 * macroblocks, the least a BlobNet is trained on; a plane row of at most 32 words), else COVAHIP_ERR_UNSUPPORTED, checked before
 * the ctx is touched as covahip_mog_create_grid does; streams, history and var_threshold as there.  The steps are exactly the
 * macroblock grid's: the working image is src/2 by the 2x2 rounded mean (work_w = src_w/2, work_h = src_h/2; either may be odd
 * and neither need be a multiple of 8 or 64), MOG2, close 4x4, open 6x6 and the hole fill in working pixels, and
 * label[i][j] = filled[8i][8j] for 8i < work_h, 8j < work_w: ceil(src_h/16) x ceil(src_w/16) labels, whose last row and column
 * read a started macroblock.  The image ends at column work_w - 1 and row work_h - 1: those are the edge the hole fill starts
 * from, and beyond them is 0 for dilate and 1 for erode.  1280x960 gives 60x80 labels, 704x576 36x44, 2592x1944 122x162.
 * Every entry below takes such a labeller: dims, apply, apply_yuv (NV12 and I420, both ranges, any admitted layout; a picture of
 * 960 rows in a taller coded surface is fine, nothing outside its rows is read), yuv_tight, reset and destroy, with n_valid,
 * ragged streams and mixed apply / apply_yuv calls as for the others.  This entry always runs the general kernels (geometry
 * as kernel arguments, the post kernel in row bands), also at a size covahip_mog_create_grid takes, where both give the same
 * labels, masks and model bit for bit (DESIGN.md section 4 has the rates of both).  Model memory is 101 bytes per pixel of the
 * working image at a row pitch of work_w rounded up to 64. */
enum { COVAHIP_MOG_ANY_MIN = 256, COVAHIP_MOG_ANY_MAX = 4096 };
int  covahip_mog_create_any(covahip_ctx *ctx, const covahip_mog_cfg *cfg, covahip_mog **out);
/* The label mode of step 6 and, for COVAHIP_MOG_LABELS_COVER, its min_cover N in 1 .. 64 (min_cover is read in that mode only).
 * A new labeller is in COVAHIP_MOG_LABELS_CORNER.  The setting holds for every later covahip_mog_apply and covahip_mog_apply_yuv
 * of the labeller, for all its streams, and covahip_mog_reset keeps it.  The model and the masks do not depend on it: a
 * labeller that switches modes between calls has, bit for bit, the state of one that never did.  COVAHIP_MOG_LABELS_COUNT
 * writes bytes 0 .. 64 and is not a trainer input.  COVAHIP_ERR_INVALID_ARG, with nothing changed: a NULL labeller, an unknown
 * mode, N outside 1 .. 64 in COVER mode.  covahip_mog_get_labels gives the setting back (min_cover: the last one set, 1 at
 * first); either pointer may be NULL. */
enum { COVAHIP_MOG_LABELS_CORNER = 0, COVAHIP_MOG_LABELS_COVER = 1, COVAHIP_MOG_LABELS_COUNT = 2 };
int  covahip_mog_set_labels(covahip_mog *m, int mode, int min_cover);
int  covahip_mog_get_labels(const covahip_mog *m, int *mode, int *min_cover);
/* Shadow detection (step 2a), per labeller.  COVAHIP_MOG_SHADOWS_OFF, the default, is the reference's detectShadows = false:
 * the test does not run, on the kernels that have none.  _DROP runs it and changes step 3 to fg = mask == 255: shadow pixels
 * enter close, open and fill as background, so a vehicle's cast shadow stays out of its label.  _KEEP runs it and leaves step 3
 * at mask > 0, which is what generate-mog.py would do with detectShadows = true: filled masks and labels are bit-identical to
 * _OFF, only the raw mask (covahip_dev_mog_masks) and the counts below differ; it is the inspection mode, which shows what _DROP
 * would remove before a label changes.  tau is read when mode != _OFF and must be finite with 0 < tau <= 1 (OpenCV's default
 * is 0.5; a shadow is at least tau times as bright as the background).  COVAHIP_ERR_INVALID_ARG, with nothing changed: a NULL
 * labeller, an unknown mode, such a tau.  covahip_mog_get_shadows gives the setting back (tau: the last one set, 0.5 at first);
 * either pointer may be NULL.  The setting holds for every later covahip_mog_apply and covahip_mog_apply_yuv, for all streams,
 * covahip_mog_reset keeps it, and it may change between calls.  The model does not depend on it (the test only reads the
 * model): a labeller that switches modes has, bit for bit, the state of one that never did.
 * covahip_mog_shadow_counts: of the last apply / apply_yuv call, per (frame, stream) as [n_frames][n_streams], the number of
 * raw-mask pixels at 127 (shadow) and at 255 (foreground) inside the image, exact integers counted on the device.  Either array
 * may be NULL; cap is the number of entries each holds, COVAHIP_ERR_OVERFLOW when that is fewer than n_frames * n_streams (with
 * *n_frames set, so a call with both NULL asks for the size).  Frames past a stream's n_valid give 0; in _OFF mode shadow is all
 * 0.  n_frames may be NULL. */
enum { COVAHIP_MOG_SHADOWS_OFF = 0, COVAHIP_MOG_SHADOWS_DROP = 1, COVAHIP_MOG_SHADOWS_KEEP = 2 };
int  covahip_mog_set_shadows(covahip_mog *m, int mode, float tau);
int  covahip_mog_get_shadows(const covahip_mog *m, int *mode, float *tau);
int  covahip_mog_shadow_counts(covahip_mog *m, uint32_t *shadow, uint32_t *foreground, size_t cap, int *n_frames);
/* The labeller's working size and label grid; any pointer may be NULL. */
int  covahip_mog_dims(const covahip_mog *m, int32_t *work_w, int32_t *work_h, int32_t *label_w, int32_t *label_h);
/* frames u8 [n_frames][n_streams][src_h][src_w][3]; labels u8 [n_frames][n_streams][45][80] (mem_kind applies to both; n_valid is
 * always a host pointer).  n_valid[s] <= n_frames: frames past it are ignored for stream s and their labels untouched (NULL = all).
 * n_frames >= 1.  Host frames are staged in launches of up to 1 GiB of frames. */
int  covahip_mog_apply(covahip_mog *m, const uint8_t *frames, int n_frames, const int32_t *n_valid,
                       uint8_t *labels, int mem_kind);
/* The same from decoder surfaces: 8-bit 4:2:0 frames as NV12 (VCN through VA-API or rocDecode) or I420 (avdec_h264), at the
 * caller's row pitch, plane offsets and strides, without a BGR24 copy.  Row r of plane p of (frame f, stream s) starts at
 *   base + f * frame_stride + s * stream_stride + offset[p] + r * pitch[p]       (64-bit arithmetic).
 * The Y plane is src_h rows of src_w bytes; NV12 chroma is src_h/2 rows of src_w bytes (U, V pairs); I420 has U and V planes of
 * src_h/2 rows of src_w/2 bytes.  The kernels read nothing outside those rows: not the padding behind a row, not the coded rows
 * behind the picture (1080 rows sit in 1088), not the gaps between frames.  From host memory the call copies, per (frame,
 * stream), the extent from the lowest plane start to the last byte of the last row (the row padding inside that extent
 * included) and nothing else, in launches within the stage budget; where the layout is frame-major and dense (stream_stride =
 * that extent, frame_stride = n_streams * stream_stride) a launch's frames are one copy.
 * Conversion, then the resize of step 1 above.  All values int32, >> arithmetic, sat clamps to 0 .. 255, h = 1 << 19,
 * uu = U - 128, vv = V - 128:
 *   limited range (the constants of OpenCV's cvtColor(.., COLOR_YUV2BGR_NV12 / _I420): round(c * 2^20) of 1.164, 2.018, 0.391,
 *   0.813, 1.596):              yy = max(0, Y - 16) * 1220542;
 *     B = sat((yy + h + 2116026 * uu) >> 20); G = sat((yy + h - 852492 * vv - 409993 * uu) >> 20); R = sat((yy + h + 1673527 * vv) >> 20);
 *   full range (JPEG, yuvj420p; round(c * 2^20) of 1.772, 0.714136, 0.344136, 1.402):      yy = Y << 20;
 *     B = sat((yy + h + 1858077 * uu) >> 20); G = sat((yy + h - 748826 * vv - 360853 * uu) >> 20); R = sat((yy + h + 1470104 * vv) >> 20).
 * Source pixel (X, Y) takes the chroma sample (X >> 1, Y >> 1), no interpolation, as cvtColor does.  Then: 640x360 copy; the 2x2
 * mean converts the block's four pixels (they share one chroma sample) and takes (a + b + c + d + 2) >> 2 per channel
 * (converting the mean of Y is not the same, because of sat); 1920x1080 on the reference grid converts the pixel at
 * (3x + 1, 3y + 1).  The working pixel is then (B, G, R) as floats, exactly as if covahip_mog_apply had been given the
 * converted frame: the same stream slots and model, so apply and apply_yuv calls may be mixed at will, on every source size
 * and grid.  n_valid, labels and mem_kind (which applies to base and labels) as for covahip_mog_apply; synchronous.
 * COVAHIP_ERR_INVALID_ARG, before anything is launched and with the model untouched: a NULL argument; an unknown format or
 * range; a negative offset, pitch or stride; pitch[0] < src_w; NV12 pitch[1] < src_w; I420 pitch[1] or pitch[2] < src_w/2; an
 * odd base, offset, pitch or stride (Y pairs and UV pairs are loaded as 16-bit words; a labeller of covahip_mog_create_any takes
 * I420's U and V planes at odd offsets and pitches, as a tight frame has them where src_w/2 is odd: those samples are loaded
 * one by one); whatever covahip_mog_apply refuses. */
enum { COVAHIP_MOG_FMT_NV12 = 1, COVAHIP_MOG_FMT_I420 = 2 };
enum { COVAHIP_MOG_RANGE_LIMITED = 0, COVAHIP_MOG_RANGE_FULL = 1 };
typedef struct covahip_mog_yuv {   /* 72 bytes */
    int32_t format, range;
    int64_t offset[3];      /* bytes from a frame's first byte to plane p: Y, UV (NV12) | Y, U, V (I420); NV12 ignores [2] */
    int64_t pitch[3];       /* bytes per row of plane p */
    int64_t frame_stride;   /* frame f -> f + 1 of one stream */
    int64_t stream_stride;  /* stream s -> s + 1 at one frame index */
} covahip_mog_yuv;
/* the tight frame-major layout [F][S][Y plane, chroma] for this labeller's source size */
int  covahip_mog_yuv_tight(const covahip_mog *m, int format, int range, covahip_mog_yuv *out);
int  covahip_mog_apply_yuv(covahip_mog *m, const covahip_mog_yuv *lay, const uint8_t *base, int n_frames,
                           const int32_t *n_valid, uint8_t *labels, int mem_kind);
/* Next video in that slot: model zeroed, n = 0. */
int  covahip_mog_reset(covahip_mog *m, int stream);
/* Model state: one stream's model as ONE little-endian blob, to keep, to look at and to put back.
 *   offset  0  u32 magic "CVHM" (0x4D485643)     4  u32 version = 1        8  i32 work_w        12  i32 work_h
 *          16  i32 history     20  f32 var_threshold (the creating cfg, for information: not compared)
 *          24  i64 n (frames the stream has learned from)                  32 .. 63 zero
 *          64  f32 W[5][P], f32 V[5][P], f32 M[5][3][P], u8 nmodes[P]      P = work_w * work_h, rows dense at work_w whatever
 *              pitch the device uses (a covahip_mog_create_any labeller keeps its rows at work_w rounded up to 64)
 *          end u32 CRC-32C (Castagnoli, as the trainer state uses it, unmasked) of every byte before it
 *   64 + 101 P + 4 bytes: about 23 MB at 640x360.  Label mode, shadow mode and the frozen flag are settings, not state: they are
 *   not in the blob, as the trainer's post is not in its checkpoint.
 *   Contract -- exact resume.  Save stream s of any labeller after any sequence of calls and load the blob into stream t of any
 *   labeller of the same working size: any source size, either grid, the table's kernels or the any-size ones, any number of
 *   streams.  From then on, on frames whose working images are equal, both streams give bit-identical raw masks, filled masks,
 *   labels, shadow counts and models; the stream's frame count is the blob's n, so the automatic learning rate continues where
 *   it was.  save -> load -> save gives the same bytes.
 * covahip_mog_state_size / covahip_mog_save_state: *n = the blob's size; COVAHIP_ERR_OVERFLOW when buf is NULL or cap < *n (as
 * covahip_train_save_state).  Host memory, synchronous.
 * covahip_mog_load_state: all or nothing, validated before anything is copied.  Wrong magic / version / size / CRC, a nmodes byte
 * above 5, n < 0: COVAHIP_ERR_BAD_DATA; work_w / work_h not the labeller's, a bad stream, a NULL argument:
 * COVAHIP_ERR_INVALID_ARG.  In every refusal the labeller is untouched. */
int  covahip_mog_state_size(const covahip_mog *m, size_t *n);
int  covahip_mog_save_state(covahip_mog *m, int stream, void *buf, size_t cap, size_t *n);
int  covahip_mog_load_state(covahip_mog *m, int stream, const void *buf, size_t n);
/* Frozen labelling, per stream (stream = -1: all of them; frozen 0 or 1, anything else COVAHIP_ERR_INVALID_ARG).  The setting
 * holds for later covahip_mog_apply / covahip_mog_apply_yuv calls, covahip_mog_reset keeps it, and a new labeller has none frozen.
 * A frozen stream's frames are classified against its model; the model and n are not changed by the call.  This is the
 * well-defined form of OpenCV's apply(frame, 0), which is not safe in the letter of MOG2Invoker: a pixel that no mode fits opens
 * a mode of weight alphaT = 0, and the next pixel that fits it computes k = alphaT / w = 0 / 0.  So it is a
 * mode of its own, read-only, and not a learning rate.  Per pixel, f32, every product and sum rounded on its own:
 *       bg = false; tw = 0
 *       for mode = 0 .. nmodes - 1:
 *           d = M[mode] - data;  dist2 = (d0*d0 + d1*d1) + d2*d2
 *           if tw < TB && dist2 < Tb * V[mode]: bg = true
 *           if dist2 < Tg * V[mode]: stop          (the first mode that fits ends the walk, as in the update)
 *           tw = tw + W[mode]
 *       mask = bg ? 0 : 255
 * That is exactly the mask steps 1 - 5 give at alphaT = 0 on a model of finite values, with nothing written.  With shadows in
 * _DROP or _KEEP the test of step 2a runs where bg is false, on the model AS IT IS: there is no updated model and no new mode.
 * Close, open, fill and labels run as ever.  An empty model (after reset) gives all foreground.  A call with learning and frozen
 * streams runs the update kernel on the former and the frozen one on the latter; per stream the result is bit-identical to a
 * labeller that holds that stream alone.  With no stream frozen a call launches exactly the kernels it did before this
 * setting existed.  A fixed learning rate (apply(frame, lr)) is not offered.  covahip_mog_get_frozen gives one stream's
 * setting (0 <= stream < n_streams). */
int  covahip_mog_set_frozen(covahip_mog *m, int stream, int frozen);
int  covahip_mog_get_frozen(const covahip_mog *m, int stream, int *frozen);
/* The background image the model believes in: u8 [work_h][work_w][3] (B, G, R) of one stream, dense; stream = -1: all streams,
 * [n_streams][work_h][work_w][3].  cap: bytes at bgr; COVAHIP_ERR_OVERFLOW when bgr is NULL or cap is less than that.  mem_kind
 * applies to bgr.  Synchronous; only reads the model.  It is getBackgroundImage_intern of OpenCV 4.x bgfg_gaussmix2.cpp,
 * restated: this text is the contract.  Per pixel, f32, every product and sum rounded on its own:
 *       acc_c = 0; tw = 0
 *       for mode = 0 .. nmodes - 1:
 *           acc_c = acc_c + W[mode] * M[mode][c]   (c = 0, 1, 2)
 *           tw = tw + W[mode]
 *           if tw > TB: stop
 *       inv = |tw| > FLT_EPSILON ? 1 / tw (correctly rounded) : 0
 *       out_c = saturate_u8(round_half_even(acc_c * inv))
 * An empty model gives (0, 0, 0). */
int  covahip_mog_background(covahip_mog *m, int stream, uint8_t *bgr, size_t cap, int mem_kind);
void covahip_mog_destroy(covahip_mog *m);

/* ------------------------------------------------------ sink formats, track export
 * Data formats either side of the hot path.               */
/* tfrecordsink (cova-rs/gst-plugins/src/tfrecordsink/imp.rs:69-198): one framed TFRecord record =
 * tf.train.Example with bytes_list features mb_type / mv_x / mv_y / gt, one w*h string per frame,
 * zero-filled to pad_to_frames strings (the `gop` property).  rgba: [n_frames][h][w][4] (a
 * metapreprocess timestep=1 frame), gt: [n_frames][h*w] or NULL.  Returns the record size. */
size_t covahip_tfrecord_example(const uint8_t *rgba, const uint8_t *gt, int n_frames, int pad_to_frames, int w, int h,
                                uint8_t *out, size_t cap, int *status);
/* bboxsink (cova-rs/gst-plugins/src/bboxsink/imp.rs:252-270): serde-CSV text, optional header. */
size_t covahip_bbox_csv(const covahip_bbox *boxes, size_t n, int with_header, char *out, size_t cap, int *status);
/* cova track export (cova-rs/gst-plugins/src/cova/tracker.rs:59-83): per dead track a 4-byte
 * big-endian length + bincode Frame{range_start, oldest, history}; boxes/track_lens as returned by
 * covahip_sort_update / covahip_sort_finalize. */
size_t covahip_tracks_export(uint64_t range_start, uint64_t oldest, const covahip_bbox *boxes, const uint32_t *track_lens,
                             size_t n_tracks, uint8_t *out, size_t cap, int *status);

/* ------------------------------------------------ analysis-aggregator join
 * Association of tracker output with DNN detections (cova-rs/analysis-aggregator/src/server/
 * assoc.rs:63-507, track.rs:47-66, dnn.rs:57-86): what the aggregator
 * does with the messages of its tracker and DNN connections, without the sockets.  Messages are
 * pushed in arrival order; the four CSV files (track, dnn, assoc, stationary) are read back as text. */
typedef struct covahip_assoc covahip_assoc;
typedef struct covahip_assoc_cfg {   /* main.rs:32-39 */
    float moving_iou;                /* 0.15 */
    float stationary_iou;            /* 0.3  */
    uint64_t stationary_maxage_s;    /* 120  */
    float scale_factor;              /* 1.3  */
} covahip_assoc_cfg;
void covahip_assoc_default_cfg(covahip_assoc_cfg *cfg);
/* range_starts: the range_start every tracker announces with its first frame (assoc.rs:473-489). */
int covahip_assoc_new(const covahip_assoc_cfg *cfg, const uint64_t *range_starts, size_t n_trackers, covahip_assoc **out);
void covahip_assoc_free(covahip_assoc *a);
/* Recieved::Track: boxes already in pixels with re-based ids (assoc.rs:370-431). */
int covahip_assoc_push_track(covahip_assoc *a, uint64_t range_start, uint64_t oldest, const covahip_bbox *boxes, size_t n);
/* One length-delimited payload of covahip_tracks_export as track.rs:47-66 handles it: bincode Frame,
 * scale_dim(16), track_id += range_start, then push_track. */
int covahip_assoc_push_track_frame(covahip_assoc *a, const uint8_t *payload, size_t len);
/* Recieved::Dnn (assoc.rs:296-367); boxes need timestamp and class_id. */
int covahip_assoc_push_dnn(covahip_assoc *a, const covahip_bbox *boxes, size_t n);
/* Detection rows "timestamp,left,top,width,height,class_id\n" as read from a DNN connection (dnn.rs:57-86). */
int covahip_assoc_push_dnn_text(covahip_assoc *a, const char *text, size_t len);
int covahip_assoc_terminate(covahip_assoc *a);   /* assoc.rs:434-467 */
/* which: 0 track.csv, 1 dnn.csv, 2 assoc.csv, 3 stationary.csv; returns the size, copies if it fits. */
size_t covahip_assoc_csv(covahip_assoc *a, int which, char *out, size_t cap, int *status);

/* --------------------------------------------- entropy-decode front end
 * What feeds `metapreprocess` in the reference is a patched FFmpeg avdec_h264 (an un-vendored submodule; README.md:94-114)
 * that stops after entropy decoding and writes one record [mb_type, mv_x, mv_y, -] per macroblock into the first bytes of its
 * output frame.  Built here, verified on the reference's demo/1m.mp4: ISO-BMFF / NAL / SPS / PPS / slice-header layer, picture
 * order (output order of the access units), the CABAC macroblock layer of frame-coded 4:2:0 streams with one slice per
 * picture and cabac_init_idc 0 (every slice must end on its last macroblock with end_of_slice_flag: 1,802 of 1,802 do) and
 * the record writer.  Anything else (CAVLC, fields / MBAFF, several slices per picture, cabac_init_idc 1 / 2, samples of more than 8 bits) returns
 * COVAHIP_ERR_UNSUPPORTED.  `file` must stay valid while the handle lives. */
typedef struct covahip_h264 covahip_h264;
typedef struct covahip_h264_info {
    int32_t width_mbs, height_mbs, n_samples;
    int32_t profile_idc, level_idc, entropy_cabac, transform_8x8, num_ref_frames, frame_mbs_only;
    int32_t weighted_pred, weighted_bipred, poc_type;
    int32_t max_num_reorder_frames, max_dec_frame_buffering;   /* VUI bitstream_restriction (E.1.1); -1 when the stream does not say */
} covahip_h264_info;
typedef struct covahip_h264_slice {
    uint64_t nal_offset;       /* file offset of the NAL unit (its header byte) */
    uint32_t nal_bytes;
    uint32_t data_bit_offset;  /* first bit of slice_data() in the unescaped RBSP behind the NAL header byte */
    int32_t nal_type;          /* 1 non-IDR, 5 IDR */
    int32_t slice_type;        /* 0 P, 1 B, 2 I (slice_type % 5) */
    int32_t first_mb, frame_num, idr, poc_lsb, qp, cabac_init_idc /* -1: none */, num_ref_l0, num_ref_l1, direct_spatial;
    int32_t nal_ref_idc, has_mmco5;  /* reference picture?  memory_management_control_operation 5 present (resets the POC)? */
} covahip_h264_slice;
int covahip_h264_open_mp4(const uint8_t *file, size_t len, covahip_h264 **out);
void covahip_h264_close(covahip_h264 *h);
int covahip_h264_get_info(const covahip_h264 *h, covahip_h264_info *info);
/* Access unit `sample` (decode order): where it sits in the file and whether the container marks it a sync sample. */
int covahip_h264_sample(const covahip_h264 *h, int sample, uint64_t *offset, uint32_t *size, int *is_sync);
/* Slice headers of the access unit (up to cap; *n = number of slice NAL units). */
int covahip_h264_sample_slices(const covahip_h264 *h, int sample, covahip_h264_slice *out, int cap, int *n);
/* Access units in OUTPUT order (ascending picture order count inside every IDR period, 8.2.1): the order in which a decoder
 * hands frames downstream, i.e. the order metapreprocess stacks them in.  samples: sample indices (decode order). */
int covahip_h264_display_order(const covahip_h264 *h, int32_t *samples, int cap, int *n);
/* Entropy-decodes access unit `sample` (decode order) into records u8 [height_mbs][width_mbs][4] (may be NULL: parse only) --
 * the first width_mbs * height_mbs * 4 bytes of the carrier frame.  Byte 0: macroblock class (0 P_Skip / B_Skip, 1 inter 16x16,
 * 2 inter 16x8 / 8x16, 3 inter 8x8, 4 B_Direct_16x16, 5 intra NxN, 6 intra 16x16, 7 I_PCM); bytes 1 / 2: |mean motion vector| of
 * the macroblock, x / y, in quarter pixels (<= 255) -- the standard's prediction (median, P_Skip, spatial direct with the
 * colZeroFlag test against RefPicList1[0], temporal direct from that picture's motion; the picture is decoded on the way when no
 * earlier call has) plus the coded difference; byte 3: 0.  What the reference's patched decoder puts into these bytes is not known here (SURVEY.md row A0:
 * unpinned); a BlobNet has to be trained on the front end it runs behind.  COVAHIP_OK only if the slice decoded exactly
 * width_mbs * height_mbs macroblocks, ended there with end_of_slice_flag and left only trailing bits. */
int covahip_h264_decode_records(const covahip_h264 *h, int sample, uint8_t *records, size_t cap);
/* The co-located picture of a B picture's direct prediction: *col_sample = the sample that is RefPicList1[0] of `sample` (list
 * initialisation 8.2.4.2.3 + modification 8.2.4.3 over the reference marking 8.2.5 of the access units before it), -1 when
 * `sample` is not a B picture or has none; *short_term = 1 when that picture is a short-term reference. */
int covahip_h264_colocated(const covahip_h264 *h, int sample, int *col_sample, int *short_term);
/* Stream form (what an element in the place of avdec_h264 uses): parameter sets from the AVCDecoderConfigurationRecord (avcC box
 * payload = codec_data of video/x-h264,stream-format=avc caps), then access units IN DECODE ORDER (length-prefixed NAL units).
 * records / cap as covahip_h264_decode_records; hdr (may be NULL) gets the slice header; *order_key (may be NULL) a key whose
 * ascending order is the output order of the pictures (IDR period << 32 | picture order count + 2^31). */
int covahip_h264_open_avcc(const uint8_t *avcc, size_t len, covahip_h264 **out);
int covahip_h264_decode_au(covahip_h264 *h, const uint8_t *au, size_t len, uint8_t *records, size_t cap, covahip_h264_slice *hdr,
                           int64_t *order_key);
/* The carrier layout: interleaves per-macroblock mb_type / mv_x / mv_y into the first width_mbs * height_mbs * 4 bytes of
 * `frame` (metapreprocess/imp.rs:233,311-312; tfrecordsink/imp.rs:105-112). */
int covahip_carrier_write_records(const uint8_t *mb_type, const uint8_t *mv_x, const uint8_t *mv_y, int width_mbs, int height_mbs,
                                  uint8_t *frame, size_t frame_bytes);

/* Packed carrier records: two bytes per macroblock, min(mb_type, 6) | min(mv_x, 6) << 3 | min(mv_y, 6) << 6 -- everything BlobNet
 * keeps of a record (its first operation is clip(x, 0, 6) on all three channels, utils/model/preprocessing.py:6-7), at half the
 * bytes: the host-to-device copy is what bounds the element path (9.1 MB per 256-frame batch over PCIe).  The pinned host
 * pipeline takes its frames in this form when asked to (covahip_pipe_set_packed); results are bit-identical. */
void covahip_carrier_pack(const uint8_t *frame, size_t n_mb, uint16_t *records);
/* covahip_filter_forward_frames on packed records [n_frames][H][W] (device pointers only): d_records aligned to 8 (four records a
 * load), the others as for covahip_filter_forward. */
int covahip_filter_forward_frames_packed(covahip_ctx *ctx, const uint16_t *d_records, int n_frames, const int32_t *stack_index,
                                         int batch, int area_thresh, covahip_box *d_boxes, int32_t *d_counts, int max_boxes,
                                         float *d_logits, uint8_t *d_mask);
/* ... with a model per stack (model_ids: see covahip_blobnet_load_set; one model per frame). */
int covahip_filter_forward_frames_packed_m(covahip_ctx *ctx, const uint16_t *d_records, int n_frames, const int32_t *stack_index,
                                           const uint8_t *model_ids, int batch, int area_thresh, covahip_box *d_boxes,
                                           int32_t *d_counts, int max_boxes, float *d_logits, uint8_t *d_mask);

/* ------------------------------------------------- metapreprocess stacking
 * Host state of the `metapreprocess` element (cova-rs/gst-plugins/src/metapreprocess/
 * imp.rs:204-332): keeps the last timestep-1 inputs, emits one stacked frame every
 * gamma-th input once warm.                                                       */
typedef struct covahip_stack covahip_stack;
/* size_per_buf = out_size / timestep (imp.rs:233) = (W/16)*(H/16)*4 bytes. */
int covahip_stack_new(size_t size_per_buf, unsigned timestep, unsigned gamma, covahip_stack **out);
void covahip_stack_free(covahip_stack *s);
/* in: >= size_per_buf bytes of carrier frame; out: timestep*size_per_buf bytes.
 * *emitted = 1 if `out` was written (GST_FLOW_OK), 0 if the element would return
 * BASE_TRANSFORM_FLOW_DROPPED. */
int covahip_stack_push(covahip_stack *s, const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap,
                       int *emitted);
/* transform_caps arithmetic (imp.rs:262-268): out = (w/16, h/16*timestep). */
void covahip_stack_out_dims(int width, int height, unsigned timestep, int *out_w, int *out_h);

/* ----------------------------------------------------------------- SORT
 * Host state of the `sorttracker` element and of cova's embedded tracker
 * (cova-rs/sort/src/lib.rs:14-214, tracker/mod.rs:15-152, state.rs:9-28).            */
typedef struct covahip_sort covahip_sort;
int covahip_sort_new(uint64_t max_age, uint64_t min_hits, float iou_threshold, covahip_sort **out);
void covahip_sort_free(covahip_sort *s);
/* Sort::update(dets, pts).  Dead active tracks' histories are appended, flattened in
 * track order, to dead_boxes (cap entries; *n_dead_boxes = total produced);
 * track_lens (cap_tracks entries; *n_tracks = number of dead tracks) holds each
 * track's history length.  Any output pointer may be NULL with cap 0.           */
int covahip_sort_update(covahip_sort *s, const covahip_bbox *dets, size_t n_dets, uint64_t pts,
                        covahip_bbox *dead_boxes, size_t cap, size_t *n_dead_boxes, uint32_t *track_lens,
                        size_t cap_tracks, size_t *n_tracks);
/* Sort::finalize (lib.rs:207-213): same output convention. */
int covahip_sort_finalize(covahip_sort *s, covahip_bbox *boxes, size_t cap, size_t *n_boxes,
                          uint32_t *track_lens, size_t cap_tracks, size_t *n_tracks);
int covahip_sort_mark_seen(covahip_sort *s, uint64_t ts);          /* lib.rs:189-193 */
int covahip_sort_num_trackers(const covahip_sort *s, size_t *n);
/* Introspection for tests: tracker i's id / active flag / hit_streaks / state box. */
int covahip_sort_tracker_info(const covahip_sort *s, size_t i, uint64_t *id, int *active,
                              uint64_t *hit_streaks, uint64_t *time_since_update, covahip_bbox *state);
/* Introspection for tests (the reference's own unit tests drive the tracker this way, sort/src/lib.rs:250-274,
 * tracker/mod.rs:154-165): KalmanBoxTracker::predict(ts) on tracker i (tracker/mod.rs:104-121; *last = history.last()),
 * KalmanBoxTracker::update(Some(det) / None) (tracker/mod.rs:71-102; det == NULL is None). */
int covahip_sort_tracker_predict(covahip_sort *s, size_t i, uint64_t ts, covahip_bbox *last);
int covahip_sort_tracker_update(covahip_sort *s, size_t i, const covahip_bbox *det);
/* linear_assignment() of lib.rs:25-56 on a column-major n_rows x n_cols f32 cost
 * matrix; writes (row, col) pairs; returns their number. */
size_t covahip_linear_assignment(const float *cost_colmajor, size_t n_rows, size_t n_cols, uint32_t *pairs,
                                 size_t cap_pairs);

/* ------------------------------------------------------------- cova filter
 * Host state of the `cova` element (cova-rs/gst-plugins/src/cova/imp.rs:90-432,
 * cova/tracker.rs:16-125): GoP buffering of encoded access units, embedded SORT,
 * decode/drop decisions and the three read-only counters.                        */
typedef struct covahip_gopfilter covahip_gopfilter;
typedef struct covahip_gopfilter_cfg {
    float sort_iou;        /* "sort-iou"     default 0.1  (imp.rs:22) */
    uint32_t sort_maxage;  /* "sort-maxage"  default 30   */
    uint32_t sort_minhits; /* "sort-minhits" default 30   */
    uint32_t alpha;        /* "alpha"        struct default 0 (imp.rs:28) */
    uint32_t beta;         /* "beta"         struct default 0 */
    uint8_t infer_i;       /* "infer-i"      default false */
} covahip_gopfilter_cfg;
void covahip_gopfilter_default_cfg(covahip_gopfilter_cfg *cfg);
int covahip_gopfilter_new(const covahip_gopfilter_cfg *cfg, covahip_gopfilter **out);
void covahip_gopfilter_free(covahip_gopfilter *g);

enum {
    COVAHIP_AU_DELTA_UNIT = 1u << 0, /* in:  not a key frame (GST_BUFFER_FLAG_DELTA_UNIT) */
    COVAHIP_AU_DISCONT = 1u << 1,    /* out: set on the copy of each GoP's key frame       */
    COVAHIP_AU_DROPPABLE = 1u << 2   /* out: decode for dependency only                    */
};
typedef struct covahip_au_out {
    uint64_t id;    /* caller's handle of the access unit (e.g. GstBuffer*) */
    uint64_t pts;   /* ns */
    uint32_t flags; /* COVAHIP_AU_* */
    uint32_t list;  /* index of the BufferList this AU belongs to (push order) */
} covahip_au_out;

/* sink_enc chain (imp.rs:320-360). */
int covahip_gopfilter_push_enc(covahip_gopfilter *g, uint64_t id, uint64_t pts, uint32_t flags);
/* sink_mask chain (imp.rs:90-317): boxes of the frame at `pts`; forwarded AUs are
 * appended to out (cap entries, *n_out = number produced).                        */
int covahip_gopfilter_push_boxes(covahip_gopfilter *g, const covahip_bbox *boxes, size_t n, uint64_t pts,
                                 covahip_au_out *out, size_t cap, size_t *n_out);
/* Both-sinks-EOS flush (imp.rs:361-432). */
int covahip_gopfilter_eos(covahip_gopfilter *g, covahip_au_out *out, size_t cap, size_t *n_out);
/* Access units the filter has discarded for good since the last call (GoP leftovers of a flushed GoP, the AU
 * popped and lost at imp.rs:167-172, everything still queued at EOS): the caller releases its buffers for
 * these ids, as the reference frees a GoP's buffers when it drops it (imp.rs:268-305).  Call until *n < cap. */
int covahip_gopfilter_take_dropped(covahip_gopfilter *g, uint64_t *ids, size_t cap, size_t *n);
/* Bytes the element's tracker writes to its aggregator socket (`port`; cova/tracker.rs:59-83,91-118): one
 * 4-byte big-endian length + bincode Frame per finished track, accumulated since the last successful call
 * (tracks that died in push_boxes, Sort::finalize() at EOS).  Returns the size; copies and clears if it fits. */
size_t covahip_gopfilter_take_track_export(covahip_gopfilter *g, uint8_t *out, size_t cap, int *status);
int covahip_gopfilter_counters(const covahip_gopfilter *g, uint64_t *dropped, uint64_t *decoded_dependency,
                               uint64_t *decoded_inference);

#ifdef __cplusplus
}
#endif
#endif /* COVAHIP_H */
