// BlobNet on gfx950: model state shared by the kernels' translation units.
#pragma once
#include <hip/hip_fp16.h>

#include <vector>

#include "blobnet_params.h"
#include "internal.h"

constexpr int BN_KTAB_STACKS = 256;   // stacks whose table (16-bit frame indices, 2 KB) travels in enc1_mfma's kernel arguments

struct BnLevelGeom {
    int H, W;  // spatial size of the tensor at this level (level 0 = network input)
};

// HBM workspace of one lane (internal.h, CtxLane): everything a forward in flight writes.  Lane 0's also serves the calls
// that run on the ctx's primary stream.
struct BnWorkspace {
    bool ready = false;
    // activations (fp16, channels-last)
    __half *act[BN_LEVELS + 1] = {};  // act[i], i=1..3: [B][T][H_i][W_i][C_i]; act[4]: [B][H_4][W_4][128] (t=0)
    __half *dact[BN_LEVELS] = {};     // dact[j], j=0..2: [B][Hd][Wd][Cout_j]
    // carrier-frame path: pooled level-0 values per carrier frame, [frames][H_1][W_1][16] (pad row / column zero)
    __half *pbuf = nullptr;
    size_t pbuf_frames = 0;
    // the level-0 skip connection's share of the logits (round 5): fp32 [B][H_1 + 1][W_1 + 1][4], written by the level-1 kernel, added by the last
    // decoder block -- the skip tensor itself (act[1]) is then neither written nor read
    float *part = nullptr;
    // bboxcc's parity planes per frame, u32 [B][2 * ceil(H / 2) + 2][E lo, E hi, O lo, O hi]: written by dec012_mfma<.., TAILF>, read by
    // cc_planes (the form in which the last decoder block runs inside the decoder launch)
    uint32_t *planes = nullptr;
    // The lane's small tables (internal.h, ResidentTable), each reserved once, on first use, for max_batch:
    ResidentTable<int32_t> index;     // stack -> frame table of a carrier-frame call, i32 [batch][4]; 4 * max_batch ints
    int index_frames = 0;             // n_frames of the call `index` was uploaded for: part of what "resident" means there
    std::vector<int32_t> kept_table;  // a table that travels BY VALUE (BnInput::h_index), alive until the launch has copied it
    ResidentTable<uint8_t> models;    // model ids of a mixed batch: u8 [batch] per stack, then u8 [n_frames] per carrier frame; 5 * max_batch bytes
    // per-stack area thresholds of the stand-alone bboxcc behind a forward whose frame does not fit the fused tail
    // (covahip_blobnet_set_area): i32 [batch]; max_batch ints
    ResidentTable<int32_t> areas;
};

struct covahip_blobnet {
    int H = 0, W = 0, max_batch = 0;
    int n_models = 1;   // models of the set; their prepared weights lie Prepared::total bytes apart from d_prepared on
    BnLevelGeom lv[BN_LEVELS + 1];
    int enc_c[BN_LEVELS + 1], dec_ci[BN_LEVELS], dec_co[BN_LEVELS];   // blobnet_params.h's, copied by the constructor
    int dec_cy[BN_LEVELS], dec_cx[BN_LEVELS];  // crop offsets (top/left) per decoder block
    BnWorkspace ws[COVAHIP_MAX_LANES];
    // prepared (MFMA path) weights
    void *d_prepared = nullptr;
    size_t prepared_bytes = 0;
    struct Prepared *prep = nullptr;
    int fuse_tail = 1;  // MFMA path, with bboxcc requested: last decoder block + bboxcc in one launch
    int fuse_dec = 1;  // MFMA path: decoder blocks 0..2 as one launch (a frame's three input tiles side by side in LDS) when they fit
    int enc1_tile16 = 1;  // MFMA path: level 1 on 16-position tiles (enc1_mfma) where the row fits its fixed LDS stride
    int tail_rows = 1;    // MFMA path: the fused tail on row tiles with ballots straight into bboxcc's planes (dec3cc_rows_mfma, round 6)
    int tail_in_dec012 = 1;   // MFMA path: the last block inside dec012_mfma, bboxcc alone behind it (cc_planes) -- 1: where it applies and
                              // the batch fills the chip, 2: wherever it applies, 0: never
    int tail_part = 1;    // MFMA path: the last decoder block's skip half computed by the level-1 kernel as partial logits (enc1_mfma only)
    int fuse_enc23 = 1;   // MFMA path: encoder levels 2 + 3 in one launch (enc23_mfma: level 2's output stays in LDS as level 3's band) when they fit
                          // and the batch / geometry make it pay; 0: never, 2: whenever they fit
    int enc_rowtiles = 1; // MFMA path: levels 2 and 3 on row-aligned tiles (enc_mfma<.., TSZ>) where the geometry suits them
    int64_t macs_per_frame = 0;
    // per-model post-processing (covahip_blobnet_set_post, covahip_blobnet_set_area): host copies of the settings, and -- from
    // the first non-default setting on -- their device tables, one allocation: fp32 threshold per model | i32 area threshold per
    // model | keep bytes u8 [n_models][H][W] | the same as bboxcc's parity planes, u32 [n_models][H][E lo, E hi, O lo, O hi]
    // (what dec3cc_rows_mfma ANDs into its ballots)
    std::vector<float> post_thr;                  // [n_models]
    std::vector<int32_t> post_area;               // [n_models]: bboxcc's area threshold of the model, 0 = unset (the call's applies)
    bool area_on = false;                         // some model has an area threshold of its own
    std::vector<std::vector<uint8_t>> post_keep;  // [n_models]: empty = keep everything, else H * W bytes of 0 / 1
    bool post_on = false;                         // some model has a non-default setting: the POST = true kernels run
    void *d_post = nullptr;
    size_t post_area_off = 0, post_keep_off = 0, post_planes_off = 0, post_keep_stride = 0, post_planes_stride = 0, post_bytes = 0;
    covahip_blobnet() {
        std::copy(BN_ENC_C, BN_ENC_C + BN_LEVELS + 1, enc_c);
        std::copy(BN_DEC_CI, BN_DEC_CI + BN_LEVELS, dec_ci);
        std::copy(BN_DEC_CO, BN_DEC_CO + BN_LEVELS, dec_co);
    }
};

// Whether encoder level 1 runs on enc1_mfma (16x16x32 tiles, fixed LDS row: grids of at most BN_E1_MAXW level-1 pixels) or on
// the round-1..3 kernel.  ONE predicate for both translation units: blobnet.hip hands the stack table over by value only to
// enc1_mfma, and blobnet_mfma.hip must then launch exactly that kernel.
constexpr int BN_E1_MAXW = 62;
inline bool bn_level1_on_enc1(const covahip_ctx *ctx, const covahip_blobnet *m) {
    return m->enc1_tile16 && m->enc_c[1] == 16 && m->enc_c[2] == 32 && m->lv[1].W <= BN_E1_MAXW && m->lv[1].H >= 2 &&
           !ctx->enc_plan[1].nbands;
}

// blobnet_mfma.hip
// n_models parameter blobs of one geometry; allpos[level] is the AND over the set and every model is prepared with it
int blobnet_prepare_mfma(covahip_ctx *ctx, covahip_blobnet *m, const float *const *h_weights, int n_models);
void blobnet_release_mfma(covahip_ctx *ctx, covahip_blobnet *m);
// cc != nullptr: bboxcc is wanted on the mask; *cc_done tells whether the forward already ran it (fused tail)
struct BnCcTail {
    int area_thresh, max_boxes;
    covahip_box *boxes;   // [batch][max_boxes]
    int32_t *counts;
};
// Input of a forward: either the stacked tensor [batch][T*H][W][4] (metapreprocess output), or carrier frames
// [n_frames][H][W][4] plus, per stack, the indices of its T = 0..3 slices (device pointers all).
// dry: planning only (every geometry / LDS check of the launch sequence, no kernel is launched).
struct BnInput {
    const uint8_t *stack = nullptr;
    const uint8_t *frames = nullptr;
    int n_frames = 0;
    const int32_t *index = nullptr;   // i32 [batch][4] on the device, or null when h_index is used / for the stacked entry
    // the same table on the host (validated): batches of at most BN_KTAB_STACKS stacks hand it to the level-1 kernel BY VALUE, in
    // its kernel arguments -- no copy in front of the kernels, nothing to cache or to order
    const int32_t *h_index = nullptr;
    bool packed = false;   // carrier frames as two-byte records (covahip_carrier_pack) instead of the decoder's four bytes
    bool dry = false;
    // model sets: either ONE model for the whole batch (model_ids == nullptr; its weights are `model` strides past model 0), or a
    // mixed batch: u8 model id per stack [batch] and per carrier frame [n_frames], on the device (the MS = true kernels)
    int model = 0;
    const uint8_t *model_ids = nullptr;
    const uint8_t *frame_models = nullptr;
    const uint8_t *h_model_ids = nullptr;   // the same ids per stack on the HOST (the caller's array, alive during the call); null with model_ids
    bool mixed = false;    // dry: plan the mixed-batch kernels
};
int blobnet_forward_mfma(covahip_ctx *ctx, covahip_blobnet *m, BnWorkspace &ws, const BnInput &in, int batch, float *d_logits,
                         uint8_t *d_mask, const BnCcTail *cc = nullptr, bool *cc_done = nullptr);
