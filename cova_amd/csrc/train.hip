// BlobNet training step on gfx950: forward, backward and Adam in fp32 (include/covahip.h, "BlobNet training"); the evaluation
// pass over the same forward kernels and the trainer's state blob ("Evaluation and resume").
//
// Layout: every activation is channels-first, NCTHW for the encoder ([B][C][T][H][W]) and NCHW for the decoder (T = 1: the
// decoder only sees the t = 0 slice of each encoder level, tests/torch_blobnet.py).  Channels-first keeps each channel's
// (T, H, W) block contiguous, which is what the per-channel reductions (BN, biases) walk, and it is the index order the
// dropout hash is defined over.
//
// Determinism: no float atomics.  Every reduction is a fixed split of its range into slabs (one workgroup each, fixed-order
// tree inside), followed by a sequential sum of the slabs; the split depends on the geometry and the batch only.  The only
// atomics are the integer TP / FP / FN counters of the metrics.
//
// Training sets: a trainer holds K models of one geometry and every kernel takes one step of all of them in one launch.  The
// model is the grid's z index.  Model m's slice of every buffer lies m * max_batch samples (m * N_PARAMS for parameters,
// gradients and Adam moments) behind model 0's, and a kernel moves its pointers there once, then runs the code of a solo step
// with the model's own batch b from the per-step table (MStep): element counts, slab counts and chunk lengths are all computed
// from b in the kernel, so model m's arithmetic and summation order are those of a solo trainer at batch b.  Grids are sized
// for the step's largest batch; a workgroup outside its model's extent (all of them when b = 0) leaves at once.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "blobnet_params.h"
#include "internal.h"

namespace {

// the architecture and the parameter layout are blobnet_params.h's; these are the short names this file uses for them
constexpr int TT = BN_T;              // timestep
constexpr int NL = BN_LEVELS;         // encoder levels / decoder blocks
constexpr size_t N_PARAMS = BN_N_PARAMS;
constexpr const int (&ENC_C)[NL + 1] = BN_ENC_C, (&DEC_CI)[NL] = BN_DEC_CI, (&DEC_CO)[NL] = BN_DEC_CO;
constexpr int BLK = 256;
constexpr int RED_CHUNK = 4096;       // elements per slab of a channel reduction
constexpr int WG_CHUNK = 1024;        // positions per slab of a weight gradient
constexpr int TMIX_BLOCKS_MAX = 512;

// ------------------------------------------------------------------------------------------------ dropout hash
__host__ __device__ inline uint64_t splitmix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
uint64_t drop_key(uint64_t seed, uint64_t step, int site) { return splitmix64(seed ^ splitmix64((step << 8) | (uint64_t)site)); }
struct Drop {
    uint64_t key;
    uint32_t thr;   // keep iff the hash's top 24 bits >= thr
    float scale;    // 1 / (1 - p)
};
__device__ inline float keep(const Drop &d, uint64_t idx) {
    return (uint32_t)(splitmix64(d.key + idx) >> 40) >= d.thr ? d.scale : 0.f;
}

inline unsigned nblk(int64_t n) { return (unsigned)((n + BLK - 1) / BLK); }

// ------------------------------------------------------------------------------------------------ per-model step table
constexpr int N_SITES = 12;           // dropout sites: 2 per encoder level, 1 per decoder block
constexpr int STAT_STRIDE = 7 * 256;  // floats of BN batch statistics per model: [7 layers][2][128]
struct MStep {                        // one per model and step, uploaded with the step
    int32_t b;                        // the model's batch this step (0: skipped, nothing of it is touched)
    int32_t first;                    // its first sample in the packed stack / label input
    float lr_t;                       // Adam's lr * sqrt(1 - b2^t) / (1 - b1^t) at the model's own t
    uint32_t pad;
    uint64_t key[N_SITES];            // drop_key(seed, step, site) of the model
};
// A set of one takes its step's values as kernel arguments instead (tab = null, nothing uploaded) and runs the kernels'
// SET = false instantiation, which has no table loads and no offsets: the solo step of covahip_train_create as it was.
struct Mdl {
    const MStep *tab;                 // null: a set of one, its values below and in DropS::key
    int maxB;                         // samples between two models' slices of an activation buffer
    int64_t slab_stride;              // floats between two models' slab workspaces
    int32_t solo_b;                   // (its chunk lengths come with each launch, solo_chunk, as the host knows its batch)
    float solo_lr_t;
};
struct DropS {                        // a dropout site; the key comes from the model's table entry
    int site;
    uint32_t thr;
    float scale;
    uint64_t key;                     // the key of a set of one
};
// Every kernel has two instantiations ("Training sets": one shared instantiation cost the solo step 3 %).
template <bool SET> __device__ inline int model_b(const Mdl &md) { return SET ? md.tab[blockIdx.z].b : md.solo_b; }
template <bool SET> __device__ inline int model_first(const Mdl &md) { return SET ? md.tab[blockIdx.z].first : 0; }
template <bool SET> __device__ inline float model_lr_t(const Mdl &md) { return SET ? md.tab[blockIdx.z].lr_t : md.solo_lr_t; }
template <bool SET> __device__ inline Drop model_drop(const Mdl &md, const DropS &d) {
    return Drop{SET ? md.tab[blockIdx.z].key[d.site] : d.key, d.thr, d.scale};
}
// A wave-uniform 64-bit value handed back through scalar registers, opaque to the optimiser: for the chunk lengths (out of a
// 64-bit division, which the compiler does in vector registers) and for the per-model offsets below.
__device__ inline int64_t uniform64(int64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
// offset of this workgroup's model in a buffer of `per` elements per sample
// `per` is written as the int product of a kernel's extents where they are ints (at most 2^29 at 1024x1024): sign-extending
// an extent itself up here makes the compiler reuse the 64-bit value in the index arithmetic of the loops, which then
// multiplies high halves per element -- 8 - 11 % on the latency-bound convT weight-gradient launches of a batch-4 step.
#define MOFF(per) (SET ? uniform64((int64_t)blockIdx.z * md.maxB * (int64_t)(per)) : (int64_t)0)
#define POFF (SET ? uniform64((int64_t)blockIdx.z * (int64_t)N_PARAMS) : (int64_t)0)
__host__ __device__ inline int64_t red_stride(int maxB) { return 2 * (int64_t)(maxB > 128 ? maxB : 128); }

// The posts of a trainer's models (include/covahip.h, "Training with a post"): device tables that only covahip_train_set_post
// writes.  Model m's keep row starts at blockIdx.z * hw, so the row is workgroup-uniform.
struct PostTab {
    const uint8_t *keep;              // [K][hw], 0 / 1; all 1 for a model without a keep map or without a post
    const float *thresh;              // [K] logit threshold of the counts
    const uint8_t *flag;              // [K] 1: the model has a post; 0: its expressions are those of the form without
};
// The three kernels that read labels end in a parameter pack `Post... post`: empty, or one PostTab.  The empty pack is the
// kernel of a trainer that never heard of posts, argument for argument and instruction for instruction; with a PostTab it is
// the POST form, launched while any model of the trainer has a post.
__device__ inline const PostTab *post_tab_of() { return nullptr; }
__device__ inline const PostTab *post_tab_of(const PostTab &pt) { return &pt; }

// slabs of a channel reduction over M = N*S elements per channel
__host__ __device__ inline int red_slabs(int64_t M) {
    int64_t np = (M + RED_CHUNK - 1) / RED_CHUNK;
    return (int)(np < 1 ? 1 : np);
}
__host__ __device__ inline int wg_slabs(int64_t P) {   // at most 4096 slabs (the grid's y extent), longer ones on large grids
    int64_t ns = (P + WG_CHUNK - 1) / WG_CHUNK;
    return (int)(ns < 1 ? 1 : ns > 4096 ? 4096 : ns);
}
__host__ __device__ inline int tmix_blocks(int64_t n) {   // workgroups (= weight-gradient slabs) of k_tmix_bwd over n positions
    int64_t nb = (n + 4 * BLK - 1) / (4 * BLK);
    return (int)(nb < 1 ? 1 : nb > TMIX_BLOCKS_MAX ? TMIX_BLOCKS_MAX : nb);
}

// ------------------------------------------------------------------------------------------------ kernels
// u8 [B][T*H][W][4] -> clip(x, 0, 6) / 6 of bytes 0..2, [B][3][T][H][W]
template <bool SET>
__global__ void k_input(Mdl md, const uint8_t *__restrict__ st, float *__restrict__ x, int H, int W) {
    const int B = model_b<SET>(md);
    const int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
    const int64_t hw = (int64_t)H * W, n = (int64_t)B * 3 * TT * hw;
    if (i >= n) return;
    st += (int64_t)model_first<SET>(md) * TT * hw * 4;
    x += MOFF(3 * TT * hw);
    const int64_t s = i % hw;
    const int t = (int)((i / hw) % TT), ch = (int)((i / (hw * TT)) % 3);
    const int64_t b = i / (hw * TT * 3);
    const float v = (float)st[((b * TT + t) * hw + s) * 4 + ch];
    x[i] = fminf(v, 6.f) / 6.f;
}

// conv 3x3 "same" + bias + ReLU per (b, t) slice; k: Keras [3][3][Ci][Co]
template <bool SET>
__global__ void k_conv3_fwd(Mdl md, const float *__restrict__ x, const float *__restrict__ k, const float *__restrict__ bias,
                            float *__restrict__ out, int Ci, int Co, int H, int W) {
    const int B = model_b<SET>(md);
    const int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
    const int64_t hw = (int64_t)H * W, n = (int64_t)B * Co * TT * hw;
    if (i >= n) return;
    x += MOFF(Ci * TT * hw);
    out += MOFF(Co * TT * hw);
    k += POFF;
    bias += POFF;
    const int xx = (int)(i % W), yy = (int)((i / W) % H);
    const int t = (int)((i / hw) % TT), co = (int)((i / (hw * TT)) % Co);
    const int64_t b = i / (hw * TT * Co);
    float acc = bias[co];
    for (int ci = 0; ci < Ci; ci++) {
        const float *xp = x + ((b * Ci + ci) * TT + t) * hw;
        for (int ky = 0; ky < 3; ky++) {
            const int y = yy + ky - 1;
            if (y < 0 || y >= H) continue;
            for (int kx = 0; kx < 3; kx++) {
                const int xq = xx + kx - 1;
                if (xq < 0 || xq >= W) continue;
                acc += xp[(int64_t)y * W + xq] * k[((ky * 3 + kx) * Ci + ci) * Co + co];
            }
        }
    }
    out[i] = fmaxf(acc, 0.f);
}

// dX of the conv: dx[b][ci][t][y][x] = sum dA[b][co][t][y-ky+1][x-kx+1] * k[ky][kx][ci][co]
template <bool SET>
__global__ void k_conv3_dgrad(Mdl md, const float *__restrict__ dA, const float *__restrict__ k, float *__restrict__ dx, int Ci,
                              int Co, int H, int W) {
    const int B = model_b<SET>(md);
    const int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
    const int64_t hw = (int64_t)H * W, n = (int64_t)B * Ci * TT * hw;
    if (i >= n) return;
    dA += MOFF(Co * TT * hw);
    dx += MOFF(Ci * TT * hw);
    k += POFF;
    const int xx = (int)(i % W), yy = (int)((i / W) % H);
    const int t = (int)((i / hw) % TT), ci = (int)((i / (hw * TT)) % Ci);
    const int64_t b = i / (hw * TT * Ci);
    float acc = 0.f;
    for (int co = 0; co < Co; co++) {
        const float *gp = dA + ((b * Co + co) * TT + t) * hw;
        for (int ky = 0; ky < 3; ky++) {
            const int y = yy - ky + 1;
            if (y < 0 || y >= H) continue;
            for (int kx = 0; kx < 3; kx++) {
                const int xq = xx - kx + 1;
                if (xq < 0 || xq >= W) continue;
                acc += gp[(int64_t)y * W + xq] * k[((ky * 3 + kx) * Ci + ci) * Co + co];
            }
        }
    }
    dx[i] = acc;
}

// dK slabs of the conv: slab s covers positions [s*chunk, (s+1)*chunk) of the B*T*H*W positions; one thread per weight.
// The slab count and chunk follow the model's own batch (wg_slabs of its positions).
template <bool SET>
__global__ void k_conv3_wgrad(Mdl md, const float *__restrict__ dA, const float *__restrict__ x, float *__restrict__ slab, int Ci,
                              int Co, int H, int W, int64_t solo_chunk) {
    const int B = model_b<SET>(md);
    const int nw = 9 * Ci * Co;
    const int wi = blockIdx.x * BLK + threadIdx.x;
    const int64_t hw = (int64_t)H * W, P = (int64_t)B * TT * hw;
    const int ns = wg_slabs(P);
    if (B == 0 || (int)blockIdx.y >= ns || wi >= nw) return;
    const int64_t chunk = SET ? uniform64((P + ns - 1) / ns) : solo_chunk;
    dA += MOFF(Co * TT * hw);
    x += MOFF(Ci * TT * hw);
    slab += blockIdx.z * md.slab_stride;
    const int co = wi % Co, ci = (wi / Co) % Ci, kk = wi / (Co * Ci), ky = kk / 3, kx = kk % 3;
    const int64_t p0 = (int64_t)blockIdx.y * chunk, p1 = p0 + chunk < P ? p0 + chunk : P;
    float acc = 0.f;
    for (int64_t p = p0; p < p1; p++) {
        const int64_t s = p % hw, bt = p / hw;
        const int64_t b = bt / TT, t = bt % TT;
        const int y = (int)(s / W) + ky - 1, xq = (int)(s % W) + kx - 1;
        if (y < 0 || y >= H || xq < 0 || xq >= W) continue;
        acc += dA[((b * Co + co) * TT + t) * hw + s] * x[((b * Ci + ci) * TT + t) * hw + (int64_t)y * W + xq];
    }
    slab[(int64_t)blockIdx.y * nw + wi] = acc;
}

// out[i] = sum over slabs s of slab[s][i], in slab order.  The model's slab count: wg_slabs (tmix: tmix_blocks) of its batch
// times `per` positions per sample.
template <bool SET>
__global__ void k_sum_slabs(Mdl md, const float *__restrict__ slab, int64_t per, int tmix, int n, float *__restrict__ out) {
    const int B = model_b<SET>(md);
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (B == 0 || i >= n) return;
    const int nslab = tmix ? tmix_blocks(B * per) : wg_slabs(B * per);
    slab += blockIdx.z * md.slab_stride;
    out += POFF;
    float acc = 0.f;
    for (int s = 0; s < nslab; s++) acc += slab[(int64_t)s * n + i];
    out[i] = acc;
}

// Per-channel reductions of a [N][C][S] tensor: slab p of channel c covers elements [p*chunk, (p+1)*chunk) of its N*S.
enum RedMode { R_SUM = 0, R_SQDEV = 1, R_BNBWD = 2, R_FINALW = 3, R_LOSS = 4 };
// N = the model's batch and C = Cc, but for R_LOSS, where N = 1 and C = the model's batch (Cc: the grid's y extent).
// POST (R_LOSS only, S = hw): a macroblock outside the model's keep row enters I and S as y = p = 0, a select in front of the same
// two statements, so a row of ones gives the sums of the form without, bit for bit, and its label byte reaches nothing.
template <bool SET, class... Post>
__global__ void k_reduce(Mdl md, int mode, int Cc, int64_t S, const float *__restrict__ x, const float *__restrict__ g, int Cg,
                         const float *__restrict__ aux, const uint8_t *__restrict__ gt, float *__restrict__ part, int64_t solo_chunk,
                         Post... post) {
    constexpr bool POST = sizeof...(Post) != 0;
    __shared__ float sa[BLK], sb[BLK];
    const int Bm = model_b<SET>(md);
    const int N = mode == R_LOSS ? 1 : Bm, C = mode == R_LOSS ? Bm : Cc;
    const int c = blockIdx.y, p = blockIdx.x;
    const int64_t M = (int64_t)N * S;
    const int NP = red_slabs(M);
    if (Bm == 0 || c >= C || p >= NP) return;
    const int64_t chunk = SET ? uniform64((M + NP - 1) / NP) : solo_chunk;
    x += MOFF(mode == R_LOSS ? S : Cc * S);
    if (g) g += MOFF(Cg * S);
    if (aux) aux += blockIdx.z * STAT_STRIDE;
    if (gt) gt += (int64_t)model_first<SET>(md) * S;
    part += blockIdx.z * md.slab_stride;
    const uint8_t *kp = POST ? post_tab_of(post...)->keep + (int64_t)blockIdx.z * S : nullptr;
    const int64_t e0 = (int64_t)p * chunk, e1 = e0 + chunk < M ? e0 + chunk : M;
    float a = 0.f, bsum = 0.f;
    for (int64_t e = e0 + threadIdx.x; e < e1; e += BLK) {
        const int64_t n = e / S, s = e % S;
        const int64_t xi = (n * C + c) * S + s;
        switch (mode) {
        case R_SUM: a += x[xi]; break;
        case R_SQDEV: { const float v = x[xi] - aux[c]; a += v * v; } break;
        case R_BNBWD: {
            const float gv = g[(n * Cg + c) * S + s];
            a += gv;
            bsum += gv * (x[xi] - aux[c]) * aux[C + c];
        } break;
        case R_FINALW: a += x[xi] * g[n * S + s]; break;
        case R_LOSS: {   // N = 1, C = batch: x = logits, gt = labels
            float pr = 1.f / (1.f + expf(-x[xi]));
            float yv = (float)gt[xi];
            if (POST && !kp[s]) pr = yv = 0.f;
            a += yv * pr;
            bsum += yv + pr;
        } break;
        }
    }
    sa[threadIdx.x] = a;
    sb[threadIdx.x] = bsum;
    __syncthreads();
    for (int w = BLK / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) {
            sa[threadIdx.x] += sa[threadIdx.x + w];
            sb[threadIdx.x] += sb[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part[((int64_t)c * NP + p) * 2] = sa[0];
        part[((int64_t)c * NP + p) * 2 + 1] = sb[0];
    }
}

enum FinMode { F_MEAN = 0, F_VAR = 1, F_SUM2 = 2, F_SUM = 3 };
// stat: [2][C].  F_MEAN: stat[0] = mean.  F_VAR: stat[1] = 1/sqrt(var + eps), g0/g1 = batch mean / biased variance, mov0/mov1
// moving statistics (variance with n/(n-1)).  F_SUM2: stat = (sum a, sum b), g0 = sum b, g1 = sum a (BN gamma / beta
// gradients).  F_SUM: g0 = sum a.
// The slabs are summed in double: a channel of a large batch has over a thousand of them (1,125 at encoder level 0 of 45x80 at
// batch 320), and a float running sum over that many moves the batch statistics far enough to flip ReLU / max-pool decisions.
// lossmode: the slabs of k_reduce(R_LOSS) (C = the model's batch, one sample per "channel").  stat is a model's BN statistics
// or its `red` block (stat_stride floats per model); g0 / g1 / mov0 / mov1 point into gradients / parameters.
template <bool SET>
__global__ void k_finalize(Mdl md, int mode, int lossmode, int Cc, int64_t S, const float *__restrict__ part, float *stat,
                           int64_t stat_stride, float *g0, float *g1, float *mov0, float *mov1, float mom, float eps) {
    const int Bm = model_b<SET>(md);
    const int C = lossmode ? Bm : Cc;
    const int c = blockIdx.x * BLK + threadIdx.x;
    if (Bm == 0 || c >= C) return;
    const int64_t Mi = (int64_t)(lossmode ? 1 : Bm) * S;
    const int NP = red_slabs(Mi);
    const double M = (double)Mi;
    part += blockIdx.z * md.slab_stride;
    if (stat) stat += blockIdx.z * stat_stride;
    if (g0) g0 += POFF;
    if (g1) g1 += POFF;
    if (mov0) mov0 += POFF;
    if (mov1) mov1 += POFF;
    double a = 0.0, b = 0.0;
    for (int p = 0; p < NP; p++) {
        a += part[((int64_t)c * NP + p) * 2];
        b += part[((int64_t)c * NP + p) * 2 + 1];
    }
    if (mode == F_MEAN) {
        stat[c] = (float)(a / M);
    } else if (mode == F_VAR) {
        const float var = (float)(a / M), mean = stat[c];
        stat[C + c] = 1.f / sqrtf(var + eps);
        g0[c] = mean;
        g1[c] = var;
        mov0[c] = mom * mov0[c] + (1.f - mom) * mean;
        mov1[c] = mom * mov1[c] + (1.f - mom) * (float)(var * (M / (M - 1.0)));
    } else if (mode == F_SUM2) {
        stat[c] = (float)a;
        stat[C + c] = (float)b;
        if (g0) g0[c] = (float)b;
        if (g1) g1[c] = (float)a;
    } else {
        g0[c] = (float)a;
    }
}

// BN apply + 2x2 max-pool (valid) + zero row on top / column on the left for odd sizes, with the window argmax (first maximum in
// row-major order; -1 on pad positions).  c: [B][C][T][H][W] -> p: [B][C][T][Hp][Wp]
template <bool SET>
__global__ void k_bn_pool(Mdl md, const float *__restrict__ c, const float *__restrict__ stat, const float *__restrict__ gamma,
                          const float *__restrict__ beta, float *__restrict__ p, int8_t *__restrict__ arg, int C, int H, int W,
                          int Hp, int Wp) {
    const int B = model_b<SET>(md);
    const int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
    const int64_t hwp = (int64_t)Hp * Wp, n = (int64_t)B * C * TT * hwp;
    if (i >= n) return;
    c += MOFF(C * TT * H * W);
    p += MOFF(C * TT * hwp);
    arg += MOFF(C * TT * hwp);
    stat += blockIdx.z * STAT_STRIDE;
    gamma += POFF;
    beta += POFF;
    const int px = (int)(i % Wp), py = (int)((i / Wp) % Hp);
    const int64_t bct = i / hwp;
    const int ch = (int)((bct / TT) % C);
    const int pt = H & 1, pl = W & 1;
    if (py < pt || px < pl) {
        p[i] = 0.f;
        arg[i] = -1;
        return;
    }
    const float mean = stat[ch], inv = stat[C + ch], ga = gamma[ch], be = beta[ch];
    const float *src = c + bct * (int64_t)H * W + (int64_t)(2 * (py - pt)) * W + 2 * (px - pl);
    float best = 0.f;
    int bk = 0;
    for (int k = 0; k < 4; k++) {
        const float v = (src[(k >> 1) * W + (k & 1)] - mean) * inv * ga + be;
        if (k == 0 || v > best) { best = v; bk = k; }
    }
    p[i] = best;
    arg[i] = (int8_t)bk;
}

// gradient of the pool: each pre-pool element takes its window's gradient if it was the argmax; dropped rows / columns get 0
template <bool SET>
__global__ void k_pool_bwd(Mdl md, const float *__restrict__ dp, const int8_t *__restrict__ arg, float *__restrict__ dn, int C, int H,
                           int W, int Hp, int Wp) {
    const int B = model_b<SET>(md);
    const int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
    const int64_t hw = (int64_t)H * W, n = (int64_t)B * C * TT * hw;
    if (i >= n) return;
    dp += MOFF(C * TT * Hp * Wp);
    arg += MOFF(C * TT * Hp * Wp);
    dn += MOFF(C * TT * hw);
    const int xx = (int)(i % W), yy = (int)((i / W) % H);
    const int64_t bct = i / hw;
    const int pt = H & 1, pl = W & 1;
    float v = 0.f;
    if (yy < 2 * (Hp - pt) && xx < 2 * (Wp - pl)) {
        const int64_t pi = bct * Hp * Wp + (int64_t)(yy / 2 + pt) * Wp + (xx / 2 + pl);
        if (arg[pi] == (yy & 1) * 2 + (xx & 1)) v = dp[pi];
    }
    dn[i] = v;
}

// BN backward apply: out = gamma * invstd / M * (M * g - sum g - xhat * sum g*xhat), times (x > 0) when relu_in (the BN input is
// the post-ReLU conv output).  g has Cg channels per sample (a channel range of a concat buffer), out has C.  g and out may be
// the same buffer (the encoder runs it in place: each thread reads its own element before it writes it), so neither is restrict.
template <bool SET>
__global__ void k_bn_bwd(Mdl md, const float *g, int Cg, const float *__restrict__ x, const float *__restrict__ stat,
                         const float *__restrict__ red, const float *__restrict__ gamma, float *out, int C,
                         int64_t S, int relu_in) {
    const int B = model_b<SET>(md);
    const int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
    const int64_t n = (int64_t)B * C * S;
    if (i >= n) return;
    g += MOFF(Cg * S);
    x += MOFF(C * S);
    out += MOFF(C * S);
    stat += blockIdx.z * STAT_STRIDE;
    red += blockIdx.z * red_stride(md.maxB);
    gamma += POFF;
    const int64_t s = i % S;
    const int ch = (int)((i / S) % C);
    const int64_t b = i / (S * C);
    const float M = (float)((double)B * S);
    const float mean = stat[ch], inv = stat[C + ch];
    const float xv = x[i], xh = (xv - mean) * inv;
    const float gv = g[(b * Cg + ch) * S + s];
    float d = gamma[ch] * inv / M * (M * gv - red[ch] - xh * red[C + ch]);
    if (relu_in && !(xv > 0.f)) d = 0.f;
    out[i] = d;
}

// BN backward apply of a layer in inference mode (the training plan, include/covahip.h "Fine-tuning"): the layer normalised with
// constants, so out = g * gamma * invstd with no batch-mean terms; times (x > 0) when relu_in.  stat[C + ch] = 1 / sqrt(moving
// variance + eps) (k_bn_stat).  g and out may be the same buffer, as in k_bn_bwd.
template <bool SET>
__global__ void k_bn_bwd_inf(Mdl md, const float *g, int Cg, const float *__restrict__ x, const float *__restrict__ stat,
                             const float *__restrict__ gamma, float *out, int C, int64_t S, int relu_in) {
    const int B = model_b<SET>(md);
    const int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
    const int64_t n = (int64_t)B * C * S;
    if (i >= n) return;
    g += MOFF(Cg * S);
    x += MOFF(C * S);
    out += MOFF(C * S);
    stat += blockIdx.z * STAT_STRIDE;
    gamma += POFF;
    const int64_t s = i % S;
    const int ch = (int)((i / S) % C);
    const int64_t b = i / (S * C);
    float d = g[(b * Cg + ch) * S + s] * (gamma[ch] * stat[C + ch]);
    if (relu_in && !(x[i] > 0.f)) d = 0.f;
    out[i] = d;
}

// PointWiseTN forward per (b, c, y, x): o = relu(drop(relu(drop(relu(p @ w1)) @ w2)) + p); the t = 0 slice also goes to the
// decoder's concat buffer (channel c_off + c of Ctot).  Dropout indices: NCTHW of the layer's output.
template <bool SET>
__global__ void k_tmix_fwd(Mdl md, const float *__restrict__ p, const float *__restrict__ w1, const float *__restrict__ w2,
                           float *__restrict__ e, float *__restrict__ skip, int Ctot, int c_off, int C, int64_t hw, DropS s1,
                           DropS s2) {
    const int B = model_b<SET>(md);
    const int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
    const int64_t n = (int64_t)B * C * hw;
    if (i >= n) return;
    const Drop d1 = model_drop<SET>(md, s1), d2 = model_drop<SET>(md, s2);
    p += MOFF(C * TT * hw);
    e += MOFF(C * TT * hw);
    if (skip) skip += MOFF(Ctot * hw);
    w1 += POFF;
    w2 += POFF;
    const int64_t s = i % hw, bc = i / hw;
    float pv[TT], u[TT], v[TT];
    for (int t = 0; t < TT; t++) pv[t] = p[(bc * TT + t) * hw + s];
    for (int j = 0; j < TT; j++) {
        float a = 0.f;
        for (int k = 0; k < TT; k++) a += pv[k] * w1[k * TT + j];
        u[j] = fmaxf(a, 0.f) * keep(d1, (uint64_t)((bc * TT + j) * hw + s));
    }
    for (int j = 0; j < TT; j++) {
        float a = 0.f;
        for (int k = 0; k < TT; k++) a += u[k] * w2[k * TT + j];
        v[j] = fmaxf(a, 0.f) * keep(d2, (uint64_t)((bc * TT + j) * hw + s));
    }
    for (int t = 0; t < TT; t++) e[(bc * TT + t) * hw + s] = fmaxf(v[t] + pv[t], 0.f);
    if (skip) {
        const int64_t b = bc / C, c = bc % C;
        skip[(b * Ctot + c_off + c) * hw + s] = fmaxf(v[0] + pv[0], 0.f);
    }
}

// PointWiseTN backward: recomputes the forward from p, takes de (full T, may be null) plus the concat buffer's gradient of the
// t = 0 slice (dskip, may be null), writes dp and one slab of the 32 weight gradients (w1 then w2) per workgroup.
template <bool SET>
__global__ void k_tmix_bwd(Mdl md, const float *__restrict__ p, const float *__restrict__ w1, const float *__restrict__ w2,
                           const float *__restrict__ de, const float *__restrict__ dskip, int Ctot, int c_off, float *__restrict__ dp,
                           float *__restrict__ slab, int C, int64_t hw, int64_t solo_chunk, DropS s1, DropS s2) {
    __shared__ float red[32][BLK + 1];
    const int B = model_b<SET>(md);
    const int64_t n = (int64_t)B * C * hw;
    const int nb = tmix_blocks(n);   // the model's own split of its n positions
    if (B == 0 || (int)blockIdx.x >= nb) return;
    const int64_t chunk = SET ? uniform64((n + nb - 1) / nb) : solo_chunk;
    const Drop d1 = model_drop<SET>(md, s1), d2 = model_drop<SET>(md, s2);
    p += MOFF(C * TT * hw);
    dp += MOFF(C * TT * hw);
    if (de) de += MOFF(C * TT * hw);
    if (dskip) dskip += MOFF(Ctot * hw);
    slab += blockIdx.z * md.slab_stride;
    w1 += POFF;
    w2 += POFF;
    float gw[32];
    for (int q = 0; q < 32; q++) gw[q] = 0.f;
    const int64_t i0 = (int64_t)blockIdx.x * chunk, i1 = i0 + chunk < n ? i0 + chunk : n;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += BLK) {
        const int64_t s = i % hw, bc = i / hw;
        float pv[TT], pu[TT], m1[TT], u[TT], pvv[TT], m2[TT], o[TT];
        for (int t = 0; t < TT; t++) pv[t] = p[(bc * TT + t) * hw + s];
        for (int j = 0; j < TT; j++) {
            float a = 0.f;
            for (int k = 0; k < TT; k++) a += pv[k] * w1[k * TT + j];
            pu[j] = a;
            m1[j] = keep(d1, (uint64_t)((bc * TT + j) * hw + s));
            u[j] = fmaxf(a, 0.f) * m1[j];
        }
        for (int j = 0; j < TT; j++) {
            float a = 0.f;
            for (int k = 0; k < TT; k++) a += u[k] * w2[k * TT + j];
            pvv[j] = a;
            m2[j] = keep(d2, (uint64_t)((bc * TT + j) * hw + s));
            o[j] = fmaxf(a, 0.f) * m2[j] + pv[j];
        }
        float dov[TT], dpre2[TT], du[TT], dpre1[TT], dpv[TT];
        for (int t = 0; t < TT; t++) {
            float g = de ? de[(bc * TT + t) * hw + s] : 0.f;
            if (t == 0 && dskip) {
                const int64_t b = bc / C, c = bc % C;
                g += dskip[(b * Ctot + c_off + c) * hw + s];
            }
            dov[t] = o[t] > 0.f ? g : 0.f;
            dpv[t] = dov[t];
            dpre2[t] = pvv[t] > 0.f ? dov[t] * m2[t] : 0.f;
        }
        for (int k = 0; k < TT; k++) {
            float a = 0.f;
            for (int j = 0; j < TT; j++) {
                gw[16 + k * TT + j] += u[k] * dpre2[j];
                a += dpre2[j] * w2[k * TT + j];
            }
            du[k] = a;
        }
        for (int j = 0; j < TT; j++) dpre1[j] = pu[j] > 0.f ? du[j] * m1[j] : 0.f;
        for (int k = 0; k < TT; k++) {
            float a = 0.f;
            for (int j = 0; j < TT; j++) {
                gw[k * TT + j] += pv[k] * dpre1[j];
                a += dpre1[j] * w1[k * TT + j];
            }
            dp[(bc * TT + k) * hw + s] = dpv[k] + a;
        }
    }
    for (int q = 0; q < 32; q++) red[q][threadIdx.x] = gw[q];
    __syncthreads();
    for (int w = BLK / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w)
            for (int q = 0; q < 32; q++) red[q][threadIdx.x] += red[q][threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x < 32) slab[(int64_t)blockIdx.x * 32 + threadIdx.x] = red[threadIdx.x][0];
}

// decoder block input: zd = dropout(relu(z)), index = NCHW of z
template <bool SET>
__global__ void k_drop_relu(Mdl md, const float *__restrict__ z, float *__restrict__ zd, int64_t per, DropS ds) {
    const int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
    const int64_t n = model_b<SET>(md) * per;
    if (i >= n) return;
    const Drop d = model_drop<SET>(md, ds);
    z += MOFF(per);
    zd += MOFF(per);
    zd[i] = fmaxf(z[i], 0.f) * keep(d, (uint64_t)i);
}

// convT 4x4 stride 2 (valid, output 2*in + 2) + bias, cropped at (cy, cx); K: Keras [4][4][Co][Ci]
template <bool SET>
__global__ void k_convT_fwd(Mdl md, const float *__restrict__ zd, const float *__restrict__ K, const float *__restrict__ bias,
                            float *__restrict__ y, int Ci, int Co, int Hi, int Wi, int Ho, int Wo, int cy, int cx) {
    const int B = model_b<SET>(md);
    const int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
    const int64_t n = (int64_t)B * Co * Ho * Wo;
    if (i >= n) return;
    zd += MOFF(Ci * Hi * Wi);
    y += MOFF(Co * Ho * Wo);
    K += POFF;
    bias += POFF;
    const int ox = (int)(i % Wo) + cx, oy = (int)((i / Wo) % Ho) + cy;
    const int co = (int)((i / ((int64_t)Ho * Wo)) % Co);
    const int64_t b = i / ((int64_t)Ho * Wo * Co);
    float acc = bias[co];
    for (int ky = oy & 1; ky < 4; ky += 2) {
        const int iy = (oy - ky) >> 1;
        if (iy < 0 || iy >= Hi) continue;
        for (int kx = ox & 1; kx < 4; kx += 2) {
            const int ix = (ox - kx) >> 1;
            if (ix < 0 || ix >= Wi) continue;
            const float *kp = K + ((ky * 4 + kx) * Co + co) * Ci;
            const float *zp = zd + b * Ci * Hi * Wi + (int64_t)iy * Wi + ix;
            for (int ci = 0; ci < Ci; ci++) acc += zp[(int64_t)ci * Hi * Wi] * kp[ci];
        }
    }
    y[i] = acc;
}

// gradient of the block input z: convT data gradient times the dropout mask and relu(z)'
template <bool SET>
__global__ void k_convT_dgrad(Mdl md, const float *__restrict__ dy, const float *__restrict__ K, const float *__restrict__ z,
                              float *__restrict__ dz, int Ci, int Co, int Hi, int Wi, int Ho, int Wo, int cy, int cx, DropS ds) {
    const int B = model_b<SET>(md);
    const int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
    const int64_t n = (int64_t)B * Ci * Hi * Wi;
    if (i >= n) return;
    const Drop d = model_drop<SET>(md, ds);
    dy += MOFF(Co * Ho * Wo);
    z += MOFF(Ci * Hi * Wi);
    dz += MOFF(Ci * Hi * Wi);
    K += POFF;
    const float m = z[i] > 0.f ? keep(d, (uint64_t)i) : 0.f;
    if (m == 0.f) {
        dz[i] = 0.f;
        return;
    }
    const int ix = (int)(i % Wi), iy = (int)((i / Wi) % Hi);
    const int ci = (int)((i / ((int64_t)Hi * Wi)) % Ci);
    const int64_t b = i / ((int64_t)Hi * Wi * Ci);
    float acc = 0.f;
    for (int ky = 0; ky < 4; ky++) {
        const int yy = 2 * iy + ky - cy;
        if (yy < 0 || yy >= Ho) continue;
        for (int kx = 0; kx < 4; kx++) {
            const int xx = 2 * ix + kx - cx;
            if (xx < 0 || xx >= Wo) continue;
            const float *gp = dy + b * Co * Ho * Wo + (int64_t)yy * Wo + xx;
            const float *kp = K + (ky * 4 + kx) * Co * Ci + ci;
            for (int co = 0; co < Co; co++) acc += gp[(int64_t)co * Ho * Wo] * kp[co * Ci];
        }
    }
    dz[i] = acc * m;
}

// dK slabs of the convT: one thread per weight [ky][kx][co][ci], slab = a range of the B*Hi*Wi input positions
template <bool SET>
__global__ void k_convT_wgrad(Mdl md, const float *__restrict__ zd, const float *__restrict__ dy, float *__restrict__ slab, int Ci,
                              int Co, int Hi, int Wi, int Ho, int Wo, int cy, int cx, int64_t solo_chunk) {
    const int B = model_b<SET>(md);
    const int nw = 16 * Co * Ci;
    const int wi = blockIdx.x * BLK + threadIdx.x;
    const int64_t hwi = (int64_t)Hi * Wi, P = (int64_t)B * hwi;
    const int ns = wg_slabs(P);
    if (B == 0 || (int)blockIdx.y >= ns || wi >= nw) return;
    const int64_t chunk = SET ? uniform64((P + ns - 1) / ns) : solo_chunk;
    zd += MOFF(Ci * hwi);
    dy += MOFF(Co * Ho * Wo);
    slab += blockIdx.z * md.slab_stride;
    const int ci = wi % Ci, co = (wi / Ci) % Co, kk = wi / (Ci * Co), ky = kk / 4, kx = kk % 4;
    const int64_t p0 = (int64_t)blockIdx.y * chunk, p1 = p0 + chunk < P ? p0 + chunk : P;
    float acc = 0.f;
    for (int64_t p = p0; p < p1; p++) {
        const int64_t b = p / hwi, s = p % hwi;
        const int iy = (int)(s / Wi), ix = (int)(s % Wi);
        const int yy = 2 * iy + ky - cy, xx = 2 * ix + kx - cx;
        if (yy < 0 || yy >= Ho || xx < 0 || xx >= Wo) continue;
        acc += zd[(b * Ci + ci) * hwi + s] * dy[((b * Co + co) * Ho + yy) * (int64_t)Wo + xx];
    }
    slab[(int64_t)blockIdx.y * nw + wi] = acc;
}

// decoder BN apply into channels [0, C) of the next block's concat buffer (Ctot channels)
template <bool SET>
__global__ void k_bn_apply(Mdl md, const float *__restrict__ y, const float *__restrict__ stat, const float *__restrict__ gamma,
                           const float *__restrict__ beta, float *__restrict__ z, int Ctot, int C, int64_t S) {
    const int B = model_b<SET>(md);
    const int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
    const int64_t n = (int64_t)B * C * S;
    if (i >= n) return;
    y += MOFF(C * S);
    z += MOFF(Ctot * S);
    stat += blockIdx.z * STAT_STRIDE;
    gamma += POFF;
    beta += POFF;
    const int64_t s = i % S;
    const int ch = (int)((i / S) % C);
    const int64_t b = i / (S * C);
    z[(b * Ctot + ch) * S + s] = (y[i] - stat[ch]) * stat[C + ch] * gamma[ch] + beta[ch];
}

// 1x1 conv 16 -> 1 of the last block's output: logits [B][H*W]
template <bool SET>
__global__ void k_final_fwd(Mdl md, const float *__restrict__ y, const float *__restrict__ fk, const float *__restrict__ fb,
                            float *__restrict__ logit, int64_t hw) {
    const int B = model_b<SET>(md);
    const int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (i >= (int64_t)B * hw) return;
    y += MOFF(16 * hw);
    logit += MOFF(hw);
    fk += POFF;
    fb += POFF;
    const int64_t b = i / hw, s = i % hw;
    float acc = fb[0];
    for (int c = 0; c < 16; c++) acc += y[(b * 16 + c) * hw + s] * fk[c];
    logit[i] = acc;
}

// A sample's loss: the Jaccard distance (1 - (I + sm) / (S - I + sm)) * sm of its I = sum y*p and S = sum y + p
__device__ inline float jaccard_distance(float I, float S, float sm) { return (1.f - (I + sm) / (S - I + sm)) * sm; }

// One position's share of the workgroup's TP / FP / FN counters (cnt[3] in LDS)
__device__ inline void count_pos(unsigned *cnt, bool pos, uint8_t label) {
    const bool lab = label != 0;
    if (pos && lab) atomicAdd(&cnt[0], 1u);
    if (pos && !lab) atomicAdd(&cnt[1], 1u);
    if (!pos && lab) atomicAdd(&cnt[2], 1u);
}
// ... at sigmoid > 0.5
__device__ inline void count_confusion(unsigned *cnt, float pr, uint8_t label) { count_pos(cnt, pr > 0.5f, label); }
// ... of a trainer with a post: nothing outside the keep row; inside, a model with a post counts serving's logit > thresh (NaN is
// background), a model without one sigmoid > 0.5 as above.  s = the position in its sample.
__device__ inline void count_confusion_post(unsigned *cnt, const PostTab *pt, int64_t hw, int64_t s, float l, float pr,
                                            const uint8_t *label) {
    if (!pt->keep[(int64_t)blockIdx.z * hw + s]) return;
    count_pos(cnt, pt->flag[blockIdx.z] ? l > pt->thresh[blockIdx.z] : pr > 0.5f, *label);
}

// loss = mean over samples of their Jaccard distance; red = [I per sample][S per sample]
template <bool SET>
__global__ void k_loss(Mdl md, const float *__restrict__ red, float sm, float *__restrict__ loss) {
    const int B = model_b<SET>(md);
    if (threadIdx.x || blockIdx.x || B == 0) return;
    red += blockIdx.z * red_stride(md.maxB);
    loss += blockIdx.z;
    float acc = 0.f;
    for (int b = 0; b < B; b++) acc += jaccard_distance(red[b], red[B + b], sm);
    loss[0] = acc / (float)B;
}

// d loss / d logit and d loss / d y3 (= dlogit * final kernel); TP / FP / FN counts at sigmoid > 0.5 (integer atomics).
// POST: d loss / d logit = 0 outside the keep row (a select behind the expression of the form without, whose I and S are the masked sums), the
// counts by count_confusion_post.
template <bool SET, class... Post>
__global__ void k_final_bwd(Mdl md, const float *__restrict__ logit, const uint8_t *__restrict__ gt, const float *__restrict__ red,
                            const float *__restrict__ fk, float *__restrict__ dlogit, float *__restrict__ dy, int64_t hw,
                            float sm, unsigned long long *__restrict__ counts, Post... post) {
    constexpr bool POST = sizeof...(Post) != 0;
    __shared__ unsigned cnt[3];
    const int B = model_b<SET>(md);
    if ((int64_t)blockIdx.x * BLK >= (int64_t)B * hw) return;   // the whole workgroup: before the barrier
    logit += MOFF(hw);
    dlogit += MOFF(hw);
    dy += MOFF(16 * hw);
    gt += (int64_t)model_first<SET>(md) * hw;
    red += blockIdx.z * red_stride(md.maxB);
    fk += POFF;
    counts += 3 * blockIdx.z;
    if (threadIdx.x < 3) cnt[threadIdx.x] = 0;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (i < (int64_t)B * hw) {
        const int64_t b = i / hw, s = i % hw;
        const float l = logit[i];
        const float pr = 1.f / (1.f + expf(-l));
        const bool kept = !POST || post_tab_of(post...)->keep[(int64_t)blockIdx.z * hw + s];
        const float yv = kept ? (float)gt[i] : 0.f;   // an ignored label byte is never looked at
        const float I = red[b], S = red[B + b];
        const float Nn = I + sm, D = S - I + sm;
        const float dp = -(sm / (float)B) * (yv * D - Nn * (1.f - yv)) / (D * D);
        const float dl = kept ? dp * pr * (1.f - pr) : 0.f;
        dlogit[i] = dl;
        for (int c = 0; c < 16; c++) dy[(b * 16 + c) * hw + s] = dl * fk[c];
        if (POST) count_confusion_post(cnt, post_tab_of(post...), hw, s, l, pr, gt + i);
        else count_confusion(cnt, pr, gt[i]);
    }
    __syncthreads();
    if (threadIdx.x < 3 && cnt[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
}

// ------------------------------------------------------------------------------------------------ evaluation kernels
// The evaluation pass (include/covahip.h, "Evaluation and resume") is the step's forward (forward() below) with two things
// different.  BatchNorm: k_bn_stat below fills `stat` from the moving statistics, in place of the reduce / finalize launches
// that fill it from the batch.  Dropout: every site gets threshold 0 and scale 1; keep() compares an unsigned value with >= 0,
// which holds for every hash, and returns the scale 1.0f, and x * 1.0f is x for every float (the products dropped are ReLU
// outputs: no NaN payloads to quieten), so the site is the identity bit for bit.
struct BNTab {                        // where the seven BN layers keep their moving statistics in the flat parameters
    int32_t mean[2 * NL - 1], var[2 * NL - 1], C[2 * NL - 1];
};
// The stat rows of the BN layers in inference mode (bit `layer` of layers: all seven in an evaluation, a training plan's in a
// step): stat[layer] = (moving mean, 1 / sqrt(moving variance + eps)), the expression k_finalize(F_VAR) forms from the batch
// variance.  grads (a step; null in an evaluation, which never writes gradients): the layer's mean / var gradient slots take
// the moving values the forward normalises with.  Once per step: an evaluation or a state load between two steps cannot
// leave a stale row.
template <bool SET>
__global__ void k_bn_stat(Mdl md, const float *__restrict__ params, float *__restrict__ grads, float *__restrict__ stat, BNTab t,
                          uint32_t layers, float eps) {
    const int layer = blockIdx.x, c = threadIdx.x, C = t.C[layer];
    if (model_b<SET>(md) == 0 || !(layers >> layer & 1u) || c >= C) return;
    params += POFF;
    stat += blockIdx.z * STAT_STRIDE + layer * 256;
    const float mean = params[t.mean[layer] + c], var = params[t.var[layer] + c];
    stat[c] = mean;
    stat[C + c] = 1.f / sqrtf(var + eps);
    if (grads) {
        grads += POFF;
        grads[t.mean[layer] + c] = mean;
        grads[t.var[layer] + c] = var;
    }
}

// TP / FP / FN at sigmoid > 0.5 as k_final_bwd counts them (integer atomics; the counters run on over the chunks of one
// evaluation), and the per-sample Jaccard distance as k_loss forms it, to sample_loss[model][sample of the chunk].
// red = [I per sample][S per sample] of the model's chunk.
// POST: the counts by count_confusion_post (red already holds the masked sums).
template <bool SET, class... Post>
__global__ void k_eval_tail(Mdl md, const float *__restrict__ logit, const uint8_t *__restrict__ gt, const float *__restrict__ red,
                            int64_t hw, float sm, unsigned long long *__restrict__ counts, float *__restrict__ sample_loss,
                            Post... post) {
    constexpr bool POST = sizeof...(Post) != 0;
    __shared__ unsigned cnt[3];
    const int B = model_b<SET>(md);
    if ((int64_t)blockIdx.x * BLK >= (int64_t)B * hw) return;   // the whole workgroup: before the barrier
    logit += MOFF(hw);
    gt += (int64_t)model_first<SET>(md) * hw;
    red += blockIdx.z * red_stride(md.maxB);
    counts += 3 * blockIdx.z;
    if (blockIdx.x == 0) {
        sample_loss += (int64_t)blockIdx.z * md.maxB;
        for (int b = threadIdx.x; b < B; b += BLK) sample_loss[b] = jaccard_distance(red[b], red[B + b], sm);
    }
    if (threadIdx.x < 3) cnt[threadIdx.x] = 0;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (i < (int64_t)B * hw) {
        const float l = logit[i];
        if (POST) count_confusion_post(cnt, post_tab_of(post...), hw, i % hw, l, 1.f / (1.f + expf(-l)), gt + i);
        else count_confusion(cnt, 1.f / (1.f + expf(-l)), gt[i]);
    }
    __syncthreads();
    if (threadIdx.x < 3 && cnt[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
}

// Keras Adam over the flat parameter buffer; lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t) from the host
template <bool SET>
__global__ void k_adam(Mdl md, float *__restrict__ w, const float *__restrict__ g, float *__restrict__ m, float *__restrict__ v,
                       const uint8_t *__restrict__ trainable, int n, float b1, float b2, float eps) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (model_b<SET>(md) == 0 || i >= n || !trainable[i]) return;
    const float lr_t = model_lr_t<SET>(md);
    w += POFF;
    g += POFF;
    m += POFF;
    v += POFF;
    const float gi = g[i];
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    w[i] -= lr_t * mi / (sqrtf(vi) + eps);
}

// k_adam under a plan that freezes groups: mask 2 = a frozen slot, whose gradient reads 0 and whose weight and moments stay.
template <bool SET>
__global__ void k_adam_plan(Mdl md, float *__restrict__ w, float *__restrict__ g, float *__restrict__ m, float *__restrict__ v,
                            const uint8_t *__restrict__ trainable, int n, float b1, float b2, float eps) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (model_b<SET>(md) == 0 || i >= n || !trainable[i]) return;
    const float lr_t = model_lr_t<SET>(md);
    w += POFF;
    g += POFF;
    m += POFF;
    v += POFF;
    if (trainable[i] == 2) {
        g[i] = 0.f;
        return;
    }
    const float gi = g[i];
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    w[i] -= lr_t * mi / (sqrtf(vi) + eps);
}

// ------------------------------------------------------------------------------------------------ matrix-core convolutions
// COVAHIP_TRAIN_MATH_MATRIX (include/covahip.h, "Training arithmetic"): the 3x3 convolution's forward, data gradient and weight
// gradient and the transposed convolution's weight gradient as implicit GEMMs on v_mfma_f32_16x16x4_f32.  The instruction is an
// fp32 fmaf chain in k order with one rounding per product, so the arithmetic is the plain kernels' precision class; the order
// of the sums differs from theirs, which is why the mode is a choice and not a replacement.  Operands: lane l holds
// A[m = l & 15][k = l >> 4] and B[k = l >> 4][n = l & 15]; register r of the result is D[m = 4 * (l >> 4) + r][n = l & 15].
//
// The same guarantees as above: no float atomics; a weight gradient is split over the slabs wg_slabs gives for the model's own
// batch, each slab is one workgroup's fixed-order sum and k_sum_slabs adds the slabs in order; the model is the grid's z index.
// Every kernel walks tiles of consecutive positions in the tensors' own flattened order, so a row of any width is a sequence
// of tiles and a narrow level packs several rows into one.  A tap's neighbour is staged by the row it belongs to (a row outside
// the image stages zeros) and masked by the column of the position that reads it.
using f32x4 = __attribute__((ext_vector_type(4))) float;
constexpr int MM_PT = 64;             // positions per tile: conv forward / data gradient / weight gradient
constexpr int MM_KC = 8;              // summed channels staged at a time by the forward / data gradient
constexpr int MM_XS = 80;             // floats per staged row there: 66 used; 80 = 16 mod 64 keeps the four k rows of a read on distinct banks
constexpr int MM_WS = 68;             // floats per staged row of the weight gradients: = 4 mod 64, the 16 channels of a read on distinct banks
constexpr int MM_TPT = 32;            // positions per tile: transposed-conv weight gradient
constexpr int MM_TS = 36;             // floats per staged row there (= 4 mod 64)

// FWD:   out[b][co][s] = relu(bias[co] + sum_{tap, ci} in[b][ci][s + tap] * k[tap][ci][co])        (in = x, Cin = Ci, Cout = Co)
// DGRAD: out[b][ci][s] =                sum_{tap, co} in[b][co][s + tap] * k[8 - tap][ci][co]      (in = dA, Cin = Co, Cout = Ci)
// s: a position of the sample's T*H*W block, tap = (dy, dx) in -1..1.  A workgroup: 64 positions of one sample, 16 * NACC output
// channels (blockIdx.y); wave w: positions 16 w .. 16 w + 15.  M = output channel (A = weights), N = position (B = input),
// K = (tap, summed channel), MM_KC channels at a time through LDS.  grid.x = largest batch * tiles per sample.
template <bool SET, bool DGRAD, int NACC>
__global__ void __launch_bounds__(BLK) k_conv3_mm(Mdl md, const float *__restrict__ in, const float *__restrict__ k,
                                                  const float *__restrict__ bias, float *__restrict__ out, int Ci, int Co, int H, int W) {
    constexpr int NB = 16 * NACC, WST = NB + 16;
    __shared__ float xs[3 * MM_KC * MM_XS];
    __shared__ float ws[9 * MM_KC * WST];
    __shared__ int sy[MM_PT + 2];
    const int B = model_b<SET>(md);
    const int hw = H * W, S = TT * hw;
    const int ntile = (S + MM_PT - 1) / MM_PT;
    const int b = blockIdx.x / ntile, s0 = (blockIdx.x % ntile) * MM_PT;
    if (b >= B) return;   // the whole workgroup: before the barriers
    const int Cin = DGRAD ? Co : Ci, Cout = DGRAD ? Ci : Co, ob = blockIdx.y * NB;
    in += MOFF(Cin * S) + (int64_t)b * Cin * S;
    out += MOFF(Cout * S) + (int64_t)b * Cout * S;
    k += POFF;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n = lane & 15, kq = lane >> 4;
    const int s = s0 + wave * 16 + n;
    const bool valid = s < S;
    const int xq = s % W;
    const bool okx[3] = {valid && xq > 0, valid, valid && xq < W - 1};
    if (tid < MM_PT + 2) {   // the row of slot tid's position, or far outside
        const int pj = s0 + tid - 1;
        sy[tid] = pj >= 0 && pj < S ? (pj % hw) / W : -4;
    }
    f32x4 acc[NACC];
    for (int a = 0; a < NACC; a++)
        for (int r = 0; r < 4; r++) acc[a][r] = DGRAD ? 0.f : bias[POFF + ob + a * 16 + kq * 4 + r];
    // A chunk's operands go global -> registers -> LDS: all loads of a chunk are in flight together, and the next chunk's are
    // issued before this chunk's products, which hide them.
    // Thread tid stages slot 1 + tid % 64 of the 24 input rows tid / 64 + 4 it; threads 0 .. 47 also slots 0 and 65 of a row.
    constexpr int XI = 3 * MM_KC / 4, NWE = 9 * MM_KC * NB, WI = (NWE + BLK - 1) / BLK;
    float xv[XI + 1], wv[WI];
    const int er = tid >> 1, ej = (tid & 1) * (MM_PT + 1);
    auto load = [&](int c0) {
        const int yj = sy[lane + 1];
#pragma unroll
        for (int it = 0; it < XI; it++) {
            const int dyi = it >> 1, c = c0 + 4 * (it & 1) + wave, yy = yj + dyi - 1;
            xv[it] = c < Cin && yy >= 0 && yy < H ? in[(int64_t)c * S + (s0 + lane + (dyi - 1) * W)] : 0.f;
        }
        {
            const int dyi = er >> 3, c = c0 + (er & 7), yy = tid < 6 * MM_KC ? sy[ej] + dyi - 1 : -1;
            xv[XI] = c < Cin && yy >= 0 && yy < H ? in[(int64_t)c * S + (s0 + ej - 1 + (dyi - 1) * W)] : 0.f;
        }
#pragma unroll
        for (int it = 0; it < WI; it++) {
            const int e = tid + it * BLK;
            int o, kc, tp;
            if (DGRAD) { kc = e % MM_KC; o = (e / MM_KC) % NB; tp = e / (MM_KC * NB); }
            else { o = e % NB; kc = (e / NB) % MM_KC; tp = e / (NB * MM_KC); }
            const int c = c0 + kc;
            wv[it] = e < NWE && c < Cin ? (DGRAD ? k[((8 - tp) * Ci + ob + o) * Co + c] : k[(tp * Ci + c) * Co + ob + o]) : 0.f;
        }
    };
    __syncthreads();   // sy written
    load(0);
    for (int c0 = 0; c0 < Cin; c0 += MM_KC) {
        __syncthreads();   // the previous chunk read
#pragma unroll
        for (int it = 0; it < XI; it++) xs[((it >> 1) * MM_KC + 4 * (it & 1) + wave) * MM_XS + lane + 1] = xv[it];
        if (tid < 6 * MM_KC) xs[er * MM_XS + ej] = xv[XI];
#pragma unroll
        for (int it = 0; it < WI; it++) {
            const int e = tid + it * BLK;
            int o, kc, tp;
            if (DGRAD) { kc = e % MM_KC; o = (e / MM_KC) % NB; tp = e / (MM_KC * NB); }
            else { o = e % NB; kc = (e / NB) % MM_KC; tp = e / (NB * MM_KC); }
            if (e < NWE) ws[(tp * MM_KC + kc) * WST + o] = wv[it];
        }
        __syncthreads();
        if (c0 + MM_KC < Cin) load(c0 + MM_KC);
        const int ksteps = Cin - c0 > 4 ? 2 : 1;
        for (int tp = 0; tp < 9; tp++) {
            const int dyi = tp / 3, dxi = tp % 3;
            for (int ks = 0; ks < ksteps; ks++) {
                const int kc = ks * 4 + kq;
                const float xn = xs[(dyi * MM_KC + kc) * MM_XS + wave * 16 + n + dxi];
                const float bv = okx[dxi] ? xn : 0.f;
                for (int a = 0; a < NACC; a++)
                    acc[a] = __builtin_amdgcn_mfma_f32_16x16x4f32(ws[(tp * MM_KC + kc) * WST + a * 16 + n], bv, acc[a], 0, 0, 0);
            }
        }
    }
    if (!valid) return;
    for (int a = 0; a < NACC; a++)
        for (int r = 0; r < 4; r++) {
            const int ch = ob + a * 16 + kq * 4 + r;
            out[(int64_t)ch * S + s] = DGRAD ? acc[a][r] : fmaxf(acc[a][r], 0.f);
        }
}

// dK slabs of the conv on the matrix cores: the slab split of k_conv3_wgrad (wg_slabs of the model's positions, the same
// chunk), slab[s][tap][ci][co].  Per tap a GEMM with M = ci (A = x at the tap's neighbour), N = co (B = dA), K = the slab's
// positions, 64 at a time through LDS.  A workgroup: one 16-channel tile of ci, up to 64 of co (blockIdx.x), all nine taps;
// its 9 * (co tiles) output tiles go round the four waves.  Ci = 3 is a tile whose other 13 rows are zero.
template <bool SET>
__global__ void __launch_bounds__(BLK) k_conv3_wgrad_mm(Mdl md, const float *__restrict__ dA, const float *__restrict__ x,
                                                        float *__restrict__ slab, int Ci, int Co, int H, int W, int64_t solo_chunk) {
    __shared__ float xs[3 * 16 * MM_WS];
    __shared__ float ds[64 * MM_WS];
    __shared__ int sb[MM_PT + 2], srem[MM_PT + 2], sy[MM_PT + 2], fl[MM_PT];
    const int B = model_b<SET>(md);
    const int hw = H * W, S = TT * hw;
    const int64_t P = (int64_t)B * S;
    const int ns = wg_slabs(P);
    if (B == 0 || (int)blockIdx.y >= ns) return;   // the whole workgroup: before the barriers
    const int64_t chunk = SET ? uniform64((P + ns - 1) / ns) : solo_chunk;
    const int CT = Co < 64 ? Co : 64, nct = CT / 16, ncb = Co / CT;
    const int ci0 = (blockIdx.x / ncb) * 16, cob = (blockIdx.x % ncb) * CT;
    const int ntiles = 9 * nct, nw = 9 * Ci * Co;
    dA += MOFF(Co * S);
    x += MOFF(Ci * S);
    slab += blockIdx.z * md.slab_stride;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n = lane & 15, kq = lane >> 4;
    const int64_t p0 = (int64_t)blockIdx.y * chunk, p1 = p0 + chunk < P ? p0 + chunk : P;
    f32x4 acc[9];
    int xo[9], dof[9], xm[9];   // tile q of this wave: where its lane reads x and dA in LDS, and its column's bit (1 left, 2 right, 4 centre)
#pragma unroll
    for (int q = 0; q < 9; q++) {
        acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int id = wave + 4 * q, tp = id / nct, cot = id % nct, dyi = tp / 3, dxi = tp % 3;
        xo[q] = (dyi * 16 + n) * MM_WS + dxi;
        dof[q] = (cot * 16 + n) * MM_WS;
        xm[q] = dxi == 0 ? 1 : dxi == 2 ? 2 : 4;
    }
    for (int64_t pt = p0; pt < p1; pt += MM_PT) {
        __syncthreads();   // the previous tile read
        if (tid < MM_PT + 2) {   // slot tid: position pt + tid - 1
            const int64_t pj = pt + tid - 1;
            int bb = 0, rem = 0, yy = -4;
            if (pj >= 0 && pj < P) {
                bb = (int)(pj / S);
                rem = (int)(pj % S);
                const int sp = rem % hw, xq = sp % W;
                yy = sp / W;
                if (tid >= 1 && tid <= MM_PT) fl[tid - 1] = (xq > 0 ? 1 : 0) | (xq < W - 1 ? 2 : 0);
            } else if (tid >= 1 && tid <= MM_PT) {
                fl[tid - 1] = 0;
            }
            sb[tid] = bb;
            srem[tid] = rem;
            sy[tid] = yy;
        }
        __syncthreads();
        // global -> registers -> LDS: all loads of the tile are in flight together.  Thread tid stages position tid % 64 of rows
        // tid / 64 + 4 it; threads 0 .. 95 also slots 0 and 65 (the positions in front of and behind the tile) of a row of x.
        constexpr int XI = 3 * 16 / 4, DI = 64 / 4;
        float xv[XI + 1], dv[DI];
        const int j = lane + 1;   // the slot of position tid % 64 (slot 0: the position in front of the tile)
        const int64_t xb = (int64_t)sb[j] * Ci * S + srem[j], db = ((int64_t)sb[j] * Co + cob) * S + srem[j];
        const int yj = sy[j];
        const bool din = pt + lane < p1;
#pragma unroll
        for (int it = 0; it < XI; it++) {
            const int dyi = it >> 2, ci = ci0 + 4 * (it & 3) + wave, yy = yj + dyi - 1;
            xv[it] = ci < Ci && yy >= 0 && yy < H ? x[xb + (int64_t)ci * S + (dyi - 1) * W] : 0.f;
        }
        const int er = tid >> 1, ej = (tid & 1) * (MM_PT + 1);   // row er < 48, slot 0 or 65
        {
            const int dyi = er >> 4, ci = ci0 + (er & 15), yy = tid < 96 ? sy[ej] + dyi - 1 : -1;
            xv[XI] = ci < Ci && yy >= 0 && yy < H ? x[((int64_t)sb[ej] * Ci + ci) * S + (srem[ej] + (dyi - 1) * W)] : 0.f;
        }
#pragma unroll
        for (int it = 0; it < DI; it++) {
            const int co = 4 * it + wave;
            dv[it] = co < CT && din ? dA[db + (int64_t)co * S] : 0.f;
        }
#pragma unroll
        for (int it = 0; it < XI; it++) xs[((it >> 2) * 16 + 4 * (it & 3) + wave) * MM_WS + j] = xv[it];
        if (tid < 96) xs[er * MM_WS + ej] = xv[XI];
#pragma unroll
        for (int it = 0; it < DI; it++)
            if (4 * it + wave < CT) ds[(4 * it + wave) * MM_WS + lane] = dv[it];
        __syncthreads();
#pragma unroll 2
        for (int ks = 0; ks < MM_PT / 4; ks++) {
            const int i = ks * 4 + kq, f = fl[i] | 4;
#pragma unroll
            for (int q = 0; q < 9; q++) {
                if (wave + 4 * q < ntiles) {
                    const float xn = xs[xo[q] + i];
                    acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(f & xm[q] ? xn : 0.f, ds[dof[q] + i], acc[q], 0, 0, 0);
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 9; q++) {
        const int id = wave + 4 * q;
        if (id >= ntiles) continue;
        const int tp = id / nct, cot = id % nct;
        for (int r = 0; r < 4; r++) {
            const int ci = ci0 + kq * 4 + r;
            if (ci < Ci) slab[(int64_t)blockIdx.y * nw + (tp * Ci + ci) * Co + cob + cot * 16 + n] = acc[q][r];
        }
    }
}

// dK slabs of the convT on the matrix cores: the slab split of k_convT_wgrad, slab[s][ky][kx][co][ci].  Per tap a GEMM with
// M = co (A = dy at the tap's output position, zero outside the crop), N = ci (B = zd), K = the slab's input positions, 32 at a
// time through LDS.  A workgroup: 16 of co, 16 * NCI of ci (blockIdx.x), all sixteen taps; wave w: the four taps of ky = w.
template <bool SET, int NCI>
__global__ void __launch_bounds__(BLK) k_convT_wgrad_mm(Mdl md, const float *__restrict__ zd, const float *__restrict__ dy,
                                                        float *__restrict__ slab, int Ci, int Co, int Hi, int Wi, int Ho, int Wo, int cy,
                                                        int cx, int64_t solo_chunk) {
    constexpr int CIB = 16 * NCI;
    __shared__ float dys[16 * 16 * MM_TS];
    __shared__ float zs[CIB * MM_TS];
    __shared__ int pb[MM_TPT], ps[MM_TPT], piy[MM_TPT], pix[MM_TPT];
    const int B = model_b<SET>(md);
    const int hwi = Hi * Wi, hwo = Ho * Wo;
    const int64_t P = (int64_t)B * hwi;
    const int ns = wg_slabs(P);
    if (B == 0 || (int)blockIdx.y >= ns) return;   // the whole workgroup: before the barriers
    const int64_t chunk = SET ? uniform64((P + ns - 1) / ns) : solo_chunk;
    const int ncib = Ci / CIB;
    const int cob = (blockIdx.x / ncib) * 16, cib = (blockIdx.x % ncib) * CIB;
    const int nw = 16 * Co * Ci;
    zd += MOFF(Ci * hwi);
    dy += MOFF(Co * hwo);
    slab += blockIdx.z * md.slab_stride;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n = lane & 15, kq = lane >> 4;
    const int64_t p0 = (int64_t)blockIdx.y * chunk, p1 = p0 + chunk < P ? p0 + chunk : P;
    f32x4 acc[4][NCI];
    for (int kx = 0; kx < 4; kx++)
        for (int c = 0; c < NCI; c++) acc[kx][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int64_t pt = p0; pt < p1; pt += MM_TPT) {
        __syncthreads();   // the previous tile read
        if (tid < MM_TPT) {
            const int64_t p = pt + tid;
            int bb = -1, sp = 0;
            if (p < p1) {
                bb = (int)(p / hwi);
                sp = (int)(p % hwi);
            }
            pb[tid] = bb;
            ps[tid] = sp;
            piy[tid] = sp / Wi;
            pix[tid] = sp % Wi;
        }
        __syncthreads();
        // global -> registers -> LDS: all loads of the tile are in flight together.  Thread tid stages position tid % 32 throughout.
        constexpr int YI = 16 * 16 * MM_TPT / BLK, ZI = CIB * MM_TPT / BLK;
        float yv[YI], zv[ZI];
        const int i = tid % MM_TPT, bi = pb[i], iy2 = 2 * piy[i] - cy, ix2 = 2 * pix[i] - cx, si = ps[i];
#pragma unroll
        for (int it = 0; it < YI; it++) {
            const int r = tid / MM_TPT + it * (BLK / MM_TPT), co = r % 16, tap = r / 16;
            const int yy = iy2 + (tap >> 2), xx = ix2 + (tap & 3);
            yv[it] = bi >= 0 && yy >= 0 && yy < Ho && xx >= 0 && xx < Wo ? dy[((int64_t)bi * Co + cob + co) * hwo + (yy * Wo + xx)] : 0.f;
        }
#pragma unroll
        for (int it = 0; it < ZI; it++) {
            const int ci = tid / MM_TPT + it * (BLK / MM_TPT);
            zv[it] = bi >= 0 ? zd[((int64_t)bi * Ci + cib + ci) * hwi + si] : 0.f;
        }
#pragma unroll
        for (int it = 0; it < YI; it++) dys[(tid / MM_TPT + it * (BLK / MM_TPT)) * MM_TS + i] = yv[it];
#pragma unroll
        for (int it = 0; it < ZI; it++) zs[(tid / MM_TPT + it * (BLK / MM_TPT)) * MM_TS + i] = zv[it];
        __syncthreads();
        for (int ks = 0; ks < MM_TPT / 4; ks++) {
            const int i = ks * 4 + kq;
            float bv[NCI];
            for (int c = 0; c < NCI; c++) bv[c] = zs[(c * 16 + n) * MM_TS + i];
            for (int kx = 0; kx < 4; kx++) {
                const float av = dys[((wave * 4 + kx) * 16 + n) * MM_TS + i];
                for (int c = 0; c < NCI; c++) acc[kx][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[c], acc[kx][c], 0, 0, 0);
            }
        }
    }
    for (int kx = 0; kx < 4; kx++)
        for (int c = 0; c < NCI; c++)
            for (int r = 0; r < 4; r++)
                slab[(int64_t)blockIdx.y * nw + ((wave * 4 + kx) * Co + cob + kq * 4 + r) * Ci + cib + c * 16 + n] = acc[kx][c][r];
}

}  // namespace

// ------------------------------------------------------------------------------------------------ host state

struct covahip_train {
    covahip_ctx *ctx = nullptr;
    covahip_train_cfg cfg{};
    int K = 1;                 // models; model m's slice of every buffer below lies m * max_batch samples (m * N_PARAMS for
                               // params / grads / adam_*) behind model 0's
    int H[NL + 1], W[NL + 1];
    int cy[NL], cx[NL];
    std::vector<int64_t> step;         // per model: steps taken (Adam's t - 1, the dropout hash's step)
    std::vector<uint64_t> seed;        // per model: dropout seed
    std::vector<long long> last_counts;   // per model: TP, FP, FN of its last step
    std::vector<void *> allocs;
    float *params = nullptr, *grads = nullptr, *adam_m = nullptr, *adam_v = nullptr;
    uint8_t *trainable = nullptr;      // one mask for all models: 1 trained, 0 BN moving statistics, 2 frozen by the plan
    uint32_t frozen = 0;               // the plan: frozen groups as given,
    uint32_t bn_inf = 0;               // and the EFFECTIVE inference-mode BN layers (given | frozen & 0x7F)
    // activations ([B][C][T][H][W] encoder, [B][C][H][W] decoder) and their gradients
    float *x0 = nullptr, *c[NL] = {}, *p[NL] = {}, *e[NL] = {};
    int8_t *arg[NL] = {};
    float *z[NL] = {}, *zd[NL] = {}, *y[NL] = {}, *logit = nullptr;
    float *dc[NL] = {}, *dp[NL] = {}, *de[NL] = {}, *dz[NL] = {}, *dy[NL] = {}, *dlogit = nullptr;
    float *stat = nullptr;     // per model [7 BN layers][2][128]: mean, invstd
    float *red = nullptr;      // per model [2][max(128, max_batch)]: BN backward sums / per-sample loss sums
    float *slab = nullptr;     // per model slab_floats
    size_t slab_floats = 0;
    float *d_loss = nullptr;                  // [K]
    unsigned long long *d_counts = nullptr;   // [K][3]
    uint8_t *d_stack = nullptr, *d_gt = nullptr;   // packed: the step's samples, model 0's first
    MStep *d_tab = nullptr;    // [K]
    MStep *h_tab = nullptr;    // pinned
    float *h_loss = nullptr;   // pinned [K]
    float *d_sample_loss = nullptr, *h_sample_loss = nullptr;   // evaluation: [K][max_batch] per-sample losses of a chunk (h_: pinned)
    unsigned long long *h_counts = nullptr;   // pinned [K][3]
    // the models' posts: device tables (written by covahip_train_set_post only) and their host mirror
    uint8_t *d_keep = nullptr, *d_post_flag = nullptr;   // [K][hw] 0 / 1, [K]
    float *d_post_thresh = nullptr;                      // [K]
    std::vector<uint8_t> post_keep, post_flag;           // [K][hw], [K] (a post without a keep map has a row of ones)
    std::vector<float> post_thresh;                      // [K]
    bool any_post = false;             // some model has a post: the passes launch the POST forms
    int math = COVAHIP_TRAIN_MATH_EXACT;   // covahip_train_set_math: which convolution kernels the passes launch
    PostTab post_tab() const { return PostTab{d_keep, d_post_thresh, d_post_flag}; }
};

namespace {

// makes the ctx's device current and takes the primary-op gate: the start of every entry point that touches the GPU
int enter(covahip_ctx *ctx) {
    COVAHIP_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    return covahip_primary_op(ctx);
}

template <class T>
int talloc(covahip_train *tr, T **p, size_t n) {
    void *q = nullptr;
    COVAHIP_CHECK_HIP(tr->ctx, hipMalloc(&q, n * sizeof(T) > 0 ? n * sizeof(T) : 16));
    tr->allocs.push_back(q);
    *p = (T *)q;
    return COVAHIP_OK;
}

void free_train(covahip_train *tr) {
    for (void *q : tr->allocs) hipFree(q);
    if (tr->h_tab) hipHostFree(tr->h_tab);
    if (tr->h_loss) hipHostFree(tr->h_loss);
    if (tr->h_sample_loss) hipHostFree(tr->h_sample_loss);
    if (tr->h_counts) hipHostFree(tr->h_counts);
    delete tr;
}

DropS make_drop(const covahip_train *tr, int site) {
    const double p = tr->cfg.dropout;
    DropS d;
    d.site = site;
    d.key = tr->h_tab[0].key[site];   // read by the kernels of a set of one only
    d.thr = (uint32_t)std::llround(p * 16777216.0);
    d.scale = (float)(1.0 / (1.0 - p));
    return d;
}

// launch the set or the solo instantiation of kernel k on Run r's stream, for r's models, under the ctx profile's scope `k`
#define KL(r, k, grid, block, ...)                                                     \
    do {                                                                               \
        ProfScope ps_((r).tr->ctx, #k);                                                \
        if ((r).tr->K > 1) k<true><<<grid, block, 0, (r).s>>>((r).md, __VA_ARGS__);    \
        else k<false><<<grid, block, 0, (r).s>>>((r).md, __VA_ARGS__);                 \
    } while (0)
// ... of a kernel with template arguments behind SET, under the scope `name`
#define KLT(r, name, k, targs, grid, block, ...)                                                          \
    do {                                                                                                  \
        ProfScope ps_((r).tr->ctx, name);                                                                 \
        if ((r).tr->K > 1) k<true, COVAHIP_UNPAREN targs><<<grid, block, 0, (r).s>>>((r).md, __VA_ARGS__); \
        else k<false, COVAHIP_UNPAREN targs><<<grid, block, 0, (r).s>>>((r).md, __VA_ARGS__);             \
    } while (0)
#define COVAHIP_UNPAREN(...) __VA_ARGS__

// One pass (a step, or an evaluation chunk) over every model with a non-zero batch in tr->h_tab (K > 1: already uploaded to
// d_tab); B = the largest batch.
struct Run {
    covahip_train *tr;
    hipStream_t s;
    Mdl md;
    int B;   // sizes the grids
    int rc = COVAHIP_OK;
    Run(covahip_train *t, int bmax)
        : tr(t), s(t->ctx->stream),
          md{t->K > 1 ? t->d_tab : nullptr, t->cfg.max_batch, (int64_t)t->slab_floats, t->h_tab[0].b, t->h_tab[0].lr_t}, B(bmax) {}
    bool ok() {
        if (rc) return false;
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
            tr->ctx->last_hip_error = std::string("train kernel launch: ") + hipGetErrorString(e);
            rc = COVAHIP_ERR_HIP;
        }
        return rc == COVAHIP_OK;
    }
    dim3 g1(int64_t n) const { return dim3(nblk(n), 1, tr->K); }
    float *stat(int layer) const { return tr->stat + layer * 256; }   // model 0's row of a BN layer
    // per-channel reduction of [b][C][S] (R_LOSS: [1][b][S]) + finalize; every model splits by its own batch in the kernels
    void reduce(int mode, int C, int64_t S, const float *x, const float *g, int Cg, const float *aux, const uint8_t *gt,
                int fmode, float *stat, int64_t stat_stride, float *g0, float *g1_, float *mov0, float *mov1) {
        const int loss = mode == R_LOSS;
        const int Cmax = loss ? B : C;
        const int64_t M = (int64_t)(loss ? 1 : B) * S;
        const int NP = red_slabs(M);
        if (loss && tr->any_post)
            KL(*this, k_reduce, (dim3(NP, Cmax, tr->K)), BLK, mode, Cmax, S, x, g, Cg, aux, gt, tr->slab, (M + NP - 1) / NP,
                                                           tr->post_tab());
        else
            KL(*this, k_reduce, (dim3(NP, Cmax, tr->K)), BLK, mode, Cmax, S, x, g, Cg, aux, gt, tr->slab, (M + NP - 1) / NP);
        KL(*this, k_finalize, (g1(Cmax)), BLK, fmode, loss, Cmax, S, tr->slab, stat, stat_stride, g0, g1_, mov0, mov1,
                                                  tr->cfg.bn_momentum, tr->cfg.bn_eps);
    }
};

// ---------------------------------------------------------------- the matrix-core launches (COVAHIP_TRAIN_MATH_MATRIX)
// The grid of each, as 64-bit extents for a largest batch B: the launches size their grids with these, and the planning pass of
// covahip_train_set_math (mm_plan) holds them against the launch limits at max_batch before the mode is taken.
struct Grid64 {
    int64_t x, y;
    bool fits() const { return x >= 1 && x <= INT32_MAX && y >= 1 && y <= 65535; }
    dim3 dim(int K) const { return dim3((unsigned)x, (unsigned)y, (unsigned)K); }
};
inline int conv3_mm_nacc(int Cout) { return Cout >= 64 ? 4 : Cout / 16; }   // 16 * NACC output channels per workgroup
Grid64 conv3_mm_grid(int64_t B, int64_t S, int Cout) { return Grid64{B * ((S + MM_PT - 1) / MM_PT), Cout / (16 * conv3_mm_nacc(Cout))}; }
Grid64 conv3_wgrad_mm_grid(int64_t P, int Ci, int Co) { return Grid64{(int64_t)((Ci + 15) / 16) * (Co / std::min(Co, 64)), wg_slabs(P)}; }
Grid64 convT_wgrad_mm_grid(int64_t P, int Ci, int Co) { return Grid64{(int64_t)(Co / 16) * (Ci / std::min(Ci, 64)), wg_slabs(P)}; }

// conv forward (dgrad = false: in = x, bias, out = relu) or data gradient (in = dA, out = dx) of a level with Ci -> Co channels
void launch_conv3_mm(Run &r, bool dgrad, const float *in, const float *k, const float *bias, float *out, int Ci, int Co, int H, int W) {
    const int Cout = dgrad ? Ci : Co;
    const dim3 g = conv3_mm_grid(r.B, (int64_t)TT * H * W, Cout).dim(r.tr->K);
#define MM_CASE(D, N)                                                                                                    \
    if (dgrad == D && conv3_mm_nacc(Cout) == N) {                                                                        \
        KLT(r, D ? "k_conv3_mm_dgrad" : "k_conv3_mm_fwd", k_conv3_mm, (D, N), g, BLK, in, k, bias, out, Ci, Co, H, W);  \
        return;                                                                                                          \
    }
    MM_CASE(false, 1) MM_CASE(false, 2) MM_CASE(false, 4) MM_CASE(true, 1) MM_CASE(true, 2) MM_CASE(true, 4)
#undef MM_CASE
    r.rc = COVAHIP_ERR_UNSUPPORTED;   // a channel count mm_plan does not admit
}
void launch_conv3_wgrad_mm(Run &r, const float *dA, const float *x, int Ci, int Co, int H, int W) {
    const int64_t P = (int64_t)r.B * TT * H * W;
    const Grid64 g = conv3_wgrad_mm_grid(P, Ci, Co);
    KL(r, k_conv3_wgrad_mm, (g.dim(r.tr->K)), BLK, dA, x, r.tr->slab, Ci, Co, H, W, (P + g.y - 1) / g.y);
}
void launch_convT_wgrad_mm(Run &r, const float *zd, const float *dy, int Ci, int Co, int Hi, int Wi, int Ho, int Wo, int cy, int cx) {
    const int64_t P = (int64_t)r.B * Hi * Wi;
    const Grid64 g = convT_wgrad_mm_grid(P, Ci, Co);
    if (Ci >= 64)
        KLT(r, "k_convT_wgrad_mm", k_convT_wgrad_mm, (4), (g.dim(r.tr->K)), BLK, zd, dy, r.tr->slab, Ci, Co, Hi, Wi, Ho, Wo, cy, cx, (P + g.y - 1) / g.y);
    else
        KLT(r, "k_convT_wgrad_mm", k_convT_wgrad_mm, (2), (g.dim(r.tr->K)), BLK, zd, dy, r.tr->slab, Ci, Co, Hi, Wi, Ho, Wo, cy, cx, (P + g.y - 1) / g.y);
}

// The planning pass of the matrix mode: every launch of a full step at max_batch, none made.  The kernels' own limits: channel
// counts in whole 16-channel tiles (Ci = 3 of level 0 is padded inside the kernels), a sample's block and a slab's position
// within a sample in 32 bits, the grids within the launch limits, the slab workspace as the plain kernels size it (the same
// slab counts, the same floats per slab).  None of it depends on the row width: the kernels tile positions, not rows.
// For the geometry covahip_train_create_set admits (16 <= h_mb, w_mb <= 1024, a level-0 elementwise grid within 2^31) every
// check passes: the widest grid below, level 0's B * ceil(4 hw / 64), is a quarter of that elementwise grid (B * 64 hw / 256).
int mm_plan(const covahip_train *tr) {
    const int64_t mb = tr->cfg.max_batch;
    if (tr->K > 65535) return COVAHIP_ERR_UNSUPPORTED;
    for (int i = 0; i < NL; i++) {
        const int Ci = ENC_C[i], Co = ENC_C[i + 1];
        const int64_t S = (int64_t)TT * tr->H[i] * tr->W[i];
        if (Co % 16 || (i > 0 && Ci % 16) || (Co > 64 && Co % 64) || S * std::max(Ci, Co) > INT32_MAX) return COVAHIP_ERR_UNSUPPORTED;
        if (!conv3_mm_grid(mb, S, Co).fits() || (i > 0 && !conv3_mm_grid(mb, S, Ci).fits())) return COVAHIP_ERR_UNSUPPORTED;
        const Grid64 g = conv3_wgrad_mm_grid(mb * S, Ci, Co);
        if (!g.fits() || (size_t)9 * Ci * Co * g.y > tr->slab_floats) return COVAHIP_ERR_UNSUPPORTED;
    }
    for (int j = 0; j < NL; j++) {
        const int Ci = DEC_CI[j], Co = DEC_CO[j];
        const int64_t Si = (int64_t)tr->H[NL - j] * tr->W[NL - j], So = (int64_t)tr->H[NL - 1 - j] * tr->W[NL - 1 - j];
        if (Co % 16 || Ci % 32 || (Ci > 64 && Ci % 64) || Si * Ci > INT32_MAX || So * Co > INT32_MAX) return COVAHIP_ERR_UNSUPPORTED;
        const Grid64 g = convT_wgrad_mm_grid(mb * Si, Ci, Co);
        if (!g.fits() || (size_t)16 * Ci * Co * g.y > tr->slab_floats) return COVAHIP_ERR_UNSUPPORTED;
    }
    return COVAHIP_OK;
}

BNTab bn_table(const covahip_train *tr) {
    BNTab bn;
    for (int i = 0; i < NL; i++) {
        bn.mean[i] = (int32_t)BN_LAYOUT.enc[i].mean;
        bn.var[i] = (int32_t)BN_LAYOUT.enc[i].var;
        bn.C[i] = ENC_C[i + 1];
    }
    for (int j = 0; j < NL - 1; j++) {
        bn.mean[NL + j] = (int32_t)BN_LAYOUT.dec[j].mean;
        bn.var[NL + j] = (int32_t)BN_LAYOUT.dec[j].var;
        bn.C[NL + j] = DEC_CO[j];
    }
    return bn;
}

// What differs between the forward of a training step and of an evaluation chunk.
struct Fwd {
    uint32_t bn_inf;        // BN layers that normalise with their moving statistics: the plan's, or all seven
    bool stat_to_grads;     // their moving values also go to the gradient slots (never in an evaluation: it leaves grads alone)
    DropS drop[N_SITES];    // the dropout sites; an evaluation's are the identity (see k_bn_stat)
};

// The forward of every model of the run, up to the logits and the per-sample loss sums [I][S] in tr->red.  Writes activations,
// stat, red and slab, and (batch-mode BN layers, stat_to_grads) moving statistics and gradient slots.
int forward(Run &r, const Fwd &f) {
    covahip_train *tr = r.tr;
    const int B = r.B;
    float *P = tr->params, *G = tr->grads;
    const int H0 = tr->H[0], W0 = tr->W[0];
    auto inf = [&](int layer) { return (f.bn_inf >> layer & 1u) != 0; };
    const bool mm = tr->math == COVAHIP_TRAIN_MATH_MATRIX;
    if (f.bn_inf)
        KL(r, k_bn_stat, (dim3(2 * NL - 1, 1, tr->K)), 128, P, f.stat_to_grads ? G : nullptr, tr->stat, bn_table(tr), f.bn_inf,
                                                          tr->cfg.bn_eps);
    KL(r, k_input, (r.g1((int64_t)B * 3 * TT * H0 * W0)), BLK, tr->d_stack, tr->x0, H0, W0);
    for (int i = 0; i < NL; i++) {
        const int Ci = ENC_C[i], Co = ENC_C[i + 1], H = tr->H[i], W = tr->W[i], Hp = tr->H[i + 1], Wp = tr->W[i + 1];
        const BnEncOff &o = BN_LAYOUT.enc[i];
        const float *xin = i ? tr->e[i - 1] : tr->x0;
        const int64_t S = (int64_t)TT * H * W;
        if (mm) launch_conv3_mm(r, false, xin, P + o.k, P + o.b, tr->c[i], Ci, Co, H, W);
        else KL(r, k_conv3_fwd, (r.g1(B * Co * S)), BLK, xin, P + o.k, P + o.b, tr->c[i], Ci, Co, H, W);
        if (!inf(i)) {
            r.reduce(R_SUM, Co, S, tr->c[i], nullptr, 0, nullptr, nullptr, F_MEAN, r.stat(i), STAT_STRIDE, nullptr, nullptr, nullptr, nullptr);
            r.reduce(R_SQDEV, Co, S, tr->c[i], nullptr, 0, r.stat(i), nullptr, F_VAR, r.stat(i), STAT_STRIDE, G + o.mean, G + o.var, P + o.mean,
                     P + o.var);
        }
        KL(r, k_bn_pool, (r.g1((int64_t)B * Co * TT * Hp * Wp)), BLK, tr->c[i], r.stat(i), P + o.gamma, P + o.beta, tr->p[i], tr->arg[i],
                                                                         Co, H, W, Hp, Wp);
        const int zj = NL - 1 - i;   // the decoder block whose input concat holds this level's t = 0 slice
        const int c_off = i == NL - 1 ? 0 : DEC_CO[zj - 1];
        KL(r, k_tmix_fwd, (r.g1((int64_t)B * Co * Hp * Wp)), BLK, tr->p[i], P + o.w1, P + o.w2, tr->e[i], tr->z[zj], DEC_CI[zj], c_off,
                                                                    Co, (int64_t)Hp * Wp, f.drop[2 * i], f.drop[2 * i + 1]);
        if (!r.ok()) return r.rc;
    }
    for (int j = 0; j < NL; j++) {
        const int Ci = DEC_CI[j], Co = DEC_CO[j];
        const int Hi = tr->H[NL - j], Wi = tr->W[NL - j], Ho = tr->H[NL - 1 - j], Wo = tr->W[NL - 1 - j];
        const BnDecOff &o = BN_LAYOUT.dec[j];
        const int64_t per = (int64_t)Ci * Hi * Wi, So = (int64_t)Ho * Wo;
        KL(r, k_drop_relu, (r.g1(B * per)), BLK, tr->z[j], tr->zd[j], per, f.drop[2 * NL + j]);
        KL(r, k_convT_fwd, (r.g1(B * Co * So)), BLK, tr->zd[j], P + o.k, P + o.b, tr->y[j], Ci, Co, Hi, Wi, Ho, Wo, tr->cy[j], tr->cx[j]);
        if (j < NL - 1) {
            if (!inf(NL + j)) {
                r.reduce(R_SUM, Co, So, tr->y[j], nullptr, 0, nullptr, nullptr, F_MEAN, r.stat(NL + j), STAT_STRIDE, nullptr, nullptr, nullptr,
                         nullptr);
                r.reduce(R_SQDEV, Co, So, tr->y[j], nullptr, 0, r.stat(NL + j), nullptr, F_VAR, r.stat(NL + j), STAT_STRIDE, G + o.mean,
                         G + o.var, P + o.mean, P + o.var);
            }
            KL(r, k_bn_apply, (r.g1(B * Co * So)), BLK, tr->y[j], r.stat(NL + j), P + o.gamma, P + o.beta, tr->z[j + 1], DEC_CI[j + 1], Co, So);
        }
        if (!r.ok()) return r.rc;
    }
    const int64_t hw = (int64_t)H0 * W0;
    KL(r, k_final_fwd, (r.g1(B * hw)), BLK, tr->y[NL - 1], P + BN_LAYOUT.fk, P + BN_LAYOUT.fb, tr->logit, hw);
    r.reduce(R_LOSS, B, hw, tr->logit, nullptr, 0, nullptr, tr->d_gt, F_SUM2, tr->red, red_stride(tr->cfg.max_batch), nullptr, nullptr,
             nullptr, nullptr);
    return r.rc;
}

// One step: the forward, the loss, the backward and Adam.  The launch schedule follows the training plan (include/covahip.h,
// "Fine-tuning"); the empty plan gives the full step.
int run_step(covahip_train *tr, int B) {
    Run r(tr, B);
    const int K = tr->K;
    float *P = tr->params, *G = tr->grads;
    const float sm = tr->cfg.smooth;
    const int64_t RS = red_stride(tr->cfg.max_batch), hw = (int64_t)tr->H[0] * tr->W[0];
    // The plan.  enc_fz / dec_fz: the group is frozen; inf(layer): the BN layer normalises with its moving statistics.
    // enc_live(i): something of encoder levels 0..i is trained, so the backward must reach level i; dec_live(j) likewise for
    // decoder blocks 0..j.  need_dz[j]: block j's input gradient has a reader (the BN of block j - 1, or the encoder through
    // the skip channels); need_dy[j]: block j's output gradient has one (its own weights, or need_dz[j]).
    const uint32_t fz = tr->frozen, bninf = tr->bn_inf;
    const bool mm = tr->math == COVAHIP_TRAIN_MATH_MATRIX;
    auto enc_fz = [&](int i) { return (fz >> i & 1u) != 0; };
    auto dec_fz = [&](int j) { return (fz >> (NL + j) & 1u) != 0; };
    auto inf = [&](int layer) { return (bninf >> layer & 1u) != 0; };
    auto enc_live = [&](int i) { return (~fz & ((2u << i) - 1u)) != 0; };
    auto dec_live = [&](int j) { return (~fz >> NL & ((2u << j) - 1u)) != 0; };
    bool need_dz[NL], need_dy[NL];
    for (int j = 0; j < NL; j++) {
        need_dz[j] = enc_live(NL - 1) || (j > 0 && dec_live(j - 1));
        need_dy[j] = !dec_fz(j) || need_dz[j];
    }
    Fwd f{bninf, true, {}};
    for (int site = 0; site < N_SITES; site++) f.drop[site] = make_drop(tr, site);
    if (hipMemsetAsync(tr->d_counts, 0, (size_t)K * 3 * sizeof(unsigned long long), r.s) != hipSuccess) return COVAHIP_ERR_HIP;

    if (int rc = forward(r, f)) return rc;
    KL(r, k_loss, (dim3(1, 1, K)), 1, tr->red, sm, tr->d_loss);

    // ---------------------------------------------------------------- backward
    if (tr->any_post)
        KL(r, k_final_bwd, (r.g1(B * hw)), BLK, tr->logit, tr->d_gt, tr->red, P + BN_LAYOUT.fk, tr->dlogit, tr->dy[NL - 1], hw, sm,
                                                     tr->d_counts, tr->post_tab());
    else
        KL(r, k_final_bwd, (r.g1(B * hw)), BLK, tr->logit, tr->d_gt, tr->red, P + BN_LAYOUT.fk, tr->dlogit, tr->dy[NL - 1], hw, sm,
                                                tr->d_counts);
    if (!dec_fz(NL - 1)) {
        r.reduce(R_FINALW, 16, hw, tr->y[NL - 1], tr->dlogit, 1, nullptr, nullptr, F_SUM, nullptr, 0, G + BN_LAYOUT.fk, nullptr, nullptr, nullptr);
        r.reduce(R_SUM, 1, hw, tr->dlogit, nullptr, 0, nullptr, nullptr, F_SUM, nullptr, 0, G + BN_LAYOUT.fb, nullptr, nullptr, nullptr);
    }
    if (!r.ok()) return r.rc;
    for (int j = NL - 1; j >= 0 && need_dy[j]; j--) {
        const int Ci = DEC_CI[j], Co = DEC_CO[j];
        const int Hi = tr->H[NL - j], Wi = tr->W[NL - j], Ho = tr->H[NL - 1 - j], Wo = tr->W[NL - 1 - j];
        const BnDecOff &o = BN_LAYOUT.dec[j];
        const int64_t So = (int64_t)Ho * Wo;
        if (j < NL - 1) {   // BN of this block: its output gradient is channel range [0, Co) of the next block's dz
            // the sums are gamma's and beta's gradients in either mode, and the batch-mean terms of a batch-mode layer
            if (!dec_fz(j))
                r.reduce(R_BNBWD, Co, So, tr->y[j], tr->dz[j + 1], DEC_CI[j + 1], r.stat(NL + j), nullptr, F_SUM2, tr->red, RS, G + o.gamma,
                         G + o.beta, nullptr, nullptr);
            if (inf(NL + j))
                KL(r, k_bn_bwd_inf, (r.g1(B * Co * So)), BLK, tr->dz[j + 1], DEC_CI[j + 1], tr->y[j], r.stat(NL + j), P + o.gamma,
                                                               tr->dy[j], Co, So, 0);
            else
                KL(r, k_bn_bwd, (r.g1(B * Co * So)), BLK, tr->dz[j + 1], DEC_CI[j + 1], tr->y[j], r.stat(NL + j), tr->red, P + o.gamma,
                                                           tr->dy[j], Co, So, 0);
        }
        const int64_t per = (int64_t)Hi * Wi, Pp = (int64_t)B * per;
        if (!dec_fz(j)) {
            r.reduce(R_SUM, Co, So, tr->dy[j], nullptr, 0, nullptr, nullptr, F_SUM, nullptr, 0, G + o.b, nullptr, nullptr, nullptr);
            const int ns = wg_slabs(Pp);
            const int nw = 16 * Co * Ci;
            if (mm) launch_convT_wgrad_mm(r, tr->zd[j], tr->dy[j], Ci, Co, Hi, Wi, Ho, Wo, tr->cy[j], tr->cx[j]);
            else
                KL(r, k_convT_wgrad, (dim3(nblk(nw), ns, K)), BLK, tr->zd[j], tr->dy[j], tr->slab, Ci, Co, Hi, Wi, Ho, Wo, tr->cy[j],
                                                                   tr->cx[j], (Pp + ns - 1) / ns);
            KL(r, k_sum_slabs, (r.g1(nw)), BLK, tr->slab, per, 0, nw, G + o.k);
        }
        if (need_dz[j])
            KL(r, k_convT_dgrad, (r.g1(Pp * Ci)), BLK, tr->dy[j], P + o.k, tr->z[j], tr->dz[j], Ci, Co, Hi, Wi, Ho, Wo, tr->cy[j],
                                                       tr->cx[j], f.drop[2 * NL + j]);
        if (!r.ok()) return r.rc;
    }
    for (int i = NL - 1; i >= 0 && enc_live(i); i--) {
        const int Ci = ENC_C[i], Co = ENC_C[i + 1], H = tr->H[i], W = tr->W[i], Hp = tr->H[i + 1], Wp = tr->W[i + 1];
        const BnEncOff &o = BN_LAYOUT.enc[i];
        const int zj = NL - 1 - i;
        const int c_off = i == NL - 1 ? 0 : DEC_CO[zj - 1];
        const int64_t tper = (int64_t)Co * Hp * Wp;
        const int nb = tmix_blocks(B * tper);
        KL(r, k_tmix_bwd, (dim3(nb, 1, K)), BLK, tr->p[i], P + o.w1, P + o.w2, i < NL - 1 ? tr->de[i] : nullptr, tr->dz[zj],
                                                  DEC_CI[zj], c_off, tr->dp[i], tr->slab, Co, (int64_t)Hp * Wp, (B * tper + nb - 1) / nb, f.drop[2 * i],
                                                  f.drop[2 * i + 1]);
        if (!enc_fz(i)) KL(r, k_sum_slabs, (dim3(1, 1, K)), BLK, tr->slab, tper, 1, 32, G + o.w1);
        const int64_t S = (int64_t)TT * H * W;
        KL(r, k_pool_bwd, (r.g1(B * Co * S)), BLK, tr->dp[i], tr->arg[i], tr->dc[i], Co, H, W, Hp, Wp);
        if (!enc_fz(i))
            r.reduce(R_BNBWD, Co, S, tr->c[i], tr->dc[i], Co, r.stat(i), nullptr, F_SUM2, tr->red, RS, G + o.gamma, G + o.beta, nullptr, nullptr);
        if (inf(i))
            KL(r, k_bn_bwd_inf, (r.g1(B * Co * S)), BLK, tr->dc[i], Co, tr->c[i], r.stat(i), P + o.gamma, tr->dc[i], Co, S, 1);
        else
            KL(r, k_bn_bwd, (r.g1(B * Co * S)), BLK, tr->dc[i], Co, tr->c[i], r.stat(i), tr->red, P + o.gamma, tr->dc[i], Co, S, 1);
        if (!enc_fz(i)) {
            r.reduce(R_SUM, Co, S, tr->dc[i], nullptr, 0, nullptr, nullptr, F_SUM, nullptr, 0, G + o.b, nullptr, nullptr, nullptr);
            const float *xin = i ? tr->e[i - 1] : tr->x0;
            const int64_t Pp = (int64_t)B * S;
            const int ns = wg_slabs(Pp);
            const int nw = 9 * Ci * Co;
            if (mm) launch_conv3_wgrad_mm(r, tr->dc[i], xin, Ci, Co, H, W);
            else KL(r, k_conv3_wgrad, (dim3(nblk(nw), ns, K)), BLK, tr->dc[i], xin, tr->slab, Ci, Co, H, W, (Pp + ns - 1) / ns);
            KL(r, k_sum_slabs, (r.g1(nw)), BLK, tr->slab, S, 0, nw, G + o.k);
        }
        if (i > 0 && enc_live(i - 1)) {
            if (mm) launch_conv3_mm(r, true, tr->dc[i], P + o.k, nullptr, tr->de[i - 1], Ci, Co, H, W);
            else KL(r, k_conv3_dgrad, (r.g1((int64_t)B * Ci * S)), BLK, tr->dc[i], P + o.k, tr->de[i - 1], Ci, Co, H, W);
        }
        if (!r.ok()) return r.rc;
    }

    // ---------------------------------------------------------------- Adam (lr_t per model in the table)
    if (fz)
        KL(r, k_adam_plan, (r.g1((int64_t)N_PARAMS)), BLK, P, G, tr->adam_m, tr->adam_v, tr->trainable, (int)N_PARAMS, tr->cfg.beta1,
                                                            tr->cfg.beta2, tr->cfg.eps);
    else
        KL(r, k_adam, (r.g1((int64_t)N_PARAMS)), BLK, P, G, tr->adam_m, tr->adam_v, tr->trainable, (int)N_PARAMS, tr->cfg.beta1,
                                                       tr->cfg.beta2, tr->cfg.eps);
    r.ok();
    return r.rc;
}

// The inference-mode forward of one chunk, then the per-sample losses into d_sample_loss and TP / FP / FN added to d_counts.
// Writes activations, stat, red and slab only, all of which a training step rewrites before it reads them; never grads,
// parameters or Adam moments.
int run_eval(covahip_train *tr, int B) {
    Run r(tr, B);
    Fwd f{0x7Fu, false, {}};
    for (DropS &d : f.drop) d = DropS{0, 0u, 1.f, 0};   // the identity (see k_bn_stat)
    if (int rc = forward(r, f)) return rc;
    const int64_t hw = (int64_t)tr->H[0] * tr->W[0];
    if (tr->any_post)
        KL(r, k_eval_tail, (r.g1(B * hw)), BLK, tr->logit, tr->d_gt, tr->red, hw, tr->cfg.smooth, tr->d_counts,
                                                     tr->d_sample_loss, tr->post_tab());
    else
        KL(r, k_eval_tail, (r.g1(B * hw)), BLK, tr->logit, tr->d_gt, tr->red, hw, tr->cfg.smooth, tr->d_counts, tr->d_sample_loss);
    r.ok();
    return r.rc;
}

// Adam's mask under a plan: 1 trained, 0 the BN moving statistics (never trained), 2 the tensors of a frozen group.
std::vector<uint8_t> plan_mask(const covahip_train *tr, uint32_t frozen) {
    std::vector<uint8_t> m(N_PARAMS, 1);
    for (int i = 0; i < NL; i++) {
        const BnEncOff &o = BN_LAYOUT.enc[i];
        if (frozen >> i & 1u) std::fill(m.begin() + o.k, m.begin() + o.w2 + TT * TT, 2);
        std::fill(m.begin() + o.mean, m.begin() + o.w1, 0);
    }
    for (int j = 0; j < NL; j++) {
        const BnDecOff &o = BN_LAYOUT.dec[j];
        const size_t end = j < NL - 1 ? BN_LAYOUT.dec[j + 1].k : N_PARAMS;   // block 3's group ends with final.kernel / final.bias
        if (frozen >> (NL + j) & 1u) std::fill(m.begin() + o.k, m.begin() + end, 2);
        if (j < NL - 1) std::fill(m.begin() + o.mean, m.begin() + o.var + DEC_CO[j], 0);
    }
    return m;
}

bool finite_pos(float v) { return std::isfinite(v) && v > 0.f; }

int validate_cfg(const covahip_train_cfg *c) {
    if (c->h_mb < 16 || c->w_mb < 16 || c->h_mb > 1024 || c->w_mb > 1024 || c->max_batch <= 0) return COVAHIP_ERR_INVALID_ARG;
    if (!std::isfinite(c->lr) || c->lr < 0.f) return COVAHIP_ERR_INVALID_ARG;
    if (!(c->beta1 >= 0.f && c->beta1 < 1.f) || !(c->beta2 >= 0.f && c->beta2 < 1.f) || !finite_pos(c->eps)) return COVAHIP_ERR_INVALID_ARG;
    if (!(c->bn_momentum >= 0.f && c->bn_momentum <= 1.f) || !finite_pos(c->bn_eps)) return COVAHIP_ERR_INVALID_ARG;
    if (!(c->dropout >= 0.f && c->dropout < 1.f) || !finite_pos(c->smooth)) return COVAHIP_ERR_INVALID_ARG;
    return COVAHIP_OK;
}

int create_body(covahip_train *tr, const void *const *blobs) {
    covahip_ctx *ctx = tr->ctx;
    const covahip_train_cfg &cf = tr->cfg;
    const int K = tr->K;
    const int64_t B = (int64_t)K * cf.max_batch;   // samples all models hold together
    tr->H[0] = cf.h_mb;
    tr->W[0] = cf.w_mb;
    for (int i = 0; i < NL; i++) {
        tr->H[i + 1] = (tr->H[i] + 1) / 2;
        tr->W[i + 1] = (tr->W[i] + 1) / 2;
    }
    for (int j = 0; j < NL; j++) {   // convT output 2 * in + 2, surplus cropped ceil(p / 2) top / left (decoder.py)
        const int ph = 2 * tr->H[NL - j] + 2 - tr->H[NL - 1 - j], pw = 2 * tr->W[NL - j] + 2 - tr->W[NL - 1 - j];
        if (ph < 0 || pw < 0) return COVAHIP_ERR_UNSUPPORTED;
        tr->cy[j] = ph / 2 + ph % 2;
        tr->cx[j] = pw / 2 + pw % 2;
    }
    const int64_t hw0 = (int64_t)tr->H[0] * tr->W[0];
    // A set's totals must stay inside what is 32-bit on the way: the samples of all models (the `first` column of the step
    // table, the packed input's sample index), the x extent of the largest elementwise grid of one model (level 0's conv
    // output) and the y extent of the per-sample loss reduction (one row per sample of a model).
    if (B > INT32_MAX / 2 || ((int64_t)cf.max_batch * 16 * TT * hw0 + BLK - 1) / BLK > INT32_MAX || (K > 1 && cf.max_batch > 65535))
        return COVAHIP_ERR_UNSUPPORTED;
    tr->step.assign(K, 0);
    tr->last_counts.assign((size_t)K * 3, 0);
    int rc;
#define TA(p, n) if ((rc = talloc(tr, &(p), (size_t)(n)))) return rc
    TA(tr->params, K * N_PARAMS);
    TA(tr->grads, K * N_PARAMS);
    TA(tr->adam_m, K * N_PARAMS);
    TA(tr->adam_v, K * N_PARAMS);
    TA(tr->trainable, N_PARAMS);
    TA(tr->x0, B * 3 * TT * hw0);
    const int64_t mb = cf.max_batch;   // the slab workspace is per model: sized for one model's largest batch
    size_t slab = 0;
    for (int i = 0; i < NL; i++) {
        const int64_t Co = ENC_C[i + 1], S = (int64_t)TT * tr->H[i] * tr->W[i], Sp = (int64_t)TT * tr->H[i + 1] * tr->W[i + 1];
        TA(tr->c[i], B * Co * S);
        TA(tr->dc[i], B * Co * S);
        TA(tr->p[i], B * Co * Sp);
        TA(tr->arg[i], B * Co * Sp);
        TA(tr->e[i], B * Co * Sp);
        TA(tr->dp[i], B * Co * Sp);
        TA(tr->de[i], B * Co * Sp);
        slab = std::max(slab, (size_t)Co * red_slabs(mb * S) * 2);
        slab = std::max(slab, (size_t)9 * ENC_C[i] * Co * wg_slabs(mb * S));
        slab = std::max(slab, (size_t)TMIX_BLOCKS_MAX * 32);
    }
    for (int j = 0; j < NL; j++) {
        const int64_t Ci = DEC_CI[j], Co = DEC_CO[j];
        const int64_t Si = (int64_t)tr->H[NL - j] * tr->W[NL - j], So = (int64_t)tr->H[NL - 1 - j] * tr->W[NL - 1 - j];
        TA(tr->z[j], B * Ci * Si);
        TA(tr->zd[j], B * Ci * Si);
        TA(tr->dz[j], B * Ci * Si);
        TA(tr->y[j], B * Co * So);
        TA(tr->dy[j], B * Co * So);
        slab = std::max(slab, (size_t)Co * red_slabs(mb * So) * 2);
        slab = std::max(slab, (size_t)16 * Ci * Co * wg_slabs(mb * Si));
    }
    slab = std::max(slab, (size_t)mb * red_slabs(hw0) * 2);
    TA(tr->logit, B * hw0);
    TA(tr->dlogit, B * hw0);
    TA(tr->stat, (size_t)K * STAT_STRIDE);
    TA(tr->red, (size_t)K * red_stride(cf.max_batch));
    TA(tr->slab, (size_t)K * slab);
    tr->slab_floats = slab;
    TA(tr->d_loss, K);
    TA(tr->d_counts, (size_t)K * 3);
    TA(tr->d_sample_loss, B);
    TA(tr->d_stack, B * TT * hw0 * 4);
    TA(tr->d_gt, B * hw0);
    TA(tr->d_tab, K);
    TA(tr->d_keep, (size_t)K * hw0);
    TA(tr->d_post_flag, K);
    TA(tr->d_post_thresh, K);
#undef TA
    tr->post_keep.assign((size_t)K * hw0, 1);
    tr->post_flag.assign(K, 0);
    tr->post_thresh.assign(K, 0.f);
    COVAHIP_CHECK_HIP(ctx, hipHostMalloc((void **)&tr->h_tab, (size_t)K * sizeof(MStep), hipHostMallocDefault));
    COVAHIP_CHECK_HIP(ctx, hipHostMalloc((void **)&tr->h_loss, (size_t)K * sizeof(float), hipHostMallocDefault));
    COVAHIP_CHECK_HIP(ctx, hipHostMalloc((void **)&tr->h_sample_loss, (size_t)B * sizeof(float), hipHostMallocDefault));
    COVAHIP_CHECK_HIP(ctx, hipHostMalloc((void **)&tr->h_counts, (size_t)K * 3 * sizeof(unsigned long long), hipHostMallocDefault));
    const std::vector<uint8_t> tmask = plan_mask(tr, 0);
    const hipStream_t s = ctx->stream;
    for (int k = 0; k < K; k++)
        COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(tr->params + (size_t)k * N_PARAMS, static_cast<const uint8_t *>(blobs[k]) + BN_HEADER_BYTES,
                                              N_PARAMS * sizeof(float), hipMemcpyHostToDevice, s));
    COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(tr->trainable, tmask.data(), N_PARAMS, hipMemcpyHostToDevice, s));
    COVAHIP_CHECK_HIP(ctx, hipMemsetAsync(tr->grads, 0, (size_t)K * N_PARAMS * sizeof(float), s));
    COVAHIP_CHECK_HIP(ctx, hipMemsetAsync(tr->adam_m, 0, (size_t)K * N_PARAMS * sizeof(float), s));
    COVAHIP_CHECK_HIP(ctx, hipMemsetAsync(tr->adam_v, 0, (size_t)K * N_PARAMS * sizeof(float), s));
    COVAHIP_CHECK_HIP(ctx, hipMemsetAsync(tr->d_keep, 1, (size_t)K * hw0, s));
    COVAHIP_CHECK_HIP(ctx, hipMemsetAsync(tr->d_post_flag, 0, (size_t)K, s));
    COVAHIP_CHECK_HIP(ctx, hipMemsetAsync(tr->d_post_thresh, 0, (size_t)K * sizeof(float), s));
    COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));   // tmask leaves scope
    return COVAHIP_OK;
}

// The per-model table of one pass: row k = model k's batch b[k] and its first sample in the packing; for a step (lrs not
// null) also its Adam step size at its own t and its dropout keys, zeros otherwise.  Uploaded where the kernels read it (K > 1).
int set_tab(covahip_train *tr, const int32_t *b, const float *lrs) {
    int first = 0;
    for (int k = 0; k < tr->K; k++) {
        MStep &ms = tr->h_tab[k];
        ms = MStep{};
        ms.b = b[k];
        ms.first = first;
        first += b[k];
        if (!lrs) continue;
        const double t = (double)(tr->step[k] + 1);
        ms.lr_t = (float)(lrs[k] * std::sqrt(1.0 - std::pow((double)tr->cfg.beta2, t)) / (1.0 - std::pow((double)tr->cfg.beta1, t)));
        for (int site = 0; site < N_SITES; site++) ms.key[site] = drop_key(tr->seed[k], (uint64_t)tr->step[k], site);
    }
    if (tr->K > 1)
        COVAHIP_CHECK_HIP(tr->ctx, hipMemcpyAsync(tr->d_tab, tr->h_tab, (size_t)tr->K * sizeof(MStep), hipMemcpyHostToDevice, tr->ctx->stream));
    return COVAHIP_OK;
}

// The samples of a pass written into the trainer's staging by the data set's gather launch instead of a copy: `first`[k] is
// model k's first entry of `samples`, of which the pass takes h_tab[k].b to the model's place in the packing.
int fill_from_data(covahip_train *tr, covahip_train_data *d, const covahip_train_sample *samples, const int64_t *first) {
    int total = 0;
    for (int k = 0; k < tr->K; k++) total += tr->h_tab[k].b;
    covahip_train_sample *tab = nullptr;
    if (int rc = covahip_train_data_table(d, total, &tab)) return rc;
    for (int k = 0; k < tr->K; k++) {
        const MStep &ms = tr->h_tab[k];
        if (ms.b) std::memcpy(tab + ms.first, samples + first[k], (size_t)ms.b * sizeof(covahip_train_sample));
    }
    return covahip_train_data_launch(d, total, tr->d_stack, tr->d_gt);
}

// The step of a set: batches / lrs / losses have K entries, the samples are packed in model order.  With a data set `d` they are
// `samples` of it (a host table, checked here before anything is launched) and stack / gt / mem_kind are unused.
int step_body(covahip_train *tr, const uint8_t *stack, const uint8_t *gt, const int *batches, const float *lrs, float *losses,
              int mem_kind, covahip_train_data *d = nullptr, const covahip_train_sample *samples = nullptr) {
    const int K = tr->K;
    int64_t total = 0;
    int bmax = 0;
    for (int k = 0; k < K; k++) {
        if (batches[k] < 0 || batches[k] > tr->cfg.max_batch || !std::isfinite(lrs[k]) || lrs[k] < 0.f) return COVAHIP_ERR_INVALID_ARG;
        total += batches[k];
        bmax = std::max(bmax, batches[k]);
    }
    if (total == 0) return COVAHIP_ERR_INVALID_ARG;
    if (d) {
        if (int rc = covahip_train_data_check(d, tr->ctx, tr->H[0], tr->W[0], samples, total)) return rc;
    } else if (mem_kind != COVAHIP_MEM_HOST && mem_kind != COVAHIP_MEM_DEVICE) {
        return COVAHIP_ERR_INVALID_ARG;
    }
    covahip_ctx *ctx = tr->ctx;
    if (int rc = enter(ctx)) return rc;
    if (int rc = set_tab(tr, batches, lrs)) return rc;
    if (d) {
        std::vector<int64_t> first(K);
        for (int k = 0; k < K; k++) first[k] = tr->h_tab[k].first;
        if (int rc = fill_from_data(tr, d, samples, first.data())) return rc;
    } else {
        const size_t hw = (size_t)tr->H[0] * tr->W[0];
        const hipMemcpyKind kind = mem_kind == COVAHIP_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
        COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(tr->d_stack, stack, (size_t)total * TT * hw * 4, kind, ctx->stream));
        COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(tr->d_gt, gt, (size_t)total * hw, kind, ctx->stream));
    }
    if (int rc = run_step(tr, bmax)) return rc;
    COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(tr->h_loss, tr->d_loss, (size_t)K * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(tr->h_counts, tr->d_counts, (size_t)K * 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                                          ctx->stream));
    COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < K; k++) {
        if (!batches[k]) {   // skipped: its loss slot was not written, its metrics and step stay
            losses[k] = 0.f;
            continue;
        }
        losses[k] = tr->h_loss[k];
        for (int q = 0; q < 3; q++) tr->last_counts[(size_t)k * 3 + q] = (long long)tr->h_counts[(size_t)k * 3 + q];
        tr->step[k]++;
    }
    return COVAHIP_OK;
}

// Evaluation of counts[k] samples of model k (packed in model order), in chunks of max_batch per model.  With a data set `d` the
// samples are `samples` of it (step_body); mem_kind then applies to sample_loss and logits alone.
int eval_body(covahip_train *tr, const uint8_t *stack, const uint8_t *gt, const int32_t *counts, float *sample_loss, float *logits,
              covahip_train_eval_result *out, int mem_kind, covahip_train_data *d = nullptr,
              const covahip_train_sample *samples = nullptr) {
    const int K = tr->K, mb = tr->cfg.max_batch;
    std::vector<int64_t> base(K);
    int64_t total = 0;
    int32_t cmax = 0;
    for (int k = 0; k < K; k++) {
        if (counts[k] < 0) return COVAHIP_ERR_INVALID_ARG;
        base[k] = total;
        total += counts[k];
        cmax = std::max(cmax, counts[k]);
    }
    if (total == 0 || total > INT32_MAX) return COVAHIP_ERR_INVALID_ARG;
    if (mem_kind != COVAHIP_MEM_HOST && mem_kind != COVAHIP_MEM_DEVICE) return COVAHIP_ERR_INVALID_ARG;
    if (d)
        if (int rc = covahip_train_data_check(d, tr->ctx, tr->H[0], tr->W[0], samples, total)) return rc;
    covahip_ctx *ctx = tr->ctx;
    if (int rc = enter(ctx)) return rc;
    const hipStream_t s = ctx->stream;
    const size_t hw = (size_t)tr->H[0] * tr->W[0], stack_b = TT * hw * 4;
    const bool host = mem_kind == COVAHIP_MEM_HOST;
    const hipMemcpyKind in_kind = host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    const hipMemcpyKind out_kind = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    const int nchunks = (cmax + mb - 1) / mb;
    std::vector<double> loss_sum(K, 0.0);
    std::vector<int32_t> cb(K);   // the chunk's batch per model
    COVAHIP_CHECK_HIP(ctx, hipMemsetAsync(tr->d_counts, 0, (size_t)K * 3 * sizeof(unsigned long long), s));
    for (int c = 0; c < nchunks; c++) {
        for (int k = 0; k < K; k++) cb[k] = (int32_t)std::min<int64_t>(mb, std::max<int64_t>(0, (int64_t)counts[k] - (int64_t)c * mb));
        if (int rc = set_tab(tr, cb.data(), nullptr)) return rc;   // keys and lr_t: unused
        if (d) {
            std::vector<int64_t> first(K);
            for (int k = 0; k < K; k++) first[k] = base[k] + (int64_t)c * mb;
            if (int rc = fill_from_data(tr, d, samples, first.data())) return rc;
        } else if (nchunks == 1) {   // the caller's packing is the chunk's
            COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(tr->d_stack, stack, (size_t)total * stack_b, in_kind, s));
            COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(tr->d_gt, gt, (size_t)total * hw, in_kind, s));
        } else {
            for (int k = 0; k < K; k++) {
                const MStep &ms = tr->h_tab[k];
                if (!ms.b) continue;
                const size_t src = (size_t)(base[k] + (int64_t)c * mb);
                COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(tr->d_stack + (size_t)ms.first * stack_b, stack + src * stack_b, (size_t)ms.b * stack_b,
                                                      in_kind, s));
                COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(tr->d_gt + (size_t)ms.first * hw, gt + src * hw, (size_t)ms.b * hw, in_kind, s));
            }
        }
        if (int rc = run_eval(tr, *std::max_element(cb.begin(), cb.end()))) return rc;
        COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(tr->h_sample_loss, tr->d_sample_loss, (size_t)K * mb * sizeof(float), hipMemcpyDeviceToHost, s));
        for (int k = 0; k < K; k++) {
            const int b = tr->h_tab[k].b;
            if (!b) continue;
            const size_t dst = (size_t)(base[k] + (int64_t)c * mb);
            if (logits)
                COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(logits + dst * hw, tr->logit + (size_t)k * mb * hw, (size_t)b * hw * sizeof(float),
                                                      out_kind, s));
            if (sample_loss && !host)
                COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(sample_loss + dst, tr->d_sample_loss + (size_t)k * mb, (size_t)b * sizeof(float),
                                                      out_kind, s));
        }
        COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));   // h_tab and h_sample_loss are reused by the next chunk
        for (int k = 0; k < K; k++) {
            const int b = tr->h_tab[k].b;
            const float *sl = tr->h_sample_loss + (size_t)k * mb;
            for (int i = 0; i < b; i++) loss_sum[k] += (double)sl[i];
            if (b && sample_loss && host) std::memcpy(sample_loss + base[k] + (int64_t)c * mb, sl, (size_t)b * sizeof(float));
        }
    }
    COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(tr->h_counts, tr->d_counts, (size_t)K * 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(s));
    for (int k = 0; k < K; k++) {
        covahip_train_eval_result &o = out[k];
        o = covahip_train_eval_result{};
        if (!counts[k]) continue;
        o.loss = loss_sum[k] / (double)counts[k];
        o.tp = (int64_t)tr->h_counts[(size_t)k * 3];
        o.fp = (int64_t)tr->h_counts[(size_t)k * 3 + 1];
        o.fn = (int64_t)tr->h_counts[(size_t)k * 3 + 2];
        o.samples = counts[k];
    }
    return COVAHIP_OK;
}

// ------------------------------------------------------------------------------------------------ trainer state blob
constexpr uint32_t S_MAGIC = 0x53485643;  // "CVHS"
constexpr uint32_t S_VERSION = 1;
constexpr size_t S_HEADER = 64, S_MODEL = 16 + 3 * N_PARAMS * sizeof(float);
size_t state_bytes(size_t n_models) { return S_HEADER + n_models * S_MODEL + 4; }

template <class T>
void put(uint8_t *p, size_t off, T v) { std::memcpy(p + off, &v, sizeof v); }
template <class T>
T get(const uint8_t *p, size_t off) {
    T v;
    std::memcpy(&v, p + off, sizeof v);
    return v;
}

}  // namespace

extern "C" {

void covahip_train_default_cfg(covahip_train_cfg *cfg) {
    if (!cfg) return;
    cfg->h_mb = 45;
    cfg->w_mb = 80;
    cfg->max_batch = 4;
    cfg->lr = 1e-3f;
    cfg->beta1 = 0.9f;
    cfg->beta2 = 0.999f;
    cfg->eps = 1e-7f;
    cfg->bn_momentum = 0.99f;
    cfg->bn_eps = 1e-3f;
    cfg->dropout = 0.2f;
    cfg->smooth = 100.f;
    cfg->seed = 0;
}

int covahip_train_create_set(covahip_ctx *ctx, const covahip_train_cfg *cfg, int n_models, const void *const *weights,
                             const size_t *weights_bytes, const uint64_t *seeds, covahip_train **out) {
    if (out) *out = nullptr;
    if (!ctx || !cfg || !weights || !weights_bytes || !out || n_models < 1 || n_models > COVAHIP_MAX_MODELS)
        return COVAHIP_ERR_INVALID_ARG;
    for (int k = 0; k < n_models; k++)
        if (!weights[k]) return COVAHIP_ERR_INVALID_ARG;
    if (int rc = validate_cfg(cfg)) return rc;
    for (int k = 0; k < n_models; k++)
        if (!bn_check_blob(weights[k], weights_bytes[k])) return COVAHIP_ERR_BAD_WEIGHTS;
    if (int rc = enter(ctx)) return rc;
    covahip_train *tr = new covahip_train();
    tr->ctx = ctx;
    tr->cfg = *cfg;
    tr->K = n_models;
    tr->seed.resize(n_models);
    for (int k = 0; k < n_models; k++) tr->seed[k] = seeds ? seeds[k] : cfg->seed;
    const int rc = create_body(tr, weights);
    if (rc) {
        hipStreamSynchronize(ctx->stream);
        (void)hipGetLastError();
        free_train(tr);
        return rc;
    }
    *out = tr;
    return COVAHIP_OK;
}

int covahip_train_create(covahip_ctx *ctx, const covahip_train_cfg *cfg, const void *cvhw, size_t cvhw_bytes, covahip_train **out) {
    if (out) *out = nullptr;
    if (!ctx || !cfg || !cvhw || !out) return COVAHIP_ERR_INVALID_ARG;
    return covahip_train_create_set(ctx, cfg, 1, &cvhw, &cvhw_bytes, nullptr, out);
}

int covahip_train_num_models(covahip_train *tr, int *n_models) {
    if (!tr || !n_models) return COVAHIP_ERR_INVALID_ARG;
    *n_models = tr->K;
    return COVAHIP_OK;
}

int covahip_train_step_set(covahip_train *tr, const uint8_t *stack, const uint8_t *gt, const int32_t *batches, const float *lrs,
                           float *losses, int mem_kind) {
    if (!tr || !stack || !gt || !batches || !lrs || !losses) return COVAHIP_ERR_INVALID_ARG;
    return step_body(tr, stack, gt, batches, lrs, losses, mem_kind);
}

int covahip_train_step(covahip_train *tr, const uint8_t *stack, const uint8_t *gt, int batch, float lr, float *loss, int mem_kind) {
    if (!tr || !stack || !gt || !loss || batch <= 0 || tr->K != 1) return COVAHIP_ERR_INVALID_ARG;
    return step_body(tr, stack, gt, &batch, &lr, loss, mem_kind);
}

int covahip_train_step_set_data(covahip_train *tr, covahip_train_data *d, const covahip_train_sample *samples, const int32_t *batches,
                                const float *lrs, float *losses) {
    if (!tr || !d || !samples || !batches || !lrs || !losses) return COVAHIP_ERR_INVALID_ARG;
    return step_body(tr, nullptr, nullptr, batches, lrs, losses, COVAHIP_MEM_DEVICE, d, samples);
}

int covahip_train_step_data(covahip_train *tr, covahip_train_data *d, const covahip_train_sample *samples, int batch, float lr,
                            float *loss) {
    if (!tr || !d || !samples || !loss || batch <= 0 || tr->K != 1) return COVAHIP_ERR_INVALID_ARG;
    return step_body(tr, nullptr, nullptr, &batch, &lr, loss, COVAHIP_MEM_DEVICE, d, samples);
}

int covahip_train_metrics_m(covahip_train *tr, int model, int64_t tp_fp_fn[3]) {
    if (!tr || !tp_fp_fn || model < 0 || model >= tr->K) return COVAHIP_ERR_INVALID_ARG;
    for (int k = 0; k < 3; k++) tp_fp_fn[k] = tr->last_counts[(size_t)model * 3 + k];
    return COVAHIP_OK;
}

int covahip_train_metrics(covahip_train *tr, int64_t tp_fp_fn[3]) { return covahip_train_metrics_m(tr, 0, tp_fp_fn); }

int covahip_train_weights_m(covahip_train *tr, int model, void *cvhw, size_t cap, size_t *n) {
    if (!tr || !n || model < 0 || model >= tr->K) return COVAHIP_ERR_INVALID_ARG;
    const size_t need = BN_BLOB_BYTES;
    *n = need;
    if (!cvhw || cap < need) return COVAHIP_ERR_OVERFLOW;
    covahip_ctx *ctx = tr->ctx;
    if (int rc = enter(ctx)) return rc;
    std::memcpy(cvhw, BN_HEADER, BN_HEADER_BYTES);
    COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(static_cast<uint8_t *>(cvhw) + BN_HEADER_BYTES, tr->params + (size_t)model * N_PARAMS,
                                          N_PARAMS * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return COVAHIP_OK;
}

int covahip_train_weights(covahip_train *tr, void *cvhw, size_t cap, size_t *n) { return covahip_train_weights_m(tr, 0, cvhw, cap, n); }

int covahip_train_grads_m(covahip_train *tr, int model, float *flat, size_t n) {
    if (!tr || !flat || n != N_PARAMS || model < 0 || model >= tr->K) return COVAHIP_ERR_INVALID_ARG;
    covahip_ctx *ctx = tr->ctx;
    if (int rc = enter(ctx)) return rc;
    COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(flat, tr->grads + (size_t)model * N_PARAMS, N_PARAMS * sizeof(float), hipMemcpyDeviceToHost,
                                          ctx->stream));
    COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return COVAHIP_OK;
}

int covahip_train_grads(covahip_train *tr, float *flat, size_t n) { return covahip_train_grads_m(tr, 0, flat, n); }

int covahip_train_set_plan(covahip_train *tr, const covahip_train_plan *plan) {
    if (!tr || !plan) return COVAHIP_ERR_INVALID_ARG;
    if ((plan->frozen_groups & ~0xFFu) || (plan->bn_inference & ~0x7Fu) || plan->frozen_groups == 0xFFu) return COVAHIP_ERR_INVALID_ARG;
    if (plan->frozen_groups != tr->frozen) {   // the mask is uploaded first: a failure leaves the plan as it was
        covahip_ctx *ctx = tr->ctx;
        if (int rc = enter(ctx)) return rc;
        const std::vector<uint8_t> m = plan_mask(tr, plan->frozen_groups);
        COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(tr->trainable, m.data(), N_PARAMS, hipMemcpyHostToDevice, ctx->stream));
        COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));   // m leaves scope
    }
    tr->frozen = plan->frozen_groups;
    tr->bn_inf = plan->bn_inference | (plan->frozen_groups & 0x7Fu);
    return COVAHIP_OK;
}

int covahip_train_get_plan(covahip_train *tr, covahip_train_plan *plan) {
    if (!tr || !plan) return COVAHIP_ERR_INVALID_ARG;
    plan->frozen_groups = tr->frozen;
    plan->bn_inference = tr->bn_inf;
    return COVAHIP_OK;
}

int covahip_train_set_math(covahip_train *tr, int math) {
    if (!tr || (math != COVAHIP_TRAIN_MATH_EXACT && math != COVAHIP_TRAIN_MATH_MATRIX)) return COVAHIP_ERR_INVALID_ARG;
    if (math == COVAHIP_TRAIN_MATH_MATRIX)
        if (int rc = mm_plan(tr)) return rc;   // before anything changes
    // every entry point of the trainer is synchronous: no step is in flight that the switch could divide
    tr->math = math;
    return COVAHIP_OK;
}

int covahip_train_get_math(covahip_train *tr, int *math) {
    if (!tr || !math) return COVAHIP_ERR_INVALID_ARG;
    *math = tr->math;
    return COVAHIP_OK;
}

int covahip_train_set_post(covahip_train *tr, int model, const covahip_blobnet_post *post) {
    if (!tr || model < 0 || model >= tr->K) return COVAHIP_ERR_INVALID_ARG;
    const size_t hw = (size_t)tr->H[0] * tr->W[0];
    std::vector<uint8_t> row(hw, 1);   // no post, or a post without a keep map: everything is kept
    if (post) {
        if (!std::isfinite(post->logit_thresh)) return COVAHIP_ERR_INVALID_ARG;
        if (post->keep) {
            size_t kept = 0;
            for (size_t i = 0; i < hw; i++) kept += row[i] = post->keep[i] != 0;
            if (!kept) return COVAHIP_ERR_INVALID_ARG;   // nothing to train on
        }
    }
    const uint8_t flag = post ? 1 : 0;
    const float thresh = post ? post->logit_thresh : 0.f;
    covahip_ctx *ctx = tr->ctx;
    if (int rc = enter(ctx)) return rc;
    // every entry point of the trainer is synchronous: nothing of it is in flight that could read the tables
    COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(tr->d_keep + (size_t)model * hw, row.data(), hw, hipMemcpyHostToDevice, ctx->stream));
    COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(tr->d_post_thresh + model, &thresh, sizeof thresh, hipMemcpyHostToDevice, ctx->stream));
    COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(tr->d_post_flag + model, &flag, 1, hipMemcpyHostToDevice, ctx->stream));
    COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));   // row, thresh and flag leave scope
    std::copy(row.begin(), row.end(), tr->post_keep.begin() + (size_t)model * hw);
    tr->post_flag[model] = flag;
    tr->post_thresh[model] = thresh;
    tr->any_post = std::find(tr->post_flag.begin(), tr->post_flag.end(), (uint8_t)1) != tr->post_flag.end();
    return COVAHIP_OK;
}

int covahip_train_get_post(covahip_train *tr, int model, float *logit_thresh, uint8_t *keep_or_null, int *has_post) {
    if (!tr || model < 0 || model >= tr->K) return COVAHIP_ERR_INVALID_ARG;
    const size_t hw = (size_t)tr->H[0] * tr->W[0];
    if (logit_thresh) *logit_thresh = tr->post_thresh[model];
    if (keep_or_null) std::memcpy(keep_or_null, tr->post_keep.data() + (size_t)model * hw, hw);
    if (has_post) *has_post = tr->post_flag[model];
    return COVAHIP_OK;
}

int covahip_train_eval_set(covahip_train *tr, const uint8_t *stack, const uint8_t *gt, const int32_t *counts, float *sample_loss,
                           float *logits, covahip_train_eval_result *out, int mem_kind) {
    if (!tr || !stack || !gt || !counts || !out) return COVAHIP_ERR_INVALID_ARG;
    return eval_body(tr, stack, gt, counts, sample_loss, logits, out, mem_kind);
}

int covahip_train_eval(covahip_train *tr, const uint8_t *stack, const uint8_t *gt, int n, float *sample_loss, float *logits,
                       covahip_train_eval_result *out, int mem_kind) {
    if (!tr || !stack || !gt || !out || n < 1 || tr->K != 1) return COVAHIP_ERR_INVALID_ARG;
    const int32_t count = n;
    return eval_body(tr, stack, gt, &count, sample_loss, logits, out, mem_kind);
}

int covahip_train_eval_set_data(covahip_train *tr, covahip_train_data *d, const covahip_train_sample *samples, const int32_t *counts,
                                float *sample_loss, float *logits, covahip_train_eval_result *out, int mem_kind) {
    if (!tr || !d || !samples || !counts || !out) return COVAHIP_ERR_INVALID_ARG;
    return eval_body(tr, nullptr, nullptr, counts, sample_loss, logits, out, mem_kind, d, samples);
}

int covahip_train_eval_data(covahip_train *tr, covahip_train_data *d, const covahip_train_sample *samples, int n, float *sample_loss,
                            float *logits, covahip_train_eval_result *out, int mem_kind) {
    if (!tr || !d || !samples || !out || n < 1 || tr->K != 1) return COVAHIP_ERR_INVALID_ARG;
    const int32_t count = n;
    return eval_body(tr, nullptr, nullptr, &count, sample_loss, logits, out, mem_kind, d, samples);
}

int covahip_train_state_size(covahip_train *tr, size_t *n) {
    if (!tr || !n) return COVAHIP_ERR_INVALID_ARG;
    *n = state_bytes((size_t)tr->K);
    return COVAHIP_OK;
}

int covahip_train_save_state(covahip_train *tr, uint64_t user_tag, void *buf, size_t cap, size_t *n) {
    if (!tr || !n) return COVAHIP_ERR_INVALID_ARG;
    const size_t need = state_bytes((size_t)tr->K);
    *n = need;
    if (!buf || cap < need) return COVAHIP_ERR_OVERFLOW;
    covahip_ctx *ctx = tr->ctx;
    if (int rc = enter(ctx)) return rc;
    uint8_t *p = static_cast<uint8_t *>(buf);
    const covahip_train_cfg &cf = tr->cfg;
    put<uint32_t>(p, 0, S_MAGIC);
    put<uint32_t>(p, 4, S_VERSION);
    put<uint32_t>(p, 8, (uint32_t)tr->K);
    put<uint32_t>(p, 12, (uint32_t)N_PARAMS);
    put<int32_t>(p, 16, cf.h_mb);
    put<int32_t>(p, 20, cf.w_mb);
    const float scalars[8] = {cf.lr, cf.beta1, cf.beta2, cf.eps, cf.bn_momentum, cf.bn_eps, cf.dropout, cf.smooth};
    std::memcpy(p + 24, scalars, sizeof scalars);
    put<uint64_t>(p, 56, user_tag);
    const size_t pb = N_PARAMS * sizeof(float);
    for (int k = 0; k < tr->K; k++) {
        uint8_t *q = p + S_HEADER + (size_t)k * S_MODEL;
        put<uint64_t>(q, 0, (uint64_t)tr->step[k]);
        put<uint64_t>(q, 8, tr->seed[k]);
        const float *src[3] = {tr->params, tr->adam_m, tr->adam_v};
        for (int a = 0; a < 3; a++)
            COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(q + 16 + a * pb, src[a] + (size_t)k * N_PARAMS, pb, hipMemcpyDeviceToHost, ctx->stream));
    }
    COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    put<uint32_t>(p, need - 4, covahip_crc32c(p, need - 4));
    return COVAHIP_OK;
}

int covahip_train_load_state(covahip_train *tr, const void *buf, size_t n, uint64_t *user_tag) {
    if (!tr || !buf) return COVAHIP_ERR_INVALID_ARG;
    const uint8_t *p = static_cast<const uint8_t *>(buf);
    if (n < S_HEADER + 4 || get<uint32_t>(p, 0) != S_MAGIC || get<uint32_t>(p, 4) != S_VERSION) return COVAHIP_ERR_BAD_DATA;
    const uint32_t nm = get<uint32_t>(p, 8), np = get<uint32_t>(p, 12);
    if (nm < 1 || nm > COVAHIP_MAX_MODELS || np == 0) return COVAHIP_ERR_BAD_DATA;
    if (n != S_HEADER + (size_t)nm * (16 + 3 * (size_t)np * sizeof(float)) + 4) return COVAHIP_ERR_BAD_DATA;
    if (get<uint32_t>(p, n - 4) != covahip_crc32c(p, n - 4)) return COVAHIP_ERR_BAD_DATA;
    if ((int)nm != tr->K || np != N_PARAMS) return COVAHIP_ERR_INVALID_ARG;
    for (int k = 0; k < tr->K; k++)
        if (get<uint64_t>(p, S_HEADER + (size_t)k * S_MODEL) > (uint64_t)INT64_MAX) return COVAHIP_ERR_BAD_DATA;
    covahip_ctx *ctx = tr->ctx;
    if (int rc = enter(ctx)) return rc;
    const size_t pb = N_PARAMS * sizeof(float);
    for (int k = 0; k < tr->K; k++) {
        const uint8_t *q = p + S_HEADER + (size_t)k * S_MODEL;
        float *dst[3] = {tr->params, tr->adam_m, tr->adam_v};
        for (int a = 0; a < 3; a++)
            COVAHIP_CHECK_HIP(ctx, hipMemcpyAsync(dst[a] + (size_t)k * N_PARAMS, q + 16 + a * pb, pb, hipMemcpyHostToDevice, ctx->stream));
    }
    COVAHIP_CHECK_HIP(ctx, hipMemsetAsync(tr->grads, 0, (size_t)tr->K * pb, ctx->stream));
    COVAHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));   // buf is the caller's
    for (int k = 0; k < tr->K; k++) {
        const uint8_t *q = p + S_HEADER + (size_t)k * S_MODEL;
        tr->step[k] = (int64_t)get<uint64_t>(q, 0);
        tr->seed[k] = get<uint64_t>(q, 8);
    }
    std::fill(tr->last_counts.begin(), tr->last_counts.end(), 0);   // the loaded state describes no step
    if (user_tag) *user_tag = get<uint64_t>(p, 56);
    return COVAHIP_OK;
}

void covahip_train_destroy(covahip_train *tr) {
    if (!tr) return;
    hipSetDevice(tr->ctx->device);
    covahip_sync_all(tr->ctx);
    free_train(tr);
}

}  // extern "C"
