// BlobNet forward on gfx950 matrix cores (production path).
//
// Every convolution is an implicit GEMM on v_mfma_f32_{32x32x16,16x16x32}_f16 with
//   M = output positions, N = output channels, K = taps x input channels,
// fp16 operands, fp32 accumulation.  Design (see DESIGN.md for the numbers):
//   * activations live in HBM as fp16 channels-last tensors, so one MFMA A-fragment
//     (8 consecutive k = 8 consecutive input channels of one tap) is one 16-byte LDS read;
//   * a workgroup stages an input band (with halo, zero padded, XOR-swizzled so the
//     ds_read_b128 lane groups are bank-conflict free) into LDS once and every wave
//     reads its A fragments from there;
//   * the weight (B) fragments of a wave's N-tile stay in VGPRs for the whole kernel
//     (workgroups are persistent and loop over (frame, band) items);
//   * the M index is laid out as m = 4*window + position so that the four conv outputs
//     of one 2x2 max-pool window land in the four consecutive accumulator registers of a
//     lane: bias/ReLU/BN/max-pool, and -- with the four T slices kept in four
//     accumulators -- the temporal 4->4->4 MLP + residual all run in-register, and only
//     the pooled tensor (1/4 of the conv output) is written back;
//   * a transposed convolution (4x4, stride 2) is ONE 2x2-tap convolution over the input
//     grid whose N axis stacks the four output parities (N = 4*Cout), so the decoder
//     reuses the same tiling; the last block and the final 1x1 conv have no
//     non-linearity between them and are folded into a single 32->1 transposed conv that
//     runs on the vector ALU together with the threshold.
//
// Reference semantics: utils/model/preprocessing.py:6-7, encoder.py:30-80, pointwise.py:8-26,
// decoder.py:5-134, blobnet.py:8-48; hyper-parameters utils/train-blobnet.py:57-69.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <type_traits>
#include <utility>
#include <vector>

#include "bboxcc_body.h"
#include "bboxcc_wave.h"
#include "blobnet.h"
#include "covahip_dev.h"

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));

namespace {

constexpr float BN_EPS = 1e-3f;
constexpr int WG = 256;  // 4 waves

// ------------------------------------------------------------------ prepared weights
struct EncPrep {
    size_t wfrag;  // byte offset of the B fragments: [NT][KSTEPS][64 lanes] x half8
    size_t epi;    // byte offset of fp32 epilogue constants: bias[C], scale[C], shift[C], w1[16], w2[16]
};
struct DecPrep {
    size_t wfrag;  // [NTT][KSTEPS][64] x half8
    size_t epi;    // bias[C], scale[C], shift[C]
};

}  // namespace

struct Prepared {
    EncPrep enc[BN_LEVELS];
    DecPrep dec[BN_LEVELS - 1];
    size_t enc1w;    // level 1 again, in the fragment order of enc1_mfma: [2 N tiles][5 K steps][64] x half8
    size_t final_w;  // B fragments of the folded (convT 32->16) x (1x1 16->1) last block: [KSTEPS][64] x half8
    size_t final_epi;  // folded bias (fp32)
    size_t final_w_up;   // the same fold restricted to the "up" half of the last block's input (channels 0..15): [4][64] x half8
    size_t tail_w;       // ... and to the skip half (channels 16..31) as fragments of v_mfma_f32_16x16x32_f16 for enc1_mfma, in the K-step
                         // order of its main convolution: [2][64] x half8
    size_t zero;     // 256 zero bytes (LDS-DMA source for halo chunks)
    bool allpos[BN_LEVELS];  // all BN scales of encoder level i are >= 0
    size_t total;
};

namespace {

inline _Float16 f2h(float v) { return (_Float16)v; }

// ------------------------------------------------------------------ helpers
// Division by a launch-time constant d >= 2: q = umulhi(n, magic(d)), exact while n*d < 2^32.
// (magic(1) = 0 marks the identity.)
__device__ __forceinline__ uint32_t fdiv(uint32_t n, uint32_t mul) { return mul ? __umulhi(n, mul) : n; }
inline uint32_t magic(uint32_t d) { return d <= 1 ? 0u : (uint32_t)(((1ull << 32) / d) + 1); }

// Model sets ("Model sets"): the K models' prepared weights lie back to back, `stride` bytes apart (Prepared::total).
// A kernel instantiated with MS = true reads the model id of its item (a stack, or a carrier frame for enc0p_mfma) from the u8 table
// `mid` and offsets every weight pointer by id * stride.  The item is workgroup-uniform, so the offset is made a scalar.  MS = false
// is the single-model kernel: no table, offset 0.
template <bool MS>
__device__ __forceinline__ uint32_t model_off(const uint8_t *mid, uint32_t stride, int idx) {
    if constexpr (!MS) return 0u;
    else return __builtin_amdgcn_readfirstlane((uint32_t)mid[idx] * stride);
}
// A vector value the compiler cannot see through: what is computed from it stays where it is written (is not hoisted out of a loop)
__device__ __forceinline__ int opaque_v(int v) {
    asm volatile("" : "+v"(v));
    return v;
}
template <typename T>
__device__ __forceinline__ const T *at_model(const T *ptr, uint32_t off) {
    return reinterpret_cast<const T *>(reinterpret_cast<const uint8_t *>(ptr) + off);
}
// Weight loads are GLOBAL loads ("Weight loads are global loads").  A pointer that went through an opaque
// `asm` (the hoisting barriers below) or came out of at_model's byte arithmetic has lost its address space, and a load through it
// becomes flat_load: that counts on lgkmcnt as well as vmcnt, so every LDS wait -- lds_barrier() ends in one -- also waits for
// the weights in flight.  Everything the kernels read through these pointers lies in device memory; saying so gives
// global_load (vmcnt alone, returned in order, waited for with a counted vmcnt where the value is used).
template <typename T>
using gptr = const __attribute__((address_space(1))) T *;
template <typename T>
__device__ __forceinline__ gptr<T> as_global(const T *ptr) {
    return (gptr<T>)ptr;
}

// relu -> BN affine -> 2x2 max-pool of the four conv outputs of one window.  BN runs between ReLU and the pool
// (encoder.py:61-66) and gamma may be negative.  The BN scale s of a channel is folded into its weights and bias on the host
// WHATEVER ITS SIGN (a' = s * conv, b' = s * bias), which turns the per-pixel expression relu(conv + bias) * s + shift into
//   s >= 0:  max(a' + b', 0) + shift        s < 0:  min(a' + b', 0) + shift
// and both commute with the window's max (s < 0: the folded weights have flipped the order, the window's max of
// relu(.) * s is at the max of a'):
//   s >= 0:  max(mx, -b') + (b' + shift)    s < 0:  min(mx, -b') + (b' + shift),      mx = max of the four a'
// ALLPOS (every scale of the level >= 0, checked on the host): two v_max3 and one add, e0 = -b', e1 = b' + shift.
// Otherwise ONE form for both signs (round 4): r = med3(mx, lo, hi) + e1 with (lo, hi) = (-b', +big) or (-big, -b') per
// channel (e0 = lo, e2 = hi): v_max3, v_max, v_med3, v_add -- four instructions per window instead of the ~10 of the
// select-max-or-min form of rounds 1-3, so one negative gamma no longer costs the level 10 %.
template <bool ALLPOS>
__device__ __forceinline__ float pool4(float a0, float a1, float a2, float a3, float e0, float e1, float e2) {
    if constexpr (ALLPOS) {
        const float t = fmaxf(fmaxf(a0, a1), a2);
        return fmaxf(fmaxf(t, a3), e0) + e1;
    } else {
        const float mx = fmaxf(fmaxf(fmaxf(a0, a1), a2), a3);
        return __builtin_amdgcn_fmed3f(mx, e0, e2) + e1;
    }
}

// PointWiseTN (pointwise.py:16-26): u = relu(W1^T p), v = relu(W2^T u), out = relu(v + p), on the
// matrix pipe: the two 4x4 products run as v_mfma_f32_4x4x4_16B_f16 (16 independent 4x4x4 blocks
// per instruction).  Operand maps: A[i][k] lives in lane i + 4*block (k in the 4 halves), B[k][j] in
// lane j + 4*block, D[i][j] in lane j + 4*block, register i.  Every lane feeds ITS element's
// 4 T-values as a B column and gets that element's 4 outputs back as its D column; the A rows
// (row lane%4 of W^T) are per-lane constants.  Inputs of the products are rounded to fp16 (like
// every other MFMA operand here).
struct TmixW {
    half4 a1, a2, id;   // id: row lane%4 of the 4x4 identity (brings the residual into the accumulator, see tmix_core)
};
__device__ __forceinline__ TmixW load_tmix(const float *tm, int lane) {
    const int i = lane & 3;
    TmixW w;
#pragma unroll
    for (int t = 0; t < BN_T; t++) {
        w.a1[t] = (_Float16)tm[t * BN_T + i];
        w.a2[t] = (_Float16)tm[16 + t * BN_T + i];
        w.id[t] = (_Float16)(t == i ? 1.f : 0.f);
    }
    return w;
}
// The pooled values are rounded to fp16 ONCE, before both uses (product operand and residual): the carrier-frame
// path keeps them as an fp16 tensor between its level-0 kernel and this MLP, and both paths compute identical bits.
// The MLP is bound by vector-ALU instructions, not by the matrix pipe, so everything that can run on the matrix pipe
// does: the residual p enters as the accumulator of the second product, and it gets there as I * p (exact) instead of
// four conversions and two packed adds.  N independent elements go through the three products phase by phase: a
// 4x4x4 product has a handful of cycles of latency that the next element's instructions fill.
template <int N>
__device__ __forceinline__ void tmix_core(const TmixW &w, const half4 (&pb)[N], f32x4 (&sum)[N], f32x4 (&pvf)[N]) {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    const half4 hz = {(_Float16)0, (_Float16)0, (_Float16)0, (_Float16)0};
    f32x4 u[N];
#pragma unroll
    for (int e = 0; e < N; e++) u[e] = __builtin_amdgcn_mfma_f32_4x4x4f16(w.a1, pb[e], z, 0, 0, 0);
#pragma unroll
    for (int e = 0; e < N; e++) pvf[e] = __builtin_amdgcn_mfma_f32_4x4x4f16(w.id, pb[e], z, 0, 0, 0);
#pragma unroll
    for (int e = 0; e < N; e++) {
        // relu after the rounding to fp16 (same value as rounding after the relu; packed max)
        const half4 ub = __builtin_elementwise_max(__builtin_convertvector(u[e], half4), hz);
        sum[e] = __builtin_amdgcn_mfma_f32_4x4x4f16(w.a2, ub, pvf[e], 0, 0, 0);
    }
}
// relu(relu(v) + p) = max(v + p, p, 0), taken in fp32 at every call site (one finish everywhere: the stacked, the fused and
// the carrier-frame kernels are compared bit for bit)
template <int N>
__device__ __forceinline__ void tmix4f(const TmixW &w, const half4 (&pb)[N], f32x4 (&r)[N]) {
    f32x4 sum[N], pvf[N];
    tmix_core<N>(w, pb, sum, pvf);
#pragma unroll
    for (int e = 0; e < N; e++)
#pragma unroll
        for (int t = 0; t < BN_T; t++) r[e][t] = fmaxf(fmaxf(sum[e][t], pvf[e][t]), 0.f);
}
template <int N>
__device__ __forceinline__ void tmix4h(const TmixW &w, const half4 (&pb)[N], half4 (&o)[N]) {
    f32x4 r[N];
    tmix4f<N>(w, pb, r);
#pragma unroll
    for (int e = 0; e < N; e++) o[e] = __builtin_convertvector(r[e], half4);
}
__device__ __forceinline__ void tmix4h(const TmixW &w, const half4 pb, half4 &o) {
    const half4 pbs[1] = {pb};
    half4 os[1];
    tmix4h<1>(w, pbs, os);
    o = os[0];
}
// Asynchronous 16-byte global -> LDS copy (LDS-DMA): every lane supplies its own global source
// address, the data lands at lds_base (wave-uniform) + lane*16.  Completion is covered by the
// an explicit wait_vmem() before the workgroup barrier.
// The LDS base is made provably wave-uniform with readfirstlane (it goes to M0).
typedef __attribute__((address_space(3))) void lds_void;
__device__ __forceinline__ void glds16(const void *gsrc, uint8_t *lds_base_uniform) {
    const uint32_t a = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lds_void *)lds_base_uniform);
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)gsrc,
                                     (lds_void *)(uintptr_t)a, 16, 0, 0);
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains the vector-memory
// counter, i.e. every wave would sit at the barrier until its own global stores have been written
// to L2; the kernels below never read back what they store, so only LDS needs ordering.  Where an
// LDS-DMA copy (a vector-memory operation) has to have landed, wait_vmem() is called explicitly.
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}
__device__ __forceinline__ void wait_vmem() { __builtin_amdgcn_s_waitcnt(0x0F70); }   // vmcnt(0), nothing else
// vmcnt(N), nothing else: everything but the N youngest vector-memory operations has completed (gfx9 encoding: the count's low four
// bits at [3:0], its high two at [15:14])
// lds_barrier() behind LDS-DMA requests, with the N youngest vector-memory operations (plain loads issued behind the requests)
// left in flight.  Written out -- wait, barrier, and the compiler kept from moving memory accesses across either -- because a
// release fence behind LDS-DMA makes hipcc wait for vmcnt(0) whatever wait stands in front of it.
template <int N>
__device__ __forceinline__ void lds_barrier_vmem_but() {
    static_assert(N >= 0 && N < 64, "vmcnt is a six-bit counter");
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_waitcnt(0x0070 | (N & 15) | ((N >> 4) << 14));   // vmcnt(N) lgkmcnt(0)
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}
// The issue order of a product loop whose LDS fragments come through a ring of AD registers, AD reads ahead of their use: left to
// itself hipcc schedules "ds_read_b128; s_waitcnt lgkmcnt(0); v_mfma" with one fragment register, and with two to four waves per
// SIMD the matrix pipe then idles for most of every LDS latency.  Called right behind the (unrolled) loop of NS reads, it pins
// AD LDS reads in front, then PER MFMAs and -- while reads remain -- one LDS read per step.
template <int NS, int AD, int PER = 1>
__device__ __forceinline__ void pin_ring() {
    __builtin_amdgcn_sched_group_barrier(0x100, AD, 0);
#pragma unroll
    for (int s = 0; s < NS; s++) {
        __builtin_amdgcn_sched_group_barrier(0x008, PER, 0);
        if (s + AD < NS) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    }
}

// LDS pixel swizzle: the 16-byte chunk c of tile pixel (xx, yy) sits at chunk c ^ s(xx, yy).  s comes
// from a small linear family whose parameters the host picks per level and band geometry with a
// model of the ds_read_b128 lane groups (choose_swz below; the model reproduces the
// SQ_LDS_BANK_CONFLICT share rocprofv3 reports for the fixed swizzles it replaces):
//   s = (((yy*L + xx) >> p) * a  +  yy * b  +  (yy & 1) * c)  mod  chunks-per-pixel
struct Swz {
    int p, a, b, c, L;
};
template <int CPP>
__device__ __forceinline__ int swz_eval(const Swz &w, int xx, int yy) {
    return ((((yy * w.L + xx) >> w.p) * w.a) + yy * w.b + (yy & 1) * w.c) & (CPP - 1);
}

// Item order of the persistent encoder kernels.  Static round robin (item = blockIdx + k * grid) by
// default.  With two workgroups per CU the second-dispatched one runs ~25 % slower (the SIMDs issue
// oldest-wave-first; measured per-workgroup times 21.9 vs 27.3 us at level 1), so when the grid is
// exactly two workgroups per CU and a frame has an even number of bands the host switches to a
// PAIRED order: workgroups w and w + grid/2 (the two the dispatcher places on one CU) share frames
// w, w + grid/2, ...; the first takes the larger half of the frame's bands, the second the smaller
// half (band sizes differ by one window row).  No atomics, and both read the same frame.
struct ItemPlan {
    int paired;            // 0: round robin
    int cnt[2];            // bands per frame of the first / second workgroup of a pair
    // the bands of the two roles, one byte each.  Packed into a scalar on purpose: an array in the kernel arguments
    // indexed at run time becomes a vector load followed by s_waitcnt vmcnt(0), and that wait also covers every store
    // of the item just finished (measured: ~2 us per item at level 1)
    unsigned long long band[2];
};
struct ItemIter {
    int b, band;           // current item
    int k, j, role, half;  // state
    int my_cnt;
    unsigned long long my_bands;
    __device__ __forceinline__ bool start(const ItemPlan &pl, int B, int nbands) {
        k = 0; j = 0;
        half = (int)gridDim.x >> 1;
        role = pl.paired && (int)blockIdx.x >= half;
        my_cnt = role ? pl.cnt[1] : pl.cnt[0];
        my_bands = role ? pl.band[1] : pl.band[0];
        return next(pl, B, nbands);
    }
    __device__ __forceinline__ bool next(const ItemPlan &pl, int B, int nbands) {
        if (!pl.paired) {
            const int item = (int)blockIdx.x + k * (int)gridDim.x;
            k++;
            if (item >= B * nbands) return false;
            b = item / nbands;
            band = item - b * nbands;
            return true;
        }
        if (j >= my_cnt) { j = 0; k++; }
        b = ((int)blockIdx.x - role * half) + k * half;
        if (b >= B) return false;
        band = (int)((my_bands >> (8 * j)) & 0xFF);
        j++;
        return true;
    }
};

// ------------------------------------------------------------------ geometry structs
struct EncArgs {
    const __half *in;  // [B][T][H][W][CIN]
    __half *out;       // [B][To][Ho][Wo][COUT]
    const half8 *wfrag;
    const float *epi;
    int B, H, W, Hp, Wp, Ho, Wo, oy, ox, To;
    int RB, nbands, TR, TC;
    uint32_t mWp, mNb, mRC;
    const void *zero;  // >= 16 zero bytes in global memory (source of halo / padding chunks)
    Swz swz;           // LDS pixel swizzle of this launch (choose_swz)
    int scr_off;       // byte offset of the per-wave output transpose scratch (2 KB per wave) in LDS
    int nbuf, buf_stride;   // LDS band buffers (1 or 2) and their distance in bytes
    ItemPlan plan;
    // PRE (level 1 of the carrier-frame path): `in` is the tensor P of enc0p_mfma, [F][H][W][CIN]; stack b takes its
    // T = 0..3 slices from frames pidx[4b .. 4b+3]; the temporal MLP of the level below (weights tm_pre) is
    // applied to the staged tile in LDS; its T = 0 slice goes to skip [B][T][H][W][CIN] (decoder skip input).
    const int32_t *pidx;
    __half *skip;
    const float *tm_pre;
    const uint8_t *model_ids;   // MS: model id per stack [B]
    uint32_t mstride;     // MS: bytes between two models' prepared weights
};

struct DecArgs {
    const __half *up;    // [B][Hi][Wi][C1] or null
    const __half *skip;  // [B][Ts][Hi][Wi][C2], t = 0 used
    __half *out;         // [B][Hd][Wd][COUT]           (blocks 0..2)
    float *logits;       // [B][Hd][Wd] or null         (last block)
    uint8_t *mask;       // [B][Hd][Wd] or null         (last block)
    const half8 *wfrag;
    const float *epi;    // blocks 0..2: scale[COUT], shift'[COUT]; last block: folded bias
    int B, Hi, Wi, Hd, Wd, cy, cx, Ts;
    int nbands;          // bands of grid rows per frame
    uint32_t mNb, mGW, mRC;
    const void *zero;
    Swz swz;             // LDS pixel swizzle of this launch (choose_swz)
    int scr_off;         // blocks 0..2: byte offset of the per-wave store transpose scratch (2 KB per wave)
    int mask_off;        // last block: byte offset of the band's mask rows in LDS
    const float *part;   // last block without a skip input (C2 == 0): the skip half's share of the logits, fp32 [B][Hi + 1][Wi + 1][4 parities] (Enc1Args::part)
};
// Model sets (model_off): the decoder kernels' own argument behind DecArgs / at the end of Dec3ccArgs, so that the single-model
// kernels keep their argument layout
struct DecMs {
    const uint8_t *model_ids;   // model id per stack [B]
    uint32_t mstride;           // bytes between two models' prepared weights
};
// Per-model post-processing ("Per-model post-processing"; covahip_blobnet_set_post):
//   mask = (logit > threshold of the stack's model) && keep map of the stack's model
// in the kernels that turn logits into a mask, instantiated with POST = true.  Behind DecMs in the argument lists, for the same
// reason (a POST = false kernel gets the empty DecNoPost).  A batch of one model gets that model's threshold by value and its keep pointers; a mixed batch (MS) gets model 0's
// and takes every stack's through the model id, like the weights: thr_tab[id], keep + id * keep_stride, planes + id * planes_stride.
// POST = false is the kernel without any of it: threshold 0, no keep map, these arguments are not read.
struct DecPost {
    float thr;                  // logit threshold of the batch's model
    const float *thr_tab;       // MS: threshold per model
    int area;                   // bboxcc's area threshold of the batch's model, already resolved: the model's own when set, else the call's
    const int32_t *area_tab;    // MS: area threshold per model, 0 = unset (the call's applies; covahip_blobnet_set_area)
    const uint8_t *keep;        // u8 [Hd][Wd], 1 = the macroblock may be foreground (always present: all ones without a keep map)
    const uint32_t *planes;     // the same as bboxcc's parity planes: u32 [Hd][E lo, E hi, O lo, O hi] (dec3cc_rows_mfma)
    uint32_t keep_stride, planes_stride;   // MS: bytes between two models' maps
};
// the argument of a POST = false kernel: nothing
struct DecNoPost {};
template <bool POST>
using PostArg = std::conditional_t<POST, DecPost, DecNoPost>;
// The settings of stack b: of the batch's model, or through the stack's model id (MS; a scalar, the stack is workgroup-uniform).
// POST = false: the literal threshold 0 and no maps -- the flag-off kernels contain none of this.
struct StackPost {
    float thr;
    const uint8_t *keep;
    const uint32_t *planes;
};
template <bool POST, bool MS>
__device__ __forceinline__ StackPost stack_post(const PostArg<POST> &pp, const uint8_t *mid, int b) {
    if constexpr (!POST) {
        return StackPost{0.f, nullptr, nullptr};
    } else if constexpr (!MS) {
        return StackPost{pp.thr, pp.keep, pp.planes};
    } else {
        const uint32_t id = __builtin_amdgcn_readfirstlane((uint32_t)mid[b]);
        return StackPost{pp.thr_tab[id], at_model(pp.keep, id * pp.keep_stride), at_model(pp.planes, id * pp.planes_stride)};
    }
}
// bboxcc's area threshold of stack b, the last of its settings: the same three cases (area_call: the call's threshold, which a
// model without one of its own takes; POST = false: nothing but that).  A function of its own, called where bboxcc starts: taken at
// the top of the frame with the others, the scalar lived across the tile loop, whose scalar registers are all in use
// (dec3cc_mfma<false, false, true, true> spilled it: 8 bytes of scratch).
template <bool POST, bool MS>
__device__ __forceinline__ int stack_area(const PostArg<POST> &pp, const uint8_t *mid, int b, int area_call) {
    if constexpr (!POST) {
        return area_call;
    } else if constexpr (!MS) {
        return pp.area;
    } else {
        const int a = pp.area_tab[__builtin_amdgcn_readfirstlane((uint32_t)mid[b])];
        return a >= 1 ? a : area_call;
    }
}

#ifdef PHASE_TIMING
// developer build only (tools/phase_timing.sh): wall-clock ticks (s_memrealtime, 100 MHz) per phase of the item loop,
// summed over the workgroups' wave 0
__device__ unsigned long long g_phase[80];
#define PHASE_MARK(i)                                                     \
    do {                                                                  \
        const unsigned long long now_ = __builtin_amdgcn_s_memrealtime(); \
        ph_[i] += now_ - last_;                                           \
        last_ = now_;                                                     \
    } while (0)
#else
#define PHASE_MARK(i) do { } while (0)
#endif
#if defined(PHASE_TIMING) || defined(WGSPAN_ONLY)
// per-workgroup life span of the last launch of a kernel: {start, end} in s_memrealtime ticks (10 ns) and the hardware id
// (which workgroups shared a CU).  -DWGSPAN_ONLY: the spans without the phase marks (which add waits to the item loop)
__device__ unsigned long long g_wgspan[6][1024][4];
#define WGSPAN_BEGIN() const unsigned long long wg_t0_ = __builtin_amdgcn_s_memrealtime(), wg_c0_ = __builtin_amdgcn_s_memtime()
#define WGSPAN_END(kid)                                                                          \
    do {                                                                                         \
        if (threadIdx.x == 0 && blockIdx.x < 1024) {                                             \
            g_wgspan[kid][blockIdx.x][0] = wg_t0_;                                               \
            g_wgspan[kid][blockIdx.x][1] = __builtin_amdgcn_s_memrealtime();                     \
            g_wgspan[kid][blockIdx.x][2] = __builtin_amdgcn_s_getreg(4 | (0 << 6) | (31 << 11)); \
            g_wgspan[kid][blockIdx.x][3] = __builtin_amdgcn_s_memtime() - wg_c0_;                \
        }                                                                                        \
    } while (0)
#else
#define WGSPAN_BEGIN() do { } while (0)
#define WGSPAN_END(kid) do { } while (0)
#endif
#ifdef WGSPAN_ONLY
// time line of the first four items of every workgroup of enc_mfma (wave 0): item start, band requested, band landed (after the
// barrier), tiles done -- s_memrealtime ticks
__device__ unsigned long long g_itemspan[3][1024][4][4];
#define ITEM_MARK(j) do { if (it_n_ < 4) it_t_[it_n_][j] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define ITEM_MARK(j) do { } while (0)
#endif
// ------------------------------------------------------------------ enc level 0
// u8 RGBA carrier frame -> conv3x3 (3->16) on v_mfma_f32_16x16x32_f16.
// K layout: one K-step = 2 kernel rows x (4 pixels x 4 channels); pixel 3 and channel 3
// carry zero weights, the 1/6 of clip(x,0,6)/6 is folded into the weights, so the LDS tile
// holds min(x,6) as exact small integers in fp16, 8 bytes per macroblock.
// Tile: row r <-> input row y0-1+r, col c <-> input col c-2 (cols 0,1 and W+2,W+3 are zero),
// TC = W+4 so rows are 16-byte multiples and 4-pixel groups land 16-byte aligned.
// One tile = 8 pool windows.  The 16 rows of an MFMA are the 8 windows x 2 conv rows (dy) of ONE column parity: conv
// pixels with even x and with odd x go to two MFMAs with two weight sets, so that the 4-pixel K group every lane reads
// starts at an even tile column, i.e. is one 16-byte aligned ds_read_b128:
//   even x: tile cols [x, x+3]   = inputs x-2..x+1 -> weights [0, k0, k1, k2]
//   odd  x: tile cols [x+1, x+4] = inputs x-1..x+2 -> weights [k0, k1, k2, 0]
// (tile col = input col + 2).  D rows 4*(lane>>4)+r -> window 2*(lane>>4) + (r>>1), dy = r&1, so both windows of a lane
// pool in-register over {even, odd} x {dy}.
// u8 -> fp16 without integer->float conversions: v_perm builds the fp16 bit pattern 0x6400 | n (= 1024 + n, exact for
// n < 1024) for two channels at a time, then a packed min with 1030 (the clip at 6) and a packed subtract of 1024.  The
// alpha byte lands in channel 3, whose weights are zero.
constexpr int WG0 = 512;  // 8 waves: the per-tile dependency chain is latency bound, so run 4 waves per SIMD
// ------------------------------------------------------------------ enc level 0, one carrier frame (= one T slice) at a time
// conv + ReLU + BN + pool of level 0 work on single T slices (kernel depth 1, encoder.py:35-52), and with gamma = 1 a
// carrier frame is a slice of four consecutive stacks.  This kernel runs that part ONCE per carrier frame and leaves the
// pooled values -- the input of the level's temporal MLP -- as an fp16 tensor P [F][Ho][Wo][16]; the MLP itself moves
// into the staging of level 1 (enc1_mfma / enc_mfma<.., PRE>), which gathers the four frames of a stack by index.
// BOTH entry points run it (round 4): the stacked tensor [B][T*H][W][4] of covahip_filter_forward is B*T carrier frames
// whose stack b takes its T = 0..3 slices from frames 4b .. 4b+3 -- one kernel chain, identical bits by construction.
struct Enc0pArgs {
    const uint8_t *in;  // [F][H][W][4]
    __half *out;        // [F][Ho][Wo][16]
    const half8 *wfrag;
    const float *epi;
    int F, H, W, Hp, Wp, Ho, Wo, oy, ox;
    int nbands, TC;
    uint32_t mWp, mNb, mW4;
    int scr_off;        // per-wave output scratch (1 KB per wave) behind the tile
    const uint8_t *model_ids; // MS: model id per carrier frame [F]
    uint32_t mstride;   // MS: bytes between two models' prepared weights
};
template <bool ALLPOS, bool PACKED, bool MS = false>
__global__ __launch_bounds__(WG0, 4) void enc0p_mfma(Enc0pArgs p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    WGSPAN_BEGIN();
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int TC = p.TC;
    half8 be0 = p.wfrag[lane], be1 = p.wfrag[64 + lane];
    half8 bo0 = p.wfrag[128 + lane], bo1 = p.wfrag[192 + lane];
    const int co = lane & 15;
    float e0 = p.epi[co], e1 = p.epi[16 + co], e2 = p.epi[32 + co];
    [[maybe_unused]] uint32_t moff_cur = 0;   // MS: the model whose weights are in registers (model 0 above)
    // the lane's part of its fragment addresses: window m >> 1 of a tile, conv row m & 1; g: K half (kernel row) and pixel pair
    const int m = lane & 15, g = lane >> 4;
    const uint32_t lc0 = (uint32_t)((((m & 1) + (g >> 1)) * TC + 2 * (m >> 1) + 2 * (g & 1)) * 8);
    const uint32_t lc1 = (uint32_t)((((m & 1) + 2) * TC + 2 * (m >> 1) + 2 * (g & 1)) * 8);
    const int n_items = p.F * p.nbands;
    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int f = fdiv(item, p.mNb), band = item - f * p.nbands;
        if constexpr (MS) {   // uniform branch: the frame's model differs from the one in registers
            const uint32_t mo = model_off<MS>(p.model_ids, p.mstride, f);
            if (mo != moff_cur) {
                moff_cur = mo;
                const half8 *wf = at_model(p.wfrag, mo);
                const float *ep = at_model(p.epi, mo);
                be0 = wf[lane]; be1 = wf[64 + lane]; bo0 = wf[128 + lane]; bo1 = wf[192 + lane];
                e0 = ep[co]; e1 = ep[16 + co]; e2 = ep[32 + co];
            }
        }
        const int y0 = 2 * ((band * p.Hp) / p.nbands);
        const int rows = 2 * (((band + 1) * p.Hp) / p.nbands) - y0;
        const int n2 = rows + 2;
        lds_barrier();
        {   // stage rows y0-1 .. y0+rows as fp16 (the u8 -> fp16 conversion described above WG0); the host keeps n2 * W/4 <= 2 * WG0
            const int W4 = p.W >> 2;
            const int per_t = n2 * W4;
            // PACKED: two bytes per macroblock, min(type, 6) | min(mv_x, 6) << 3 | min(mv_y, 6) << 6 (covahip_carrier_pack) --
            // what the network keeps of a record anyway (clip at 6, preprocessing.py:6-7), at half the PCIe bytes
            const uint8_t *fb = p.in + (size_t)f * p.H * p.W * (PACKED ? 2 : 4);
            uint4 v[2];
            int dsto[2];
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const int i = tid + k * WG0;
                dsto[k] = -1;
                v[k] = make_uint4(0, 0, 0, 0);
                if (i < per_t) {
                    const int r = fdiv(i, p.mW4), c4 = i - r * W4;
                    const int y = y0 - 1 + r;
                    dsto[k] = r * TC * 8 + 16 + c4 * 32;
                    if (y >= 0 && y < p.H) {
                        if constexpr (PACKED) {
                            const uint2 w = *reinterpret_cast<const uint2 *>(fb + ((size_t)y * p.W + c4 * 4) * 2);
                            v[k].x = w.x; v[k].y = w.y;
                        } else {
                            v[k] = *reinterpret_cast<const uint4 *>(fb + ((size_t)y * p.W + c4 * 4) * 4);
                        }
                    }
                }
            }
            const half2v clip = {(_Float16)1030.f, (_Float16)1030.f}, off = {(_Float16)1024.f, (_Float16)1024.f};
#pragma unroll
            for (int k = 0; k < 2; k++) {
                if (dsto[k] >= 0) {
                    uint32_t o[8];
                    if constexpr (PACKED) {
                        const uint32_t pw[2] = {v[k].x, v[k].y};
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            const uint32_t r = (pw[q >> 1] >> (16 * (q & 1))) & 0xFFFFu;
                            const uint32_t c01 = 0x64006400u | (r & 7u) | (((r >> 3) & 7u) << 16);
                            const uint32_t c23 = 0x64006400u | ((r >> 6) & 7u);
                            o[2 * q] = __builtin_bit_cast(uint32_t, __builtin_bit_cast(half2v, c01) - off);
                            o[2 * q + 1] = __builtin_bit_cast(uint32_t, __builtin_bit_cast(half2v, c23) - off);
                        }
                    } else {
                        const uint32_t px[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            const uint32_t c01 = __builtin_amdgcn_perm(0x64646464u, px[q], 0x05010500u);
                            const uint32_t c23 = __builtin_amdgcn_perm(0x64646464u, px[q], 0x05030502u);
                            const half2v h01 = __builtin_elementwise_min(__builtin_bit_cast(half2v, c01), clip) - off;
                            const half2v h23 = __builtin_elementwise_min(__builtin_bit_cast(half2v, c23), clip) - off;
                            o[2 * q] = __builtin_bit_cast(uint32_t, h01);
                            o[2 * q + 1] = __builtin_bit_cast(uint32_t, h23);
                        }
                    }
                    uint8_t *d = smem + dsto[k];
                    *reinterpret_cast<uint4 *>(d) = make_uint4(o[0], o[1], o[2], o[3]);
                    *reinterpret_cast<uint4 *>(d + 16) = make_uint4(o[4], o[5], o[6], o[7]);
                }
            }
            for (int i = tid; i < n2 * 2; i += WG0)   // zero halo columns 0,1 and W+2,W+3
                *reinterpret_cast<uint4 *>(smem + (i >> 1) * TC * 8 + ((i & 1) ? (p.W + 2) * 8 : 0)) = make_uint4(0, 0, 0, 0);
        }
        lds_barrier();
        // four tiles of 8 pool windows per wave pass: 32 consecutive windows of ONE window row (round 4: a pass is (window row,
        // half-row index) -- wave-uniform -- so a fragment's address is a lane constant + the pass's base + 128 bytes per tile as an
        // immediate, where passes over a band-wide window index cost a division and twelve vector instructions per tile; the lanes
        // of windows past the row's end compute on what the band holds there and store nothing).  The 32 windows x 16 channels
        // leave the wave as one 16-byte store per lane
        const int nhalf = (p.Wp + 31) >> 5;
        const int ngroups = (rows / 2) * nhalf;
        uint8_t *const scr = smem + p.scr_off + wave * 1024;
        __half *const ob = p.out + (size_t)f * p.Ho * p.Wo * 16;
        int g_wy = 0, g_h = wave;
        for (int grp = wave; grp < ngroups; grp += WG0 / 64, g_h += WG0 / 64) {
            while (g_h >= nhalf) { g_h -= nhalf; g_wy++; }
            const uint32_t gbase = (uint32_t)(((2 * g_wy) * TC + 64 * g_h) * 8);
            // 16-byte aligned (even tile column, row stride a multiple of 16): one ds_read_b128 each
            const uint8_t *const a0 = smem + (gbase + lc0), *const a1 = smem + (gbase + lc1);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const half8 ae0 = *reinterpret_cast<const half8 *>(__builtin_assume_aligned(a0 + k * 128, 16));
                const half8 ae1 = *reinterpret_cast<const half8 *>(__builtin_assume_aligned(a1 + k * 128, 16));
                const half8 ao0 = *reinterpret_cast<const half8 *>(__builtin_assume_aligned(a0 + k * 128 + 16, 16));
                const half8 ao1 = *reinterpret_cast<const half8 *>(__builtin_assume_aligned(a1 + k * 128 + 16, 16));
                f32x4 ce = {0.f, 0.f, 0.f, 0.f}, co_ = {0.f, 0.f, 0.f, 0.f};
                ce = __builtin_amdgcn_mfma_f32_16x16x32_f16(ae0, be0, ce, 0, 0, 0);
                co_ = __builtin_amdgcn_mfma_f32_16x16x32_f16(ao0, bo0, co_, 0, 0, 0);
                ce = __builtin_amdgcn_mfma_f32_16x16x32_f16(ae1, be1, ce, 0, 0, 0);
                co_ = __builtin_amdgcn_mfma_f32_16x16x32_f16(ao1, bo1, co_, 0, 0, 0);
                _Float16 *sw = reinterpret_cast<_Float16 *>(scr + (k * 8 + 2 * g) * 32) + co;
                // the fp32 value is made opaque before the conversion: hipcc would otherwise fuse the BN multiply-add and
                // the conversion into one v_fma_mixlo_f16 (ONE rounding), while the level's other forms round to fp32 and then to fp16
                float v0 = pool4<ALLPOS>(ce[0], ce[1], co_[0], co_[1], e0, e1, e2);
                float v1 = pool4<ALLPOS>(ce[2], ce[3], co_[2], co_[3], e0, e1, e2);
                asm volatile("" : "+v"(v0), "+v"(v1));
                sw[0] = (_Float16)v0;
                sw[16] = (_Float16)v1;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const int owx = 32 * g_h + (lane >> 1);
            if (owx < p.Wp) {
                const int gy = y0 / 2 + g_wy + p.oy, gx = owx + p.ox;
                *reinterpret_cast<uint4 *>(ob + (gy * p.Wo + gx) * 16 + 8 * (lane & 1)) =
                    *reinterpret_cast<const uint4 *>(scr + lane * 16);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the next pass's values stay behind these reads
            __builtin_amdgcn_wave_barrier();
        }
    }
    WGSPAN_END(5);
}

// ------------------------------------------------------------------ enc levels 1..3
// conv3x3 CIN -> COUT on v_mfma_f32_32x32x16_f16.  Wave roles: N-tile = wave % NT,
// M-group = wave / NT.  One K-step = one tap x 16 input channels.
// TSZ > 0 (round 4, levels 2 and 3 where the geometry suits it): ROW-ALIGNED tiles -- a tile is eight consecutive windows of ONE
// window row (tile column tc = windows 8 tc .. 8 tc + 7; lanes of windows past the row's end compute on whatever the band holds
// there and store nothing) -- on a band whose T slices lie TSZ bytes apart (compile time), with a swizzle that is periodic over
// 16 pixels and 2 rows (the host picks one: choose_swz(periodic)).  A fragment's LDS address is then
//     [tile base: wave-uniform] + [lane constant of the tap, set once per kernel] ^ [channel chunk << 5] + [T slice: immediate],
// i.e. one add per tap and one xor per further channel chunk per tile, where the general form below evaluates the swizzle and
// the pixel address for every tap of every tile (216 of the 270 vector instructions of a level-2 tile's matrix part).
template <int CIN, int COUT, int TPAR, int OCC, int NWV, bool ALLPOS, bool PRE = false, int TSZ = 0, bool MS = false>
__global__ __launch_bounds__(NWV * 64, OCC) void enc_mfma(EncArgs p) {
    constexpr int WGS = NWV * 64;
    constexpr int NT = COUT / 32, MG = NWV / NT, KC = CIN / 16, KSTEPS = 9 * KC;
    constexpr int CPP = CIN / 8, PS = CIN * 2;
    constexpr int AD = CIN == 32 ? 8 : 0;   // depth of the A-fragment ring (see the tile loop): what the register budget allows
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ntile = wave % NT, mgroup = wave / NT;
    const int TR = p.TR, TC = p.TC;
    const int tsz = TSZ > 0 ? TSZ : TR * TC * PS;
    static_assert(TSZ == 0 || (TSZ % 16 == 0 && (TPAR - 1) * TSZ < 65536 && !PRE), "T-slice offsets must fit a DS instruction's offset field");

    WGSPAN_BEGIN();
#ifdef PHASE_TIMING
    unsigned long long ph_[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, last_ = __builtin_amdgcn_s_memrealtime();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
    // ---- PRE: temporal MLP of the level below, in place, on the 16-byte pieces THIS thread requested (the staging loop
    // and this one walk the same piece indices): a thread needs nothing but its own vmcnt(0) before it, so the pass
    // runs while other waves' pieces are still landing and no workgroup barrier separates it from the staging.  A lane
    // takes one piece (8 channels of a pixel) of all four T slices; the MLP does not depend on the channel, so the
    // swizzle is irrelevant here.  Zero padding stays zero (no bias).
    auto mlp_own = [&](uint8_t *base, int band_, const TmixW &tmp) {
        const int n2_ = 2 * (((band_ + 1) * p.Hp) / p.nbands) - 2 * ((band_ * p.Hp) / p.nbands) + 2;
        const int nchunk = n2_ * TC * CPP;
        for (int sidx = tid; sidx < nchunk; sidx += WGS) {
            half8 v[BN_T], o[BN_T];
#pragma unroll
            for (int t = 0; t < BN_T; t++) v[t] = *reinterpret_cast<const half8 *>(base + t * tsz + sidx * 16);
#pragma unroll
            for (int j0 = 0; j0 < 8; j0 += 4) {
                half4 pb[4];
                f32x4 r[4];
#pragma unroll
                for (int j = 0; j < 4; j++) pb[j] = half4{v[0][j0 + j], v[1][j0 + j], v[2][j0 + j], v[3][j0 + j]};
                tmix4f<4>(tmp, pb, r);
#pragma unroll
                for (int j = 0; j < 4; j++)
#pragma unroll
                    for (int t = 0; t < BN_T; t++) o[t][j0 + j] = (_Float16)r[j][t];
            }
#pragma unroll
            for (int t = 0; t < BN_T; t++) *reinterpret_cast<half8 *>(base + t * tsz + sidx * 16) = o[t];
        }
    };
    // ---- stage one band with LDS-DMA: the tile is swept linearly in 16-byte chunks (64 per wave-instruction);
    // chunk -> (row, col, physical chunk) -> swizzled source chunk; halo columns / out-of-image rows read the zero
    // buffer.  The decomposition is done once per chunk position and reused for the four T slices (source + t * plane,
    // LDS + t * tsz).
    auto stage = [&](int sb, int sband, uint8_t *dst, int ll) {
        const int sy0 = 2 * ((sband * p.Hp) / p.nbands);
        const int sn2 = 2 * (((sband + 1) * p.Hp) / p.nbands) - sy0 + 2;
        int fidx[BN_T] = {0, 1, 2, 3};   // frame that holds T slice t: the stack's row of the table (PRE) or the stack's own slices
        if constexpr (PRE) {
            // a SCALAR load (constant address space; the table is uploaded before the launch and never written by a
            // kernel): a vector load here would sit behind the previous item's stores in vmcnt order, and the LDS-DMA
            // below could not be issued before those have drained
            typedef int i32x4 __attribute__((ext_vector_type(4)));
            typedef const __attribute__((address_space(4))) i32x4 *const_i32x4_ptr;
            if (p.pidx) {
                const i32x4 row = *(const_i32x4_ptr)(uintptr_t)(p.pidx + sb * BN_T);
                fidx[0] = row[0]; fidx[1] = row[1]; fidx[2] = row[2]; fidx[3] = row[3];
            } else {   // stacked entry: stack sb = frames 4 sb .. 4 sb + 3
                fidx[0] = BN_T * sb; fidx[1] = BN_T * sb + 1; fidx[2] = BN_T * sb + 2; fidx[3] = BN_T * sb + 3;
            }
        }
        const int RC = TC * CPP;  // chunks per tile row
        const int nchunk = sn2 * RC;
        const size_t tplane = (size_t)p.H * p.W * CIN * 2;   // bytes
        const uint8_t *fbase = reinterpret_cast<const uint8_t *>(p.in) + (PRE ? 0 : (size_t)sb * BN_T * tplane);
        size_t foff[BN_T];   // byte offset of the frame that holds T slice t
#pragma unroll
        for (int t = 0; t < BN_T; t++) foff[t] = (size_t)fidx[t] * tplane;
        for (int s0 = wave * 64; s0 < nchunk; s0 += WGS) {
            const int sidx = s0 + ll;
            if (sidx < nchunk) {
                const int r = fdiv(sidx, p.mRC), within = sidx - r * RC;
                const int c = within / CPP, chp = within % CPP;
                const int ch = chp ^ swz_eval<CPP>(p.swz, c, r);
                const int y = sy0 - 1 + r, x = c - 1;
                const bool in = y >= 0 && y < p.H && x >= 0 && x < p.W;
                const uint8_t *src = in ? fbase + ((size_t)(y * p.W + x) * CIN + ch * 8) * 2
                                        : reinterpret_cast<const uint8_t *>(p.zero);
#pragma unroll
                for (int t = 0; t < BN_T; t++) glds16(src + (in ? foff[t] : 0), dst + t * tsz + s0 * 16);
            }
        }
    };
    // Items (frame, band) of this workgroup, one after the other.  With two LDS buffers (p.nbuf == 2, when the host
    // found room) the next item's band is in flight while this one is computed: ONE barrier per item, right after
    // the item's own band has landed -- every wave has then left the previous item, whose buffer the next band may
    // overwrite.  With one buffer: barrier, stage, wait, barrier.
#ifdef WGSPAN_ONLY
    unsigned long long it_t_[4][4] = {};
    int it_n_ = 0;
#endif
    ItemIter it;
    bool more = it.start(p.plan, p.B, p.nbands);
    const bool dbl = p.nbuf == 2;
    int cur = 0;
    if (more && dbl) {
        stage(it.b, it.band, smem, lane);
        wait_vmem();
        if constexpr (PRE) mlp_own(smem, it.band, load_tmix(at_model(p.tm_pre, model_off<MS>(p.model_ids, p.mstride, it.b)), lane));
    }
    // one buffer: the first band is requested BEFORE the weight fragments (36 - 144 registers per lane, every workgroup of
    // the launch pulling the same 37 - 295 KB through L2 at once), so that both are in flight together
    bool first_staged = false;
    if (more && !dbl) { stage(it.b, it.band, smem, lane); first_staged = true; }
    half8 bf[KSTEPS];
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ks++) bf[ks] = p.wfrag[(ntile * KSTEPS + ks) * 64 + lane];
    const int co = ntile * 32 + (lane & 31);
    float e0 = p.epi[co], e1 = p.epi[COUT + co], e2 = p.epi[2 * COUT + co];   // see pool4
    TmixW tm = load_tmix(p.epi + 3 * COUT, lane);
    // TSZ > 0: the lane's part of a fragment address per tap: pixel (lane's window of the tile, position, tap) of tile (0, 0),
    // xor the 16-byte chunk (kh ^ swizzle) -- the K half kh and the swizzle meet in the chunk bits, which the pixel address
    // leaves clear
    [[maybe_unused]] uint32_t kq[9];
    if constexpr (TSZ > 0) {
        const int m0 = lane & 31, kh0 = lane >> 5;
        const int yl = (m0 >> 1) & 1, xl = 2 * (m0 >> 2) + (m0 & 1);
#pragma unroll
        for (int tap = 0; tap < 9; tap++) {
            const int yy = yl + tap / 3, xx = xl + tap % 3;
            kq[tap] = (uint32_t)((yy * TC + xx) * PS) ^ (uint32_t)((kh0 ^ swz_eval<CPP>(p.swz, xx, yy)) << 4);
        }
    }
#ifdef PHASE_TIMING
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    PHASE_MARK(8);   // weight fragments and epilogue constants in registers
#endif
    while (more) {
        const int b = it.b, band = it.band;
        [[maybe_unused]] const uint32_t moff = model_off<MS>(p.model_ids, p.mstride, b);
        // balanced bands of whole pool-window rows
        const int y0 = 2 * ((band * p.Hp) / p.nbands);
        const int rows = 2 * (((band + 1) * p.Hp) / p.nbands) - y0;
        // opaque per-item copy of the lane id: keeps hipcc from hoisting (and, at level 3, spilling) the
        // lane-only index math out of the item loop
        int ll = lane;
        asm volatile("" : "+v"(ll));
        uint8_t *const bandp = smem + cur * p.buf_stride;   // this item's band in LDS
        PHASE_MARK(0);   // item bookkeeping
        ITEM_MARK(0);
        // the weights of the level below's temporal MLP: fetched here so that the loads are in flight together with the
        // band's (they are waited for with it), not on their own between two barriers
        TmixW tmp;
        if constexpr (PRE) tmp = load_tmix(at_model(p.tm_pre, moff), ll);
        if (!dbl) {
            if (!first_staged) {
                lds_barrier();
                PHASE_MARK(1);   // waiting for the workgroup's other waves to finish the previous item
                stage(b, band, bandp, ll);
            }
            first_staged = false;
            PHASE_MARK(2);   // issuing the band's LDS-DMA
            ITEM_MARK(1);
            wait_vmem();
            if constexpr (PRE) mlp_own(bandp, band, tmp);
            PHASE_MARK(4);   // own pieces landed, temporal MLP applied
        }
        lds_barrier();
        PHASE_MARK(3);   // the band landing / the other waves leaving the previous item
        ITEM_MARK(2);
        more = it.next(p.plan, p.B, p.nbands);
        // Two buffers: the next band is requested now and waited for (vmcnt(0), in `landed()`) right before this item's
        // first global store -- NOT at the top of the next item: the counter is in order, and a wait placed behind the
        // epilogue's stores is a wait for those stores to be acknowledged (measured: 1.6 us per item).  At the
        // first store the youngest outstanding operation is the request itself, one MLP pass or one tile old.
        bool in_flight = false;
        if (dbl) {
            if (more) { stage(it.b, it.band, smem + (cur ^ 1) * p.buf_stride, ll); in_flight = true; }
            cur ^= 1;
            PHASE_MARK(2);
        }
        auto landed = [&]() {
            if (in_flight) {
                wait_vmem();
                if constexpr (PRE && MS) mlp_own(smem + cur * p.buf_stride, it.band, load_tmix(at_model(p.tm_pre, model_off<MS>(p.model_ids, p.mstride, it.b)), ll));
                else if constexpr (PRE) mlp_own(smem + cur * p.buf_stride, it.band, tmp);   // `cur` already names the next item's buffer
                in_flight = false;
            }
        };
        if constexpr (PRE) {
            landed();
            // ---- T = 0 slice of the band's own rows -> skip tensor (the last band also owns the odd last row)
            const int ya = y0, yb = (band == p.nbands - 1) ? p.H : y0 + rows;
            const int npc = (yb - ya) * p.W * CPP;
            __half *const sk = p.skip + (size_t)b * BN_T * p.H * p.W * CIN;
            for (int i = tid; i < npc; i += WGS) {
                const int pix = i / CPP, ch = i % CPP;
                const int ry = pix / p.W, x = pix - ry * p.W;
                const int r = ya - y0 + 1 + ry, c = x + 1;
                const uint4 v = *reinterpret_cast<const uint4 *>(bandp + (r * TC + c) * PS + ((ch ^ swz_eval<CPP>(p.swz, c, r)) * 16));
                *reinterpret_cast<uint4 *>(sk + ((size_t)(ya + ry) * p.W + x) * CIN + ch * 8) = v;
            }
        }
        PHASE_MARK(5);   // skip slice out
        if constexpr (MS) {   // this stack's weights, loaded where the staging's registers are free again (one copy, no spill)
            const half8 *wf = at_model(p.wfrag, moff);
            const float *ep = at_model(p.epi, moff);
#pragma unroll
            for (int ks = 0; ks < KSTEPS; ks++) bf[ks] = wf[(ntile * KSTEPS + ks) * 64 + lane];
            e0 = ep[co]; e1 = ep[COUT + co]; e2 = ep[2 * COUT + co];
            tm = load_tmix(ep + 3 * COUT, lane);
        }
        // ---- compute
        const int nwin = (rows / 2) * p.Wp;
        const int ntc = (p.Wp + 7) >> 3;                    // TSZ > 0: tile columns of a window row
        const int ntiles = TSZ > 0 ? (rows / 2) * ntc : (nwin + 7) / 8;
        const int m = ll & 31, kh = ll >> 5;
        int t_wy = 0, t_tc = mgroup;                        // TSZ > 0: the tile's window row and tile column (wave-uniform)
        for (int tile = mgroup; tile < ntiles; tile += MG, t_tc += MG) {
            [[maybe_unused]] int yy0 = 0, xx0 = 0;
            [[maybe_unused]] uint32_t fa[9];                // TSZ > 0: fragment addresses of the nine taps, channel chunk 0, T slice 0
            if constexpr (TSZ > 0) {
                while (t_tc >= ntc) { t_tc -= ntc; t_wy++; }
                const uint32_t tbase = (uint32_t)(cur * p.buf_stride + ((2 * t_wy) * TC + 16 * t_tc) * PS);
#pragma unroll
                for (int tap = 0; tap < 9; tap++) fa[tap] = kq[tap] + tbase;
            } else {
                const int win = min(tile * 8 + (m >> 2), nwin - 1);
                const int wy = fdiv(win, p.mWp), wx = win - wy * p.Wp;
                yy0 = 2 * wy + ((m >> 1) & 1); xx0 = 2 * wx + (m & 1);
            }
            // TPAR T-slices are accumulated at a time (register budget); the pooled values of all
            // four slices are kept for the temporal MLP.
            half4 pb4[4];   // the pooled values of window g, T = 0..3, already as the temporal MLP's fp16 operand
            // The A fragments come through a ring of AD registers, AD MFMAs ahead of their use, across taps and across the
            // T groups; pin_ring (below the loop) pins that issue order.
            constexpr int NSG = 9 * KC * TPAR;            // MFMAs per T group
            constexpr int NS = NSG * (BN_T / TPAR);       // MFMAs per tile
            auto frag = [&](int s) -> half8 {
                const int grp = s / NSG, r = s % NSG;
                const int tap = r / (KC * TPAR), kc = (r / TPAR) % KC, t = r % TPAR;
                if constexpr (TSZ > 0) {
                    const uint8_t *a = smem + (fa[tap] ^ (uint32_t)(kc << 5));
                    return *reinterpret_cast<const half8 *>(__builtin_assume_aligned(a + (grp * TPAR + t) * TSZ, 16));
                }
                const int yy = yy0 + tap / 3, xx = xx0 + tap % 3;
                const int pbase = (yy * TC + xx) * PS;
                const int sw = swz_eval<CPP>(p.swz, xx, yy);
                return *reinterpret_cast<const half8 *>(bandp + (grp * TPAR + t) * tsz + pbase + (((kc * 2 + kh) ^ sw) * 16));
            };
            if constexpr (AD > 0) {
                half8 ab[AD > 0 ? AD : 1];
#pragma unroll
                for (int s = 0; s < AD; s++) ab[s] = frag(s);
                f32x16 acc[TPAR];
#pragma unroll
                for (int s = 0; s < NS; s++) {
                    const int grp = s / NSG, r = s % NSG, t = r % TPAR;
                    if (r < TPAR) {
#pragma unroll
                        for (int q = 0; q < 16; q++) acc[t][q] = 0.f;
                    }
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ab[s % AD], bf[r / TPAR], acc[t], 0, 0, 0);
                    if (s + AD < NS) ab[s % AD] = frag(s + AD);
                    if (r == NSG - 1) {
                        // reg q -> row (q&3) + 8*(q>>2) + 4*kh -> window 2*(q>>2)+kh, position q&3
#pragma unroll
                        for (int tt = 0; tt < TPAR; tt++)
#pragma unroll
                            for (int g = 0; g < 4; g++)
                                pb4[g][grp * TPAR + tt] = (_Float16)pool4<ALLPOS>(acc[tt][4 * g], acc[tt][4 * g + 1], acc[tt][4 * g + 2],
                                                                                  acc[tt][4 * g + 3], e0, e1, e2);
                    }
                }
                // pin_ring<NS, AD>(), written out: called as the function, this kernel's register allocation comes out differently
                __builtin_amdgcn_sched_group_barrier(0x100, AD, 0);
#pragma unroll
                for (int s = 0; s < NS; s++) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    if (s + AD < NS) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                }
            } else {
                // (level 3: 144 weight registers leave no room for a ring; the compiler's own order, one fragment at a time)
#pragma unroll
                for (int grp = 0; grp < BN_T / TPAR; grp++) {
                    f32x16 acc[TPAR];
#pragma unroll
                    for (int t = 0; t < TPAR; t++)
#pragma unroll
                        for (int q = 0; q < 16; q++) acc[t][q] = 0.f;
#pragma unroll
                    for (int ky = 0; ky < 3; ky++)
#pragma unroll
                        for (int kx = 0; kx < 3; kx++) {
                            const int yy = yy0 + ky, xx = xx0 + kx;
                            const int pbase = (yy * TC + xx) * PS;
                            const int sw = swz_eval<CPP>(p.swz, xx, yy);
#pragma unroll
                            for (int kc = 0; kc < KC; kc++) {
                                const int off = TSZ > 0 ? 0 : pbase + (((kc * 2 + kh) ^ sw) * 16);
#pragma unroll
                                for (int t = 0; t < TPAR; t++) {
                                    const uint8_t *ap = TSZ > 0 ? smem + ((fa[ky * 3 + kx] + (uint32_t)(grp * TPAR * TSZ)) ^ (uint32_t)(kc << 5)) + t * TSZ
                                                                : bandp + (grp * TPAR + t) * tsz + off;
                                    const half8 a = *reinterpret_cast<const half8 *>(__builtin_assume_aligned(ap, 16));
                                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bf[(ky * 3 + kx) * KC + kc], acc[t], 0, 0, 0);
                                }
                            }
                        }
#pragma unroll
                    for (int tt = 0; tt < TPAR; tt++)
#pragma unroll
                        for (int g = 0; g < 4; g++)
                            pb4[g][grp * TPAR + tt] = (_Float16)pool4<ALLPOS>(acc[tt][4 * g], acc[tt][4 * g + 1], acc[tt][4 * g + 2],
                                                                              acc[tt][4 * g + 3], e0, e1, e2);
                }
            }
            // Materialise the pooled values here (empty asm = opaque use): the accumulators die before the epilogue
            // starts.  Without this point hipcc interleaves the pooling of later T-slices with the epilogue and the
            // 64->128 level spills >150 registers.
#pragma unroll
            for (int g = 0; g < 4; g++) {
                typedef int i32x2 __attribute__((ext_vector_type(2)));
                i32x2 bits = __builtin_bit_cast(i32x2, pb4[g]);
                asm volatile("" : "+v"(bits));
                pb4[g] = __builtin_bit_cast(half4, bits);
            }
            PHASE_MARK(6);   // tiles: matrix part (A fragments, MFMAs, pooling)
            landed();
            // ---- epilogue: temporal MLP + residual per pooled window, then store
            const uint32_t tstride = (uint32_t)(p.Ho * p.Wo * COUT);
            // the last level feeds the decoder, which takes T = 0 only (To == 1 there; the host sets it so): a constant
            // lets the other three outputs of the temporal MLP and their stores fall away at compile time
            const int To = COUT == 128 ? 1 : p.To;
            __half *const ob = p.out + (size_t)b * To * tstride;   // wave-uniform; lanes add a 32-bit offset
            {
                // wave-private LDS transpose: lanes drop their fp16 values as S[t][window][32 channels] into the wave's 2 KB of
                // scratch and take them back as two 16-byte pieces per lane -> two global_store_dwordx4 per tile instead of
                // sixteen 2-byte stores
                uint8_t *const scr = smem + p.scr_off + wave * 2048;
                half4 o4[4];
                if constexpr (CIN == 64) {   // 144 weight registers: one element at a time
#pragma unroll
                    for (int g = 0; g < 4; g++) tmix4h(tm, pb4[g], o4[g]);
                } else {
                    tmix4h<4>(tm, pb4, o4);
                }
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    _Float16 *sw = reinterpret_cast<_Float16 *>(scr + (2 * g + kh) * 64) + (ll & 31);
#pragma unroll
                    for (int t = 0; t < BN_T; t++) sw[t * 256] = o4[g][t];
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                const int owin = TSZ > 0 ? 8 * t_tc + ((ll >> 2) & 7) : tile * 8 + ((ll >> 2) & 7);   // TSZ > 0: window within its row
                if (owin < (TSZ > 0 ? p.Wp : nwin)) {
                    const int owy = TSZ > 0 ? t_wy : (int)fdiv(owin, p.mWp), owx = TSZ > 0 ? owin : owin - owy * p.Wp;
                    const int gy = y0 / 2 + owy + p.oy, gx = owx + p.ox;
                    const uint32_t eo = (uint32_t)((gy * p.Wo + gx) * COUT + ntile * 32 + 8 * (ll & 3));
#pragma unroll
                    for (int j = 0; j < 2; j++) {
                        const int t = 2 * j + (ll >> 5);
                        if (t < To) {
                            const uint4 v = *reinterpret_cast<const uint4 *>(scr + (j * 64 + ll) * 16);
                            *reinterpret_cast<uint4 *>(ob + t * tstride + eo) = v;
                        }
                    }
                }
            }
            PHASE_MARK(7);   // tiles: epilogue (temporal MLP, transpose, stores)
        }
        landed();   // a wave without a tile in this item
        PHASE_MARK(6);
#ifdef WGSPAN_ONLY
        ITEM_MARK(3);
        it_n_++;
#endif
    }
#ifdef WGSPAN_ONLY
    if (tid == 0 && blockIdx.x < 1024)
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 4; j++) g_itemspan[COUT == 32 ? 0 : COUT == 64 ? 1 : 2][blockIdx.x][i][j] = it_t_[i][j];
#endif
#ifdef PHASE_TIMING
#ifndef PHASE_WAVE
#define PHASE_WAVE 0
#endif
    if (tid == 64 * (PHASE_WAVE < 0 ? NWV + PHASE_WAVE : PHASE_WAVE))
        for (int i = 0; i < 9; i++) atomicAdd(&g_phase[i + (PRE ? 0 : COUT == 64 ? 16 : COUT == 128 ? 32 : 48)], ph_[i]);
#endif
    WGSPAN_END(COUT == 32 ? 0 : COUT == 64 ? 1 : 2);
}

// ------------------------------------------------------------------ enc level 1 on 16-position tiles (round 4)
// conv3x3 16 -> 32 on v_mfma_f32_16x16x32_f16: tiles of 4 pool windows x 4 positions (M = 16), a wave owns both
// 16-channel N tiles of its tile; one K step = TWO taps x 16 input channels, five K steps (the tenth tap carries zero
// weights).  Eight waves per workgroup (40 weight + 16 accumulator + 16 ring registers: 128 per lane), two workgroups
// per CU.  Against enc_mfma<16,32> (32x32x16 products, swizzled band, LDS-DMA; kept for grids wider than this kernel's
// fixed LDS row and as the A/B partner, covahip_blobnet_set_impl(ctx, 5)):
//   * LDS band: [T][row][pixel][16 ch] with a FIXED row stride of E1_RS bytes == 128 mod 256 -- with the 16x16 lane map
//     (lane = 16 * (tap-of-the-pair, channel half) + position) every ds_read_b128 lane group then covers all 64 banks
//     once, without a swizzle.  No swizzle means the address of every fragment of a tile is ONE per-lane base plus a
//     compile-time constant (tap, T slice): twenty ds_read_b128 with immediate offsets, no address arithmetic between
//     the products (the swizzled form spends seven vector instructions per tap), and every fragment feeds two products;
//   * staging through registers (global_load -> temporal MLP of the level below -> ds_write_b128): every piece goes
//     through the vector ALU anyway, the T = 0 result leaves for the skip tensor straight from the registers, and a
//     kernel without LDS-DMA keeps hipcc from draining the vector-memory counter in front of LDS reads (it does that in
//     every kernel that has one: an LDS-DMA is a pending LDS write).  The loads of an item are issued BEFORE the barrier
//     that ends the previous item;
//   * tiles of 16 positions: 23 per three-row band over 8 waves (3 + 3 + ... + 2) where 32-position tiles gave 12 over 8.
// Measured on one box (HIP events, b = 256, 68x120): 32.0 us against 36.1 for enc_mfma<16,32,PRE>; a form with sixteen
// waves of 16 channels each (64 registers, eight waves per SIMD -- the candidate round 3 named) 34.6: it reads every
// fragment for ONE product and needs the LDS array's full 256 B/clk to keep the matrix pipe busy.
// Reference semantics: encoder.py:58-80 (conv -> ReLU -> BN -> pool -> pad -> PointWiseTN), pointwise.py:16-26.
// T-slice strides of the row-aligned forms of levels 2 and 3 (enc_mfma<.., TSZ>): the 1080p bands exactly (8 rows x 32 pixels x
// 64 B; 12 rows x 17 pixels x 128 B); smaller bands leave the tail of a slice unused
constexpr int E2_TSZ = 16384, E3_TSZ = 26112;
constexpr int E1_RS = 2176;              // bytes per band row: 66 pixels x 32 B + 64 B, == 128 mod 256
constexpr int E1_TR = 8;                 // band rows per T slice (three pool-window rows + halo)
constexpr int E1_TSZ = E1_RS * E1_TR;    // bytes per T slice
constexpr int E1_MAXW = BN_E1_MAXW;      // (62) 8 rows x 2 (W + 2) pieces <= 2 pieces per thread; (W + 2) * 32 + 32 <= E1_RS (the
                                         // zero-weight tap of the last K step reads one pixel past the row)
static_assert(8 * 2 * (E1_MAXW + 2) <= 2 * 512 && (E1_MAXW + 2) * 32 + 32 <= E1_RS, "enc1_mfma's staging / row limits");
struct Enc1Args {
    const __half *in;    // P [F][H][W][16]: pooled level-0 values per carrier frame (enc0p_mfma)
    __half *out;         // [B][T][Ho][Wo][32]
    const half8 *wfrag;  // [2 N tiles][5 K steps][64 lanes]
    const float *epi;    // e0[32], e1[32], e2[32] (pool4), w1[16], w2[16]
    int B, H, W, Hp, Wp, Ho, Wo, oy, ox;
    int nbands;
    uint32_t mWp, mRC;   // magic of Wp and of 2 * (W + 2)
    int scr_off;         // per-wave store scratch (1 KB per wave) behind the band
    ItemPlan plan;
    const int32_t *pidx; // frames of the T = 0..3 slices of every stack; null: stack b = frames 4b .. 4b+3 (stacked entry)
    __half *skip;        // [B][T][H][W][16], T = 0 written (the decoder's skip input)
    const float *tm_pre; // w1[16], w2[16] of the level below
    // the stack table BY VALUE (use_ktab): frames of stack b = ktab[4b .. 4b+3]; read from the kernel-argument segment with
    // scalar loads.  A table that changes from call to call then costs no copy in front of the kernels.
    int use_ktab;
    // the level-0 skip connection's share of the LOGITS (round 5): the last decoder block is linear in its concatenated input
    // (convT of concat(up, skip) = convT_up(up) + convT_skip(skip), decoder.py:122-134, no non-linearity up to the final 1x1
    // conv), and its skip half is exactly the T = 0 slice this kernel has just computed and holds in LDS.  part != null: the
    // kernel runs that half (folded with the final conv: 16 channels x 4 taps -> 4 output parities per grid position) on its
    // band and writes fp32 partial logits -- four per grid position of the transposed convolution (its 2 x 2 output pixels), laid
    // out [B][H + 1][W + 1][4] exactly as the last block's own tiles walk them: 34 KB per frame instead of the 65 KB skip slice,
    // which then is neither written here nor read by the decoder tail (33 MB per step at b = 256).  One unconditional 16-byte
    // store per position (a first form wrote [Hd][Wd] pixels: sixteen masked 4-byte stores per tile, 500 instructions per item).
    float *part;
    const half8 *wtail;  // [2 K steps][64 lanes]: A fragments of the folded skip half (prep_tail)
    uint32_t mXe;        // magic of 2 * Wp (columns of the grid rows the edge pass walks)
    uint16_t ktab[BN_KTAB_STACKS * BN_T];
    const uint8_t *model_ids;   // MS: model id per stack [B]
    uint32_t mstride;     // MS: bytes between two models' prepared weights
};
// Per-lane constants live in a small LDS table behind the scratch instead of registers (hipcc keeps every loop-invariant
// load in a register for the whole kernel):
//   [0, 384)    e0[32], e1[32], e2[32]                      (pool4)
//   [384, 448)  this level's temporal MLP: rows lane % 4 of W1^T and W2^T as fp16 (TmixW::a1, a2), 16 B per lane % 4
//   [448, 512)  the same for the level below
//   [512, 2560) the folded skip half of the last decoder block (Enc1Args::wtail): 2 K steps x 64 lanes x 16 B
constexpr int E1_CONST = 2560;
#ifndef E1_ABL
#define E1_ABL 0   // developer builds (tools/ablate_enc1.sh): 1 no temporal MLP, 3 no tile epilogue, 4 no tiles, 5 no staging
#endif
template <bool ALLPOS, bool MS = false>
__global__ __launch_bounds__(512, 4) void enc1_mfma(Enc1Args p) {
    constexpr int NWV = 8, WGS = NWV * 64, MG = NWV;
    constexpr int AD = 4;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    WGSPAN_BEGIN();
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < BN_T * E1_TSZ / 16; i += WGS) *reinterpret_cast<uint4 *>(smem + i * 16) = make_uint4(0, 0, 0, 0);
    uint8_t *const cst = smem + p.scr_off + NWV * 1024;
    if (tid < 96) reinterpret_cast<float *>(cst)[tid] = p.epi[tid];
    if (p.part && tid >= 256 && tid < 384) reinterpret_cast<half8 *>(cst + 512)[tid - 256] = p.wtail[tid - 256];
    if (tid >= 128 && tid < 136) {
        const int i = tid & 3;
        const float *tmw = (tid & 4) ? p.tm_pre : p.epi + 96;
        {
            half4 a1, a2;
#pragma unroll
            for (int t = 0; t < BN_T; t++) { a1[t] = (_Float16)tmw[t * BN_T + i]; a2[t] = (_Float16)tmw[16 + t * BN_T + i]; }
            *reinterpret_cast<half4 *>(cst + 384 + (tid & 4) * 16 + i * 16) = a1;
            *reinterpret_cast<half4 *>(cst + 384 + (tid & 4) * 16 + i * 16 + 8) = a2;
        }
    }
    // MS: the same table of the model `mo` bytes past model 0, rewritten between two barriers when the stack's model changes
    [[maybe_unused]] auto load_cst = [&](uint32_t mo) {
        const float *epi = at_model(p.epi, mo);
        if (tid < 96) reinterpret_cast<float *>(cst)[tid] = epi[tid];
        if (p.part && tid >= 256 && tid < 384) reinterpret_cast<half8 *>(cst + 512)[tid - 256] = at_model(p.wtail, mo)[tid - 256];
        if (tid >= 128 && tid < 136) {
            const int i = tid & 3;
            const float *tmw = (tid & 4) ? at_model(p.tm_pre, mo) : epi + 96;
            half4 a1, a2;
#pragma unroll
            for (int t = 0; t < BN_T; t++) { a1[t] = (_Float16)tmw[t * BN_T + i]; a2[t] = (_Float16)tmw[16 + t * BN_T + i]; }
            *reinterpret_cast<half4 *>(cst + 384 + (tid & 4) * 16 + i * 16) = a1;
            *reinterpret_cast<half4 *>(cst + 384 + (tid & 4) * 16 + i * 16 + 8) = a2;
        }
    };
    [[maybe_unused]] uint32_t moff_cur = 0;
    const int RCr = 2 * (p.W + 2);
    const uint32_t plane = (uint32_t)p.H * p.W * 32;
#ifdef PHASE_TIMING
    unsigned long long ph_[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, last_ = __builtin_amdgcn_s_memrealtime();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif

    ItemIter it;
    for (bool more = it.start(p.plan, p.B, p.nbands); more; more = it.next(p.plan, p.B, p.nbands)) {
        const int b = it.b, band = it.band;
        [[maybe_unused]] const uint32_t moff = model_off<MS>(p.model_ids, p.mstride, b);
        if constexpr (MS) {   // uniform branch (the item is the workgroup's): every wave has left the previous item before the table changes
            if (moff != moff_cur) {
                moff_cur = moff;
                lds_barrier();
                load_cst(moff);
                lds_barrier();
            }
        }
        const int y0 = 2 * ((band * p.Hp) / p.nbands);
        const int rows = 2 * (((band + 1) * p.Hp) / p.nbands) - y0;
        const int n2 = rows + 2;
        auto lane_id = []() -> int {
            uint32_t zero = 0;
            asm volatile("" : "+v"(zero));
            return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, zero));
        };
        const int ll = lane_id();
        // frames of the stack's T = 0..3 slices: a SCALAR load (constant address space; the table is uploaded before the
        // launch and never written by a kernel); the stacked entry's frames are 4b .. 4b+3
        int fidx[BN_T] = {BN_T * b, BN_T * b + 1, BN_T * b + 2, BN_T * b + 3};
        const uint8_t *const fbase = reinterpret_cast<const uint8_t *>(p.in);
        if (p.use_ktab) {
            typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
            typedef const __attribute__((address_space(4))) u32x2 *const_u32x2_ptr;
            const __attribute__((address_space(4))) uint8_t *ka = (const __attribute__((address_space(4))) uint8_t *)__builtin_amdgcn_kernarg_segment_ptr();
            const u32x2 row = *(const_u32x2_ptr)(ka + offsetof(Enc1Args, ktab) + (size_t)b * 8);
            fidx[0] = row[0] & 0xFFFF; fidx[1] = row[0] >> 16; fidx[2] = row[1] & 0xFFFF; fidx[3] = row[1] >> 16;
        } else if (p.pidx) {
            typedef int i32x4 __attribute__((ext_vector_type(4)));
            typedef const __attribute__((address_space(4))) i32x4 *const_i32x4_ptr;
            const i32x4 row = *(const_i32x4_ptr)(uintptr_t)(p.pidx + b * BN_T);
            fidx[0] = row[0]; fidx[1] = row[1]; fidx[2] = row[2]; fidx[3] = row[3];
        }
        const int ya = y0, yb = (band == p.nbands - 1) ? p.H : y0 + rows;
        const int nreal = n2 * RCr;
        // ---- stage: two 16-byte pieces of all four T slices per thread (the host keeps 8 * RCr <= 2 * WGS), loads in flight
        // across the barrier
        half8 v[2][BN_T];
        int dst[2];
        uint32_t eoff[2];
        bool inb[2], have[2], own[2];
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int i = wave * 64 + ll + k * WGS;
            const int ic = min(i, nreal - 1);
            const int r = fdiv(ic, p.mRC), within = ic - r * RCr;
            const int c = within >> 1, hf = within & 1;
            const int y = y0 - 1 + r, x = c - 1;
            inb[k] = y >= 0 && y < p.H && x >= 0 && x < p.W;
            dst[k] = r * E1_RS + c * 32 + hf * 16;
            eoff[k] = (uint32_t)((min(max(y, 0), p.H - 1) * p.W + min(max(x, 0), p.W - 1)) * 32 + hf * 16);
            have[k] = (E1_ABL != 5) && i < nreal;
            own[k] = have[k] && inb[k] && y >= ya && y < yb;
#pragma unroll
            for (int t = 0; t < BN_T; t++) {
                const uint64_t fo = (uint64_t)(uint32_t)fidx[t] * plane;
                const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)fo), hi = __builtin_amdgcn_readfirstlane((uint32_t)(fo >> 32));
                v[k][t] = *reinterpret_cast<const half8 *>(fbase + (((uint64_t)hi << 32) | lo) + eoff[k]);
            }
        }
        PHASE_MARK(0);   // item bookkeeping, addresses, loads issued
        lds_barrier();   // every wave has left the previous item's band
        PHASE_MARK(1);   // barrier: the other waves finishing the previous item
#ifdef PHASE_TIMING
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        PHASE_MARK(2);   // loads landing
#endif
#pragma unroll
        for (int k = 0; k < 2; k++) {
            if (!inb[k]) {
#pragma unroll
                for (int t = 0; t < BN_T; t++)
#pragma unroll
                    for (int j = 0; j < 8; j++) v[k][t][j] = (_Float16)0;
            }
            if constexpr (E1_ABL != 1 && E1_ABL != 5) {
                TmixW tmp;
                {
                    const uint4 w = *reinterpret_cast<const uint4 *>(cst + 448 + (ll & 3) * 16);
                    tmp.a1 = __builtin_bit_cast(half4, make_uint2(w.x, w.y));
                    tmp.a2 = __builtin_bit_cast(half4, make_uint2(w.z, w.w));
#pragma unroll
                    for (int t = 0; t < BN_T; t++) tmp.id[t] = (_Float16)(t == (ll & 3) ? 1.f : 0.f);
                }
                half8 o[BN_T];
#pragma unroll
                for (int j0 = 0; j0 < 8; j0 += 4) {
                    half4 pb[4];
                    f32x4 rr[4];
#pragma unroll
                    for (int j = 0; j < 4; j++) pb[j] = half4{v[k][0][j0 + j], v[k][1][j0 + j], v[k][2][j0 + j], v[k][3][j0 + j]};
                    tmix4f<4>(tmp, pb, rr);
#pragma unroll
                    for (int j = 0; j < 4; j++)
#pragma unroll
                        for (int t = 0; t < BN_T; t++) o[t][j0 + j] = (_Float16)rr[j][t];
                }
                if (have[k]) {
#pragma unroll
                    for (int t = 0; t < BN_T; t++) *reinterpret_cast<half8 *>(smem + t * E1_TSZ + dst[k]) = o[t];
                }
                if (own[k] && !p.part) *reinterpret_cast<half8 *>(reinterpret_cast<uint8_t *>(p.skip) + (size_t)b * BN_T * plane + eoff[k]) = o[0];
            } else {
                if (have[k]) {
#pragma unroll
                    for (int t = 0; t < BN_T; t++) *reinterpret_cast<half8 *>(smem + t * E1_TSZ + dst[k]) = v[k][t];
                }
            }
        }
        PHASE_MARK(3);   // temporal MLP, LDS writes, skip stores
        // weight fragments of both N tiles, (re)loaded per item (the temporal MLP needs the registers)
        half8 bf[2][5];
        {
            const half8 *wp = (MS ? at_model(p.wfrag, moff) : p.wfrag) + ll;
            asm volatile("" : "+v"(wp));
            const gptr<half8> wg = as_global(wp);
#pragma unroll
            for (int nt = 0; nt < 2; nt++)
#pragma unroll
                for (int s = 0; s < 5; s++) bf[nt][s] = wg[(nt * 5 + s) * 64];
        }
        lds_barrier();   // the band is complete
        PHASE_MARK(4);   // barrier: the band complete
#ifdef PHASE_TIMING
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        PHASE_MARK(5);   // weights landing
#endif
        const int m = ll & 15, kg = ll >> 4;
        const bool ride = p.part != nullptr;
        const int nwin = (rows / 2) * p.Wp;
        const int ntiles = (nwin + 3) / 4;
        const uint32_t tstride = (uint32_t)(p.Ho * p.Wo * 32);
        __half *const ob = p.out + (size_t)b * BN_T * tstride;
        uint8_t *const scr = smem + p.scr_off + wave * 1024;
        // ---- the skip half of the last decoder block on this band's T = 0 slice (see Enc1Args::part), IN FRONT of the tile loop:
        // behind it the phase's first LDS read sat behind `s_waitcnt vmcnt(0)` = the acknowledgement of the tile epilogues' stores
        // (2.2 us per item, measured with the phase clock); here the only outstanding vector-memory operations are the weight
        // fragments the tile loop waits for anyway.: grid rows u = ya .. yb - 1
        // (the last band: + the row behind the image) x W + 1 columns, tiles of 16 positions, transposed (A = weights, B =
        // activations: a lane < 16 ends up with the four parities of ITS position = a 2 x 2 block of output pixels).
        // out[2u + py - cy][2v + px - cx] += sum_{a, b, c} skip[u - a][v - b][c] * w[py + 2a][px + 2b][c]
        // Partial logits (see Enc1Args::part).  The grid positions (u, v) = (y, x) that ARE positions of the main convolution ride on
        // its tiles: K steps 0 and 1 of a tile's T = 0 slice hold exactly the four taps (u - a, v - bb) the folded skip half needs
        // (rows y - 1, y; columns x - 1, x), so two more products per tile -- weights as the B operand, the fragments the tile has in
        // registers anyway -- give four parities x sixteen positions.  What no tile covers is done here, IN FRONT of the tile loop:
        // the grid column(s) behind the last pooled column and, in the last band, the grid row(s) behind the last pooled row -- 6 of a
        // band's 366 positions, 65 in the last band.  (Behind the tile loop the phase's first LDS read sat behind `s_waitcnt
        // vmcnt(0)` = the acknowledgement of the tile epilogues' stores, 2.2 us per item; here the only outstanding vector-memory
        // operations are the weight fragments the tile loop waits for anyway.  The first form of this pass covered EVERY position:
        // ~85 instructions per wave and item on an issue port that is 88 % busy, +2.0 us per launch.)
        const int GW = p.W + 1;
        f32x4 *const pb4 = reinterpret_cast<f32x4 *>(p.part) + (size_t)b * (p.H + 1) * GW;
        if (p.part) {
            const int ub = (band == p.nbands - 1) ? p.H + 1 : yb;
            const int xe = 2 * p.Wp, ce = GW - xe;                  // edge columns xe .. W (one of them: W is even)
            const int ne1 = (ub - ya) * ce;                          // ... of every grid row of the band
            const int ne2 = max(0, ub - (y0 + rows)) * xe;           // + the grid rows behind the last pooled row, columns 0 .. xe - 1
            const int npos = ne1 + ne2;
            const int nptiles = (npos + 15) / 16;
            if (wave < nptiles) {
                const half8 w0 = *reinterpret_cast<const half8 *>(cst + 512 + ll * 16), w1 = *reinterpret_cast<const half8 *>(cst + 1536 + ll * 16);
                for (int pt = wave; pt < nptiles; pt += MG) {
                    const int q = pt * 16 + m;
                    const int qc = min(q, npos - 1);
                    int u, v;
                    if (qc < ne1) {
                        const int ul = ce == 1 ? qc : qc >> 1;
                        u = ya + ul; v = xe + (qc - ul * ce);
                    } else {
                        const int q2 = qc - ne1, ul = fdiv(q2, p.mXe);
                        u = y0 + rows + ul; v = q2 - ul * xe;
                    }
                    // K step 0 = input row u - 1 (band row u - y0), K step 1 = row u; lane group kg: column v - 1 + (kg >> 1) (band
                    // column v + (kg >> 1)), channel half kg & 1.  A row behind the image that the band does not hold (odd H: the
                    // row of u = H) is read from the band's first halo pixel instead, which is zero
                    const int o1 = (u - y0) * E1_RS + (v + (kg >> 1)) * 32 + (kg & 1) * 16;
                    const int o0 = u >= p.H ? 0 : o1 + E1_RS;
                    const half8 b1 = *reinterpret_cast<const half8 *>(__builtin_assume_aligned(smem + o1, 16));
                    const half8 b0 = *reinterpret_cast<const half8 *>(__builtin_assume_aligned(smem + o0, 16));
                    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
                    f32x4 pe = __builtin_amdgcn_mfma_f32_16x16x32_f16(w0, b1, z4, 0, 0, 0);       // weights as A: a lane < 16 gets the four
                    pe = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1, b0, pe, 0, 0, 0);             // parities of ITS position
                    if (kg == 0 && q < npos) pb4[u * GW + v] = pe;
                }
            }
            PHASE_MARK(8);   // partial logits: the positions no tile covers
        }
        for (int tile = wave; tile < (E1_ABL == 4 ? 0 : ntiles); tile += MG) {
            const int win = min(tile * 4 + (m >> 2), nwin - 1);
            const int wy = fdiv(win, p.mWp), wx = win - wy * p.Wp;
            const int yy0 = 2 * wy + ((m >> 1) & 1), xx0 = 2 * wx + (m & 1);
            const int base = yy0 * E1_RS + xx0 * 32 + (kg & 1) * 16;
            const uint8_t *const aH = smem + base + (kg >> 1) * 32, *const aV = smem + base + (kg >> 1) * E1_RS;
            auto frag = [&](int idx) -> half8 {
                const int s = (idx % 10) >> 1, t = 2 * (idx / 10) + (idx & 1);
                const uint8_t *a = s == 3 ? aV + 64 : s == 4 ? aH + 2 * E1_RS + 64 : aH + s * E1_RS;
                return *reinterpret_cast<const half8 *>(__builtin_assume_aligned(a + t * E1_TSZ, 16));
            };
            half8 ab[AD];
#pragma unroll
            for (int k = 0; k < AD; k++) ab[k] = frag(k);
            const float *cf = reinterpret_cast<const float *>(cst);
            float e0[2], e1[2], e2[2];
#pragma unroll
            for (int nt = 0; nt < 2; nt++) {
                e0[nt] = cf[nt * 16 + m]; e1[nt] = cf[32 + nt * 16 + m];
                e2[nt] = ALLPOS ? 0.f : cf[64 + nt * 16 + m];
            }
            const uint4 tw = *reinterpret_cast<const uint4 *>(cst + 384 + (m & 3) * 16);
            f32x4 acc[2][2];
            f32x4 pooled[2];
            const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
            f32x4 pride = z4;        // partial logits of the tile's sixteen positions, parity = lane & 15 (< 4)
#pragma unroll
            for (int k = 0; k < 20; k++) {
                const int s = (k % 10) >> 1, tp = k & 1;
#pragma unroll
                for (int nt = 0; nt < 2; nt++)
                    acc[nt][tp] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ab[k % AD], bf[nt][s], s == 0 ? z4 : acc[nt][tp], 0, 0, 0);
                if ((k == 0 || k == 2) && ride)   // T = 0, K steps 0 and 1: the fragment in ab[] is the one the folded skip half needs
                    pride = __builtin_amdgcn_mfma_f32_16x16x32_f16(ab[k % AD], *reinterpret_cast<const half8 *>(cst + 512 + (k >> 1) * 1024 + ll * 16),
                                                                   pride, 0, 0, 0);
                if (k + AD < 20) ab[k % AD] = frag(k + AD);
#if E1_ABL == 3
                if (s == 4) asm volatile("" :: "v"(acc[0][tp]), "v"(acc[1][tp]));
                if (false) {
#else
                if (s == 4) {
#endif
#pragma unroll
                    for (int nt = 0; nt < 2; nt++) {
                        float pv = pool4<ALLPOS>(acc[nt][tp][0], acc[nt][tp][1], acc[nt][tp][2], acc[nt][tp][3], e0[nt], e1[nt], e2[nt]);
                        asm volatile("" : "+v"(pv));   // one rounding point (fp32, then fp16) whatever the instantiation
                        pooled[nt][2 * (k / 10) + tp] = pv;
                    }
                }
            }
            pin_ring<20, AD, 2>();   // (two products per fragment)
#if E1_ABL == 3
            asm volatile("" :: "v"(tw.x), "v"(e0[0]), "v"(e1[0]), "v"(e0[1]), "v"(e1[1]));
            continue;
#endif
#ifdef PHASE_TIMING
            asm volatile("" : "+v"(pooled[0]), "+v"(pooled[1]));
            PHASE_MARK(6);   // tiles: fragments, products, pooling
#endif
            TmixW tm;
            tm.a1 = __builtin_bit_cast(half4, make_uint2(tw.x, tw.y));
            tm.a2 = __builtin_bit_cast(half4, make_uint2(tw.z, tw.w));
#pragma unroll
            for (int t = 0; t < BN_T; t++) tm.id[t] = (_Float16)(t == (m & 3) ? 1.f : 0.f);
            half4 pb2[2], o2[2];
#pragma unroll
            for (int nt = 0; nt < 2; nt++) pb2[nt] = __builtin_convertvector(pooled[nt], half4);
            tmix4h<2>(tm, pb2, o2);
            // ---- store through a wave-private transpose: S[window][t][32 channels] (64 contiguous bytes per window and T slice
            // in the output tensor); lane (window kg, m) then moves the 16 bytes (t = m >> 2, quarter m & 3) of ITS window
#pragma unroll
            for (int nt = 0; nt < 2; nt++) {
                _Float16 *sw = reinterpret_cast<_Float16 *>(scr + kg * 256) + nt * 16 + m;
#pragma unroll
                for (int t = 0; t < BN_T; t++) sw[t * 32] = o2[nt][t];
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const int owin = tile * 4 + kg;
            const uint4 sv = *reinterpret_cast<const uint4 *>(scr + ll * 16);   // = kg * 256 + (m >> 2) * 64 + (m & 3) * 16
            if (owin < nwin) {
                const int owy = fdiv(owin, p.mWp), owx = owin - owy * p.Wp;
                const int gy = y0 / 2 + owy + p.oy, gx = owx + p.ox;
                const uint32_t eo = (uint32_t)((gy * p.Wo + gx) * 32 + 8 * (m & 3));
                *reinterpret_cast<uint4 *>(ob + (m >> 2) * tstride + eo) = sv;
                // the ride's results: D rows 4 kg + r = position r of window kg, column m = parity -> float m of the position's four
                if (ride && m < 4) {
                    float *const pw = reinterpret_cast<float *>(pb4 + (y0 + 2 * owy) * GW + 2 * owx) + m;
                    pw[0] = pride[0]; pw[4] = pride[1]; pw[4 * GW] = pride[2]; pw[4 * GW + 4] = pride[3];
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            PHASE_MARK(7);   // tiles: epilogue
        }
    }
#ifdef PHASE_TIMING
    if (tid == 64 * (PHASE_WAVE < 0 ? NWV + PHASE_WAVE : PHASE_WAVE))
        for (int i = 0; i < 9; i++) atomicAdd(&g_phase[i], ph_[i]);
#endif
    WGSPAN_END(0);
}

// ------------------------------------------------------------------ enc levels 2 + 3 in one launch (round 5)
// One eight-wave workgroup takes a frame through level 2 AND level 3.  A frame's level-2 output (4 x 9 x 15 x 64 fp16 at
// 1080p, 69 KB) IS level 3's input band, so it is written -- after level 2's temporal MLP -- straight into that band in LDS,
// with the band's swizzle, and never crosses the fabric; only its T = 0 slice leaves for HBM (the decoder's skip input,
// blobnet.py:32).  Against the two launches (enc_mfma<32,64,..,E2_TSZ> + enc_mfma<64,128,..,E3_TSZ>):
//   * level 2's input streams through a RING of six input rows per T slice (48 KB): the step of window row s computes on
//     rows 2s-1 .. 2s+2 while the LDS-DMA of rows 2s+3, 2s+4 lands in the two slots step s-1 has left -- the request +
//     landing of a band (2.5 - 3.7 us per item in the two-launch form, serial in front of its tiles) is off the critical path;
//   * a window row of level 2 is two tile columns x two N tiles = four 32x32 tiles for eight waves, so a wave takes a tile
//     and HALF of its T slices (T-half th = wave >> 2: 36 products instead of 72, 32 accumulator registers), the two waves
//     of a tile swap their pooled values through LDS (8 bytes per lane each way) and each runs the temporal MLP for half of
//     the tile's windows: every wave has work in every step, one frame per CU, no second round of items;
//   * level 3 starts on a band that is already in LDS (the two-launch form: 3 us of landing per frame), its weights are
//     requested while the T = 0 slice of level 2 is copied out.
// Same products in the same order per accumulator, same pooling / rounding / MLP expressions: bit-identical to the two
// launches (tests/test_gpu_blobnet.py).  Reference semantics: encoder.py:58-80, pointwise.py:16-26.
constexpr int E23_RP2 = 2048;                     // ring row pitch per T slice: 32 pixels x 64 B
constexpr int E23_NSLOT = 6;                      // ring rows per T slice
constexpr int E23_TSZ2 = E23_NSLOT * E23_RP2;     // bytes per T slice of the ring
struct Enc23Args {
    const __half *in;    // act[2] [B][T][H2][W2][32]
    __half *mid;         // act[3] [B][T][H3][W3][64]: only T = 0 is written (decoder skip)
    __half *out;         // act[4] [B][1][H4][W4][128]
    const half8 *wf2, *wf3;
    const float *epi2, *epi3;
    int B;
    int H2, W2, Hp2, Wp2;
    int H3, W3, Hp3, Wp3, oy3, ox3;   // level 3's input = level 2's pooled output at offset (oy3, ox3) = (H2 & 1, W2 & 1)
    int H4, W4, oy4, ox4;
    Swz swz2, swz3;      // periodic swizzles of the ring and of level 3's band (choose_swz_periodic)
    int ring_off, xchg_off, scr_off;   // LDS: [band3: BN_T * E3_TSZ][ring: BN_T * E23_TSZ2 (level 3's store scratch reuses it)][xchg: 4 KB]
    const uint8_t *model_ids;   // MS: model id per stack [B]
    uint32_t mstride;           // MS: bytes between two models' prepared weights
};
template <bool AP2, bool AP3, bool MS = false>
__global__ __launch_bounds__(512, 2) void enc23_mfma(Enc23Args p) {
    extern __shared__ __attribute__((aligned(256))) uint8_t smem[];
    WGSPAN_BEGIN();
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    uint8_t *const ring = smem + p.ring_off;
    uint8_t *const xchg = smem + p.xchg_off;
    const int TC3 = p.W3 + 2;
    bool first = true;
    const int tc2 = wave & 1, nt2 = (wave >> 1) & 1, th = wave >> 2;   // level 2: tile column, N tile, T half
    const int nt3 = wave & 3, mg3 = wave >> 2;                         // level 3: N tile, M group
    for (int b = blockIdx.x; b < p.B; b += gridDim.x) {
        [[maybe_unused]] const uint32_t moff = model_off<MS>(p.model_ids, p.mstride, b);
        int ll = lane;
        asm volatile("" : "+v"(ll));
        lds_barrier();   // the previous frame's level 3 has left the band and its scratch (= the ring)
        const uint8_t *const src_b = reinterpret_cast<const uint8_t *>(p.in) + (size_t)b * BN_T * p.H2 * p.W2 * 64;
        // staging through registers (a kernel with LDS-DMA makes hipcc drain the vector-memory counter in front of every LDS
        // read, which would put each step's landing back in front of its tiles): a thread owns ONE 16-byte piece position
        // (T slice tid >> 7, pixel, chunk) of every ring row; per step it loads that piece of the two new rows right after
        // the step's barrier and writes them into their slots behind its tile
        const int st_t = tid >> 7, st_i = tid & 127, st_c = st_i >> 2, st_x = st_c - 1;
        const bool st_xin = st_x >= 0 && st_x < p.W2;
        uint32_t st_so[2];   // source offset of the piece within its row, per row parity (the swizzle depends on it)
#pragma unroll
        for (int k = 0; k < 2; k++)
            st_so[k] = (uint32_t)((min(max(st_x, 0), p.W2 - 1)) * 64 + (((st_i & 3) ^ swz_eval<4>(p.swz2, st_c, k)) << 4));
        const uint8_t *const st_src = src_b + (size_t)st_t * p.H2 * p.W2 * 64;
        uint8_t *const st_dst = ring + st_t * E23_TSZ2 + st_i * 16;
        auto load_rows = [&](int r0, uint4 (&v)[2]) {    // rows r0, r0 + 1 (r0 odd): yy = row + 1 has parity k
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const int rc = min(max(r0 + k, 0), p.H2 - 1);
                v[k] = *reinterpret_cast<const uint4 *>(st_src + (size_t)rc * p.W2 * 64 + st_so[k]);
            }
        };
        auto store_rows = [&](int r0, const uint4 (&v)[2]) {
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const int row = r0 + k;
                const bool in = st_xin && row >= 0 && row < p.H2;
                *reinterpret_cast<uint4 *>(st_dst + ((row + 1) % E23_NSLOT) * E23_RP2) = in ? v[k] : make_uint4(0, 0, 0, 0);
            }
        };
        {
            uint4 va[2], vb[2];
            load_rows(-1, va);
            load_rows(1, vb);
            if (first) {
                // level 3's band: halo, pad row / column and the tail of every T slice stay zero for the whole launch (written
                // while the first rows are on their way)
                for (int i = tid; i < BN_T * E3_TSZ / 16; i += 512) *reinterpret_cast<uint4 *>(smem + i * 16) = make_uint4(0, 0, 0, 0);
                first = false;
            }
            store_rows(-1, va);
            store_rows(1, vb);
        }
        {   // ---------------- level 2
            const int m0 = ll & 31, kh = ll >> 5;
            const int yl = (m0 >> 1) & 1, xl = 2 * (m0 >> 2) + (m0 & 1);
            // the lane's part of a fragment address per tap (pixel within the ring row, chunk = K half ^ swizzle); the ring row
            // (slot) of the tap is added per step.  yy = row + 1 of the absolute input row: its parity is the tap row's parity
            // within a step.  (Per frame, from an opaque lane id: nothing of level 2 stays live across level 3's 240 registers.)
            uint32_t xq2[9];
#pragma unroll
            for (int tap = 0; tap < 9; tap++) {
                const int yy = yl + tap / 3, xx = xl + 16 * tc2 + tap % 3;
                xq2[tap] = (uint32_t)(p.ring_off + th * 2 * E23_TSZ2 + xx * 64) ^ (uint32_t)((kh ^ swz_eval<4>(p.swz2, xx, yy)) << 4);
            }
            half8 bf[18];
            {
                const half8 *wp = at_model(p.wf2, moff) + nt2 * 18 * 64 + ll;
                asm volatile("" : "+v"(wp));
                const gptr<half8> wg = as_global(wp);
#pragma unroll
                for (int ks = 0; ks < 18; ks++) bf[ks] = wg[ks * 64];
            }
            const int co = nt2 * 32 + (ll & 31);
            const float *const epi2 = at_model(p.epi2, moff);
            const float e0 = epi2[co], e1 = epi2[64 + co], e2 = epi2[128 + co];
            const TmixW tm = load_tmix(epi2 + 192, ll);
            int s0 = 0;   // ring slot of the step's first row (input row 2s - 1)
            for (int s = 0; s < p.Hp2; s++) {
                lds_barrier();   // the step's rows are in the ring; every wave has left step s - 1 (its ring rows, the exchange area)
                uint4 vn[2];
                const bool pre = s + 1 < p.Hp2;
                if (pre) load_rows(2 * s + 3, vn);
                uint32_t fa[9];
                {
#pragma unroll
                    for (int ty = 0; ty < 3; ty++) {
                        int slot = s0 + ty + yl;   // per lane (written as arithmetic: a select between wave-uniform values becomes a scratch array)
                        slot = slot >= E23_NSLOT ? slot - E23_NSLOT : slot;
                        const uint32_t rr = (uint32_t)(slot * E23_RP2);
#pragma unroll
                        for (int tx = 0; tx < 3; tx++) fa[ty * 3 + tx] = xq2[ty * 3 + tx] + rr;
                    }
                }
                s0 = s0 + 2 >= E23_NSLOT ? s0 + 2 - E23_NSLOT : s0 + 2;
                // 36 products: tap x channel chunk x the wave's two T slices; A fragments through a ring of eight registers
                constexpr int AD = 8, NS = 36;
                auto frag = [&](int i) -> half8 {
                    const int tap = i >> 2, kc = (i >> 1) & 1, t = i & 1;
                    const uint8_t *a = smem + (fa[tap] ^ (uint32_t)(kc << 5));
                    return *reinterpret_cast<const half8 *>(__builtin_assume_aligned(a + t * E23_TSZ2, 16));
                };
                half8 ab[AD];
#pragma unroll
                for (int i = 0; i < AD; i++) ab[i] = frag(i);
                f32x16 acc[2];
#pragma unroll
                for (int i = 0; i < NS; i++) {
                    const int t = i & 1;
                    if (i < 2) {
#pragma unroll
                        for (int q = 0; q < 16; q++) acc[t][q] = 0.f;
                    }
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ab[i % AD], bf[i >> 1], acc[t], 0, 0, 0);
                    if (i + AD < NS) ab[i % AD] = frag(i + AD);
                }
                pin_ring<NS, AD>();
                // pooled values of windows 2g + kh (g = 0..3) for the wave's T slices, rounded to fp16 (the MLP's operand)
                half2v hp[4];
#pragma unroll
                for (int g = 0; g < 4; g++)
#pragma unroll
                    for (int t = 0; t < 2; t++)
                        hp[g][t] = (_Float16)pool4<AP2>(acc[t][4 * g], acc[t][4 * g + 1], acc[t][4 * g + 2], acc[t][4 * g + 3], e0, e1, e2);
                // the partner wave (same tile, other T half) runs the MLP of windows g = 2 (1 - th), 2 (1 - th) + 1: hand it ours
                {
                    typedef _Float16 half4x __attribute__((ext_vector_type(4)));
                    const half4x give = th ? half4x{hp[0][0], hp[0][1], hp[1][0], hp[1][1]} : half4x{hp[2][0], hp[2][1], hp[3][0], hp[3][1]};
                    *reinterpret_cast<half4x *>(xchg + (wave * 64 + ll) * 8) = give;
                }
                if (pre) store_rows(2 * s + 3, vn);
                lds_barrier();
                half4 pb[2], o[2];
                {
                    const half4 got = *reinterpret_cast<const half4 *>(xchg + ((wave ^ 4) * 64 + ll) * 8);
                    if (th == 0) {
                        pb[0] = half4{hp[0][0], hp[0][1], got[0], got[1]};
                        pb[1] = half4{hp[1][0], hp[1][1], got[2], got[3]};
                    } else {
                        pb[0] = half4{got[0], got[1], hp[2][0], hp[2][1]};
                        pb[1] = half4{got[2], got[3], hp[3][0], hp[3][1]};
                    }
                }
                tmix4h<2>(tm, pb, o);
                // -> level 3's band: pixel (gy + 1, gx + 1) of every T slice, channel co, at the band's swizzle
#pragma unroll
                for (int gl = 0; gl < 2; gl++) {
                    const int owx = 8 * tc2 + 2 * (2 * th + gl) + kh;
                    if (owx < p.Wp2) {
                        const int yy = s + p.oy3 + 1, xx = owx + p.ox3 + 1;
                        uint8_t *d = smem + (yy * TC3 + xx) * 128 + ((((co >> 3) ^ swz_eval<8>(p.swz3, xx, yy))) << 4) + (co & 7) * 2;
#pragma unroll
                        for (int t = 0; t < BN_T; t++) *reinterpret_cast<_Float16 *>(d + t * E3_TSZ) = o[gl][t];
                    }
                }
            }
        }
        {   // ---------------- level 3 (the tile loop of enc_mfma<64, 128, 2, .., E3_TSZ> on the band in LDS)
            int l3 = lane;
            asm volatile("" : "+v"(l3));
            const int m0 = l3 & 31, kh = l3 >> 5;
            const int yl = (m0 >> 1) & 1, xl = 2 * (m0 >> 2) + (m0 & 1);
            // Requested in front of the barrier that completes the band and in flight across it and the T = 0 copy-out: global loads,
            // so neither the barrier's LDS wait nor the copy-out's LDS reads wait for them; the tile loop's preheader does (vmcnt(0))
            half8 bf[36];
            {
                const half8 *wp = at_model(p.wf3, moff) + nt3 * 36 * 64 + ll;
                asm volatile("" : "+v"(wp));
                const gptr<half8> wg = as_global(wp);
#pragma unroll
                for (int ks = 0; ks < 36; ks++) bf[ks] = wg[ks * 64];
            }
            lds_barrier();   // level 3's band is complete
            // T = 0 slice of level 2's output -> act[3] (rows / columns of the pad are zero in HBM and never written)
            {
                __half *const mb = p.mid + (size_t)b * BN_T * p.H3 * p.W3 * 64;
                const int npc = p.Hp2 * p.Wp2 * 8;
                for (int i = tid; i < npc; i += 512) {
                    const int pix = i >> 3, j = i & 7;
                    const int wy = pix / p.Wp2, wx = pix - wy * p.Wp2;
                    const int yy = wy + p.oy3 + 1, xx = wx + p.ox3 + 1;
                    const uint4 v = *reinterpret_cast<const uint4 *>(smem + (yy * TC3 + xx) * 128 + ((j ^ swz_eval<8>(p.swz3, xx, yy)) << 4));
                    *reinterpret_cast<uint4 *>(mb + ((size_t)(yy - 1) * p.W3 + (xx - 1)) * 64 + j * 8) = v;
                }
            }
            const int co = nt3 * 32 + (ll & 31);
            const float *const epi3 = at_model(p.epi3, moff);
            const float e0 = epi3[co], e1 = epi3[128 + co], e2 = epi3[256 + co];
            const TmixW tm = load_tmix(epi3 + 384, ll);
            uint32_t kq[9];
#pragma unroll
            for (int tap = 0; tap < 9; tap++) {
                const int yy = yl + tap / 3, xx = xl + tap % 3;
                kq[tap] = (uint32_t)((yy * TC3 + xx) * 128) ^ (uint32_t)((kh ^ swz_eval<8>(p.swz3, xx, yy)) << 4);
            }
            const int ntc = (p.Wp3 + 7) >> 3;
            const int ntiles = p.Hp3 * ntc;
            int t_wy = 0, t_tc = mg3;
            __half *const ob = p.out + (size_t)b * p.H4 * p.W4 * 128;
            uint8_t *const scr = smem + p.scr_off + wave * 2048;
            for (int tile = mg3; tile < ntiles; tile += 2, t_tc += 2) {
                while (t_tc >= ntc) { t_tc -= ntc; t_wy++; }
                const uint32_t tbase = (uint32_t)(((2 * t_wy) * TC3 + 16 * t_tc) * 128);
                uint32_t fa[9];
#pragma unroll
                for (int tap = 0; tap < 9; tap++) fa[tap] = kq[tap] + tbase;
                half4 pb4[4];
#pragma unroll
                for (int grp = 0; grp < 2; grp++) {
                    f32x16 acc[2];
#pragma unroll
                    for (int t = 0; t < 2; t++)
#pragma unroll
                        for (int q = 0; q < 16; q++) acc[t][q] = 0.f;
#pragma unroll
                    for (int tap = 0; tap < 9; tap++) {
#pragma unroll
                        for (int kc = 0; kc < 4; kc++)
#pragma unroll
                            for (int t = 0; t < 2; t++) {
                                const uint8_t *ap = smem + ((fa[tap] + (uint32_t)(grp * 2 * E3_TSZ)) ^ (uint32_t)(kc << 5)) + t * E3_TSZ;
                                const half8 a = *reinterpret_cast<const half8 *>(__builtin_assume_aligned(ap, 16));
                                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bf[tap * 4 + kc], acc[t], 0, 0, 0);
                            }
                    }
#pragma unroll
                    for (int tt = 0; tt < 2; tt++)
#pragma unroll
                        for (int g = 0; g < 4; g++)
                            pb4[g][grp * 2 + tt] = (_Float16)pool4<AP3>(acc[tt][4 * g], acc[tt][4 * g + 1], acc[tt][4 * g + 2], acc[tt][4 * g + 3], e0, e1, e2);
                }
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    typedef int i32x2 __attribute__((ext_vector_type(2)));
                    i32x2 bits = __builtin_bit_cast(i32x2, pb4[g]);
                    asm volatile("" : "+v"(bits));
                    pb4[g] = __builtin_bit_cast(half4, bits);
                }
                // epilogue: temporal MLP, T = 0 only (the decoder takes nothing else), 16-byte stores through the wave's transpose
                half4 o4[4];
#pragma unroll
                for (int g = 0; g < 4; g++) tmix4h(tm, pb4[g], o4[g]);
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    _Float16 *sw = reinterpret_cast<_Float16 *>(scr + (2 * g + kh) * 64) + (ll & 31);
                    sw[0] = o4[g][0];
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                const int owin = 8 * t_tc + ((ll >> 2) & 7);
                if (owin < p.Wp3 && ll < 32) {
                    const int gy = t_wy + p.oy4, gx = owin + p.ox4;
                    const uint32_t eo = (uint32_t)((gy * p.W4 + gx) * 128 + nt3 * 32 + 8 * (ll & 3));
                    *reinterpret_cast<uint4 *>(ob + eo) = *reinterpret_cast<const uint4 *>(scr + ll * 16);
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
    WGSPAN_END(1);
}

// ------------------------------------------------------------------ decoder blocks 0..3
// relu -> convT(4x4, s2) -> crop -> BN as ONE 2x2-tap convolution over the (Hi+1)x(Wi+1) grid:
//   out[2u+py-cy, 2v+px-cx][co] = sum_{a,b,c} in[u-a, v-b][c] * w[py+2a][px+2b][co][c]
// with the four output parities stacked next to the output channels (4*COUT rows).
// The MFMA runs "transposed": A = weight fragments (32 (parity,co) rows), B = activations
// (32 grid positions), so a lane owns ONE position and its 16 accumulator registers are 4 groups
// of 4 consecutive output channels -> one (u,v) decomposition per lane per tile and 8-byte packed
// stores.  The last block (FINAL) has the final 1x1 conv folded in (no non-linearity between
// them): 4 rows = the 4 parities, output = logit (+ threshold).

// ---- the pieces that the decoder kernels share: each form calls them, so "the same products in the same order, the same epilogue
// expression" holds between the forms by construction
// A band's tile by LDS-DMA: concat(up, skip[t=0]) rows u0-1 .. u0+nu-1 of frame b, swept linearly in 16-byte chunks (64 per wave
// instruction), swizzled; chunks outside the frame read the zero buffer.  Both sources hold relu'd values.  NW waves.
template <int C1, int C2, int NW>
__device__ __forceinline__ void dec_stage_band(const DecArgs &p, int b, int u0, int nu, uint8_t *dst, int wave, int lane) {
    constexpr int C = C1 + C2, CPP = C / 8;
    const int RC = (p.Wi + 2) * CPP;
    const int nchunk = (nu + 1) * RC;
    [[maybe_unused]] const __half *su = p.up + ((size_t)b) * p.Hi * p.Wi * C1;
    [[maybe_unused]] const __half *ss = p.skip + ((size_t)b * p.Ts) * p.Hi * p.Wi * C2;
    for (int s0 = wave * 64; s0 < nchunk; s0 += NW * 64) {
        const int sidx = s0 + lane;
        if (sidx < nchunk) {
            const int r = fdiv(sidx, p.mRC), within = sidx - r * RC;
            const int c = within / CPP, chp = within % CPP;
            const int cb = (chp ^ swz_eval<CPP>(p.swz, c, r)) * 8;
            const int y = u0 - 1 + r, x = c - 1;
            const void *src = p.zero;
            if (y >= 0 && y < p.Hi && x >= 0 && x < p.Wi) {
                const size_t pix = (size_t)y * p.Wi + x;
                if constexpr (C1 == 0) src = ss + pix * C2 + cb;
                else if constexpr (C2 == 0) src = su + pix * C1 + cb;
                else src = cb < C1 ? (const void *)(su + pix * C1 + cb) : (const void *)(ss + pix * C2 + (cb - C1));
            }
            glds16(src, dst + s0 * 16);
        }
    }
}
// The products of one tile of 32 grid positions: the lane's position is (ul, v) of the band in `tile` (TC pixels per row), 2x2
// taps x C / 16 channel chunks in this order
template <int C>
__device__ __forceinline__ f32x16 dec_tile_acc(const uint8_t *tile, int TC, const Swz &swz, const half8 (&wf)[4 * (C / 16)], int ul, int v, int kh) {
    constexpr int KC = C / 16, CPP = C / 8, PS = C * 2;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.f;
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int bb = 0; bb < 2; bb++) {
            const int yy = ul + 1 - a, xx = v + 1 - bb;   // tile coordinates of input (u-a, v-b)
            const int pbase = (yy * TC + xx) * PS;
            const int s = swz_eval<CPP>(swz, xx, yy);
#pragma unroll
            for (int kc = 0; kc < KC; kc++) {
                const half8 av = *reinterpret_cast<const half8 *>(tile + pbase + (((kc * 2 + kh) ^ s) * 16));
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[(a * 2 + bb) * KC + kc], av, acc, 0, 0, 0);
            }
        }
    return acc;
}
// The last block's output of grid position (u, v) of frame b, for a lane of the kh == 0 half: accumulator rows 0..3 = the four
// output parities (py, px) = (r >> 1, r & 1).  Logit = product + folded bias (+ PART: the position's partial logits, `part` = the
// frame's), stored when the caller asked for logits; mask byte = logit > threshold (&& POST: keep map) into `mask`, LDS bytes
// [row][Wd] that start at frame row Y0.
template <bool PART, bool POST>
__device__ __forceinline__ void dec_final_out(const DecArgs &p, const StackPost &sp, const f32x16 acc, float fbias, const f32x4 *part, int b, int u, int v,
                                              uint8_t *mask, int Y0) {
    const int GW = p.Wi + 1;
    f32x4 pl = {0.f, 0.f, 0.f, 0.f};
    if constexpr (PART) pl = part[u * GW + v];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int Y = 2 * u + (r >> 1) - p.cy, X = 2 * v + (r & 1) - p.cx;
        if (Y >= 0 && Y < p.Hd && X >= 0 && X < p.Wd) {
            float l = acc[r] + fbias;
            if constexpr (PART) l += pl[r];
            if (p.logits) p.logits[((size_t)b * p.Hd + Y) * p.Wd + X] = l;
            bool fg = l > sp.thr;
            if constexpr (POST) fg = fg && sp.keep[Y * p.Wd + X];
            mask[(Y - Y0) * p.Wd + X] = fg ? 1 : 0;
        }
    }
}
// mask bytes LDS -> global memory, four at a time where the caller's alignment condition holds.  NTH threads.
template <int NTH>
__device__ __forceinline__ void dec_mask_out(const uint8_t *src, uint8_t *dst, int nbytes, bool aligned4, int tid) {
    if (aligned4) {
        for (int i = tid; i < nbytes / 4; i += NTH) reinterpret_cast<uint32_t *>(dst)[i] = reinterpret_cast<const uint32_t *>(src)[i];
    } else {
        for (int i = tid; i < nbytes; i += NTH) dst[i] = src[i];
    }
}
// ReLU(BN(acc)) of register group g (four consecutive output channels) as fp16
__device__ __forceinline__ half4 dec_relu_bn4(const f32x16 acc, const float (&es)[16], const float (&eb)[16], int g) {
    half4 o;
#pragma unroll
    for (int j = 0; j < 4; j++) o[j] = (_Float16)fmaxf(acc[4 * g + j] * es[4 * g + j] + eb[4 * g + j], 0.f);
    return o;
}
// A frame's partial logits (src: fp32 [npos][4 parities]) into LDS: one 16-byte piece per grid position.  NW waves.
template <int NW>
__device__ __forceinline__ void dec_stage_part(const float *src, int npos, uint8_t *dst, int wave, int lane) {
    const uint8_t *ps = reinterpret_cast<const uint8_t *>(src);
    for (int s0 = wave * 64; s0 < npos; s0 += NW * 64)
        if (s0 + lane < npos) glds16(ps + (size_t)(s0 + lane) * 16, dst + s0 * 16);
}

// A wave's weight fragments of M-tile mtile and its epilogue constants per register: reg 4g+j <-> row 8g + 4kh + j <-> (parity, co = row % COUT);
// the last block has its folded bias instead.  A register group's four consecutive channels are one 16-byte load each of scale and
// shift: epi is 16-byte aligned (the prepared blocks start at multiples of 256 bytes, and so does a model's stride under MS), as
// dec012_load relies on for the same arrays
template <int KSTEPS, int COUT, bool FINAL>
__device__ __forceinline__ void dec_load_w(half8 (&wf)[KSTEPS], float (&es)[16], float (&eb)[16], float &fbias, const half8 *wfrag, const float *epi,
                                           int mtile, int lane, int kh) {
    static_assert(FINAL || (COUT % 4 == 0 && (COUT & (COUT - 1)) == 0), "a register group's four channels do not wrap");
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ks++) wf[ks] = wfrag[(mtile * KSTEPS + ks) * 64 + lane];
    if constexpr (!FINAL) {   // registers 4g .. 4g+3: four consecutive channels, one 16-byte load each of scale and shift
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const int c0 = (mtile * 32 + 8 * g + 4 * kh) & (COUT - 1);
            const f32x4 sc = *reinterpret_cast<const f32x4 *>(epi + c0), sh = *reinterpret_cast<const f32x4 *>(epi + COUT + c0);
#pragma unroll
            for (int j = 0; j < 4; j++) { es[4 * g + j] = sc[j]; eb[4 * g + j] = sh[j]; }
        }
    } else {
        fbias = epi[0];
    }
}
template <int C1, int C2, int COUT, bool FINAL, bool MS = false, bool POST = false>
__global__ __launch_bounds__(((FINAL ? 1 : 4 * COUT / 32) > 4 ? 4 * COUT / 32 : 4) * 64, 2) void dec_mfma(DecArgs p, DecMs pm, PostArg<POST> pp) {
    static_assert(FINAL || !POST, "post-processing belongs to the block that writes the mask");
    constexpr int C = C1 + C2, MT = FINAL ? 1 : 4 * COUT / 32, NW = MT > 4 ? MT : 4, PG = NW / MT;
    constexpr int KC = C / 16, KSTEPS = 4 * KC, CPP = C / 8, PS = C * 2;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mtile = wave % MT, pgroup = wave / MT;
    const int TC = p.Wi + 2;
    const int GW = p.Wi + 1, GH = p.Hi + 1;
    const int kh = lane >> 5;

    half8 wf[KSTEPS];
    float es[16], eb[16], fbias = 0.f;
    dec_load_w<KSTEPS, COUT, FINAL>(wf, es, eb, fbias, p.wfrag, p.epi, mtile, lane, kh);

    const int n_items = p.B * p.nbands;
    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int b = fdiv(item, p.mNb), band = item - b * p.nbands;
        [[maybe_unused]] const StackPost sp = stack_post<POST, MS>(pp, pm.model_ids, b);
        if constexpr (MS) {   // every item takes its stack's weights: one copy in registers, no second one kept for a compare
            const uint32_t moff = model_off<MS>(pm.model_ids, pm.mstride, b);
            dec_load_w<KSTEPS, COUT, FINAL>(wf, es, eb, fbias, at_model(p.wfrag, moff), at_model(p.epi, moff), mtile, lane, kh);
        }
        const int u0 = band * GH / p.nbands, u1 = (band + 1) * GH / p.nbands;
        const int nu = u1 - u0;   // grid rows of this band; tile rows = nu + 1 (input rows u0-1 .. u1-1)
        lds_barrier();
        dec_stage_band<C1, C2, NW>(p, b, u0, nu, smem, wave, lane);
        wait_vmem();
        lds_barrier();
        // last block: the band's mask rows [Yb, Ye) are assembled in LDS behind the tile and leave
        // as coalesced 4-byte stores (they are contiguous in the mask tensor)
        uint8_t *const mrows = smem + p.mask_off;
        const int Yb = max(0, 2 * u0 - p.cy), Ye = min(p.Hd, 2 * u1 - p.cy);
        [[maybe_unused]] const f32x4 *part = nullptr;   // C2 == 0: the frame's partial logits, from global memory
        if constexpr (C2 == 0) part = reinterpret_cast<const f32x4 *>(p.part) + (size_t)b * GH * GW;
        // ---- compute over the band's flattened (u, v) positions
        const int npos = nu * GW;
        const int ntiles = (npos + 31) / 32;
        for (int tile = pgroup; tile < ntiles; tile += PG) {
            const int q = tile * 32 + (lane & 31);
            const int qc = min(q, npos - 1);
            const int ul = fdiv(qc, p.mGW), v = qc - ul * GW;   // ul = u - u0
            // dec_tile_acc<C>(smem, TC, p.swz, wf, ul, v, kh), written out: as the call, block 1's loop is scheduled differently and
            // measured 0.9 % slower than the parent build, beyond its run-to-run spread
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; r++) acc[r] = 0.f;
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int bb = 0; bb < 2; bb++) {
                    const int yy = ul + 1 - a, xx = v + 1 - bb;   // tile coordinates of input (u-a, v-b)
                    const int pbase = (yy * TC + xx) * PS;
                    const int s = swz_eval<CPP>(p.swz, xx, yy);
#pragma unroll
                    for (int kc = 0; kc < KC; kc++) {
                        const half8 av = *reinterpret_cast<const half8 *>(smem + pbase + (((kc * 2 + kh) ^ s) * 16));
                        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[(a * 2 + bb) * KC + kc], av, acc, 0, 0, 0);
                    }
                }
            if constexpr (FINAL) {
                // only the kh == 0 half holds the parities' rows
                if (q < npos && kh == 0)
                    dec_final_out<C2 == 0, POST>(p, sp, acc, fbias, part, b, u0 + ul, v, mrows, Yb);
            } else {
                // 16-byte stores through a wave-private LDS transpose: the wave's 32 rows (parity, channel) x 32
                // positions are 64 contiguous bytes per position in the output tensor; lanes drop their 8-byte
                // pieces at position * 64 + (chunk ^ ((position >> 2) & 3)) * 16 (+8 for the kh half) and every
                // lane then moves two 16-byte pieces.
                uint8_t *const scr = smem + p.scr_off + wave * 2048;
                const int pos = lane & 31;
#pragma unroll
                for (int g = 0; g < 4; g++)
                    *reinterpret_cast<half4 *>(scr + pos * 64 + ((g ^ ((pos >> 2) & 3)) * 16) + kh * 8) = dec_relu_bn4(acc, es, eb, g);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    const int c = j * 64 + lane;                 // 16-byte piece of the wave's 2 KB
                    const int rp = c >> 2;                       // position of the tile
                    const int g = (c & 3) ^ ((rp >> 2) & 3);     // logical 16-byte chunk = 8 rows n0 .. n0+7
                    const int rq = tile * 32 + rp;
                    if (rq < npos) {
                        const int rul = fdiv(rq, p.mGW), rv = rq - rul * GW;
                        const int n0 = mtile * 32 + 8 * g;
                        const int phase = n0 / COUT, co0 = n0 % COUT;
                        const int Y = 2 * (u0 + rul) + (phase >> 1) - p.cy, X = 2 * rv + (phase & 1) - p.cx;
                        if (Y >= 0 && Y < p.Hd && X >= 0 && X < p.Wd)
                            *reinterpret_cast<uint4 *>(p.out + (((size_t)b * p.Hd + Y) * p.Wd + X) * COUT + co0) =
                                *reinterpret_cast<const uint4 *>(scr + c * 16);
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the next tile's pieces stay behind these reads
                __builtin_amdgcn_wave_barrier();
            }
        }
        if constexpr (FINAL) {
            if (p.mask) {
                lds_barrier();
                dec_mask_out<NW * 64>(mrows, p.mask + ((size_t)b * p.Hd + Yb) * p.Wd, (Ye - Yb) * p.Wd,
                                      (p.Wd & 3) == 0 && (reinterpret_cast<uintptr_t>(p.mask) & 3) == 0, tid);
            }
        }
    }
}

// ------------------------------------------------------------------ decoder blocks 0..2 in one launch
// Blocks 0..2 are three short launches of 9-12 us for ~4.5 us of MFMA work between them: each stages a band,
// waits, runs a handful of tiles and writes an intermediate that the next launch reads back.  One frame's
// intermediates are small (9x15x64, 17x30x32 at 1080p), so here ONE workgroup takes a frame through all three
// blocks: the three input tiles live in LDS side by side, the skip halves (encoder outputs) of all of them are
// requested at once, and block j's epilogue writes its BN'd, relu'd output straight into the "up" half of block
// j+1's tile (with that tile's swizzle) instead of HBM.  Block 2's output leaves through the same 16-byte-store
// transpose as in dec_mfma.  Same products in the same order, same epilogue expression: bit-identical to the
// three launches (tests/test_gpu_blobnet.py).
struct DecLvl {
    int Hi, Wi, Hd, Wd, cy, cx;
    uint32_t mGW, mRC;
    Swz swz;
    int tile_off;   // byte offset of the block's input tile [Hi+2][Wi+2][C] in LDS
};
struct Dec012Args {
    const __half *skip[3];   // act[4] [B][1][..][128], act[3] [B][T][..][64], act[2] [B][T][..][32]: T index 0 is used
    int Ts[3];
    __half *out;             // dact[2] [B][Hd][Wd][16]
    const half8 *wf[3];
    const float *epi[3];
    DecLvl lv[3];
    int B, scr_off;
    const void *zero;
    const uint8_t *model_ids;   // MS: model id per stack [B]
    uint32_t mstride;           // MS: bytes between two models' prepared weights
};
// dec012_mfma<.., TAILF>: the folded last block runs behind block 2, on block 2's output in LDS, and the launch ends in bboxcc's
// parity planes (cc_planes takes them from there).  The kernel's own argument behind Dec012Args, so that the form without it keeps
// its argument layout (it gets the empty Dec012NoTail).
struct Dec012Tail {
    DecLvl lv;                  // the last block: Hi x Wi = block 2's output, Hd x Wd = the frame; tile_off: the tile t3
    const half8 *wfrag;         // the four folded fragments of the "up" half (Prepared::final_w_up)
    const float *epi;           // the folded bias
    const float *part;          // partial logits, fp32 [B][Hi + 1][Wi + 1][4]
    float *logits;              // [B][Hd][Wd] or null
    uint8_t *mask;              // [B][Hd][Wd] or null
    uint32_t *planes_out;       // [B][rows_bytes / 4]: the frames' parity planes (BnWorkspace::planes)
    int planes_off, rows_bytes; // the planes in LDS (ccwave::WvGeom::rows_bytes)
    uint32_t mW4;               // magic(Wd / 4): the mask expansion's division
};
struct Dec012NoTail {};
template <bool TAILF>
using Dec012TailArg = std::conditional_t<TAILF, Dec012Tail, Dec012NoTail>;

// The border of a block's tile (the zero padding of the transposed convolution's input) is written once per launch:
// nothing ever overwrites it, interior pixels are refilled for every frame (skip half by DMA, "up" half by the block
// before).
template <int C>
__device__ __forceinline__ void dec012_zero_border(uint8_t *tile, const DecLvl &g, int tid) {
    constexpr int CPP = C / 8;
    const int RC = (g.Wi + 2) * CPP;
    const int n_rows = 2 * RC, n_cols = 2 * CPP * g.Hi;   // top + bottom row; left + right pixel of the rows between
    for (int i = tid; i < n_rows + n_cols; i += 512) {
        int piece;
        if (i < n_rows) {
            piece = i < RC ? i : (g.Hi + 1) * RC + (i - RC);
        } else {
            const int j = i - n_rows, y = j / (2 * CPP), k = j % (2 * CPP);
            piece = (y + 1) * RC + (k < CPP ? k : (g.Wi + 1) * CPP + (k - CPP));
        }
        *reinterpret_cast<uint4 *>(tile + piece * 16) = uint4{0, 0, 0, 0};
    }
}
// requests the skip half of one block's tile, row by row: a wave takes whole rows (wave-uniform row arithmetic), its
// lanes the row's interior 16-byte pieces, 64 per request; the lanes of "up" pieces sit the request out
template <int C1, int C2>
__device__ __forceinline__ void dec012_stage(uint8_t *tile, const __half *ss, const DecLvl &g, int wave, int lane, int first) {
    constexpr int C = C1 + C2, CPP = C / 8;
    const int RC = (g.Wi + 2) * CPP, NI = g.Wi * CPP;   // pieces per tile row / interior pieces per row
    for (int y = (wave + 8 - first) & 7; y < g.Hi; y += 8) {
        const int r = y + 1;
        const __half *rowp = ss + (size_t)y * g.Wi * C2;
        uint8_t *rowl = tile + (r * RC + CPP) * 16;   // the row's first interior piece
        for (int q0 = 0; q0 < NI; q0 += 64) {
            const int q = q0 + lane;
            const int px = q / CPP, chp = q % CPP;
            const int cb = (chp ^ swz_eval<CPP>(g.swz, px + 1, r)) * 8;
            if (q < NI && cb >= C1) glds16(rowp + px * C2 + (cb - C1), rowl + q0 * 16);
        }
    }
}

// one block over the whole frame, eight waves.  CN > 0: output into the next block's tile (CN channels per pixel);
// CN == 0: output to global memory.
template <int C, int COUT>
struct Dec012W {   // a wave's weight fragments and epilogue constants of one block
    half8 wf[4 * (C / 16)];
    float es[16], eb[16];
};
constexpr int DEC012_W0_KEPT = 4 * (128 / 16);   // block 0's fragment loads: what dec012_mfma leaves in flight across its first barrier
template <int C, int COUT>
__device__ __forceinline__ void dec012_load(Dec012W<C, COUT> &w, const half8 *wfrag, const float *epi, int wave, int lane) {
    constexpr int MT = 4 * COUT / 32, KSTEPS = 4 * (C / 16);
    const int mtile = wave % MT, kh = lane >> 5;
    // opaque pointers: the fragments are loaded here, per frame and per block -- hoisted out of the frame loop the three
    // blocks' weights (320 registers) would be live together and spill
    asm volatile("" : "+s"(wfrag), "+s"(epi));
    const gptr<half8> wg = as_global(wfrag);
    const gptr<float> eg = as_global(epi);
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ks++) w.wf[ks] = wg[(mtile * KSTEPS + ks) * 64 + lane];
    // registers 4g .. 4g+3 <-> rows n0 .. n0+3, n0 = mtile*32 + 8g + 4kh: four consecutive channels, one 16-byte load
#pragma unroll
    for (int gq = 0; gq < 4; gq++) {
        const int c0 = (mtile * 32 + 8 * gq + 4 * kh) % COUT;
        const f32x4 sc = *(gptr<f32x4>)(eg + c0), sh = *(gptr<f32x4>)(eg + COUT + c0);
#pragma unroll
        for (int j = 0; j < 4; j++) { w.es[4 * gq + j] = sc[j]; w.eb[4 * gq + j] = sh[j]; }
    }
}
template <int C1, int C2, int COUT, int CN>
__device__ __forceinline__ void dec012_block(const uint8_t *lds0, const uint8_t *tile, uint8_t *next_tile, __half *gout, uint8_t *scr_base,
                                             const Dec012W<C1 + C2, COUT> &w, const DecLvl &g, const DecLvl &gn,
                                             int wave, int lane) {
    constexpr int C = C1 + C2, MT = 4 * COUT / 32, PG = 8 / MT;
    constexpr int KC = C / 16, KSTEPS = 4 * KC, CPP = C / 8, PS = C * 2;
    constexpr int AD = C == 128 ? 4 : 8;   // B fragments in flight ahead of their MFMA (ring, as in enc_mfma); what the registers allow
    const int mtile = wave % MT, pgroup = wave / MT;
    const int TC = g.Wi + 2, GW = g.Wi + 1, GH = g.Hi + 1;
    const int kh = lane >> 5;
    const half8 (&wf)[KSTEPS] = w.wf;
    const float (&es)[16] = w.es, (&eb)[16] = w.eb;
    const int npos = GH * GW;
    const int ntiles = (npos + 31) / 32;
    for (int tile_i = pgroup; tile_i < ntiles; tile_i += PG) {
        const int q = tile_i * 32 + (lane & 31);
        const int qc = min(q, npos - 1);
        const int u = fdiv(qc, g.mGW), v = qc - u * GW;
        // the four taps' tile offsets and swizzles, then the K steps in dec_mfma's order with their B fragments AD steps ahead
        // chunk (2 kc + kh) ^ swizzle = (kc << 1) ^ (kh ^ swizzle): the tap's pixel address (from the start of LDS: the tiles start
        // at multiples of 256 bytes) and (kh ^ swizzle) << 4 once per tile, then one xor per K step (the pixel address leaves
        // the chunk bits clear)
        const uint32_t toff = (uint32_t)(uintptr_t)(lds_void *)tile;   // LDS address (dec012_mfma aligns its LDS to 256)
        uint32_t pk[4];
#pragma unroll
        for (int tp = 0; tp < 4; tp++) {
            const int yy = u + 1 - (tp >> 1), xx = v + 1 - (tp & 1);   // tile coordinates of input (u-a, v-b)
            pk[tp] = (toff + (uint32_t)((yy * TC + xx) * PS)) | (uint32_t)((kh ^ swz_eval<CPP>(g.swz, xx, yy)) << 4);
        }
        auto frag = [&](int ks) -> half8 {
            const int tp = ks / KC, kc = ks % KC;
            typedef const __attribute__((address_space(3))) half8 *lds_half8_ptr;
            return *(lds_half8_ptr)(uintptr_t)(pk[tp] ^ (uint32_t)(kc << 5));
        };
        half8 ring[AD];
#pragma unroll
        for (int ks = 0; ks < AD; ks++) ring[ks] = frag(ks);
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; r++) acc[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ks++) {
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[ks], ring[ks % AD], acc, 0, 0, 0);
            if (ks + AD < KSTEPS) ring[ks % AD] = frag(ks + AD);
        }
        pin_ring<KSTEPS, AD>();
        if constexpr (CN > 0 && COUT == 16) {
            // Block 2 into the row tail's tile (dec012_mfma<.., TAILF>; CN = 16 channels of 32 bytes per pixel, the 16-byte halves
            // swizzled by (xx >> 3) & 1).  Rows n0 + j, n0 = mtile*32 + 8 gq + 4 kh, with COUT = 16: parity 2 mtile + (gq >> 1), channels
            // 8 (gq & 1) + 4 kh + j -- a lane's four register groups are TWO output pixels (px = 0, 1 of output row 2u + mtile) x two
            // 8-channel chunks, of which it holds four channels each: two bounds tests, four 8-byte writes
            static_assert(CN == 16 && MT == 2, "the row tail's tile");
            const int TCN = gn.Wi + 2;
            const int Y = 2 * u + mtile - g.cy;
            if (q < npos && Y >= 0 && Y < g.Hd) {
#pragma unroll
                for (int px = 0; px < 2; px++) {
                    const int X = 2 * v + px - g.cx;
                    if (X >= 0 && X < g.Wd) {
                        const int yy = Y + 1, xx = X + 1;
                        uint8_t *const pix = next_tile + (yy * TCN + xx) * 32 + kh * 8;
                        const int sw = (xx >> 3) & 1;
#pragma unroll
                        for (int c = 0; c < 2; c++) {
                            *reinterpret_cast<half4 *>(pix + ((c ^ sw) * 16)) = dec_relu_bn4(acc, es, eb, 2 * px + c);
                        }
                    }
                }
            }
        } else if constexpr (CN > 0) {
            // reg 4g+j <-> row n0 + j, n0 = mtile*32 + 8g + 4kh: one parity, four consecutive channels
            constexpr int CPPN = CN / 8, PSN = CN * 2;
            const int TCN = gn.Wi + 2;
            // rows n0 + 8 gq, n0 = mtile*32 + 4kh: with COUT >= 32 the four register groups of a lane are four 8-channel chunks of
            // ONE output pixel (same parity), so the pixel, its bounds test and its swizzle are computed once per tile
            static_assert(COUT >= 32 && COUT % 32 == 0, "one output pixel per lane and tile");
            const int nb = mtile * 32 + 4 * kh;
            const int phase = nb / COUT, cob = nb % COUT;
            const int Y = 2 * u + (phase >> 1) - g.cy, X = 2 * v + (phase & 1) - g.cx;
            if (q < npos && Y >= 0 && Y < g.Hd && X >= 0 && X < g.Wd) {
                const int yy = Y + 1, xx = X + 1;
                uint8_t *const pix = next_tile + (yy * TCN + xx) * PSN + (cob & 7) * 2;
                const int sw = swz_eval<CPPN>(gn.swz, xx, yy);
#pragma unroll
                for (int gq = 0; gq < 4; gq++)
                    *reinterpret_cast<half4 *>(pix + ((((cob >> 3) + gq) ^ sw) * 16)) = dec_relu_bn4(acc, es, eb, gq);
            }
        } else {
            // 16-byte stores through a wave-private LDS transpose, as in dec_mfma
            uint8_t *const scr = scr_base + wave * 2048;
            const int pos = lane & 31;
#pragma unroll
            for (int gq = 0; gq < 4; gq++)
                *reinterpret_cast<half4 *>(scr + pos * 64 + ((gq ^ ((pos >> 2) & 3)) * 16) + kh * 8) = dec_relu_bn4(acc, es, eb, gq);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int c = j * 64 + lane;
                const int rp = c >> 2;
                const int gq = (c & 3) ^ ((rp >> 2) & 3);
                const int rq = tile_i * 32 + rp;
                if (rq < npos) {
                    const int ru = fdiv(rq, g.mGW), rv = rq - ru * GW;
                    const int n0 = mtile * 32 + 8 * gq;
                    const int phase = n0 / COUT, co0 = n0 % COUT;
                    const int Y = 2 * ru + (phase >> 1) - g.cy, X = 2 * rv + (phase & 1) - g.cx;
                    if (Y >= 0 && Y < g.Hd && X >= 0 && X < g.Wd)
                        *reinterpret_cast<uint4 *>(gout + ((size_t)Y * g.Wd + X) * COUT + co0) =
                            *reinterpret_cast<const uint4 *>(scr + c * 16);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
}

// ---- the row tail's pieces that dec3cc_rows_mfma and dec012_mfma<.., TAILF> share (the kernels' comments say what they are)
// lane constants of the two tile halves x two tap columns: pixel column xx = 32 h + pos + 1 - bb (clamped to the grid's last
// position: lanes past the row's end compute on that pixel and are masked out of the ballots)
__device__ __forceinline__ void tail_row_lanes(uint32_t (&lc)[2][2], int GW, int lane) {
    const int kh = lane >> 5, pos = lane & 31;
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
        for (int bb = 0; bb < 2; bb++) {
            const int xx = min(32 * h + pos, GW - 1) + 1 - bb;
            lc[h][bb] = (uint32_t)(xx * 32 + ((kh ^ ((xx >> 3) & 1)) << 4));
        }
}
// One row tile: half h of grid row u of frame b.  tile: the frame's [Hi + 2][Wi + 2] pixels of 16 channels (row_b bytes per row);
// pl: the tile's partial logits (position u * GW + min(32 h + pos, GW - 1)); planes: [2 BH + 2][E lo, E hi, O lo, O hi] in LDS.
// tail_row_acc: the tile's four products; tail_row_out: logits, ballots, planes; tail_row_tile: both.
__device__ __forceinline__ f32x16 tail_row_acc(const uint8_t *tile, uint32_t row_b, const uint32_t (&lc)[2][2], const half8 (&wf)[4], int u, int h) {
    const uint32_t rb = (uint32_t)(u * row_b);   // tile row u holds input row u - 1 (tap a = 1); tap a = 0 one row further
    const uint32_t a00 = rb + row_b + (h ? lc[1][0] : lc[0][0]), a01 = rb + row_b + (h ? lc[1][1] : lc[0][1]);
    const uint32_t a10 = rb + (h ? lc[1][0] : lc[0][0]), a11 = rb + (h ? lc[1][1] : lc[0][1]);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.f;
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[0], *reinterpret_cast<const half8 *>(tile + a00), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[1], *reinterpret_cast<const half8 *>(tile + a01), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[2], *reinterpret_cast<const half8 *>(tile + a10), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[3], *reinterpret_cast<const half8 *>(tile + a11), acc, 0, 0, 0);
    return acc;
}
__device__ __forceinline__ void tail_row_out(const f32x16 acc, const f32x4 pl, float fbias, float thr, float *logits, int Hd, int Wd, int cy, int cx,
                                             int GW, int b, int u, int h, int lane, uint32_t *planes) {
    const int kh = lane >> 5, pos = lane & 31;
    const int v = 32 * h + pos;
    const bool live = kh == 0 && v < GW;
    float l[4];
#pragma unroll
    for (int r = 0; r < 4; r++) l[r] = (acc[r] + fbias) + pl[r];
    if (logits && live) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int Y = 2 * u + (r >> 1) - cy, X = 2 * v + (r & 1) - cx;
            if (Y >= 0 && Y < Hd && X >= 0 && X < Wd) logits[((size_t)b * Hd + Y) * Wd + X] = l[r];
        }
    }
    // bit v - 32 h of parity r's ballot = output pixel (Y, 2 v + X0): plane X0 & 1, plane bit v + (X0 >> 1).  Lane r < 4 takes parity
    // r's ballot, shifts it by the crop offset and ORs it into the row's 64-bit plane word: one masked ds_or_b64 per tile
    uint32_t bal[4];
#pragma unroll
    for (int r = 0; r < 4; r++) bal[r] = (uint32_t)__ballot(live && l[r] > thr);
    {
        const int r = lane & 3;
        const uint64_t bits = (uint64_t)(r == 0 ? bal[0] : r == 1 ? bal[1] : r == 2 ? bal[2] : bal[3]) << (32 * h);
        const int Y = 2 * u + (r >> 1) - cy, X0 = (r & 1) - cx;
        const int pln = X0 & 1, sh = X0 >> 1;                         // (arithmetic shift: floor)
        const int nb = (Wd - pln + 1) >> 1;                            // pixels of this plane in a row
        uint64_t w = sh >= 0 ? bits << sh : bits >> (-sh);
        w &= nb >= 64 ? ~0ull : ((1ull << nb) - 1);
        if (lane < 4 && Y >= 0 && Y < Hd && w)
            atomicOr(reinterpret_cast<unsigned long long *>(planes + (Y + 1) * 4 + 2 * pln), (unsigned long long)w);
    }
}
__device__ __forceinline__ void tail_row_tile(const uint8_t *tile, uint32_t row_b, const uint32_t (&lc)[2][2], const half8 (&wf)[4], const f32x4 pl,
                                              float fbias, float thr, float *logits, int Hd, int Wd, int cy, int cx, int GW, int b, int u,
                                              int h, int lane, uint32_t *planes) {
    tail_row_out(tail_row_acc(tile, row_b, lc, wf, u, h), pl, fbias, thr, logits, Hd, Wd, cy, cx, GW, b, u, h, lane, planes);
}
// the frame's mask bytes out of its planes: four bytes per thread and store (W is a multiple of 8: ccwave::wv_plan; dst 4-byte aligned)
template <int NTH>
__device__ __forceinline__ void tail_mask_from_planes(const uint32_t *planes, uint8_t *mask_frame, int Hd, int Wd, uint32_t mW4, int tid) {
    uint32_t *dst = reinterpret_cast<uint32_t *>(mask_frame);
    const int wq = Wd >> 2, nq = Hd * wq;
    for (int i = tid; i < nq; i += NTH) {
        const int y = fdiv(i, mW4), xq = i - y * wq;   // (mW4 = magic(Wd / 4))
        const int bx = 2 * xq;
        const uint32_t *rw = planes + (y + 1) * 4 + (bx >> 5);
        const uint32_t e2 = (rw[0] >> (bx & 31)) & 3u, o2 = (rw[2] >> (bx & 31)) & 3u;
        dst[i] = (e2 & 1u) | ((o2 & 1u) << 8) | ((e2 >> 1) << 16) | ((o2 >> 1) << 24);
    }
}

// What dec012_mfma<.., TAILF>'s fold holds in registers from in front of block 2 on, so that their loads land under block 2's tiles
// (block 2 leaves a third of the kernel's registers free): the four folded fragments, the bias, and the partial logits of the
// wave's first DEC012_PF tiles.  A wave takes DEC012_TI tiles per iteration -- a tile is ONE dependent chain (read, four products,
// compare, ballot, ds_or), and the fold has two waves per SIMD to hide it with -- and keeps the partial logits of two iterations.
constexpr int DEC012_TI = 3, DEC012_PF = 2 * DEC012_TI;
struct Dec012Fold {
    half8 wf[4];
    f32x4 ring[DEC012_PF];
    float fbias;
};
struct Dec012NoFold {};
// the partial logits of the wave's tile t of frame b, one 16-byte load per position (the kh == 0 lanes hold the four parities'
// accumulator rows; the others load the same addresses).  No branch around the load -- past the frame's last tile it reads that
// tile's again, for nothing: behind a divergent branch the compiler loses count of the loads in flight and waits for ALL of them,
// the ones just issued for two iterations ahead included
__device__ __forceinline__ f32x4 dec012_part(const Dec012Tail &pt, int b, int t, int lane) {
    const int GW = pt.lv.Wi + 1, GH = pt.lv.Hi + 1, tpr = GW > 32 ? 2 : 1;
    const int tc = min(t, tpr * GH - 1);
    const int u = tpr == 2 ? tc >> 1 : tc, h = tpr == 2 ? tc & 1 : 0;
    return as_global(reinterpret_cast<const f32x4 *>(pt.part) + (size_t)b * GH * GW)[u * GW + min(32 * h + (lane & 31), GW - 1)];
}

// TAILF: the launch ends in bboxcc's parity planes instead of dact[2].  Block 2 scatters its output into the row tail's tile t3
// in LDS (over t0 + t1, dead once block 1 has finished), the folded last block runs on it behind a barrier -- tail_row_tile, the
// text dec3cc_rows_mfma runs, on eight waves, the partial logits straight from global memory a few tiles ahead of their use -- and
// behind a second barrier the planes leave for the workspace (cc_planes reads them), with the mask bytes and logits the caller asked
// for.  Same products in the same order, same logit expression, same ballots: bit-identical to the two launches
// (tests/test_gpu_tail_in_dec012.py).  t3 overwrites the borders of t0 and t1, so this form writes them per frame.
template <bool MS = false, bool TAILF = false>
__global__ __launch_bounds__(512, 2) void dec012_mfma(Dec012Args p, Dec012TailArg<TAILF> pt) {
    static_assert(!(MS && TAILF), "the form that ends in planes is the single-model kernel's");
    extern __shared__ __attribute__((aligned(256))) uint8_t smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint8_t *const t0 = smem + p.lv[0].tile_off, *const t1 = smem + p.lv[1].tile_off, *const t2 = smem + p.lv[2].tile_off;
    WGSPAN_BEGIN();
#ifdef PHASE_TIMING
    unsigned long long ph_[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, last_ = __builtin_amdgcn_s_memrealtime();
#endif
    // border pieces only: disjoint from what the tile requests fill, and ordered in front of the first tile reads by the barrier
    // behind the landing
    if constexpr (!TAILF) {
        dec012_zero_border<128>(t0, p.lv[0], tid);
        dec012_zero_border<128>(t1, p.lv[1], tid);
    }
    dec012_zero_border<64>(t2, p.lv[2], tid);
    for (int b = blockIdx.x; b < p.B; b += gridDim.x) {
        [[maybe_unused]] const uint32_t moff = model_off<MS>(p.model_ids, p.mstride, b);
        // the previous frame's last block has left its tiles (TAILF: its fold has left t3, and its planes are out).  The FIRST frame
        // of a workgroup (at b <= CUs the only one) has nothing to wait for: its weights and tile requests go out at once (round 6)
        if (b != (int)blockIdx.x) lds_barrier();
        PHASE_MARK(0);
        if constexpr (TAILF) {   // (behind the barrier: the previous frame's t3 lay over them)
            const int tid_f = opaque_v(tid);
            dec012_zero_border<128>(t0, p.lv[0], tid_f);
            dec012_zero_border<128>(t1, p.lv[1], tid_f);
        }
        {
            // The three tiles are requested FIRST, block 0's weights behind them, and the barrier waits for the tiles alone: the
            // vector-memory counter returns in order, so "at most DEC012_W0_KEPT operations outstanding" says that everything
            // older than the youngest DEC012_W0_KEPT has landed -- the tile requests are older than all of block 0's loads (32
            // fragments, then its constants; the fragments cannot merge, so there are never fewer).  The weights stay in flight
            // across the barrier and the first tile takes them fragment by fragment.  The scheduling barriers keep the three
            // groups -- requests, loads, wait -- in this order.
            // (the rows of the three tiles start at different waves so that the requests spread evenly)
            dec012_stage<0, 128>(t0, p.skip[0] + (size_t)b * p.Ts[0] * p.lv[0].Hi * p.lv[0].Wi * 128, p.lv[0], wave, lane, 0);
            dec012_stage<64, 64>(t1, p.skip[1] + (size_t)b * p.Ts[1] * p.lv[1].Hi * p.lv[1].Wi * 64, p.lv[1], wave, lane, p.lv[0].Hi & 7);
            dec012_stage<32, 32>(t2, p.skip[2] + (size_t)b * p.Ts[2] * p.lv[2].Hi * p.lv[2].Wi * 32, p.lv[2], wave, lane,
                                 (p.lv[0].Hi + p.lv[1].Hi) & 7);
            __builtin_amdgcn_sched_barrier(0);
            Dec012W<128, 64> w0;
            dec012_load(w0, at_model(p.wf[0], moff), at_model(p.epi[0], moff), wave, lane);
            __builtin_amdgcn_sched_barrier(0);
            PHASE_MARK(1);   // requesting the three tiles and block 0's weights
            lds_barrier_vmem_but<DEC012_W0_KEPT>();
            PHASE_MARK(2);   // tiles landing
            dec012_block<0, 128, 64, 128>(smem, t0, t1, nullptr, nullptr, w0, p.lv[0], p.lv[1], wave, lane);
        }
        PHASE_MARK(3);       // block 0: tiles
        {
            Dec012W<128, 32> w1;
            dec012_load(w1, at_model(p.wf[1], moff), at_model(p.epi[1], moff), wave, lane);
            lds_barrier();   // block 0's output is in block 1's tile
#ifdef PHASE_TIMING
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
            PHASE_MARK(4);   // block 1: weights + barrier
            dec012_block<64, 64, 32, 64>(smem, t1, t2, nullptr, nullptr, w1, p.lv[1], p.lv[2], wave, lane);
        }
        PHASE_MARK(5);       // block 1: tiles
        [[maybe_unused]] std::conditional_t<TAILF, Dec012Fold, Dec012NoFold> fold;
        {
            Dec012W<64, 16> w2;
            dec012_load(w2, at_model(p.wf[2], moff), at_model(p.epi[2], moff), wave, lane);
            lds_barrier();
#ifdef PHASE_TIMING
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
            PHASE_MARK(6);   // block 2: weights + barrier
            if constexpr (!TAILF) {
                dec012_block<32, 32, 16, 0>(smem, t2, nullptr, p.out + (size_t)b * p.lv[2].Hd * p.lv[2].Wd * 16, smem + p.scr_off, w2,
                                            p.lv[2], p.lv[2], wave, lane);
            } else {
                // t0 and t1 are dead from the barrier above on: t3's border and the planes as zeros (disjoint from what block 2
                // scatters), ordered in front of the fold by the barrier behind block 2
                uint8_t *const t3 = smem + pt.lv.tile_off;
                const int tid_f = opaque_v(tid);
                dec012_zero_border<16>(t3, pt.lv, tid_f);
                for (int i = tid_f; i < pt.rows_bytes / 4; i += 512) reinterpret_cast<uint32_t *>(smem + pt.planes_off)[i] = 0;
                // the fold's loads (Dec012Fold)
                const gptr<half8> wg = as_global(pt.wfrag);
#pragma unroll
                for (int ks = 0; ks < 4; ks++) fold.wf[ks] = wg[ks * 64 + (tid_f & 63)];
                fold.fbias = pt.epi[0];
#pragma unroll
                for (int k = 0; k < DEC012_PF; k++) fold.ring[k] = dec012_part(pt, b, (tid_f >> 6) + 8 * k, tid_f & 63);
                dec012_block<32, 32, 16, 16>(smem, t2, t3, nullptr, nullptr, w2, p.lv[2], pt.lv, wave, lane);
            }
        }
        PHASE_MARK(7);       // block 2: tiles + stores
        if constexpr (TAILF) {
            // (the fold's lane values are made per frame, in this scope: hoisted out of the frame loop they would live across blocks
            // 0 and 1, which use every register the kernel has)
            const int tid = opaque_v((int)threadIdx.x), lane = tid & 63, wave = tid >> 6;
            const DecLvl &g = pt.lv;
            const int GW = g.Wi + 1, GH = g.Hi + 1;
            const uint32_t row_b = (uint32_t)((g.Wi + 2) * 32);
            const uint8_t *const t3 = smem + g.tile_off;
            uint32_t *const planes = reinterpret_cast<uint32_t *>(smem + pt.planes_off);
            // a row of up to 32 positions is one tile, a longer one two: tile t of the frame is half t % tpr of grid row t / tpr
            const int tpr = GW > 32 ? 2 : 1, ntl = tpr * GH;
            uint32_t lc[2][2];
            tail_row_lanes(lc, GW, lane);
            lds_barrier();   // block 2's output is in t3, its border and the planes are zero
            PHASE_MARK(8);   // the fold: barrier
            for (int t0 = wave; t0 < ntl; t0 += 8 * DEC012_TI) {
                f32x4 pl[DEC012_TI];
                f32x16 acc[DEC012_TI];
#pragma unroll
                for (int j = 0; j < DEC012_TI; j++) pl[j] = fold.ring[j];
#pragma unroll
                for (int k = 0; k + DEC012_TI < DEC012_PF; k++) fold.ring[k] = fold.ring[k + DEC012_TI];
#pragma unroll
                for (int j = 0; j < DEC012_TI; j++) fold.ring[DEC012_PF - DEC012_TI + j] = dec012_part(pt, b, t0 + 8 * (DEC012_PF + j), lane);
                // the products of the iteration's tiles first: independent chains side by side (a tile past the wave's last computes
                // the iteration's first again and leaves nothing)
#pragma unroll
                for (int j = 0; j < DEC012_TI; j++) {
                    const int t = t0 + 8 * j < ntl ? t0 + 8 * j : t0;
                    acc[j] = tail_row_acc(t3, row_b, lc, fold.wf, tpr == 2 ? t >> 1 : t, tpr == 2 ? t & 1 : 0);
                }
#pragma unroll
                for (int j = 0; j < DEC012_TI; j++) {
                    const int t = t0 + 8 * j;
                    if (t < ntl)
                        tail_row_out(acc[j], pl[j], fold.fbias, 0.f, pt.logits, g.Hd, g.Wd, g.cy, g.cx, GW, b, tpr == 2 ? t >> 1 : t, tpr == 2 ? t & 1 : 0,
                                     lane, planes);
                }
            }
            PHASE_MARK(9);   // the fold: tiles
            lds_barrier();   // the frame's planes are complete
            PHASE_MARK(10);  // the fold: barrier
            {
                const uint4 *const src = reinterpret_cast<const uint4 *>(planes);
                uint4 *const dst = reinterpret_cast<uint4 *>(pt.planes_out) + (size_t)b * (pt.rows_bytes / 16);
                for (int i = tid; i < pt.rows_bytes / 16; i += 512) dst[i] = src[i];
            }
            if (pt.mask) tail_mask_from_planes<512>(planes, pt.mask + (size_t)b * g.Hd * g.Wd, g.Hd, g.Wd, pt.mW4, tid);
            PHASE_MARK(11);  // planes + mask out
        }
    }
#ifdef PHASE_TIMING
    if (tid == 0)
        for (int i = 0; i < 12; i++) atomicAdd(&g_phase[48 + i], ph_[i]);
#endif
    WGSPAN_END(3);
}

// ------------------------------------------------------------------ last decoder block + bboxcc fused
// One 16-wave workgroup per frame: the last block runs band by band (double-buffered LDS-DMA of the
// next band behind the tiles of the current one), its threshold output is assembled as the frame's
// H x W mask bytes in LDS, and bboxcc (bboxcc_body.h) runs on that LDS image in the same launch: no
// second kernel, no trip of the mask through HBM (it is still written out when the caller asks for
// it).  bboxcc's LDS region reuses the two band buffers.
struct Dec3ccArgs {
    DecArgs d;                 // the last block's arguments (up, skip, logits, mask, weights, geometry, nbands)
    ccbody::CcGeom g;
    ccwave::WvGeom wg;         // run-based bboxcc (bboxcc_wave.h) when the frame's shape allows it (use_wv)
    int use_wv;
    covahip_box *boxes;        // [B][max_boxes]
    int32_t *counts;           // [B]
    int area_thresh, max_boxes;
    int tile_bytes;            // one band buffer; two of them at LDS offsets 0 and tile_bytes
    int mfull_off, cc_off;     // LDS offsets of the frame's mask bytes and of bboxcc's region
    int part_off;              // PART: LDS offset of the frame's partial logits (fp32 [Hd][Wd], DecArgs::part)
    DecMs ms;                  // MS: the stacks' models
};

// WV: the run-based bboxcc body (bboxcc_wave.h) instead of the block-based one (bboxcc_body.h); one body per instantiation, so
// that the kernel's single register allocation of 128 VGPRs (16 waves per CU) holds the tile loop and ONE bboxcc.
// PART (round 5): the block's input is its "up" half alone (16 channels, half the tile, half the products, the whole frame in
// one buffer); the skip half's share of every logit comes as fp32 partial logits from the level-1 kernel (Enc1Args::part),
// lands in LDS beside the tile and is added in the epilogue.
template <bool WV, bool PART, bool MS = false, bool POST = false>
__global__ __launch_bounds__(ccbody::CC_THREADS) void dec3cc_mfma(Dec3ccArgs q, PostArg<POST> qp) {
    constexpr int C1 = 16, C2 = PART ? 0 : 16, C = C1 + C2, NW = ccbody::CC_THREADS / 64;
    constexpr int KSTEPS = 4 * (C / 16);
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const DecArgs &p = q.d;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int TC = p.Wi + 2;
    const int GW = p.Wi + 1, GH = p.Hi + 1;
    const int kh = lane >> 5;
    float fbias = p.epi[0];
    uint8_t *const mfull = smem + q.mfull_off;
    WGSPAN_BEGIN();
#ifdef PHASE_TIMING
    unsigned long long ph_[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, last_ = __builtin_amdgcn_s_memrealtime();
#endif

    for (int b = blockIdx.x; b < p.B; b += gridDim.x) {
        const StackPost sp = stack_post<POST, MS>(qp, q.ms.model_ids, b);
        // the weight fragments are (re)loaded per frame: their registers are free again while bboxcc runs
        half8 wf[KSTEPS];
        const uint32_t moff = model_off<MS>(q.ms.model_ids, q.ms.mstride, b);
        if constexpr (MS) fbias = at_model(p.epi, moff)[0];
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ks++) wf[ks] = (MS ? at_model(p.wfrag, moff) : p.wfrag)[ks * 64 + lane];
        auto stage = [&](int u0, int u1, uint8_t *buf) { dec_stage_band<C1, C2, NW>(p, b, u0, u1 - u0, buf, wave, lane); };
        if (b != (int)blockIdx.x) lds_barrier();   // the previous frame's bboxcc is done with the band buffers it reuses (the first frame has none)
        PHASE_MARK(0);
        if constexpr (PART) dec_stage_part<NW>(p.part + (size_t)b * GH * GW * 4, GH * GW, smem + q.part_off, wave, lane);
        stage(0, GH / p.nbands, smem);
        PHASE_MARK(1);   // requesting band 0 (+ weights)
        for (int band = 0; band < p.nbands; band++) {
            uint8_t *const cur = smem + (band & 1) * q.tile_bytes;
            wait_vmem();
            lds_barrier();   // this band has landed; every wave is done with the other buffer
            PHASE_MARK(2);   // band landing
            const int u0 = band * GH / p.nbands, u1 = (band + 1) * GH / p.nbands;
            if (band + 1 < p.nbands) stage(u1, (band + 2) * GH / p.nbands, smem + ((band + 1) & 1) * q.tile_bytes);
            PHASE_MARK(3);   // requesting the next band
            const int npos = (u1 - u0) * GW;
            const int ntiles = (npos + 31) / 32;
            for (int tile = wave; tile < ntiles; tile += NW) {
                const int qi = tile * 32 + (lane & 31);
                const int qc = min(qi, npos - 1);
                const int ul = fdiv(qc, p.mGW), v = qc - ul * GW;
                const f32x16 acc = dec_tile_acc<C>(cur, TC, p.swz, wf, ul, v, kh);
                if (qi < npos && kh == 0)   // rows 0..3 = the four output parities of position (u, v)
                    dec_final_out<PART, POST>(p, sp, acc, fbias, reinterpret_cast<const f32x4 *>(smem + q.part_off), b, u0 + ul, v, mfull, 0);
            }
        }
        PHASE_MARK(4);   // tiles
        lds_barrier();   // the frame's mask is complete; the band buffers are free
        PHASE_MARK(5);   // barrier
        if (p.mask) {
            const int nbytes = p.Hd * p.Wd;
            dec_mask_out<NW * 64>(mfull, p.mask + (size_t)b * nbytes, nbytes, (nbytes & 3) == 0 && (reinterpret_cast<uintptr_t>(p.mask) & 3) == 0, tid);
        }
        PHASE_MARK(6);   // mask out
        const int area = stack_area<POST, MS>(qp, q.ms.model_ids, b, q.area_thresh);
        if constexpr (WV)
            ccwave::frame_wg<ccbody::CC_THREADS>(mfull, smem + q.cc_off, q.wg, area, q.boxes + (size_t)b * q.max_boxes,
                                                 q.counts + b, q.max_boxes, tid);
        else
            ccbody::bboxcc_frame(mfull, smem + q.cc_off, q.g, area, q.boxes + (size_t)b * q.max_boxes, q.counts + b,
                                 q.max_boxes, tid);
        PHASE_MARK(7);   // bboxcc
    }
#ifdef PHASE_TIMING
    if (tid == 0)
        for (int i = 0; i < 9; i++) atomicAdd(&g_phase[64 + i], ph_[i]);
#endif
    WGSPAN_END(4);
}

// ------------------------------------------------------------------ last decoder block + bboxcc fused, ROW tiles (round 6)
// dec3cc_mfma<true, true> spent most of its vector instructions around four products per tile: positions of a band wrap around grid rows
// at tile-dependent places (a division, four tap addresses with their swizzles per tile), every lane tests the bounds of its four
// output pixels and stores them as BYTES into the frame's mask in LDS (bank-conflicted ds_write_b8), the staging loop decomposes
// every 16-byte piece, and bboxcc then reads those bytes back and packs them into its parity planes.  Here
//   * a tile is 32 consecutive grid positions of ONE grid row (two tiles per row for rows of up to 64 positions): the row is
//     wave-uniform, a tap's fragment address is [lane constant of the tile half] + [row offset], the swizzle depends on the pixel
//     column alone ((xx >> 3) & 1: the 16 lanes of a ds_read_b128 group that fall on one bank group are 8 or 24 pixels apart);
//   * the four logits of a position are compared and BALLOTED: bit v of a ballot is output pixel (2u + py - cy, 2v + px - cx), i.e.
//     a ballot IS a piece of a parity plane of bboxcc (E = even x, O = odd x, bboxcc_wave.h) -- shifted by the crop offset and ORed
//     into the plane words by one lane; no mask bytes exist in LDS, bboxcc starts at its phase B;
//   * the mask bytes the caller asked for are expanded from the planes, 4 bytes per thread and store;
//   * the tile's skip-less input ("up" half, 16 channels) is requested row by row (a wave takes whole rows, two requests per row),
//     its border is written as zeros.
// Same products in the same order, same logit expression: logits, mask, boxes and their order are bit-identical to dec3cc_mfma<true,
// true> (tests/test_gpu_blobnet.py).  Taken when the partial-logit form runs, the frame's tile fits one buffer, a grid row has at
// most 64 positions and the run-based bboxcc body takes the shape.
// POST: the ballot compares with the stack's threshold, and once the frame's ballots are complete its planes are ANDed with the
// keep planes of the stack's model (same [row][E lo, E hi, O lo, O hi] layout, from HBM: one word per thread) -- before the mask
// bytes are expanded from them and before bboxcc reads them.
template <bool MS = false, bool POST = false>
__global__ __launch_bounds__(ccbody::CC_THREADS) void dec3cc_rows_mfma(Dec3ccArgs q, PostArg<POST> qp) {
    constexpr int NW = ccbody::CC_THREADS / 64, PS = 32;   // 16 channels per pixel
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const DecArgs &p = q.d;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int TC = p.Wi + 2, GW = p.Wi + 1, GH = p.Hi + 1;
    const int pos = lane & 31;
    const float fbias0 = p.epi[0];
    uint32_t *const planes = reinterpret_cast<uint32_t *>(smem + q.mfull_off);   // [2 BH + 2][E lo, E hi, O lo, O hi], pixel row y at y + 1
    const f32x4 *const part = reinterpret_cast<const f32x4 *>(smem + q.part_off);
    WGSPAN_BEGIN();
#ifdef PHASE_TIMING
    unsigned long long ph_[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, last_ = __builtin_amdgcn_s_memrealtime();
#endif
    uint32_t lc[2][2];
    tail_row_lanes(lc, GW, lane);
    const int row_b = TC * PS;
    for (int b = blockIdx.x; b < p.B; b += gridDim.x) {
        const uint32_t moff = model_off<MS>(q.ms.model_ids, q.ms.mstride, b);
        const float fbias = MS ? at_model(p.epi, moff)[0] : fbias0;
        const StackPost sp = stack_post<POST, MS>(qp, q.ms.model_ids, b);
        half8 wf[4];   // (re)loaded per frame: their registers are free again while bboxcc runs
#pragma unroll
        for (int ks = 0; ks < 4; ks++) wf[ks] = (MS ? at_model(p.wfrag, moff) : p.wfrag)[ks * 64 + lane];
        if (b != (int)blockIdx.x) lds_barrier();   // the previous frame's bboxcc is done with the tile buffer it reuses
        PHASE_MARK(0);
        dec_stage_part<NW>(p.part + (size_t)b * GH * GW * 4, GH * GW, smem + q.part_off, wave, lane);
        {   // the tile: rows 1 .. Hi by request (a wave takes whole rows), the border as zeros (bboxcc's arrays overwrite it every frame)
            const __half *su = p.up + (size_t)b * p.Hi * p.Wi * 16;
            const int NI = 2 * p.Wi;   // interior 16-byte pieces of a row
            for (int y = wave; y < p.Hi; y += NW) {
                const __half *rowp = su + (size_t)y * p.Wi * 16;
                uint8_t *rowl = smem + ((y + 1) * TC + 1) * PS;
                for (int q0 = 0; q0 < NI; q0 += 64) {
                    const int qq = q0 + lane, px = qq >> 1;
                    const int cb = ((qq & 1) ^ (((px + 1) >> 3) & 1)) * 8;
                    if (qq < NI) glds16(rowp + px * 16 + cb, rowl + q0 * 16);
                }
            }
            const int n_rows = 4 * TC, n_cols = 4 * p.Hi;   // top + bottom row; left + right pixel of the rows between (2 pieces per pixel)
            for (int i = tid; i < n_rows + n_cols; i += NW * 64) {
                int piece;
                if (i < n_rows) {
                    piece = i < 2 * TC ? i : (p.Hi + 1) * 2 * TC + (i - 2 * TC);
                } else {
                    const int j = i - n_rows, y = j >> 2, k = j & 3;
                    piece = (y + 1) * 2 * TC + (k < 2 ? k : (p.Wi + 1) * 2 + (k - 2));
                }
                *reinterpret_cast<uint4 *>(smem + piece * 16) = uint4{0, 0, 0, 0};
            }
            for (int i = tid; i < q.wg.rows_bytes / 4; i += NW * 64) planes[i] = 0;
        }
        PHASE_MARK(1);   // requesting the tile (+ weights)
        wait_vmem();
        lds_barrier();
        PHASE_MARK(2);   // tile landing
        for (int t = wave; t < 2 * GH; t += NW) {
            const int u = t >> 1, h = t & 1;
            if (32 * h >= GW) continue;   // rows of at most 32 positions have one tile
            const int v = 32 * h + pos;
            tail_row_tile(smem, (uint32_t)row_b, lc, wf, part[u * GW + min(v, GW - 1)], fbias, sp.thr, p.logits, p.Hd, p.Wd, p.cy, p.cx, GW, b, u, h,
                          lane, planes);
        }
        PHASE_MARK(4);   // tiles
        lds_barrier();   // the frame's planes are complete; the tile buffer is free
        if constexpr (POST) {   // pixel row y is plane row y + 1
            for (int i = tid; i < 4 * p.Hd; i += NW * 64) planes[4 + i] &= sp.planes[i];
            lds_barrier();
        }
        PHASE_MARK(5);   // barrier
        // four mask bytes per thread and store, out of the planes (W is a multiple of 8: ccwave::wv_plan; mRC = magic(Wd / 4) for this kernel)
        if (p.mask) tail_mask_from_planes<NW * 64>(planes, p.mask + (size_t)b * p.Hd * p.Wd, p.Hd, p.Wd, p.mRC, tid);
        PHASE_MARK(6);   // mask out
        ccwave::frame_wg<ccbody::CC_THREADS, true>(nullptr, smem + q.cc_off, q.wg, stack_area<POST, MS>(qp, q.ms.model_ids, b, q.area_thresh), q.boxes + (size_t)b * q.max_boxes,
                                                   q.counts + b, q.max_boxes, tid, planes);
        PHASE_MARK(7);   // bboxcc
    }
#ifdef PHASE_TIMING
    if (tid == 0)
        for (int i = 0; i < 9; i++) atomicAdd(&g_phase[64 + i], ph_[i]);
#endif
    WGSPAN_END(4);
}

// ------------------------------------------------------------------ bboxcc on the planes of dec012_mfma<.., TAILF>
// What is left of the tail when the last block has run in dec012_mfma: one 16-wave workgroup per frame copies the frame's parity
// planes ((2 BH + 2) x 16 bytes) from the workspace into LDS and runs the run-based bboxcc on them, the call dec3cc_rows_mfma makes.
struct CcPlanesArgs {
    const uint32_t *planes;    // [B][rows_bytes / 4] (BnWorkspace::planes)
    ccwave::WvGeom wg;
    covahip_box *boxes;        // [B][max_boxes]
    int32_t *counts;           // [B]
    int B, area_thresh, max_boxes;
    int cc_off, planes_off;    // LDS offsets of bboxcc's region (wg.wave_bytes) and of the planes (wg.rows_bytes)
};
__global__ __launch_bounds__(ccbody::CC_THREADS) void cc_planes(CcPlanesArgs q) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x;
    uint32_t *const planes = reinterpret_cast<uint32_t *>(smem + q.planes_off);
    WGSPAN_BEGIN();
    for (int b = blockIdx.x; b < q.B; b += gridDim.x) {
        if (b != (int)blockIdx.x) lds_barrier();   // the previous frame's bboxcc is done with its planes
        const uint4 *const src = reinterpret_cast<const uint4 *>(q.planes) + (size_t)b * (q.wg.rows_bytes / 16);
        for (int i = tid; i < q.wg.rows_bytes / 16; i += ccbody::CC_THREADS) reinterpret_cast<uint4 *>(planes)[i] = src[i];
        lds_barrier();
        ccwave::frame_wg<ccbody::CC_THREADS, true>(nullptr, smem + q.cc_off, q.wg, q.area_thresh, q.boxes + (size_t)b * q.max_boxes, q.counts + b,
                                                   q.max_boxes, tid, planes);
    }
    WGSPAN_END(4);
}

// ------------------------------------------------------------------ host-side weight preparation
// Epilogue constants of an encoder level (see pool4): the BN scale is folded into the weights.
void enc_epilogue(int cout, bool allpos, const float *bias, const float *gamma, const float *beta, const float *mean,
                  const float *var, std::vector<float> &wscale, float *epi) {
    wscale.assign(cout, 1.f);
    for (int c = 0; c < cout; c++) {
        const float sc = gamma[c] / std::sqrt(var[c] + BN_EPS), sh = beta[c] - mean[c] * sc;
        wscale[c] = sc;                      // folded into the weights whatever its sign (see pool4)
        const float bp = bias[c] * sc;
        epi[cout + c] = bp + sh;
        if (allpos) {
            epi[c] = -bp;
            epi[2 * cout + c] = 0.f;
        } else {
            epi[c] = sc >= 0.f ? -bp : -3.0e38f;          // lo
            epi[2 * cout + c] = sc >= 0.f ? 3.0e38f : -bp;  // hi
        }
    }
}

void prep_enc0(bool allpos, const float *k, const float *bias, const float *gamma, const float *beta, const float *mean,
               const float *var, const float *w1, const float *w2, _Float16 *wfrag, float *epi) {
    std::vector<float> ws;
    enc_epilogue(16, allpos, bias, gamma, beta, mean, var, ws, epi);
    // 16x16x32 B fragment: lane l: n = l&15, k = 8*(l>>4)+j.  k <-> (kernel row, pixel of the
    // 4-pixel group, channel).  Set 0 serves even-x conv pixels (group = inputs x-2..x+1, so group
    // pixel px carries tap kx = px-1), set 1 odd-x pixels (group = inputs x-1..x+2, kx = px).
    for (int set = 0; set < 2; set++)
        for (int ks = 0; ks < 2; ks++)
            for (int l = 0; l < 64; l++)
                for (int j = 0; j < 8; j++) {
                    const int n = l & 15, g = l >> 4;
                    const int px = 2 * (g & 1) + (j >> 2), ch = j & 3;
                    const int kx = set == 0 ? px - 1 : px;
                    int ky = -1;
                    if (ks == 0) ky = g >> 1;
                    else if ((g >> 1) == 0) ky = 2;
                    float w = 0.f;
                    if (ky >= 0 && kx >= 0 && kx < 3 && ch < 3) w = k[((ky * 3 + kx) * 3 + ch) * 16 + n] * ws[n] / 6.0f;
                    wfrag[((set * 2 + ks) * 64 + l) * 8 + j] = f2h(w);
                }
    std::memcpy(epi + 48, w1, 16 * sizeof(float));
    std::memcpy(epi + 64, w2, 16 * sizeof(float));
}

void prep_enc(bool allpos, int cin, int cout, const float *k, const float *bias, const float *gamma, const float *beta,
              const float *mean, const float *var, const float *w1, const float *w2, _Float16 *wfrag, float *epi) {
    const int NT = cout / 32, KC = cin / 16, KSTEPS = 9 * KC;
    std::vector<float> ws;
    enc_epilogue(cout, allpos, bias, gamma, beta, mean, var, ws, epi);
    // 32x32x16 B fragment: lane l: n = l&31, k = 8*(l>>5)+j
    for (int nt = 0; nt < NT; nt++)
        for (int ks = 0; ks < KSTEPS; ks++)
            for (int l = 0; l < 64; l++)
                for (int j = 0; j < 8; j++) {
                    const int tap = ks / KC, kc = ks % KC;
                    const int c = kc * 16 + 8 * (l >> 5) + j, n = nt * 32 + (l & 31);
                    wfrag[(((size_t)nt * KSTEPS + ks) * 64 + l) * 8 + j] = f2h(k[((size_t)tap * cin + c) * cout + n] * ws[n]);
                }
    std::memcpy(epi + 3 * cout, w1, 16 * sizeof(float));
    std::memcpy(epi + 3 * cout + 16, w2, 16 * sizeof(float));
}

// level 1 for enc1_mfma: 16x16x32 B fragment, lane l: n = l & 15, k = 8 * (l >> 4) + j; one K step = two taps x 16
// channels: k < 16 -> first tap of the pair, k >= 16 -> second.  Pairs (ky,kx): (0,0)|(0,1), (1,0)|(1,1), (2,0)|(2,1),
// (0,2)|(1,2), (2,2)|none.
void prep_enc1w(bool allpos, const float *k, const float *bias, const float *gamma, const float *beta, const float *mean,
                const float *var, _Float16 *wfrag) {
    static const int pairs[5][2] = {{0, 1}, {3, 4}, {6, 7}, {2, 5}, {8, -1}};
    std::vector<float> ws, epi(3 * 32);
    enc_epilogue(32, allpos, bias, gamma, beta, mean, var, ws, epi.data());
    for (int nt = 0; nt < 2; nt++)
        for (int s = 0; s < 5; s++)
            for (int l = 0; l < 64; l++)
                for (int j = 0; j < 8; j++) {
                    const int kg = l >> 4, tap = pairs[s][kg >> 1], c = 8 * (kg & 1) + j, n = nt * 16 + (l & 15);
                    wfrag[(((size_t)nt * 5 + s) * 64 + l) * 8 + j] = f2h(tap < 0 ? 0.f : k[((size_t)tap * 16 + c) * 32 + n] * ws[n]);
                }
}

void prep_dec(int cin, int cout, const float *k, const float *bias, const float *gamma, const float *beta,
              const float *mean, const float *var, _Float16 *wfrag, float *epi) {
    const int NTT = 4 * cout / 32, KC = cin / 16, KSTEPS = 4 * KC;
    for (int nt = 0; nt < NTT; nt++)
        for (int ks = 0; ks < KSTEPS; ks++)
            for (int l = 0; l < 64; l++)
                for (int j = 0; j < 8; j++) {
                    const int tap = ks / KC, kc = ks % KC, a = tap >> 1, bb = tap & 1;
                    const int c = kc * 16 + 8 * (l >> 5) + j, n = nt * 32 + (l & 31);
                    const int phase = n / cout, co = n % cout, py = phase >> 1, px = phase & 1;
                    const int ky = py + 2 * a, kx = px + 2 * bb;
                    wfrag[(((size_t)nt * KSTEPS + ks) * 64 + l) * 8 + j] =
                        f2h(k[(((size_t)ky * 4 + kx) * cout + co) * cin + c]);
                }
    // epilogue: relu((acc + bias) * scale + shift) = relu(acc * scale + (bias * scale + shift))
    for (int c = 0; c < cout; c++) {
        const float sc = gamma[c] / std::sqrt(var[c] + BN_EPS);
        epi[c] = sc;
        epi[cout + c] = bias[c] * sc + (beta[c] - mean[c] * sc);
    }
}

// last block folded with the final 1x1 conv: logit = sum_c fk[c]*(convT_c(x) + b_c) + fb.
// Rows 0..3 of the single 32-row tile are the four parities, the rest are zero.
// folded weight of (parity n, tap (a, bb), input channel c): sum over the 16 intermediate channels
float final_fold(int cin, int cout, const float *k, const float *fk, int n, int a, int bb, int c) {
    const int ky = (n >> 1) + 2 * a, kx = (n & 1) + 2 * bb;
    double sacc = 0.0;
    for (int o = 0; o < cout; o++) sacc += (double)fk[o] * k[(((size_t)ky * 4 + kx) * cout + o) * cin + c];
    return (float)sacc;
}
// cwin input channels starting at c0 (the whole concatenated input, or its "up" half alone)
void prep_final(int cin, int cout, const float *k, const float *bias, const float *fk, const float *fb,
                _Float16 *wfrag, float *epi, int c0 = 0, int cwin = 0) {
    if (!cwin) cwin = cin;
    const int KC = cwin / 16, KSTEPS = 4 * KC;
    for (int ks = 0; ks < KSTEPS; ks++)
        for (int l = 0; l < 64; l++)
            for (int j = 0; j < 8; j++) {
                const int tap = ks / KC, kc = ks % KC, a = tap >> 1, bb = tap & 1;
                const int c = c0 + kc * 16 + 8 * (l >> 5) + j, n = l & 31;
                wfrag[((size_t)ks * 64 + l) * 8 + j] = f2h(n < 4 ? final_fold(cin, cout, k, fk, n, a, bb, c) : 0.f);
            }
    if (epi) {
        double bsum = fb[0];
        for (int o = 0; o < cout; o++) bsum += (double)fk[o] * bias[o];
        epi[0] = (float)bsum;
    }
}
// The skip half of the same fold for the level-1 kernel (enc1_mfma's partial logits): fragments of v_mfma_f32_16x16x32_f16 whose
// row / column index i < 4 is the output parity and whose K index follows enc1_mfma's main convolution: for a position (y, x) K step
// 0 holds input row y - 1 (a = 1) and K step 1 row y (a = 0); within a step k < 16 is column x - 1 (bb = 1), k >= 16 column x
// (bb = 0).  A[i][k] and B[k][n] of that instruction share the lane decomposition (lane = 16 * (k / 8) + i), so ONE set serves the
// tiles of the main convolution (weights as the B operand) and the edge pass (weights as the A operand).
void prep_tail(int cin, int cout, const float *k, const float *fk, int c0, _Float16 *wfrag) {
    for (int s = 0; s < 2; s++)
        for (int l = 0; l < 64; l++)
            for (int j = 0; j < 8; j++) {
                const int i = l & 15, kg = l >> 4, c = c0 + 8 * (kg & 1) + j;
                wfrag[((size_t)s * 64 + l) * 8 + j] = f2h(i < 4 ? final_fold(cin, cout, k, fk, i, 1 - s, 1 - (kg >> 1), c) : 0.f);
            }
}

// ------------------------------------------------------------------ LDS bank-conflict model (host)
// A ds_read_b128 is served in four groups of 16 lanes ({0-3,12-15,20-27}, {4-11,16-19,28-31} and the
// same + 32); a group takes one LDS cycle per distinct address that falls into the same 16-byte slot
// column (byte address / 16 mod 16) -- MI355X_MICROARCH.md, LDS section.  model_* replay the fragment
// reads of a level for one band geometry and return the LDS cycles; choose_swz scans the swizzle
// family of swz_eval for the cheapest member.
inline int swz_host(const Swz &w, int cpp, int xx, int yy) {
    return ((((yy * w.L + xx) >> w.p) * w.a) + yy * w.b + (yy & 1) * w.c) & (cpp - 1);
}
inline long long lds_cycles(const int (&addr)[64]) {
    static const int grp[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                   {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                   {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
                                   {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
    long long tot = 0;
    for (int g = 0; g < 4; g++) {
        int cnt[16] = {0}, worst = 0;
        for (int k = 0; k < 16; k++) {
            const int a = addr[grp[g][k]];
            bool dup = false;
            for (int j = 0; j < k; j++) dup = dup || addr[grp[g][j]] == a;
            if (!dup) worst = std::max(worst, ++cnt[(a >> 4) & 15]);
        }
        tot += worst;
    }
    return tot;
}
// encoder level: tiles of 8 pool windows x 4 positions (enc_mfma), band of rb window rows
long long model_enc(int cin, int W, int Wp, int rb, const Swz &w) {
    const int TC = W + 2, PS = cin * 2, KC = cin / 16, CPP = cin / 8, nwin = rb * Wp;
    long long tot = 0;
    for (int tile = 0; tile < (nwin + 7) / 8; tile++)
        for (int ky = 0; ky < 3; ky++)
            for (int kx = 0; kx < 3; kx++)
                for (int kc = 0; kc < KC; kc++) {
                    int addr[64];
                    for (int lane = 0; lane < 64; lane++) {
                        const int m = lane & 31, kh = lane >> 5;
                        const int win = std::min(tile * 8 + (m >> 2), nwin - 1);
                        const int wy = win / Wp, wx = win % Wp;
                        const int yy = 2 * wy + ((m >> 1) & 1) + ky, xx = 2 * wx + (m & 1) + kx;
                        addr[lane] = (yy * TC + xx) * PS + (((kc * 2 + kh) ^ swz_host(w, CPP, xx, yy)) * 16);
                    }
                    tot += lds_cycles(addr);
                }
    return tot;
}
// encoder level on ROW-ALIGNED tiles (enc_mfma<.., TSZ>): eight windows of one window row; lanes of windows past the row's end
// read on (what they fetch is discarded, but their bank conflicts count).  Two window rows cover every (tile column, row parity)
// a periodic swizzle can tell apart.
long long model_enc_rows(int cin, int W, int Wp, const Swz &w) {
    const int TC = W + 2, PS = cin * 2, KC = cin / 16, CPP = cin / 8;
    long long tot = 0;
    for (int tc = 0; tc < (Wp + 7) / 8; tc++)
        for (int wy = 0; wy < 2; wy++)
            for (int ky = 0; ky < 3; ky++)
                for (int kx = 0; kx < 3; kx++)
                    for (int kc = 0; kc < KC; kc++) {
                        int addr[64];
                        for (int lane = 0; lane < 64; lane++) {
                            const int m = lane & 31, kh = lane >> 5;
                            const int yy = 2 * wy + ((m >> 1) & 1) + ky, xx = 2 * (8 * tc + (m >> 2)) + (m & 1) + kx;
                            addr[lane] = (yy * TC + xx) * PS + (((kc * 2 + kh) ^ swz_host(w, CPP, xx, yy)) * 16);
                        }
                        tot += lds_cycles(addr);
                    }
    return tot;
}
// decoder block: tiles of 32 consecutive grid positions (dec_mfma), band of nu grid rows
long long model_dec(int C, int Wi, int nu, const Swz &w) {
    const int TC = Wi + 2, PS = C * 2, KC = C / 16, CPP = C / 8, GW = Wi + 1, npos = nu * GW;
    long long tot = 0;
    for (int tile = 0; tile < (npos + 31) / 32; tile++)
        for (int a = 0; a < 2; a++)
            for (int b = 0; b < 2; b++)
                for (int kc = 0; kc < KC; kc++) {
                    int addr[64];
                    for (int lane = 0; lane < 64; lane++) {
                        const int q = std::min(tile * 32 + (lane & 31), npos - 1);
                        const int yy = q / GW + 1 - a, xx = q % GW + 1 - b;
                        addr[lane] = (yy * TC + xx) * PS + (((kc * 2 + (lane >> 5)) ^ swz_host(w, CPP, xx, yy)) * 16);
                    }
                    tot += lds_cycles(addr);
                }
    return tot;
}
std::mutex g_swz_mutex;
// enc = true: (C = cin, W, Wp, rows = rb); enc = false: (C, W = Wi, rows = nu).  Results are cached per key.
Swz choose_swz(bool enc, int C, int W, int Wp, int rows) {
    struct Key { bool enc; int C, W, Wp, rows; Swz s; };
    static std::vector<Key> cache;
    std::lock_guard<std::mutex> lock(g_swz_mutex);
    for (auto &k : cache)
        if (k.enc == enc && k.C == C && k.W == W && k.Wp == Wp && k.rows == rows) return k.s;
    const int cpp = C / 8, TC = W + 2;
    Swz best{0, 0, 0, 0, 0};
    long long best_cost = -1;
    const long long ideal = enc ? 4LL * ((rows * Wp + 7) / 8) * 9 * (C / 16) : 4LL * ((rows * (W + 1) + 31) / 32) * 4 * (C / 16);
    static const int mult[3] = {0, 1, 3};
    bool done = false;
    for (int L = 0; L <= TC && !done; L += TC)
        for (int p = 0; p < 3 && !done; p++)
            for (int ai = 0; ai < 3 && !done; ai++)
                for (int b = 0; b < cpp && !done; b++)
                    for (int c = 0; c < cpp && !done; c++) {
                        const Swz w{p, mult[ai] % cpp, b, c, L};
                        const long long cost = enc ? model_enc(C, W, Wp, rows, w) : model_dec(C, W, rows, w);
                        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = w; }
                        if (ideal && cost == ideal) done = true;   // conflict free
                    }
    cache.push_back(Key{enc, C, W, Wp, rows, best});
    return best;
}

// The member of the family that is periodic over 16 pixels and 2 rows (L = 0, b = 0, (16 >> p) * a = 0 mod chunks per pixel)
// with the fewest conflicts on row-aligned tiles: what enc_mfma<.., TSZ> needs for its per-kernel lane constants.
Swz choose_swz_periodic(int C, int W, int Wp) {
    struct Key { int C, W, Wp; Swz s; };
    static std::vector<Key> cache;
    std::lock_guard<std::mutex> lock(g_swz_mutex);
    for (auto &k : cache)
        if (k.C == C && k.W == W && k.Wp == Wp) return k.s;
    const int cpp = C / 8;
    Swz best{0, 0, 0, 0, 0};
    long long best_cost = -1;
    for (int p = 0; p < 4; p++)
        for (int a = 0; a < cpp; a++) {
            if (((16 >> p) * a) % cpp) continue;
            for (int c = 0; c < cpp; c++) {
                const Swz w{p, a, 0, c, 0};
                const long long cost = model_enc_rows(C, W, Wp, w);
                if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = w; }
            }
        }
    cache.push_back(Key{C, W, Wp, best});
    return best;
}

// PAIRED item order (see ItemPlan) when it applies: exactly two workgroups per CU, an even band count of at most 16,
// whole frames per pair.  Bands are the balanced partition the kernels use: band k has ((k+1)*Hp)/nb - (k*Hp)/nb rows.
ItemPlan make_plan(int grid, int num_cu, int wgs_per_cu, int batch, int nbands, int Hp) {
    ItemPlan pl{};
    if (wgs_per_cu != 2 || grid != 2 * num_cu || (nbands & 1) || nbands > 16 || batch * nbands < grid) return pl;
    std::vector<int> order(nbands);
    for (int k = 0; k < nbands; k++) order[k] = k;
    auto rows = [&](int k) { return ((k + 1) * Hp) / nbands - (k * Hp) / nbands; };
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return rows(x) > rows(y); });
    pl.paired = 1;
    pl.cnt[0] = pl.cnt[1] = nbands / 2;
    for (int k = 0; k < nbands / 2; k++) {
        pl.band[0] |= (unsigned long long)order[k] << (8 * k);                 // the larger bands: first (older, faster) workgroup
        pl.band[1] |= (unsigned long long)order[nbands / 2 + k] << (8 * k);
    }
    return pl;
}


// What every kernel here that needs more than the default 64 KB of dynamic LDS is opened to (covahip_open_lds): the 160 KB a CU
// has, minus the 256 B the runtime keeps.
constexpr size_t LDS_LIMIT = 160 * 1024 - 256;
// A decoder band (plan_dec_block, plan_tail_fused): its grid rows when a frame's GH rows are cut into nb bands (the largest band's),
// and the bytes of its input tile -- one input row more than grid rows, as a multiple of 16.
inline int band_rows(int GH, int nb) { return (GH + nb - 1) / nb; }
inline size_t band_tile_bytes(int rows, size_t row_bytes) { return (((size_t)rows + 1) * row_bytes + 15) & ~(size_t)15; }
// Whether run_dec012 takes the form that ends in planes (dec012_mfma<.., TAILF> + cc_planes) on its own where it applies; the
// developer switches reach it either way (DESIGN.md section 6 has the measurement that decides this).
constexpr bool TAIL_IN_DEC012_AUTO = true;

// Run-time bools as template arguments: with_bools(f, b0, b1, ..) calls f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ..)
// and returns its code, so that a generic lambda names a kernel family once and instantiates one kernel per combination of
// its own bools (and no other: combinations that never run, such as PRE with CIN != 16, are kept apart by separate calls).
template <typename F>
int with_bools(F &&f) {
    return f();
}
template <typename F, typename... Bs>
int with_bools(F &&f, bool b, Bs... bs) {
    return b ? with_bools([&](auto... rest) { return f(std::true_type{}, rest...); }, bs...)
             : with_bools([&](auto... rest) { return f(std::false_type{}, rest...); }, bs...);
}

// Band planner of the encoder levels: bands of whole pool-window rows.  Workgroups are persistent (`slots` of them on the
// device) and take items round-robin, so a launch lasts ceil(items / slots) rounds of one band each; a band costs its window
// rows plus about one row of halo staging + barriers.  Returns the band count whose bands (of at most rb window rows) pass
// fits(rb) and that minimises rounds x (rows + 1) -- the smallest such count -- or 0 when no band count fits.
template <typename Fit>
int plan_bands(int Hp, int batch, long long slots, Fit fits) {
    long long best = -1;
    int nbands = 0;
    for (int nb = 1; nb <= Hp; nb++) {
        const int rb = (Hp + nb - 1) / nb;  // max window rows per band
        if (!fits(rb)) continue;
        const long long rounds = ((long long)batch * nb + slots - 1) / slots;
        const long long cost = rounds * (rb + 1);
        if (best < 0 || cost < best) { best = cost; nbands = nb; }
    }
    return nbands;
}

}  // namespace

int blobnet_prepare_mfma(covahip_ctx *ctx, covahip_blobnet *m, const float *const *ws, int n_models) {
    const BnEncOff *const he = BN_LAYOUT.enc;   // where the tensors lie in a model's parameters (blobnet_params.h)
    const BnDecOff *const hd = BN_LAYOUT.dec;

    Prepared *pr = new Prepared();
    size_t off = 0;
    for (int i = 0; i < BN_LEVELS; i++) {
        const int ci = m->enc_c[i], co = m->enc_c[i + 1];
        const size_t nfrag = (i == 0) ? 4 * 64 : (size_t)(co / 32) * (9 * ci / 16) * 64;
        pr->enc[i].wfrag = off; off = align256(off + nfrag * 16);
        pr->enc[i].epi = off; off = align256(off + (3 * co + 32) * sizeof(float));
    }
    for (int j = 0; j < BN_LEVELS - 1; j++) {
        const int ci = m->dec_ci[j], co = m->dec_co[j];
        const size_t nfrag = (size_t)(4 * co / 32) * (4 * ci / 16) * 64;
        pr->dec[j].wfrag = off; off = align256(off + nfrag * 16);
        pr->dec[j].epi = off; off = align256(off + 3 * co * sizeof(float));
    }
    pr->enc1w = off; off = align256(off + (size_t)2 * 5 * 64 * 16);
    pr->final_w = off; off = align256(off + (size_t)(4 * m->dec_ci[3] / 16) * 64 * 16);
    pr->final_epi = off; off = align256(off + 16 * sizeof(float));
    pr->final_w_up = off; off = align256(off + (size_t)4 * 64 * 16);
    pr->tail_w = off; off = align256(off + (size_t)2 * 64 * 16);
    pr->zero = off; off = align256(off + 256);
    pr->total = off;

    // the K models lie `off` bytes apart; allpos (which kernel template and which epilogue form) is shared by the set
    std::vector<uint8_t> host_all(off * (size_t)n_models, 0);
    for (int i = 0; i < BN_LEVELS; i++) pr->allpos[i] = true;
    for (int k = 0; k < n_models; k++)
        for (int i = 0; i < BN_LEVELS; i++)
            for (int c = 0; c < m->enc_c[i + 1]; c++) pr->allpos[i] = pr->allpos[i] && ws[k][he[i].gamma + c] >= 0.f;
    for (int k = 0; k < n_models; k++) {
        const float *const w = ws[k], *const fk = w + BN_LAYOUT.fk, *const fb = w + BN_LAYOUT.fb;
        uint8_t *const host = host_all.data() + (size_t)k * off;
        prep_enc0(pr->allpos[0], w + he[0].k, w + he[0].b, w + he[0].gamma, w + he[0].beta, w + he[0].mean, w + he[0].var, w + he[0].w1,
                  w + he[0].w2, (_Float16 *)(host + pr->enc[0].wfrag), (float *)(host + pr->enc[0].epi));
        for (int i = 1; i < BN_LEVELS; i++)
            prep_enc(pr->allpos[i], m->enc_c[i], m->enc_c[i + 1], w + he[i].k, w + he[i].b, w + he[i].gamma, w + he[i].beta, w + he[i].mean,
                     w + he[i].var, w + he[i].w1, w + he[i].w2, (_Float16 *)(host + pr->enc[i].wfrag),
                     (float *)(host + pr->enc[i].epi));
        if (m->enc_c[1] == 16 && m->enc_c[2] == 32)
            prep_enc1w(pr->allpos[1], w + he[1].k, w + he[1].b, w + he[1].gamma, w + he[1].beta, w + he[1].mean, w + he[1].var,
                       (_Float16 *)(host + pr->enc1w));
        for (int j = 0; j < BN_LEVELS - 1; j++)
            prep_dec(m->dec_ci[j], m->dec_co[j], w + hd[j].k, w + hd[j].b, w + hd[j].gamma, w + hd[j].beta, w + hd[j].mean, w + hd[j].var,
                     (_Float16 *)(host + pr->dec[j].wfrag), (float *)(host + pr->dec[j].epi));
        prep_final(m->dec_ci[3], m->dec_co[3], w + hd[3].k, w + hd[3].b, fk, fb, (_Float16 *)(host + pr->final_w),
                   (float *)(host + pr->final_epi));
        if (m->dec_ci[3] == 32) {   // the last block's input = concat(up 16, skip 16): decoder.py:122-134
            prep_final(32, m->dec_co[3], w + hd[3].k, w + hd[3].b, fk, fb, (_Float16 *)(host + pr->final_w_up), nullptr, 0, 16);
            prep_tail(32, m->dec_co[3], w + hd[3].k, fk, 16, (_Float16 *)(host + pr->tail_w));
        }
    }
    m->prep = pr;   // (released with the model whatever happens below)
    COVAHIP_CHECK_HIP(ctx, hipMalloc(&m->d_prepared, host_all.size()));
    COVAHIP_CHECK_HIP(ctx, hipMemcpy(m->d_prepared, host_all.data(), host_all.size(), hipMemcpyHostToDevice));
    m->prepared_bytes = host_all.size();
    m->n_models = n_models;
    return COVAHIP_OK;
}

void blobnet_release_mfma(covahip_ctx *, covahip_blobnet *m) {
    if (m->d_prepared) hipFree(m->d_prepared);
    m->d_prepared = nullptr;
    delete m->prep;
    m->prep = nullptr;
}

// ------------------------------------------------------------------ the forward: one function per stage
namespace {

// What the stages of one forward share.  part_written is the one thing a stage tells a later one.
struct Fwd {
    covahip_ctx *ctx;
    const covahip_blobnet *m;
    const Prepared *pr;
    BnWorkspace &ws;
    const BnInput &inp;
    int batch;
    const uint8_t *prep;       // the batch's model; of a mixed batch model 0 (every item adds its model's mstride)
    uint32_t mstride;
    bool ms;                   // a mixed batch: the MS = true instantiations
    bool dry;                  // planning only: every check runs, no kernel is launched
    bool by_frames;
    int num_cu;
    const uint8_t *d_frames;   // carrier frames (the stacked tensor is B * T of them with an implicit table)
    int n_frames;
    const int32_t *d_index;
    float *d_logits;
    uint8_t *d_mask;
    const BnCcTail *cc;
    bool part_written = false;   // the level-1 kernel wrote partial logits instead of the level-0 skip tensor
    bool post = false;           // some model has non-default post-processing: the POST = true kernels, with these arguments
    DecPost pp{};
};

template <bool POST>
PostArg<POST> post_arg(const Fwd &f) {
    if constexpr (POST) return f.pp;
    else return DecNoPost{};
}

// One launch: opens the kernel's dynamic-LDS limit (covahip_open_lds: nothing to do up to 64 KB), brackets the launch for the
// profile as `name` and launches -- unless the pass is planning only, which goes through every check and still opens the limit
// (this is how covahip_blobnet_load opens the kernels before the first forward).  Returns the opener's code; the launch's own
// error is launched()'s.
template <typename K, typename... A>
int launch(const Fwd &f, const char *name, K kernel, int grid, int block, size_t lds, const A &...args) {
    if (int rc = covahip_open_lds(f.ctx, kernel, lds, LDS_LIMIT)) return rc;
    ProfScope ps(f.ctx, name);
    if (!f.dry) hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds, f.ctx->stream, args...);
    return COVAHIP_OK;
}
// the end of a stage: launch()'s code, then the launch's own error
int launched(const Fwd &f, int rc) {
    if (rc) return rc;
    COVAHIP_CHECK_HIP(f.ctx, hipGetLastError());
    return COVAHIP_OK;
}

// Level 0 up to the pool runs ONCE per carrier frame (enc0p_mfma -> P); level 1 gathers the four frames of a stack,
// applies level 0's temporal MLP while staging and writes the decoder's skip slice.  The stacked tensor of the other
// entry point is B * T carrier frames with an implicit table (stack b = frames 4b .. 4b+3).
int run_enc0p(const Fwd &f) {
    const covahip_blobnet *m = f.m;
    const Prepared *pr = f.pr;
    const int H = m->lv[0].H, W = m->lv[0].W, Hp = H / 2, Wp = W / 2;
    const int TC = ((W + 4 - 16 + 31) / 32) * 32 + 16;
    if (W % 4) return COVAHIP_ERR_UNSUPPORTED;
    // bands of whole pool-window rows: at most 2 * WG0 16-byte pieces per band (two per thread), <= 38 KB of LDS
    int nbands = 0;
    for (int nb = 1; nb <= Hp; nb++) {
        const int rb = (Hp + nb - 1) / nb, n2 = 2 * rb + 2;
        if (n2 * (W / 4) > 2 * WG0 || (size_t)n2 * TC * 8 > 30 * 1024) continue;
        if ((long long)f.n_frames * nb < 2LL * f.num_cu && nb < Hp) continue;   // keep every CU busy
        nbands = nb;
        break;
    }
    if (!nbands) return COVAHIP_ERR_UNSUPPORTED;
    const int rbmax = (Hp + nbands - 1) / nbands;
    const size_t tile_bytes = (((size_t)(2 * rbmax + 2) * TC * 8) + 15) & ~(size_t)15;
    Enc0pArgs a;
    a.in = f.d_frames; a.out = f.ws.pbuf;
    a.wfrag = (const half8 *)(f.prep + pr->enc[0].wfrag); a.epi = (const float *)(f.prep + pr->enc[0].epi);
    a.F = f.n_frames; a.H = H; a.W = W; a.Hp = Hp; a.Wp = Wp; a.Ho = m->lv[1].H; a.Wo = m->lv[1].W;
    a.oy = H & 1; a.ox = W & 1; a.nbands = nbands; a.TC = TC;
    a.mWp = magic(Wp); a.mNb = magic(nbands); a.mW4 = magic(W / 4); a.scr_off = (int)tile_bytes;
    a.model_ids = f.inp.frame_models; a.mstride = f.mstride;
    const size_t lds = tile_bytes + (size_t)(WG0 / 64) * 1024;
    // three persistent workgroups per CU: measured 13.9 - 14.6 us at 280 frames against 15.0 with four (the kernel sits
    // on its latency floor: band count 3 .. 7 and 2 .. 4 workgroups per CU all land within 1.5 us)
    const int grid = std::min(f.n_frames * nbands, 3 * f.num_cu);
    return launched(f, with_bools([&](auto AP, auto PACKED, auto MS) {
        return launch(f, "enc0p_mfma", enc0p_mfma<AP.value, PACKED.value, MS.value>, grid, WG0, lds, a);
    }, pr->allpos[0], f.inp.packed, f.ms));
}

// Level 1 on enc1_mfma: bands of at most three pool-window rows (E1_TR rows per T slice), two eight-wave workgroups per CU.
// False: level 1 is run_enc_level's.  True: it ran, or failed with rc set.
bool run_enc1_tile16(Fwd &f, int &rc) {
    const covahip_blobnet *m = f.m;
    const Prepared *pr = f.pr;
    if (!bn_level1_on_enc1(f.ctx, m)) return false;   // (the predicate blobnet.hip's prepare_frames uses for the table by value)
    const int H = m->lv[1].H, W = m->lv[1].W, Hp = H / 2, Wp = W / 2;
    const int nbands = plan_bands(Hp, f.batch, 2LL * f.num_cu, [](int rb) { return 2 * rb + 2 <= E1_TR; });
    if (!nbands) return false;
    Enc1Args a;
    a.in = f.ws.pbuf; a.out = f.ws.act[2];
    a.wfrag = (const half8 *)(f.prep + pr->enc1w); a.epi = (const float *)(f.prep + pr->enc[1].epi);
    a.B = f.batch; a.H = H; a.W = W; a.Hp = Hp; a.Wp = Wp; a.Ho = m->lv[2].H; a.Wo = m->lv[2].W;
    a.oy = H & 1; a.ox = W & 1; a.nbands = nbands;
    a.mWp = magic(Wp); a.mRC = magic(2 * (W + 2));
    a.scr_off = BN_T * E1_TSZ;
    const int grid = std::min(f.batch * nbands, 2 * f.num_cu);
    a.plan = make_plan(grid, f.num_cu, 2, f.batch, nbands, Hp);
    a.pidx = f.d_index; a.skip = f.ws.act[1]; a.tm_pre = (const float *)(f.prep + pr->enc[0].epi) + 48;
    // the level-0 skip connection as partial logits instead of a tensor (Enc1Args::part)
    f.part_written = m->tail_part && f.ws.part && m->dec_ci[3] == 32 && m->dec_co[3] == 16 && m->enc_c[1] == 16;
    a.part = f.part_written ? f.ws.part : nullptr;
    a.wtail = (const half8 *)(f.prep + pr->tail_w);
    a.mXe = magic(2 * Wp);
    a.use_ktab = 0;
    if (f.by_frames && f.inp.h_index && f.batch <= BN_KTAB_STACKS) {
        a.use_ktab = 1;
        for (int k = 0; k < f.batch * BN_T; k++) a.ktab[k] = (uint16_t)f.inp.h_index[k];
    } else if (f.by_frames && !f.d_index && !f.dry) {
        rc = COVAHIP_ERR_INVALID_ARG;
        return true;
    }
    const size_t lds = (size_t)BN_T * E1_TSZ + 8 * 1024 + E1_CONST;   // (twice this fits a CU's 160 KB)
    a.model_ids = f.inp.model_ids; a.mstride = f.mstride;
    rc = launched(f, with_bools([&](auto AP, auto MS) {
        return launch(f, "enc1_mfma", enc1_mfma<AP.value, MS.value>, grid, 512, lds, a);
    }, pr->allpos[1], f.ms));
    return true;
}

// Levels 2 + 3 in one launch (enc23_mfma) when a ring row holds level 2's row, its windows make at most two tile columns
// and level 3's band fits the compile-time slice stride; one workgroup per frame.
// False: the levels are run_enc_level's.  True: both ran, or failed with rc set.
bool run_enc23(const Fwd &f, int &rc) {
    const covahip_blobnet *m = f.m;
    const Prepared *pr = f.pr;
    if (!(m->fuse_enc23 && m->enc_rowtiles && !f.ctx->enc_plan[2].nbands && !f.ctx->enc_plan[3].nbands && m->enc_c[2] == 32 &&
          m->enc_c[3] == 64 && m->enc_c[4] == 128))
        return false;
    const int H = m->lv[2].H, W = m->lv[2].W, Hp = H / 2, Wp = W / 2;
    const int H3 = m->lv[3].H, W3 = m->lv[3].W, Hp3 = H3 / 2, Wp3 = W3 / 2;
    const size_t lds = (size_t)BN_T * E3_TSZ + (size_t)BN_T * E23_TSZ2 + 4096;
    // ... and when it pays: one workgroup per frame wants about a frame per CU (a batch of 32 leaves seven CUs in eight idle
    // where the two launches spread a frame's bands over them: 62 -> 76 us per step at b = 32), and row-aligned tiles want rows
    // that fill their tile columns (45 x 80: 10 of 16 and 5 of 8 windows, 3 % slower than the two launches at b = 512).
    // fuse_enc23 == 2 (developer switch "enc23_force", the tests) takes it whenever it fits
    const bool pays = 4 * f.batch >= 3 * f.num_cu && 20 * Wp >= 17 * 8 * ((Wp + 7) / 8) && 20 * Wp3 >= 17 * 8 * ((Wp3 + 7) / 8);
    // a mixed batch (model sets) takes it whenever it fits: the two-launch form's level-3 kernel cannot hold a per-stack model's
    // fragments without spilling ("Model sets")
    if (!((pays || m->fuse_enc23 == 2 || f.ms) && (W + 2) * 64 <= E23_RP2 && Wp <= 16 && Hp >= 1 && Hp3 >= 1 && Wp3 >= 1 &&
          (size_t)std::max(2 * Hp3 + 2, H3 + 1) * (W3 + 2) * 128 <= (size_t)E3_TSZ && lds <= LDS_LIMIT))
        return false;
    Enc23Args a;
    a.in = f.ws.act[2]; a.mid = f.ws.act[3]; a.out = f.ws.act[4];
    a.wf2 = (const half8 *)(f.prep + pr->enc[2].wfrag); a.wf3 = (const half8 *)(f.prep + pr->enc[3].wfrag);
    a.epi2 = (const float *)(f.prep + pr->enc[2].epi); a.epi3 = (const float *)(f.prep + pr->enc[3].epi);
    a.B = f.batch;
    a.H2 = H; a.W2 = W; a.Hp2 = Hp; a.Wp2 = Wp;
    a.H3 = H3; a.W3 = W3; a.Hp3 = Hp3; a.Wp3 = Wp3; a.oy3 = H & 1; a.ox3 = W & 1;
    a.H4 = m->lv[4].H; a.W4 = m->lv[4].W; a.oy4 = H3 & 1; a.ox4 = W3 & 1;
    a.swz2 = choose_swz_periodic(32, 30, Wp); a.swz3 = choose_swz_periodic(64, W3, Wp3);
    a.ring_off = BN_T * E3_TSZ; a.xchg_off = a.ring_off + BN_T * E23_TSZ2; a.scr_off = a.ring_off;
    a.model_ids = f.inp.model_ids; a.mstride = f.mstride;
    const int grid = std::min(f.batch, f.num_cu);
    rc = launched(f, with_bools([&](auto AP2, auto AP3, auto MS) {
        return launch(f, "enc23_mfma", enc23_mfma<AP2.value, AP3.value, MS.value>, grid, 512, lds, a);
    }, pr->allpos[2], pr->allpos[3], f.ms));
    return true;
}

// Encoder level i = 1 .. 3 on enc_mfma.  Level 1 here is the round-1..3 level-1 kernel: grids wider than enc1_mfma's LDS
// row, developer band plans, set_impl(5).
int run_enc_level(const Fwd &f, int i) {
    const covahip_blobnet *m = f.m;
    const Prepared *pr = f.pr;
    const int H = m->lv[i].H, W = m->lv[i].W, Hp = H / 2, Wp = W / 2;
    const int cin = m->enc_c[i];
    const size_t px_bytes = (size_t)cin * 2;
    const int TC = W + 2;
    // band height: largest even RB whose tile (RB+2 rows, all T) fits in ~78 KB of LDS
    // (two workgroups per CU; the 64->128 level keeps 144 weight VGPRs per wave and runs one
    //  workgroup per CU with up to 150 KB)
    // output transpose scratch behind the tile: 2 KB per wave
    static const int enc_waves[BN_LEVELS] = {0, 8, 4, 8};
    int nbuf = 1, wgs_per_cu = (i == BN_LEVELS - 1) ? 1 : 2;
    int nbands = 0;
    const size_t scr_bytes = (size_t)enc_waves[i] * 2048;
    if (f.ctx->enc_plan[i].nbands) {
        // developer override (covahip_blobnet_set_enc_plan)
        nbands = std::min(f.ctx->enc_plan[i].nbands, Hp);
        nbuf = f.ctx->enc_plan[i].nbuf;
        const size_t need = (size_t)nbuf * BN_T * (2 * ((Hp + nbands - 1) / nbands) + 2) * TC * px_bytes + scr_bytes;
        if (need > LDS_LIMIT) return COVAHIP_ERR_UNSUPPORTED;
        wgs_per_cu = (i == BN_LEVELS - 1) ? 1 : (int)std::min<size_t>(2, LDS_LIMIT / need);
    } else {
        // the band count that fits in LDS and minimises rounds x (rows + 1) (plan_bands)
        const size_t lds_cap = (wgs_per_cu == 1 ? 150 * 1024 : 80 * 1024) - scr_bytes;
        nbands = plan_bands(Hp, f.batch, (long long)wgs_per_cu * f.num_cu,
                            [&](int rb) { return (size_t)BN_T * (2 * rb + 2) * TC * px_bytes <= lds_cap; });
        if (!nbands) return COVAHIP_ERR_UNSUPPORTED;
    }
    const int RB = 2 * ((Hp + nbands - 1) / nbands);
    // levels 2 and 3 on row-aligned tiles (enc_mfma<.., TSZ>) when a T slice of the band fits the kernel's compile-time
    // slice stride and a row's windows fill its tile columns about as well as the general form's tiles fill a band
    const int fix_tsz = i == 2 ? E2_TSZ : i == 3 ? E3_TSZ : 0;
    bool rowtiles = false;
    if (fix_tsz && m->enc_rowtiles && !f.ctx->enc_plan[i].nbands && cin == (i == 2 ? 32 : 64) && m->enc_c[i + 1] == 2 * cin &&
        (size_t)(RB + 2) * TC * px_bytes <= (size_t)fix_tsz) {
        long long t_rows = (long long)Hp * ((Wp + 7) / 8), t_gen = 0;
        for (int k = 0; k < nbands; k++) t_gen += ((((k + 1) * Hp) / nbands - (k * Hp) / nbands) * Wp + 7) / 8;
        rowtiles = t_rows <= t_gen;
    }
    const size_t tile_bytes = rowtiles ? (size_t)BN_T * fix_tsz : (((size_t)BN_T * (RB + 2) * TC * px_bytes) + 15) & ~(size_t)15;
    const size_t lds = nbuf * tile_bytes + scr_bytes;
    if (lds > LDS_LIMIT) return COVAHIP_ERR_UNSUPPORTED;
    const int items = f.batch * nbands;
    const int grid = std::min(items, wgs_per_cu * f.num_cu);
    EncArgs a;
    a.in = i == 1 ? f.ws.pbuf : f.ws.act[i]; a.out = f.ws.act[i + 1];
    a.wfrag = (const half8 *)(f.prep + pr->enc[i].wfrag); a.epi = (const float *)(f.prep + pr->enc[i].epi);
    a.B = f.batch; a.H = H; a.W = W; a.Hp = Hp; a.Wp = Wp; a.Ho = m->lv[i + 1].H; a.Wo = m->lv[i + 1].W;
    a.oy = H & 1; a.ox = W & 1; a.To = (i == BN_LEVELS - 1) ? 1 : BN_T;
    a.RB = RB; a.nbands = nbands; a.TR = RB + 2; a.TC = TC;
    a.mWp = magic(Wp); a.mNb = magic(nbands); a.mRC = magic(TC * (cin / 8)); a.zero = f.prep + pr->zero;
    a.nbuf = nbuf; a.buf_stride = (int)tile_bytes; a.scr_off = (int)(nbuf * tile_bytes);
    a.plan = make_plan(grid, f.num_cu, wgs_per_cu, f.batch, nbands, Hp);
    a.swz = rowtiles ? choose_swz_periodic(cin, W, Wp) : choose_swz(true, cin, W, Wp, RB / 2);
    a.pidx = f.d_index; a.skip = f.ws.act[1]; a.tm_pre = (const float *)(f.prep + pr->enc[0].epi) + 48;
    a.model_ids = f.inp.model_ids; a.mstride = f.mstride;
    const bool ap = pr->allpos[i];
    // one arm per level: PRE (level 0's temporal MLP while staging) is level 1's alone, row tiles are levels 2's and 3's
    if (i == 1) {
        // (a null table means "stack b = frames 4b .. 4b+3" to this kernel: a carrier-frame call must bring its table)
        if (f.by_frames && !f.d_index && !f.dry) return COVAHIP_ERR_INVALID_ARG;
        return launched(f, with_bools([&](auto AP, auto MS) {
            return launch(f, "enc1_mfma", enc_mfma<16, 32, 2, 4, 8, AP.value, true, 0, MS.value>, grid, 512, lds, a);
        }, ap, f.ms));
    }
    if (i == 2)
        return launched(f, with_bools([&](auto AP, auto ROWS, auto MS) {
            return launch(f, "enc2_mfma", enc_mfma<32, 64, 4, 2, 4, AP.value, false, ROWS.value ? E2_TSZ : 0, MS.value>, grid, WG, lds, a);
        }, ap, rowtiles, f.ms));
    return launched(f, with_bools([&](auto AP, auto ROWS, auto MS) {
        return launch(f, "enc3_mfma", enc_mfma<64, 128, 2, 2, 8, AP.value, false, ROWS.value ? E3_TSZ : 0, MS.value>, grid, 512, lds, a);
    }, ap, rowtiles, f.ms));
}

// The fused tail's plan (plan_tail_fused): the arguments of its launch, its LDS, and whether it is the row form.
struct TailPlan {
    Dec3ccArgs t;
    size_t lds;
    bool rows;
    bool in_dec012;   // the row tiles take the frame's geometry (run_dec012's form that ends in planes asks no more of it)
};

// Decoder blocks 0..2 in one launch when a frame's three input tiles fit in LDS together.
// False: the blocks are run_dec_block's.  True: they ran, or failed with rc set.
// tail: the fused tail's plan when row tiles take the frame's geometry (TailPlan::in_dec012), else null.  tail_in: the last block
// ran here as well (dec012_mfma<.., TAILF>) and left the frames' planes in the workspace: run_cc_planes is what remains.  That form
// is taken when the row tail would run behind this launch, for a single model without per-model post-processing, when its LDS
// plan fits -- t3 over t0 + t1, then t2, then the planes -- and when the batch fills the chip by enc23_mfma's rule (at small
// batches the existing tests pin the two launches and their intermediate dact[2]); a call that asks for the logits keeps the two
// launches and every intermediate of theirs in the workspace.  tail_in_dec012 == 2 (developer switch "tail_in_dec012") takes it
// wherever the geometry and the LDS plan allow it, whatever the batch and the outputs; 0 ("tail_separate") never.
bool run_dec012(const Fwd &f, int &rc, const TailPlan *tail, bool &tail_in) {
    const covahip_blobnet *m = f.m;
    const Prepared *pr = f.pr;
    tail_in = false;
    if (!(m->fuse_dec && m->dec_ci[0] == 128 && m->dec_ci[1] == 128 && m->dec_ci[2] == 64 && m->dec_co[0] == 64 &&
          m->dec_co[1] == 32 && m->dec_co[2] == 16))
        return false;
    Dec012Args a;
    size_t off = 0, tile_bytes[3];
    for (int j = 0; j < 3; j++) {
        const BnLevelGeom in = m->lv[BN_LEVELS - j], out = m->lv[BN_LEVELS - 1 - j];
        DecLvl &g = a.lv[j];
        g.Hi = in.H; g.Wi = in.W; g.Hd = out.H; g.Wd = out.W; g.cy = m->dec_cy[j]; g.cx = m->dec_cx[j];
        g.mGW = magic(in.W + 1);
        g.mRC = magic((in.W + 2) * (m->dec_ci[j] / 8));
        g.swz = choose_swz(false, m->dec_ci[j], in.W, 0, in.H + 1);
        g.tile_off = (int)off;
        tile_bytes[j] = align256((size_t)(in.H + 2) * (in.W + 2) * m->dec_ci[j] * 2);   // 256: dec012_block's xor addressing
        off += tile_bytes[j];
        a.skip[j] = f.ws.act[BN_LEVELS - j];
        a.Ts[j] = j == 0 ? 1 : BN_T;
        a.wf[j] = (const half8 *)(f.prep + pr->dec[j].wfrag);
        a.epi[j] = (const float *)(f.prep + pr->dec[j].epi);
    }
    a.scr_off = (int)off;
    const size_t lds = off + 8 * 2048;
    if (lds > LDS_LIMIT) return false;
    a.out = f.ws.dact[2]; a.B = f.batch; a.zero = f.prep + pr->zero;
    a.model_ids = f.inp.model_ids; a.mstride = f.mstride;
    const int grid = std::min(f.batch, f.num_cu);
    if (tail && m->tail_in_dec012 && !f.ms && !f.post && f.ws.planes &&
        (m->tail_in_dec012 == 2 || (TAIL_IN_DEC012_AUTO && tail->rows && 4 * f.batch >= 3 * f.num_cu && !f.d_logits))) {
        const DecArgs &d = tail->t.d;
        Dec012Tail t;
        t.lv = DecLvl{d.Hi, d.Wi, d.Hd, d.Wd, d.cy, d.cx, 0u, 0u, Swz{3, 1, 0, 0, 0}, 0};
        const size_t t3 = align256((size_t)(d.Hi + 2) * (d.Wi + 2) * 32);
        const size_t t2_off = std::max(tile_bytes[0] + tile_bytes[1], t3);
        const size_t planes_off = t2_off + tile_bytes[2];
        const size_t lds_t = planes_off + (size_t)tail->t.wg.rows_bytes;
        if (lds_t <= LDS_LIMIT) {
            a.lv[2].tile_off = (int)t2_off;
            a.scr_off = 0; a.out = nullptr;   // (neither exists in this form)
            t.wfrag = d.wfrag; t.epi = d.epi; t.part = d.part; t.logits = d.logits; t.mask = d.mask;
            t.planes_out = f.ws.planes;
            t.planes_off = (int)planes_off; t.rows_bytes = tail->t.wg.rows_bytes;
            t.mW4 = magic(d.Wd / 4);
            tail_in = true;
            rc = launched(f, launch(f, "dec012_mfma", dec012_mfma<false, true>, grid, 512, lds_t, a, t));
            return true;
        }
    }
    rc = launched(f, with_bools([&](auto MS) {
        return launch(f, "dec012_mfma", dec012_mfma<MS.value, false>, grid, 512, lds, a, Dec012NoTail{});
    }, f.ms));
    return true;
}
// bboxcc on the planes that dec012_mfma<.., TAILF> left in the workspace
int run_cc_planes(const Fwd &f, const TailPlan &tp) {
    CcPlanesArgs q;
    q.planes = f.ws.planes; q.wg = tp.t.wg;
    q.boxes = f.cc->boxes; q.counts = f.cc->counts;
    q.B = f.batch; q.area_thresh = f.cc->area_thresh; q.max_boxes = f.cc->max_boxes;
    q.cc_off = 0; q.planes_off = tp.t.wg.wave_bytes;
    const size_t lds = (size_t)tp.t.wg.wave_bytes + (size_t)tp.t.wg.rows_bytes;
    return launch(f, "dec3_bboxcc_fused", cc_planes, std::min(f.batch, 2 * f.num_cu), ccbody::CC_THREADS, lds, q);
}

// Decoder block j on dec_mfma (the last one carries the folded final conv + threshold): its plan, which the fused tail
// starts from, and its launch.
struct DecPlan {
    DecArgs a;
    DecMs am;
    BnLevelGeom in, out;
    bool half;   // the last block on its "up" half + partial logits
    int ci, GH, grid;
    size_t row_bytes, lds;
};
int plan_dec_block(const Fwd &f, int j, DecPlan &p) {
    const covahip_blobnet *m = f.m;
    const Prepared *pr = f.pr;
    const BnLevelGeom in = m->lv[BN_LEVELS - j], out = m->lv[BN_LEVELS - 1 - j];
    const bool last = j == BN_LEVELS - 1;
    const bool half = last && f.part_written;
    const int ci_j = half ? m->dec_ci[j] / 2 : m->dec_ci[j];
    DecArgs &a = p.a;
    a.up = j == 0 ? nullptr : f.ws.dact[j - 1];
    a.skip = f.ws.act[BN_LEVELS - j];
    a.out = last ? nullptr : f.ws.dact[j];
    a.logits = last ? f.d_logits : nullptr;
    a.mask = last ? f.d_mask : nullptr;
    a.wfrag = (const half8 *)(f.prep + (half ? pr->final_w_up : last ? pr->final_w : pr->dec[j].wfrag));
    a.part = half ? f.ws.part : nullptr;
    a.epi = (const float *)(f.prep + (last ? pr->final_epi : pr->dec[j].epi));
    a.B = f.batch; a.Hi = in.H; a.Wi = in.W; a.Hd = out.H; a.Wd = out.W; a.cy = m->dec_cy[j]; a.cx = m->dec_cx[j];
    a.Ts = j == 0 ? 1 : BN_T;
    p.am = DecMs{f.inp.model_ids, f.mstride};
    const int GH = in.H + 1;
    const size_t row_bytes = (size_t)(in.W + 2) * ci_j * 2;
    // band planner.  A workgroup keeps its M-tile's weight fragments in registers, so the weights
    // cross the L2 -> CU path once per workgroup: block 0 (256 KB of fragments per workgroup) runs
    // one workgroup per CU over whole frames.  The lighter blocks are bound by the latency of
    // stage -> barrier -> compute, which only other workgroups on the CU can hide: bands of at most
    // ~30 KB of LDS so that four to five of them are resident per CU.
    const size_t wbytes = (size_t)(last ? 1 : 4 * m->dec_co[j] / 32) * (4 * ci_j / 16) * 1024;
    const bool heavy = wbytes >= 192 * 1024 && (size_t)(GH + 1) * row_bytes <= 72 * 1024;
    int nbands = 1;
    if (!heavy)
        while (nbands < GH && (((size_t)band_rows(GH, nbands) + 1) * row_bytes > 30 * 1024 ||
                               (long long)f.batch * nbands < 2LL * f.num_cu))
            nbands++;
    a.nbands = nbands; a.mNb = magic(nbands); a.mGW = magic(in.W + 1);
    a.mRC = magic((in.W + 2) * (ci_j / 8)); a.zero = f.prep + pr->zero;
    const int rows = band_rows(GH, nbands);
    a.swz = choose_swz(false, ci_j, in.W, 0, rows);
    const size_t tile_bytes = band_tile_bytes(rows, row_bytes);
    const size_t mask_bytes = last ? ((((size_t)2 * rows * out.W) + 15) & ~(size_t)15) : 0;
    const size_t scr_bytes = last ? 0 : (size_t)std::max(4, 4 * m->dec_co[j] / 32) * 2048;   // one 2 KB transpose scratch per wave
    p.lds = tile_bytes + mask_bytes + scr_bytes;
    a.mask_off = (int)tile_bytes;
    a.scr_off = (int)tile_bytes;
    if (p.lds > LDS_LIMIT) return COVAHIP_ERR_UNSUPPORTED;
    p.in = in; p.out = out; p.half = half; p.ci = ci_j; p.GH = GH; p.row_bytes = row_bytes;
    p.grid = std::min(f.batch * nbands, (heavy ? 1 : 4) * f.num_cu);
    return COVAHIP_OK;
}
int launch_dec_block(const Fwd &f, int j, const DecPlan &p) {
    if (j == 0)
        return launched(f, with_bools([&](auto MS) {
            return launch(f, "dec0_mfma", dec_mfma<0, 128, 64, false, MS.value>, p.grid, 512, p.lds, p.a, p.am, DecNoPost{});
        }, f.ms));
    if (j == 1)
        return launched(f, with_bools([&](auto MS) {
            return launch(f, "dec1_mfma", dec_mfma<64, 64, 32, false, MS.value>, p.grid, 256, p.lds, p.a, p.am, DecNoPost{});
        }, f.ms));
    if (j == 2)
        return launched(f, with_bools([&](auto MS) {
            return launch(f, "dec2_mfma", dec_mfma<32, 32, 16, false, MS.value>, p.grid, 256, p.lds, p.a, p.am, DecNoPost{});
        }, f.ms));
    return launched(f, with_bools([&](auto HALF, auto MS, auto POST) {
        return launch(f, "dec3_final_mfma", dec_mfma<16, HALF.value ? 0 : 16, 16, true, MS.value, POST.value>, p.grid, 256, p.lds, p.a,
                      p.am, post_arg<POST.value>(f));
    }, p.half, f.ms, f.post));
}
int run_dec_block(const Fwd &f, int j) {
    DecPlan p;
    if (int rc = plan_dec_block(f, j, p)) return rc;
    return launch_dec_block(f, j, p);
}

// Last block + bboxcc in one launch when the frame's LDS plan fits: two band buffers (which bboxcc's region reuses) + the
// frame's mask bytes.  p: the last block's own plan.  False: it does not fit -- a kernel whose LDS limit cannot be opened
// counts as that -- and the block runs alone.  The plan first (the decoder launch in front of it looks at it: run_dec012), then
// the launch.
bool plan_tail_fused(const Fwd &f, const DecPlan &p, TailPlan &tp) {
    const BnLevelGeom in = p.in, out = p.out;
    const int GH = p.GH;
    Dec3ccArgs &t = tp.t;
    size_t cc_bytes = ccbody::cc_plan(out.H, out.W, t.g);
    // the run-based body (bboxcc_wave.h) when the shape allows it: worst-case run capacity, nothing overflows
    t.use_wv = f.ctx->cc_wave_cap >= 0 && ccwave::wv_plan(out.H, out.W, ((out.H + 1) / 2) * ((out.W + 1) / 2), t.wg) ? 1 : 0;
    if (t.use_wv) cc_bytes = (size_t)t.wg.wave_bytes;
    if (!cc_bytes) return false;
    const size_t mfull = ((size_t)out.H * out.W + 15) & ~(size_t)15;
    const size_t partb = p.half ? (size_t)GH * (in.W + 1) * 16 : 0;   // partial logits beside the mask
    int best_nb = 0;
    long long best_cost = -1;
    for (int nb = 1; nb <= GH; nb++) {
        const size_t tb = band_tile_bytes(band_rows(GH, nb), p.row_bytes);
        const size_t nbuf = nb == 1 ? 1 : 2;   // the whole frame in one buffer when it fits
        if (std::max(nbuf * tb, cc_bytes) + mfull + partb > LDS_LIMIT - 256) continue;
        long long rounds = 0;   // tiles of 32 positions over 16 waves, band by band
        for (int k = 0; k < nb; k++) {
            const int nu = (k + 1) * GH / nb - k * GH / nb;
            rounds += ((nu * (in.W + 1) + 31) / 32 + 15) / 16;
        }
        const long long cost = rounds * 8 + nb;   // a band costs a barrier + DMA issue on top of its tiles
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best_nb = nb; }
    }
    if (!best_nb) return false;
    const size_t tb = band_tile_bytes(band_rows(GH, best_nb), p.row_bytes);
    t.d = p.a;
    t.ms = p.am;
    t.d.nbands = best_nb; t.d.mNb = magic(best_nb);
    t.d.swz = choose_swz(false, p.ci, in.W, 0, band_rows(GH, best_nb));
    t.boxes = f.cc->boxes; t.counts = f.cc->counts;
    t.area_thresh = f.cc->area_thresh; t.max_boxes = f.cc->max_boxes;
    t.tile_bytes = (int)tb; t.cc_off = 0;
    t.mfull_off = (int)std::max((best_nb == 1 ? 1 : 2) * tb, cc_bytes);
    t.part_off = (int)((size_t)t.mfull_off + mfull);
    tp.lds = (size_t)t.part_off + partb;
    // row tiles + ballots straight into bboxcc's planes (dec3cc_rows_mfma) when the shape allows it
    // (in_dec012: what of this is geometry of the row tiles themselves, and not of this launch's LDS plan)
    tp.in_dec012 = p.half && t.use_wv && in.W + 1 <= 64 && f.m->tail_rows && (out.W & 7) == 0 &&
                   (!f.d_mask || (reinterpret_cast<uintptr_t>(f.d_mask) & 3) == 0);
    tp.rows = tp.in_dec012 && best_nb == 1 && (size_t)t.wg.rows_bytes <= mfull;
    if (tp.rows) {
        t.d.swz = Swz{3, 1, 0, 0, 0};            // s = (xx >> 3) & 1 (what the staging of both forms evaluates)
        t.d.mRC = magic(out.W / 4);               // the mask expansion's division
    }
    return true;
}
bool launch_tail_fused(const Fwd &f, const DecPlan &p, const TailPlan &tp) {
    const Dec3ccArgs &t = tp.t;
    const size_t tl = tp.lds;
    const int grid = std::min(f.batch, 2 * f.num_cu);
    if (tp.rows) {
        if (!f.dry) f.ctx->tail_form = COVAHIP_DEV_TAIL_ROWS;
        return !with_bools([&](auto MS, auto POST) {
            return launch(f, "dec3_bboxcc_fused", dec3cc_rows_mfma<MS.value, POST.value>, grid, ccbody::CC_THREADS, tl, t, post_arg<POST.value>(f));
        }, f.ms, f.post);
    }
    if (!f.dry) f.ctx->tail_form = COVAHIP_DEV_TAIL_BANDS + (t.use_wv ? 2 : 0) + (p.half ? 1 : 0);
    return !with_bools([&](auto WV, auto PART, auto MS, auto POST) {
        return launch(f, "dec3_bboxcc_fused", dec3cc_mfma<WV.value, PART.value, MS.value, POST.value>, grid, ccbody::CC_THREADS, tl, t, post_arg<POST.value>(f));
    }, t.use_wv != 0, p.half, f.ms, f.post);
}

}  // namespace

// The chain of DESIGN.md section 4: level 0 per carrier frame -> level 1 -> levels 2 and 3 -> decoder blocks 0 .. 2 -> the
// last block; at each step the fused form first, and the launches it replaces where it does not apply.
int blobnet_forward_mfma(covahip_ctx *ctx, covahip_blobnet *m, BnWorkspace &ws, const BnInput &inp, int batch, float *d_logits,
                         uint8_t *d_mask, const BnCcTail *cc, bool *cc_done) {
    if (cc_done) *cc_done = false;
    const Prepared *pr = m->prep;
    const bool dry = inp.dry;
    const bool by_frames = inp.frames != nullptr || (dry && inp.n_frames > 0);
    // model sets: a batch of one model runs the single-model kernels on that model's weights; a mixed batch runs the MS = true
    // instantiations, which take every item's weights from its model (inp.model_ids per stack, inp.frame_models per carrier frame)
    const bool ms = inp.model_ids != nullptr || (dry && inp.mixed);
    Fwd f{ctx, m, pr, ws, inp, batch,
          (const uint8_t *)m->d_prepared + (ms ? 0 : (size_t)inp.model * pr->total), (uint32_t)pr->total,
          ms, dry, by_frames, ctx->props.multiProcessorCount,
          by_frames ? inp.frames : inp.stack, by_frames ? inp.n_frames : batch * BN_T, by_frames ? inp.index : nullptr,
          d_logits, d_mask, cc};
    if ((size_t)f.n_frames > ws.pbuf_frames && !dry) return COVAHIP_ERR_INVALID_ARG;   // (the caller sizes P: blobnet.hip)
    // per-model post-processing: while every model has the defaults the kernels without it run, as before
    f.post = m->post_on;
    if (f.post) {
        if (!m->d_post) return COVAHIP_ERR_INVALID_ARG;
        const uint8_t *const dp = (const uint8_t *)m->d_post;
        const size_t k = ms ? 0 : (size_t)inp.model;
        f.pp.thr = m->post_thr[k];
        f.pp.thr_tab = (const float *)dp;
        // the area threshold: a batch of one model gets it resolved here, a mixed batch per stack from the table behind the thresholds
        f.pp.area = m->post_area[k] >= 1 ? m->post_area[k] : (cc ? cc->area_thresh : 0);
        f.pp.area_tab = (const int32_t *)(dp + m->post_area_off);
        f.pp.keep = dp + m->post_keep_off + k * m->post_keep_stride;
        f.pp.planes = (const uint32_t *)(dp + m->post_planes_off + k * m->post_planes_stride);
        f.pp.keep_stride = (uint32_t)m->post_keep_stride;
        f.pp.planes_stride = (uint32_t)m->post_planes_stride;
    }

    int rc = run_enc0p(f);
    if (rc) return rc;
    if (!run_enc1_tile16(f, rc)) rc = run_enc_level(f, 1);
    if (rc) return rc;
    if (!run_enc23(f, rc)) {
        rc = run_enc_level(f, 2);
        if (!rc) rc = run_enc_level(f, 3);
    }
    if (rc) return rc;
    // the tail's plan first: the decoder launch takes the last block in when the row tail would run behind it (run_dec012)
    DecPlan last;
    rc = plan_dec_block(f, BN_LEVELS - 1, last);
    if (rc) return rc;
    TailPlan tp;
    const bool fused = cc && m->fuse_tail && plan_tail_fused(f, last, tp);
    bool tail_in = false;
    if (!run_dec012(f, rc, fused && tp.in_dec012 ? &tp : nullptr, tail_in))
        for (int j = 0; j < BN_LEVELS - 1 && !rc; j++) rc = run_dec_block(f, j);
    if (rc) return rc;
    if (!dry) ctx->tail_in_dec012 = tail_in;
    if (tail_in) {
        if (!dry) ctx->tail_form = COVAHIP_DEV_TAIL_ROWS;   // (the row tail's text, in the decoder launch)
        if (cc_done) *cc_done = true;
        return launched(f, run_cc_planes(f, tp));
    }
    if (!(fused && launch_tail_fused(f, last, tp))) {
        if (!dry) ctx->tail_form = COVAHIP_DEV_TAIL_ALONE;
        return launch_dec_block(f, BN_LEVELS - 1, last);
    }
    if (cc_done) *cc_done = true;   // bboxcc ran in the same launch
    return launched(f, COVAHIP_OK);
}

#if defined(PHASE_TIMING) || defined(WGSPAN_ONLY)
extern "C" int covahip_dev_wgspan_read(unsigned long long *out, int kid) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wgspan), sizeof(unsigned long long) * 1024 * 4, sizeof(unsigned long long) * 1024 * 4 * kid) != hipSuccess;
}
#endif
#ifdef WGSPAN_ONLY
extern "C" int covahip_dev_itemspan_read(unsigned long long *out, int kid) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_itemspan), sizeof(unsigned long long) * 1024 * 16, sizeof(unsigned long long) * 1024 * 16 * kid) != hipSuccess;
}
#endif
#ifdef PHASE_TIMING
extern "C" int covahip_dev_ccphase_read(unsigned long long *out8, int reset) {
    if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_ccph), sizeof(g_ccph)) != hipSuccess) return 1;
    if (reset) {
        unsigned long long z[8] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_ccph), z, sizeof(z)) != hipSuccess) return 1;
    }
    return 0;
}
extern "C" int covahip_dev_phase_read(unsigned long long *out64, int reset) {
    if (hipMemcpyFromSymbol(out64, HIP_SYMBOL(g_phase), sizeof(g_phase)) != hipSuccess) return 1;
    if (reset) {
        unsigned long long z[80] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_phase), z, sizeof(z)) != hipSuccess) return 1;
    }
    return 0;
}
#endif
