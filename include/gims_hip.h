/*
 * gims_hip.h -- C ABI of libgims_hip.so: the MI355X (gfx950) kernels behind the GIMS matcher hot path.
 *
 * The reference (songxf1024/GIMS) has no FFI boundary of its own for this path: the boundary is the
 * Python nn.Module API  GMatcher(config).forward(data)  (models/gmatcher.py:177,219) and
 * Matching(config).forward(data)  (models/matching.py:10,15).  gims_amd/gmatcher.py keeps that API and
 * calls the entry points below through ctypes; each entry point names the reference lines it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller unless its name starts with h_ (host);
 *   - every call enqueues work on `stream` (a hipStream_t passed as void*) and returns immediately,
 *     except the calls documented as synchronising;
 *   - return value: 0 on success, a negative GIMS_E* code on failure (never throws across the ABI);
 *     gims_last_error() returns a thread-local message for the last failure;
 *   - activations are POINT-MAJOR: row = keypoint, column = channel (the reference is channel-major
 *     (B,C,N); the Python shell transposes at the boundary);
 *   - no hidden global state; safe to call from several threads on different streams.
 */
#ifndef GIMS_HIP_H
#define GIMS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GIMS_ABI_VERSION 5   /* 5: gims_aux_layout is new (the layout of the auxiliary functions' buffers, from their own routines); nothing else changed.
                             4: the superseded CAR-HyNet entry points and the 3x3-convolution gather mode of gims_linear are gone; gims_linear_args keeps its size, conv_* became reserved0 / probe_delay.
                             Still 4 (the version is pinned), but NOT layout-compatible with earlier builds of 4: gims_pack_image grew from 80 to 96 bytes (src_row, in_off;
                             gims_pack_graphs indexes a device array of them by sizeof) and two reserved words of gims_linear_args became residual_rows -- header,
                             library and binding of one build go together */

#define GIMS_OK 0
#define GIMS_EINVAL (-1)   /* bad argument (shape / alignment / null pointer) */
#define GIMS_EHIP (-2)     /* a HIP runtime call failed */
#define GIMS_ENUMERIC (-3) /* numeric guard tripped (non-finite Sinkhorn marginal) */

int gims_abi_version(void);
const char* gims_last_error(void);
/* Copies a small host table (descriptor arrays, offsets, <= 1 MiB) to device memory IN STREAM ORDER without touching the
 * copy engines: the bytes travel as kernel arguments (chunks of 3968 B).  Unlike a pageable hipMemcpy this never blocks
 * the submitting thread on the stream and never pins pages, so the host can keep running ahead of the GPU.  `dev` must be
 * 16-byte aligned and padded to a multiple of 16 bytes.  No reference counterpart (host-side plumbing of this build). */
int gims_upload_table(const void* host, int64_t bytes, void* dev, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Linear layers (1x1 Conv1d / nn.Linear):   C[m, n] = act( sum_k A[m,k] * W[n,k] + bias[n] ) (+ R[m,n])
 * replaces: nn.Conv1d(k=1) stacks of MLP / MultiHeadedAttention / final_proj (gmatcher.py:11-24,
 * 106-125, 202-205, 273), SAGEConv's fc_self / fc_neigh (gmatcher.py:149-151) and the two dense
 * contractions of the path: cosine similarity D D^T (agc.py:390) and the score matrix
 * einsum('bdn,bdm->bnm') (gmatcher.py:274).
 * A is given as up to two K-segments (concat-free torch.cat([x, message]), gmatcher.py:125):
 *   k <  k0 : a0[m*lda0 + k]          k >= k0 : a1[m*lda1 + (k-k0)]
 * W is row-major [n][K] (PyTorch weight layout).  K and k0 must be multiples of 32.
 * precision: GIMS_PREC_F32   -> exact-f32 MFMA (v_mfma_f32_32x32x2_f32), f32 operands in a0/a1/w;
 *            GIMS_PREC_BF16X3-> split-bf16 MFMA (hi*hi + hi*lo + lo*hi); W comes pre-split in
 *                               w (hi plane) / w_lo (lo plane), A is split on the fly.
 * out_f32 / out_bf16 / (out_hi,out_lo) may each be NULL; `residual` (f32, same ld as out_f32) may alias out_f32.
 */
#define GIMS_PREC_F32 0
#define GIMS_PREC_BF16X3 1
#define GIMS_PREC_BF16X6 2   /* three-way split (a1+a2+a3, exact), six bf16 MFMAs per product: f32-GEMM accuracy at 6/16 of
                              the exact-f32 MFMA cost.  Operands in the SPL3 layout (gims_split_spl3); batched launches only
                              (gims_linear_put_many + gims_linear_batch), C = scale * A W^T into out_f32, GIMS_LINEAR_UPPER ok */
#define GIMS_ACT_NONE 0
#define GIMS_ACT_RELU 1

/* Device-side guard of a launch (attention_precision='auto' of the host shell: a layer that ran on cheap operands is REDONE at f32-class accuracy
 * inside the same batch when the statistic of the cheap launch says the operands did not suffice -- no host round trip, so the results of a
 * batch never leave with the cheap tier's error).  A launch whose args carry a guard with stat != NULL is a no-op unless the guard FIRES; every
 * workgroup evaluates it at entry from `stat`, the accumulator a preceding measured gims_attention launch (gims_attn_args.stat) of the same stream filled:
 *   GIMS_GUARD_PEAKED: some head's mean row maximum (stat[h][0] / stat[h][1] / 2^24) exceeds mean_thr, or its share of rows with a maximum above
 *                      1/2 (stat[h][3] / stat[h][1]) exceeds tail_thr, or -- max_thr > 0 -- its LARGEST row maximum (stat[h][2] / 2^24) reaches
 *                      max_thr: a single sharply peaked row inside a diffuse layer                  (guards a plain-bf16 attention layer);
 *   GIMS_GUARD_RANGE : max |Q|, |K| or |V| as stored (stat[n_heads][0..2]) exceeds range_limit, or is not finite   (guards an IEEE-half layer).
 * A guarded gims_attention launch that fires stores 1 into stat[n_heads][3] (the host's record that the layer was redone).  The comparisons
 * are done in float64 exactly as written here, so a host that reads `stat` back reaches the same verdict.  stat == NULL: unconditional. */
#define GIMS_GUARD_PEAKED 1
#define GIMS_GUARD_RANGE 2
typedef struct gims_attn_guard {
  uint64_t* stat;                        /* [n_heads + 1][4], see gims_attn_args.stat; NULL = no guard */
  double mean_thr, tail_thr, range_limit;
  int32_t n_heads, kind;                 /* GIMS_GUARD_* */
  double max_thr;                        /* GIMS_GUARD_PEAKED: 0 = the largest row maximum is not looked at */
} gims_attn_guard;

typedef struct gims_linear_args {
  const float* a0; int64_t lda0;
  const float* a1; int64_t lda1;       /* may be NULL when k0 == K */
  const void* w; const void* w_lo; int64_t ldw;  /* f32 (F32) or bf16 planes (BF16X3) */
  const float* bias;                   /* [n] or NULL */
  const float* residual;               /* [m][ldc] or NULL */
  float* out_f32; int64_t ldc;         /* may be NULL */
  uint16_t* out_bf16; int64_t ldc_bf16;/* may be NULL */
  int32_t m, n, k, k0;
  int32_t act;                         /* GIMS_ACT_* */
  int32_t precision;                   /* GIMS_PREC_* */
  float scale;                         /* applied to the accumulator before bias (1.0 = none) */
  /* pre-split operands (hot path of the attentional GNN): when a0_lo != NULL, a0 (and a1) and w are bf16 buffers in
   * the SPL32 layout written by the producing kernel / gims_split_spl32: logical [rows][K] stored as [rows][pitch >= 2K],
   * per row and 32-channel block 32 hi values then 32 lo values (hi = bf16(x), lo = bf16(x - hi)); channel k sits at
   * (k/32)*64 + k%32 (hi) and +32 (lo).  a0_lo = a0 + 32, w_lo = w + 32 (the kernel only uses them as flags), lda/ldw
   * are the pitches, 128-byte aligned.  precision must be GIMS_PREC_BF16X3.  Not available through gims_linear_batch. */
  const uint16_t* a0_lo; const uint16_t* a1_lo;
  /* optional split output in the SPL32 layout: out_hi = base, out_lo = base + 32, ld_split = pitch (>= 2n) */
  uint16_t* out_hi; uint16_t* out_lo; int64_t ld_split;
  /* GIMS_LINEAR_UPPER: symmetric product (A == W): skip output tiles that lie entirely below the diagonal */
  int32_t flags;
  int32_t reserved0;                   /* must be 0 (with residual_rows it keeps guard / range_stat at their kernel-argument offsets) */
  /* pre-split operands only: row r adds residual[residual_rows[r]] instead of residual[r] (the keypoint encoder's output over ALL input keypoints,
   * read at the kept ones by GraphSAGE's last layer: gims_pack_image.src_row).  NULL: residual[r]. */
  const int32_t* residual_rows;
  int32_t probe_delay;                 /* tools/gemm_probe.py only (diagnostic flag 0x1000); 0 otherwise */
  gims_attn_guard guard;               /* pre-split operands (a0_lo != NULL) only: the launch is a no-op unless the guard fires; zero = always run */
  /* pre-split operands with GIMS_LINEAR_OUT_F16 only: the launch also reports max |value| of what it stores into out_bf16, per block of
   * 256 output columns (Q | K | V of the projection in front of a GIMS_ATTN_F16 launch): range_stat[b] = max(range_stat[b], float bits of
   * the maximum) for column block b = col / 256 < 3, by integer atomics on the f32 bit patterns -- the range row of gims_attn_args.stat's
   * accumulator (pass stat + 4 * n_heads), measured where the values are produced instead of by a scan of the buffer.  NULL: not measured. */
  uint64_t* range_stat;
} gims_linear_args;
#define GIMS_LINEAR_UPPER 1
  /* GIMS_LINEAR_HI_ONLY (pre-split operands): multiply the hi planes only -- a plain bf16 product (2^-9 relative per
   * operand) at a third of the matrix work, for results that are rounded to bf16 anyway (the Q/K/V projection) */
#define GIMS_LINEAR_HI_ONLY 2
  /* (flag value 4 was GIMS_LINEAR_A1_HI_ONLY until round 5: the hi-planes-only product for the second A segment -- the attention message in MLP0 --
   * measured +1.5 % pairs/s at 6.4e-5 of the 1e-4 score bar and was removed) */
  /* (flag value 8 was a 3x3-convolution gather mode until ABI 3; gims_ch_conv_block superseded it) */
  /* GIMS_LINEAR_OUT_F16: out_bf16 receives IEEE half instead of bf16 (round to nearest even, saturated to +-65504 so that no
   * infinity is ever stored) -- the Q/K/V projection in front of the GIMS_ATTN_F16 attention kernels */
#define GIMS_LINEAR_OUT_F16 16

int gims_linear(const gims_linear_args* args, void* stream);
/* Many independent problems in ONE launch (ragged batch: per-pair score matrices, per-image similarity
 * matrices).  gims_linear_put_many validates `count` descriptors and stores them into device memory (as kernel
 * arguments: no host staging copy, no synchronisation); gims_linear_batch launches all `count` problems,
 * grid sized for the largest (max_m x max_n).  All problems of a batch share `precision`. */
int gims_linear_put_many(const gims_linear_args* h_args /* HOST array */, int32_t count, gims_linear_args* dev_dst, void* stream);
int gims_linear_batch(const gims_linear_args* dev_args, int32_t count, int32_t max_m, int32_t max_n,
                      int32_t precision, void* stream);

/* Split an f32 array into bf16 hi/lo planes (hi = bf16_rne(x), lo = bf16_rne(x - hi)). */
int gims_split_bf16(const float* src, uint16_t* hi, uint16_t* lo, int64_t n, void* stream);
/* f32 [rows][k] (pitch lds) -> SPL32 bf16 [rows][2k] (pitch ldd); k % 32 == 0. */
/* f32 [rows][k] (row pitch lds) -> SPL3 bf16 [rows][3k] (row pitch ldd elements): per 32-channel block 32 x a1, 32 x a2,
 * 32 x a3 with a = a1 + a2 + a3 exactly.  Operand format of GIMS_PREC_BF16X6. */
int gims_split_spl3(const float* src, int64_t lds, uint16_t* dst, int64_t ldd, int64_t rows, int32_t k, void* stream);
int gims_split_spl32(const float* src, int64_t lds, uint16_t* dst, int64_t ldd, int64_t rows, int32_t k, void* stream);

/* Which kernel instance served the gims_linear / gims_linear_batch launches of this process so far (host-side counters, one per instance;
 * thread-safe): counts[k] for k < min(n, GIMS_LINEAR_KERNEL_KINDS), the rest zero; reset != 0 clears them afterwards.  gims_linear picks
 * the pre-split instance from the launch shape (tile geometry, waves and ring stages: X3P_<rows>x<cols>_W<waves>_S<stages>, HI = the
 * one-pass GIMS_LINEAR_HI_ONLY body): the instance tests use this to assert that a shape reached the instance it is meant to pin.
 * Test / diagnostic hook. */
#define GIMS_LINEAR_KERNEL_F32 0                      /* linear_f32_kernel: register-staged exact-f32 MFMA */
#define GIMS_LINEAR_KERNEL_BF16X3 1                   /* linear_bf16x3_kernel: register-staged, A split on the fly */
#define GIMS_LINEAR_KERNEL_F32_BATCH 2                /* linear_f32_batch_kernel (gims_linear_batch) */
#define GIMS_LINEAR_KERNEL_BF16X3_BATCH 3             /* linear_bf16x3_batch_kernel (gims_linear_batch) */
#define GIMS_LINEAR_KERNEL_X6_BATCH 4                 /* linear_x6_kernel: the persistent six-pass GEMM (gims_linear_batch) */
#define GIMS_LINEAR_KERNEL_X3P_64X64_W4_S3 5          /* pre-split: launches of at most 128 tiles of 128 x 128 */
#define GIMS_LINEAR_KERNEL_X3P_64X64_W4_S4_HI 6
#define GIMS_LINEAR_KERNEL_X3P_128X32_W4_S2 7         /* n <= 32 */
#define GIMS_LINEAR_KERNEL_X3P_128X64_W4_S2 8         /* n <= 64 */
#define GIMS_LINEAR_KERNEL_X3P_128X128_W8_S2 9        /* up to 256 tiles: one per CU on eight waves */
#define GIMS_LINEAR_KERNEL_X3P_128X128_W4_S2 10       /* more than 256 tiles */
#define GIMS_LINEAR_KERNEL_X3P_128X128_W4_S4_HI 11
#define GIMS_LINEAR_KERNEL_X3P_256X256_W8_S2 12       /* at least 192 tiles of 256 x 256 */
#define GIMS_LINEAR_KERNEL_X3P_256X256_W8_S2_WALK 13  /* the same behind a guard, one round of workgroups that walk the tiles */
#define GIMS_LINEAR_KERNEL_X3P_256X128_W8_S3_HI 14    /* the one-pass Q/K/V projection */
#define GIMS_LINEAR_KERNEL_X3P_256X128_W8_S2_HI 15    /* GIMS_X3P_QKV=2 only */
#define GIMS_LINEAR_KERNEL_X3P_256X256_W8_S4_HI 16    /* GIMS_X3P_QKV=0 only */
#define GIMS_LINEAR_KERNEL_KINDS 17
int gims_linear_launch_counts(uint64_t* counts /* host */, int32_t n, int32_t reset);

/* ------------------------------------------------------------------------------------------------
 * Multi-head attention message   O = softmax(Q K^T / sqrt(dh)) V   per head, flash-style.
 * replaces: attention() + the head view of MultiHeadedAttention.forward (gmatcher.py:35-39,109-113).
 * qkv: bf16 [rows][ld] with, per row, Q at column q_col + h*64 + d, K at k_col + ..., V at v_col + ...
 *      (head-BLOCKED channels; the Python shell permutes the reference's interleaved heads
 *      (view(B, dh, H, N), gmatcher.py:111) into the projection weights).
 * Each problem p attends queries [q_off, q_off+n_q) to keys/values [kv_off, kv_off+n_kv).
 * out: f32 [rows][ld_out], head-blocked columns h*64 + d.       dh = 64, heads = n_heads.
 * out_hi/out_lo: the same result in the SPL32 split-bf16 layout (out_lo = out_hi + 32, ld_split = pitch >= 512) for
 * the pre-split linear that consumes the message.
 * flags: GIMS_ATTN_Q_PRESCALED = the caller already multiplied Q by log2(e)/sqrt(dh) (e.g. folded into the rows of the
 * query projection): the kernel then computes softmax as exp2(Q K^T) / sum, which saves it one multiply-add per score.
 */
#define GIMS_ATTN_Q_PRESCALED 1
/* GIMS_ATTN_X3: f32-class accuracy for sharply peaked softmaxes.  qkv is then the SPL32 split-bf16 buffer the 3-pass Q/K/V
 * projection writes (gims_linear out_hi/out_lo; pitch ld >= 2 * 768, see gims_linear_args), q_col/k_col/v_col stay LOGICAL
 * channel offsets (multiples of 32), and every product of the kernel (Q K^T and P V) is three bf16 MFMAs on hi/lo pairs
 * (hi*hi + hi*lo + lo*hi); P is split in registers.  About three times the matrix work of the plain bf16 kernel. */
#define GIMS_ATTN_X3 2
/* GIMS_ATTN_F16: qkv holds IEEE half instead of bf16 (same layout; written by gims_linear with GIMS_LINEAR_OUT_F16 from the 3-pass
 * projection) and the kernels multiply on v_mfma_f32_32x32x16_f16 -- the bf16 kernels' structure and rate with three more mantissa
 * bits (2^-12 instead of 2^-9 relative per operand), P rounded to half with a row reference that keeps it below 2^15.  For
 * peaked softmaxes, where bf16 operands miss the reference's 1e-4 score bar; |Q|, |K|, |V| must stay below 65504 (the range row of
 * `stat` reports them).  Not together with GIMS_ATTN_X3. */
#define GIMS_ATTN_F16 4
/* GIMS_ATTN_NO_RANGE: a measured launch (stat != NULL) leaves the range row of the accumulator alone -- the projection in front of it reported it
 * (gims_linear_args.range_stat), or the caller has no use for it */
#define GIMS_ATTN_NO_RANGE 8
typedef struct gims_attn_problem { int32_t q_off, n_q, kv_off, n_kv; } gims_attn_problem;

/* stat (may be NULL): the launch additionally reports how PEAKED the softmax rows were -- the quantity that decides whether plain bf16
 * operands keep the reference's 1e-4 score bar (models/gmatcher.py:35-39 computes the softmax in f32): a device array
 * [n_heads + 1][4] of uint64.  Rows 0 .. n_heads-1: {sum over the reported queries of max_k P[q,k] in 2^-24 fixed point, number of
 * reported queries, largest row maximum (same fixed point), number of reported queries with a row maximum above 1/2}; row n_heads:
 * {bit patterns of max|Q|, max|K|, max|V| as stored (f32), unused} over the rows the launch touches -- the range guard of
 * GIMS_ATTN_F16, filled by GIMS_ATTN_F16 and GIMS_ATTN_X3 launches only (bf16 operands have f32's range).  ACCUMULATED with integer atomics (zero it first; order-independent).
 * The "largest row maximum" of a head is COMPLETE for every kernel: the 8-wave bf16 kernel, whose other figures come from the sample,
 * adds for EVERY query an upper bound of its row maximum whenever that bound reaches 1/2 -- the largest share of the row's mass that fell into
 * one 32-key half tile (problems of at least 512 keys; a workgroup that had to repeat its tiles in the exact pass reports 1) -- so a single
 * sharply peaked row cannot hide behind the sample.
 * The running-maximum kernels (GIMS_ATTN_X3, the 4-wave and split-key bf16 kernels) report every query as a by-product; the
 * 8-wave bf16 kernel tracks no maximum, so for launches it serves a second, small kernel measures 32 evenly spaced queries of
 * every (problem, head) against all keys (a few microseconds).
 * guard: see gims_attn_guard; GIMS_ATTN_X3 launches without a `stat` of their own only. */
typedef struct gims_attn_args {
  const uint16_t* qkv; int64_t ld; int32_t q_col, k_col, v_col;
  const gims_attn_problem* problems /* device */; int32_t n_problems, max_n_q, n_heads;
  float* out /* may be NULL */; int64_t ld_out; uint16_t* out_hi /* may be NULL */; uint16_t* out_lo; int64_t ld_split;
  int32_t flags;                       /* GIMS_ATTN_* */
  uint64_t* stat;                      /* the peakedness accumulator, or NULL */
  gims_attn_guard guard;               /* no-op unless the guard fires; zero = always run */
} gims_attn_args;
int gims_attention(const gims_attn_args* args, void* stream);

/* Which kernel served the attention launches of this process so far (host-side counters, one per kernel family; thread-safe):
 * counts[k] for k < min(n, GIMS_ATTN_KERNEL_KINDS), the rest zero; reset != 0 clears them afterwards.  The launcher picks a kernel
 * from the launch shape (a batch that fills the chip takes the 8-wave kernel, one pair alone the split-key / 4-wave kernels):
 * parity tests use this to assert that a fixture went through the kernel it is meant to pin.  Test / diagnostic hook. */
#define GIMS_ATTN_KERNEL_WAVE4 0       /* attention_bf16_kernel<QP, F16>: 4 waves, running maximum */
#define GIMS_ATTN_KERNEL_SPLIT 1       /* attention_split_kernel<NS, F16>: key range split over wave groups */
#define GIMS_ATTN_KERNEL_WAVE8 2       /* attention8_bf16_kernel, bf16 operands (the kernel of the timed batches) */
#define GIMS_ATTN_KERNEL_WAVE8_F16 3   /* attention8_bf16_kernel, IEEE-half operands */
#define GIMS_ATTN_KERNEL_X3 4          /* attention_x3_kernel / attention_x3w_kernel, unguarded */
#define GIMS_ATTN_KERNEL_X3_GUARDED 5  /* the same behind a gims_attn_guard (the device-side redo of 'auto') */
#define GIMS_ATTN_KERNEL_KINDS 6
int gims_attention_launch_counts(uint64_t* counts /* host */, int32_t n, int32_t reset);

/* ------------------------------------------------------------------------------------------------
 * A recorded sequence of launches replayed by ONE call: the 18 layers of AttentionalGNN.forward (gmatcher.py:127-143) are
 * 72 launches whose arguments only change when the batch geometry does, and a caller in an interpreted language pays for
 * every crossing of the ABI.  ops: HOST array; each op is exactly one gims_linear, gims_attention or (GIMS_OP_AUX) small-kernel call, in order, on
 * `stream`.  Stops at (and returns) the first error.
 */
#define GIMS_OP_LINEAR 0
#define GIMS_OP_ATTENTION 1
/* GIMS_OP_MLP: one layer's MLP (gmatcher.py:141-142) in ONE launch, reached through this table only (the exported surface of this ABI
 * version is closed, see GIMS_AUX_SIFT_DESCRIBE): the payload is u.lin and describes
 *   out = residual + W1 relu(W0 [a0 | a1] + b0) + b1
 * on pre-split SPL32 operands, the hidden activation staying in registers (kernel: mlp_fused_x3_kernel, gims_amd/csrc/linear_mlp.hip).
 *   a0, a1 (lda0, lda1; a0_lo = a0 + 32, a1_lo = a1 + 32)   the two K segments, k0 = n channels each, k = 2n
 *   w (w_lo = w + 32, ldw >= 2k)   ONE SPL32 buffer of 3n rows: rows 0 .. 2n-1 are W0 [2n][k]; rows 2n .. 3n-1 are W1 [n][2n] with its K axis
 *                                  permuted inside every 32-channel block: position 16 s + 8 h + j (s, h in 0 .. 1, j in 0 .. 7) holds
 *                                  channel (r & 3) + 8 (r >> 2) + 4 h of the block, r = 8 s + j -- the order in which a lane of the first
 *                                  product holds its results
 *   bias   [3n] = b0 | b1          residual (may be NULL; may alias out_f32), out_f32 (ldc), out_hi / out_lo = out_hi + 32 (ld_split): as gims_linear.
 *                                  out_hi may alias a0 (the layer's residual stream and its SPL32 copy): a workgroup writes its rows after it has read them
 *   act = GIMS_ACT_RELU (the hidden layer's), precision = GIMS_PREC_BF16X3, scale = 1, flags = 0, out_bf16 = NULL, no guard, no range_stat.
 * The hidden values are bit for bit those of the two gims_linear launches it replaces (same K order, same split arithmetic); the second
 * product sums the two halves of its K range separately, so results differ from theirs by f32 summation order only.
 * GIMS_EINVAL before any HIP call for every shape it does not serve: anything but n = 256, k = 512, k0 = 256, and the alignment of
 * gims_linear's pre-split operands. */
#define GIMS_OP_MLP 3
/* GIMS_OP_AUX: the small kernels of the encoder stage in front of the layers (GraphSAGE, gmatcher.py:145-162, 268-269; keypoint encoder,
 * gmatcher.py:87-97, 270-271), so that that stage replays from a table like the layers do -- between the one host synchronisation of a batch and
 * the layers the device waits for the host, and a dozen calls across the ABI were most of that wait.  fn selects the entry point, p / i are its
 * pointer and integer arguments in declaration order:
 *   GIMS_AUX_SPLIT_SPL32      gims_split_spl32     p = {src, dst}                              i = {lds, ldd, rows, k}
 *   GIMS_AUX_SAGE_MEAN_SPLIT  gims_sage_mean_split p = {h, indptr, indices, out_spl}           i = {ldh, n, c, ld_spl}
 *   GIMS_AUX_KENC_FIRST       gims_kenc_first      p = {kpts, norm3, seg_of_row, w1, b1, out}  i = {c1, n}
 *     (through the table only: i = {c1, n, n_img > 0} takes the rows as n_img whole images back to back, p[2] = the first row of every image,
 *      ascending from 0, instead of one image index per row -- the encoder over all INPUT keypoints, before the kept ones are known)
 * and the small kernels of the linear_precision='f32' and use_layernorm=True variants of both stages:
 *   GIMS_AUX_SAGE_MEAN          gims_sage_mean          p = {h, indptr, indices, out}               i = {ldh, n, c, ldo}
 *   GIMS_AUX_KENC_FIRST_LINEAR  gims_kenc_first_linear  p, i as GIMS_AUX_KENC_FIRST
 *   GIMS_AUX_LAYERNORM_ACT      gims_layernorm_act      p = {x, a2, b2, out, out_hi, out_lo}        i = {ldx, rows, c, act, ldo, ld_split}  f = {eps}
 * f holds the floating-point arguments in declaration order (eps is a float in the entry point and travels as one: no conversion on the way).
 *
 * GIMS_AUX_SIFT_DESCRIBE is the one function of this table WITHOUT a stand-alone entry point: the exported surface of this ABI version
 * is closed (its count is pinned), so the descriptor stage is reached through the table only; an entry point of its own belongs to the
 * next ABI version.  It computes OpenCV 4.x calcSIFTDescriptor (d = 4, n = 8: 128 values) for n keypoints over the detector's own
 * pyramid (the detectAndCompute descriptor; NOT the pyramid cv2.SIFT.compute rebuilds from the octaves of provided keypoints).  This
 * library's restatement: parity with OpenCV is unpinned, as for detection.  kernel: sift_describe_kernel, gims_amd/csrc/sift.hip.
 *   p[0] pyr    float [n_images][image_floats], filled by gims_sift_pyramid / gims_sift_detect for the same h, w
 *   p[1] kp4    float [n][4] = x, y, size, angle, as detection returns them
 *   p[2] octave int32 [n], packed as detection returns it
 *   p[3] image  int32 [n], the image of every keypoint; may be NULL when n_images == 1
 *   p[4] out    float [n][ld]; 128 integer-valued floats in 0 .. 255 per keypoint (OpenCV's CV_32F descriptors)
 *   p[5] bad    device int32 [1]: set to the number of bad keypoints
 *   i = {n, n_images, h, w, ld, 0}
 * GIMS_EINVAL before any HIP call: a NULL pyr / kp4 / octave / out / bad while n > 0; n < 0; n_images < 1, or p[3] == NULL with
 * n_images > 1; an h, w that gims_sift_layout refuses; ld < 128; i[5] != 0.  n == 0 is GIMS_OK and touches nothing.  Asynchronous: no
 * host synchronisation (bad is written by a memset node and the kernel).
 * All arithmetic is float32 without fused multiply-add; exp, cos and sin are taken in double and rounded to float; fastAtan2 is the
 * detector's polynomial; cvRound = rint (half to even), cvFloor = floor.  Per keypoint (x, y, size, angle, octave, image b):
 *   o = octave & 255; o = o < 128 ? o : (-128 | o); layer = (octave >> 8) & 255; scale = o >= 0 ? 1.f / (1 << o) : (float)(1 << -o).
 *   The level is Gaussian image `layer` of pyramid octave o + 1 (firstOctave = -1), rows x cols.  BAD (128 zeros, counted) when o + 1
 *   is outside 0 .. n_octaves - 1, layer outside 0 .. 5, or b outside 0 .. n_images - 1.
 *   ptf = (x * scale, y * scale); scl = size * scale * 0.5f; ori = 360.f - angle, 0 when |ori - 360.f| < FLT_EPSILON;
 *   pt = (cvRound(ptf.x), cvRound(ptf.y)); cos_t = cos(ori * (float)(CV_PI / 180)), sin_t likewise; bins_per_rad = 8 / 360.f;
 *   exp_scale = -1.f / (4 * 4 * 0.5f); hist_width = 3.f * scl; radius = cvRound(hist_width * 1.4142135623730951f * 5 * 0.5f), then
 *   radius = min(radius, (int)sqrt((double)cols * cols + (double)rows * rows)); then cos_t /= hist_width, sin_t /= hist_width.
 *   (cvRound of a value beyond +-1e9 or of a NaN takes +-1e9 / -1e9: such a keypoint has no sample inside any level.)
 *   Samples, i = -radius .. radius (outer), j = -radius .. radius (inner): c_rot = j * cos_t - i * sin_t; r_rot = j * sin_t + i * cos_t;
 *   rbin = r_rot + 2 - 0.5f; cbin = c_rot + 2 - 0.5f; r = pt.y + i; c = pt.x + j; kept iff rbin > -1 && rbin < 4 && cbin > -1 && cbin < 4
 *   && r > 0 && r < rows - 1 && c > 0 && c < cols - 1.  Kept: dx = img(r, c+1) - img(r, c-1); dy = img(r-1, c) - img(r+1, c);
 *   mag = sqrtf(dx*dx + dy*dy) * (float)exp((double)((c_rot*c_rot + r_rot*r_rot) * exp_scale)); obin = (fastAtan2(dy, dx) - ori) * bins_per_rad.
 *   Trilinear vote: r0 = cvFloor(rbin), c0 = cvFloor(cbin), o0 = cvFloor(obin); rbin -= r0, cbin -= c0, obin -= o0; o0 += 8 if o0 < 0,
 *   o0 -= 8 if o0 >= 8; v_r1 = mag * rbin, v_r0 = mag - v_r1; v_rc11 = v_r1 * cbin, v_rc10 = v_r1 - v_rc11, v_rc01 = v_r0 * cbin,
 *   v_rc00 = v_r0 - v_rc01; v_rcoXY1 = v_rcXY * obin, v_rcoXY0 = v_rcXY - v_rcoXY1; the eight are added to hist[6][6][10] at
 *   idx = ((r0+1) * 6 + c0 + 1) * 10 + o0 plus 0 (000), 1 (001), 10 (010), 11 (011), 60 (100), 61 (101), 70 (110), 71 (111).
 *   An angle in -1 .. 360 (cv::KeyPoint's range; -1, "not applicable", gives ori = 361) leaves o0 in -1 .. 7 after that one wrap.  o0 = -1
 *   is kept as it is: idx - 1 is orientation entry 9 of the cell BEFORE in the flat histogram and idx entry 0 of the sample's own cell, so
 *   entry 9 is live and the fold below matters; the one share that would land before the histogram (cell 0, o0 = -1) is dropped.  A sample
 *   of any other angle whose o0 falls outside -1 .. 7 is dropped, where OpenCV would write outside its histogram.
 *   Finalise: for i, j in 0 .. 3, idx = ((i+1) * 6 + (j+1)) * 10: hist[idx] += hist[idx+8], hist[idx+1] += hist[idx+9],
 *   dst[(i*4 + j) * 8 + k] = hist[idx + k], k < 8.  nrm2 = sum of dst[k]^2, k ascending; thr = sqrtf(nrm2) * 0.2f; dst[k] = min(dst[k], thr);
 *   nrm2 summed again; f = 512.f / max(sqrtf(nrm2), FLT_EPSILON); out[k] = (float)saturate_cast<uchar>(dst[k] * f) (half to even, 0 .. 255).
 * Summation order: each of the 360 histogram entries is the sum of its contributions in ascending sample order (i outer, j inner) from 0,
 * as OpenCV's sequential loop leaves it; no float atomics; the result depends on neither launch geometry, batch composition nor run.
 * Nothing caps size: a keypoint with more samples than one LDS chunk is processed in chunks, in the same order.  Cost: one wave walks
 * all samples of a keypoint, at most the (rows - 2) * (cols - 2) interior pixels of its level, 256 at a time; a keypoint that covers the
 * 2x level of a 16384 x 16384 image is up to 2^30 samples on one wave (seconds, not microseconds).  A caller that takes keypoints from
 * an untrusted source bounds size itself.
 *
 * GIMS_AUX_DIOU_NMS is the second function of this table without a stand-alone entry point, for the same reason.  It is the reference's
 * keypoint thinning process_diou_nms(k, radius, iou_thresh) (utils/common.py:720-807: greedy DIoU non-maximum suppression over boxes
 * around the keypoints), index for index, for a batch of images in one call.  kernel: diou_nms_kernel, gims_amd/csrc/nms.hip.
 *   p[0] kp4     float [n][4] = x, y, size, angle, as detection returns them; angle is not read
 *   p[1] order   int32 [n]: the processing order, GLOBAL rows.  Segment b holds a permutation of its own rows offsets[b] .. offsets[b+1] - 1;
 *                a value outside the segment is skipped and counted bad, never dereferenced
 *   p[2] offsets device int32 [n_images + 1]: the keypoints are grouped into n_images contiguous segments; clamped to 0 .. n on the device
 *   p[3] keep    int32 [n].  Per segment: the result rows (global), then -1
 *   p[4] count   int32 [n_images + 1]: kept per image, then bad
 *   p[5] work    workspace, 16-byte aligned, of at least
 *                  2 * al256(16 n) + 3 * al256(4 n) + al256(4 * (2 n + 64 n_images)) + al256(n) bytes, al256(x) = (x + 255) & ~255
 *   i = {n, n_images, height, width, work_bytes, 0}     f = {radius, iou_thresh}
 * radius > 0 selects fixed boxes, radius == 0 boxes from the keypoint size.  0 < iou_thresh < 1.  height, width: the extent the search
 * grid covers; they affect speed only, never the result (keypoints outside it are clamped into the border cells).
 * GIMS_EINVAL before any HIP call, each with a message naming diou_nms: a NULL pointer while n > 0; n < 0 (or above 2^29); n_images < 1
 * (or above 2^20); height or width < 1; radius negative or not finite; iou_thresh outside (0, 1) or not finite; work_bytes below the
 * formula; a misaligned work; i[5] != 0.  n == 0 is GIMS_OK after the same checks and touches nothing.  One memset node and one kernel,
 * whatever the data; no host synchronisation; capturable by gims_ops_graph_create.
 * Boxes.  Half-widths and corners are computed in double and rounded once: half = (double)radius / 2, or (double)size / 2 in size mode;
 * x1 = (float)((double)x - half), y1 likewise, x2 = (float)((double)x + half), y2 likewise (what the reference's Python-float lambdas
 * followed by .astype(np.float32) produce).  Everything after that is float32, one rounding per operation, no fused multiply-add:
 *   area = (x2 - x1 + 1) * (y2 - y1 + 1); cx = (x1 + x2) / 2; cy = (y1 + y2) / 2.
 * Pair test, for a kept keypoint i and a later keypoint o:
 *   w = max(0, min(x2i, x2o) - max(x1i, x1o) + 1), h likewise; inter = w * h; iou = inter / ((area_i + area_o) - inter);
 *   diag = (max(x2i, x2o) - min(x1i, x1o))^2 + (max(y2i, y2o) - min(y1i, y1o))^2; cd = (cxi - cxo)^2 + (cyi - cyo)^2;
 *   diou = iou - cd / (diag + 1e-10f); o SURVIVES i iff diou <= (float)iou_thresh.  (beta is the reference's default 1: not exposed.)
 * Greedy rule.  Walk the processing order: the first undecided keypoint is kept, every later keypoint that does not survive it is
 * suppressed; repeat.  The result per image is the kept keypoints in processing order, each replaced by the LOWEST row of the same
 * image, among the rows of its processing order, whose four corners compare equal (float ==) to its own: the reference's
 * argwhere(...)[0][0] map-back.  With iou_thresh < 1 two identical boxes always suppress one another (diou == 1), so no row appears twice.
 * Bad keypoints.  x, y or size not finite, or size < 0 in size mode.  A bad keypoint is never kept, suppresses nothing and is counted in
 * count[n_images], as is every entry of order that lies outside its segment.
 * The order is an input: the Python layer makes it descending score, equal scores with the higher row first.  Ties between identical
 * boxes cannot change the result; ties between different boxes are decided by that rule, where the reference leaves them to NumPy's sort.
 * How it is computed.  A keypoint can only be suppressed by one whose box overlaps its own (w > 0 and h > 0: otherwise
 * diou <= 0 < iou_thresh), and then x1 and y1 of the two differ by less than the larger side + 1.  One workgroup per image bins its
 * keypoints by (x1, y1) into a uniform grid of at most 2 m + 63 cells whose cell side exceeds the image's largest side + 1, so 3 x 3 cells
 * hold every partner, and relaxes statuses in rounds: an undecided keypoint is suppressed as soon as an earlier partner it does not
 * survive is kept, kept once all such partners are suppressed.  That reproduces the sequential rule exactly, in 2-6 rounds on detector
 * output or random points and in as many rounds as keypoints on a chain of overlapping boxes with descending scores.  The locality
 * argument needs the squares of the coordinates to be finite floats (|x|, |y|, size below 1e18).
 *
 * GIMS_AUX_ASSEMBLE_ROWS is the third function of this table without a stand-alone entry point, for the same reason.  It fills the two
 * buffers the layer stage of a batch reads -- the residual stream, f32 [n_rows][k], and its SPL32 copy, bf16 [n_rows][2 k] -- from stores of
 * already encoded rows (image-set matching, DESIGN.md 4.16: an image is encoded once and matched in many pairs; every pair entry needs its
 * own copy of its images' rows because the layers update them in place).  kernel: assemble_rows_kernel, gims_amd/csrc/features.hip.
 *   p[0] table     device int64 [n_seg][4] = {source address (const float*), source pitch in floats, rows, first destination row}, 8-byte
 *                  aligned, ascending by first destination row, the destination ranges disjoint.  The same source may appear in any number
 *                  of segments.  Row j < rows of a segment is the k floats at source + j * pitch and goes to destination row first + j.
 *   p[1] out       float [n_rows][ld_out], or NULL
 *   p[2] out_split SPL32 bf16 [n_rows][ld_split], or NULL.  At least one of the two is non-NULL.
 *   i = {n_seg, n_rows, k, ld_out, ld_split, 0}
 * Per element x = source[j * pitch + c], c < k: out[r][c] = x (the bits as they are); hi = bf16(x), round to nearest even (a NaN stays a
 * NaN); lo = bf16(x - bf2f(hi)), the subtraction in float32; out_split[r][spl_col(c)] = hi and out_split[r][spl_col(c) + 32] = lo,
 * spl_col(c) = 64 (c / 32) + c % 32: bit for bit what gims_split_spl32 and the epilogues of gims_linear write.
 * GIMS_EINVAL before any HIP call, each with a message naming assemble_rows: a NULL table while n_seg > 0; both outputs NULL; n_seg or n_rows
 * negative (or above 2^31 - 1); k <= 0 or k % 32 != 0; ld_out < k or ld_split < 2 k for a non-NULL output; an output that breaks the
 * alignment rules of gims_linear's pre-split operands (out: 16-byte aligned, ld_out a multiple of 4; out_split: 128-byte aligned, ld_split a
 * multiple of 64 below 2^22); a misaligned table; i[5] != 0.  i[5] is reserved for selecting a later form of the function and is checked before
 * everything else: a non-zero value is refused as an unknown auxiliary function form of gims_run_ops (the message names both), whatever the
 * other arguments hold.  n_seg == 0 or n_rows == 0 is GIMS_OK after the same checks and touches nothing.
 * The source addresses and pitches live in device memory, so the CALLER guarantees them: every source row readable, 16-byte aligned addresses,
 * pitches that are multiples of 4 (hip.assemble_rows checks this and the order and disjointness of the destinations on the host).
 * On the device a segment is clipped to the rows 0 .. n_rows - 1 and a segment with rows <= 0 is skipped; a destination row that no segment
 * covers is left as it was.  Nothing outside rows [0, n_rows) of either output is ever written, whatever the table holds (a table that is
 * not ascending or not disjoint leaves unspecified rows inside that range).  One kernel whatever n_seg is (a wave finds the segment of its
 * rows by a binary search over the first destination rows: scalar work, no thread per table entry); no host synchronisation; capturable by
 * gims_ops_graph_create.
 *
 * GIMS_AUX_BUILD_TRACKS is the fourth function of this table without a stand-alone entry point, for the same reason.  It merges the pairwise
 * matches of a set of images (image-set matching) into multi-view tracks.  This library's own specification:
 * the reference matches one pair and has no counterpart.  kernels: trk_*_kernel, gims_amd/csrc/tracks.hip.
 *   Nodes.   Keypoint i of image k is node g = start[k] + i; start is the exclusive prefix of the keypoint counts, N = start[n_images].
 *   Edges.   Row i < n_a of a pair (a, b) with j = matches0[i] is an edge {start_a + i, start_b + j} iff 0 <= j < n_b, and scores is NULL or
 *            scores[i] >= min_score (a NaN score is no edge), and mask is NULL or mask[i] != 0.  j == -1 is "no match"; any other j outside
 *            0 .. n_b - 1 is ignored and counted in n_bad, as is a row whose nodes fall outside 0 .. N - 1: such a value is never an index.
 *            A pair may appear twice, in both directions, or with a == b (i == j is then a no-op that still counts as an accepted row).
 *   Tracks.  The connected components with at least min_length nodes.  A component CONFLICTS when two of its nodes lie in one image; without
 *            GIMS_TRACKS_KEEP_CONFLICTING the conflicting ones are dropped whole.  Tracks are numbered in ascending order of their smallest node,
 *            a track's observations are listed in ascending node order: the result is a function of the edge SET alone.
 *   p[0] table    device int64 [n_pairs + 1][GIMS_TRACKS_TABLE_WORDS], 8-byte aligned.  Entry p < n_pairs = {address of matches0 (const
 *                 int64_t [n_a]), address of scores (const float [n_a]) or 0, address of mask (const uint8_t [n_a]) or 0, n_a, n_b, start_a,
 *                 start_b, first row}; first row = the sum of n_a over the entries in front (entry 0: 0).  Entry n_pairs = seven zeros and
 *                 the total number of rows, at most 2^31 - 1.
 *   p[1] start    device int32 [n_images + 1], ascending from 0 to N
 *   p[2] track_of int32 [N]: the track of every node, or -1
 *   p[3] out      int32 [(N/2 + 1) + N + N + (N/2 + 3) / 4] (integer division): indptr [N/2 + 1] | obs_image [N] | obs_keypoint [N] | conflict, uint8 [N/2]
 *                 packed.  With T tracks and n_obs observations the call writes indptr[0 .. T], obs_*[0 .. n_obs - 1] and conflict[0 .. T - 1]
 *                 and nothing behind them.  Track t holds observations indptr[t] .. indptr[t + 1] - 1; conflict[t] is 1 for a conflicting track
 *                 (never without GIMS_TRACKS_KEEP_CONFLICTING).
 *   p[4] counters int32 [8] = {n_tracks, n_obs, n_conflicting, n_edges, n_bad, status, 0, 0}.  n_conflicting counts the conflicting components
 *                 whatever the flag and min_length; n_edges the accepted rows, duplicates included.  status: 0, or non-zero when a row's bounded
 *                 retry loop ran out (bit 0) or a parent chain was not descending (bit 1) -- neither can happen; the outputs are then unspecified
 *                 (but inside their buffers) and the caller must not use them.
 *   p[5] work     workspace, 16-byte aligned, of at least
 *                   12 * al256(4 N) + al256(4 * (N / GIMS_TRACKS_SCAN_TILE + 2)) + al256(4 * (N / (H + 1) + 1) * (N / GIMS_TRACKS_SCAN_TILE + 1)) + 256
 *                 bytes, H = max(GIMS_TRACKS_LONG_SEGMENT, N / 1024), al256(x) = (x + 255) & ~255, every division an integer division
 *   i = {n_pairs, n_images, N, min_length | flags, work_bytes, 0}     f = {min_score}
 *   min_length >= 2; the one flag is GIMS_TRACKS_KEEP_CONFLICTING.  min_score is read only by entries with scores.
 * GIMS_EINVAL before any HIP call, each with a message naming build_tracks: n_pairs outside 0 .. 2^24; n_images outside 1 .. 2^24; N outside
 * 0 .. 2^30; min_length outside 2 .. 2^24 or an unknown flag; a NaN min_score; a NULL start, out or counters; a NULL table while n_pairs > 0; a
 * NULL track_of or work while N > 0; a misaligned table (8), start / track_of / out / counters (4) or work (16); work_bytes below the formula
 * while N > 0; i[5] != 0.  i[5] is reserved for selecting a later form of the function and is checked before everything else: a non-zero value
 * is refused as an unknown auxiliary function form of gims_run_ops (the message names both), whatever the other arguments hold.
 * N == 0 or n_pairs == 0 is GIMS_OK after the same checks: it zeroes the counters, writes indptr[0] = 0 and touches nothing else (track_of
 * included: a caller that wants its -1 writes them).
 * The table lives in device memory, so the CALLER guarantees it: every matches0 / scores / mask readable for n_a elements, the first rows
 * as stated (hip.tracks_table builds it).  What matches0 HOLDS is not trusted.  Nothing outside track_of, out, counters and work is ever
 * written.  A linear sequence of memset nodes and kernels on the stream, the same whatever the data; no host synchronisation; capturable by
 * gims_ops_graph_create.
 * How it is computed.  A lock-free union-find over the rows of all pairs (a wave finds the pair of its 64 rows by binary search over the first
 * rows) hooks the larger root under the smaller by compare-and-swap, so a component's root is its smallest node whatever the interleaving.
 * Workgroups on different XCDs share parent[] in that launch: per-XCD L2s are not coherent and a CU's L1 is never refreshed by another CU's
 * stores, so every access to parent[] there is an agent-scope atomic, and a row retries at most N times (a failed compare-and-swap means
 * another hook succeeded, and there are at most N - 1).  Then, each a launch of its own: roots and component sizes; an exclusive scan of the
 * sizes (three phases, tiles of GIMS_TRACKS_SCAN_TILE); members claim slots of their component's segment; every member's position is its rank
 * by counting among the component's nodes -- one lane for a component of up to GIMS_TRACKS_SHORT_SEGMENT nodes, a wave for a larger one, s^2 / 64
 * steps for s nodes -- which removes the order of the claims.  A component of more than H nodes (see work; wrong matches glue tracks into a
 * few such components, and there are at most N / (H + 1) <= 1024 of them) is ranked by a prefix count over the nodes instead: members per
 * scan tile, a scan of those counts, and the earlier nodes of the same component inside the tile -- linear in N whatever its size.  Scans of
 * the keep flags and of the kept sizes give track numbers and indptr.
 *
 * GIMS_AUX_TRIANGULATE_TRACKS is the fifth function of this table without a stand-alone entry point, for the same reason.  It turns every track
 * of a GIMS_AUX_BUILD_TRACKS result into a 3-D point from known cameras, robustly, and says which observations of the track agree with it
 * (DESIGN.md 4.18).  This library's own specification: the reference matches one pair and has no counterpart.  kernels: tri_classify_kernel,
 * tri_track_kernel, gims_amd/csrc/triangulate.hip; tests/triangulate_ref.py is the NumPy float64 restatement.  All arithmetic is float64.
 *   p[0] indptr        device int32 [T + 1]; track t holds observations indptr[t] .. indptr[t + 1] - 1.  NOT trusted (below)
 *   p[1] obs_image     device int32 [n_obs]
 *   p[2] obs_keypoint  device int32 [n_obs]
 *   p[3] kpts          float [N][2]: the pixel (u, v) of every keypoint of every image, the images back to back
 *   p[4] cams          double [n_images][GIMS_TRI_CAMERA_WORDS], 8-byte aligned: {fx, fy, cx, cy, R row-major [9], t [3], first node, n_k}.  World
 *                      to camera is x_c = R X + t (the convention of gims_verify_pairs' pose model: camera 0 = world gives x1 ~ R x0 + t).
 *                      first node and n_k are the image's place in kpts (exact as doubles): keypoint i of image k is node first_k + i.
 *   p[5] out           8-byte aligned, never NULL: one buffer, every region on a 256-byte boundary (al256(x) = (x + 255) & ~255), in this order:
 *                        double xyz [T][3] | float max_angle [T] | float rms_error [T] | int32 n_inliers [T] | float obs_error [n_obs] |
 *                        uint8 status [T] | uint8 obs_inlier [n_obs] | int32 counters [8] | scratch: int32 [T] | int32 [T] | int32 [2]
 *                      that is al256(24 T) + 3 al256(4 T) + al256(4 n_obs) + al256(T) + al256(n_obs) + 256 bytes of outputs and
 *                      2 al256(4 T) + 256 bytes of scratch behind them (gims_aux_layout reports the offsets).
 *                      counters = {n_ok, n_low_angle, n_no_model, n_too_short, n_too_long, n_bad_obs, n_inlier_obs, 0}.
 *   i = {T, n_obs, n_images, N, max_hyp | refine_iters << 16, 0}     f = {thresh (pixels), min_angle (degrees)}
 * Observation.  Observation o of a track is (image k, keypoint i) = (obs_image, obs_keypoint)[indptr[t] + o].  Its pixel (u, v) is
 *   kpts[first_k + i] read as double, its ray d = R^T x / |x| with x = ((u - cx) / fx, (v - cy) / fy, 1), its centre C = -R^T t.  It is BAD when
 *   k is outside 0 .. n_images - 1, i is outside 0 .. n_k - 1, first_k + i is outside 0 .. N - 1, u or v is not finite, or camera k is bad: one
 *   of its 18 words is not finite, or fx <= 0, or fy <= 0.  A bad observation is ignored, counted in n_bad_obs and never used as an index;
 *   its obs_error is -1 and its obs_inlier 0.  The other observations of the track, in track order, are its USABLE observations, L of them.
 * Midpoint of a set S.  A = sum over S of (I - d d^T), b = sum of (I - d d^T) C; X = adj(A) b / det A by the cofactor formula of a symmetric
 *   3 x 3 matrix: c00 = a11 a22 - a12^2, c01 = a02 a12 - a01 a22, c02 = a01 a12 - a02 a11, c11 = a00 a22 - a02^2, c12 = a01 a02 - a00 a12,
 *   c22 = a00 a11 - a01^2, det = a00 c00 + a01 c01 + a02 c02.  DEGENERATE iff !(det > 1e-12 |S|^3); two rays at angle theta give det = 2 sin^2 theta.
 * Reprojection.  x_c = R X + t, z = x_c[2], e^2 = (fx x_c[0] / z + cx - u)^2 + (fy x_c[1] / z + cy - v)^2; INLIER iff z > 0 and e^2 <= thresh^2
 *   (thresh^2 is the float thresh squared in double).
 * Angle at X between observations p and q: atan2(|a x b|, a . b) in degrees, a = X - C_p, b = X - C_q.
 * Hypotheses, when max_hyp >= 1.  Number the pairs (p, q), p < q, of the usable observations lexicographically: E = L (L - 1) / 2 pairs.
 *   H = min(E, max_hyp); hypothesis h < H is pair number floor(h E / H) in 64-bit integers (L == 2: the one pair).  Its X is the midpoint
 *   of the two; it is INVALID when that solve is degenerate or the angle at X between the two is below min_angle.  Its score is the number
 *   n_h of inliers among ALL usable observations and the sum c_h of their e^2.  The best hypothesis has the largest n_h, then the smallest c_h,
 *   then the smallest h, and needs n_h >= 2; S is its inlier set.  max_hyp == 0: no hypothesis stage, S = every usable observation.
 * Final model.  X = the midpoint of S (degenerate: NO_MODEL).  Then at most refine_iters rounds of Gauss-Newton on the cost sum over S of e^2:
 *   with the 2 x 3 Jacobians J of the residuals r, (sum J^T J) s = -(sum J^T r) by the same cofactor solve; the round is TAKEN iff det > 0,
 *   every observation of S has z > 0 at X + s and the cost at X + s is strictly below the cost at X; the first round that is not taken ends
 *   the loop (a NaN anywhere refuses the round).  Then every usable observation is classified once at the final X: obs_inlier, obs_error =
 *   sqrt(e^2) as float (-1 when z <= 0), n_inliers, rms_error = sqrt(sum of inlier e^2 / n_inliers).  max_angle is the largest angle at X
 *   between two final inliers (the kernel takes the pair of the smallest cosine and evaluates the formula above on it).
 * status, uint8 bits: 1 TOO_SHORT, L < 2 (or a bad indptr range); 2 NO_MODEL, no valid hypothesis with two inliers, a degenerate final solve,
 *   or the final inliers are fewer than two or all lie in one image; 4 LOW_ANGLE, max_angle < min_angle; 8 TOO_LONG, more than GIMS_TRI_MAX_OBS
 *   observations (bad ones included): the track is not processed, which bounds the cost of a track (such a track can only come from
 *   GIMS_TRACKS_KEEP_CONFLICTING).  A track with status 0 or LOW_ANGLE has a model: xyz, max_angle, rms_error, n_inliers and the obs_* of its
 *   usable observations are as above.  A track with any other status has none: xyz, max_angle, rms_error and n_inliers are zero, and all its
 *   observations have obs_error -1 and obs_inlier 0.  Every output of every track is written by every call; no output is ever a NaN.
 *   n_bad_obs counts over the tracks with a good range and at most GIMS_TRI_MAX_OBS observations; n_inlier_obs is the sum of n_inliers.
 * GIMS_EINVAL before any HIP call, each with a message naming triangulate_tracks: T, n_obs or N outside 0 .. 2^30; n_images outside 0 .. 2^24;
 * i[4] negative or refine_iters above 255 (max_hyp is its low 16 bits: 0 .. 65535); thresh not finite or <= 0; min_angle not finite or outside
 * [0, 180); a NULL out; any other NULL pointer while T > 0; cams or out not 8-byte aligned, another pointer not 4-byte aligned; i[5] != 0.  i[5]
 * is reserved for selecting a later form of the function and is checked before everything else: a non-zero value is refused as an unknown
 * auxiliary function form of gims_run_ops (the message names both), whatever the other arguments hold.  T == 0 is GIMS_OK after the same
 * checks and writes the counters only.
 * indptr lives in device memory and is not trusted: a track whose range is descending or leaves 0 .. n_obs is TOO_SHORT and touches no
 * observation.  (Ranges that overlap are each processed; the slots they share hold the result of one of them.)  Nothing outside out is written.
 * A fixed sequence of memset nodes and four launches, the same whatever the data; no host synchronisation; capturable by
 * gims_ops_graph_create.
 * How it is computed.  A thread per track checks the range, writes the tracks that are not processed and appends the others to a list per
 * class.  A track of up to GIMS_TRI_SHORT_TRACK observations is served by a group of that many lanes (sixteen tracks a wave), one of up to 64 by a
 * wave, both with one observation per lane held in registers; a longer one by a wave that walks the observations in slots of 64.  Rays and
 * centres are computed once per track and staged in LDS.  Every sum over observations is the lane's own sum in ascending order, then a
 * butterfly over the group's lanes; there are no float atomics, and the group size depends on the track's length alone, so the outputs of a track
 * are bit-identical alone or inside any batch, at any position, and across runs.  Counters are integer atomics, summed per workgroup first.
 *
 * GIMS_AUX_RESECT_IMAGES is the sixth function of this table without a stand-alone entry point, for the same reason.  It gives every listed
 * image its absolute pose from 2-D to 3-D correspondences -- the keypoints whose track already has a 3-D point -- robustly (resection,
 * DESIGN.md 4.19).  This library's own specification: the reference matches one pair and has no counterpart.  kernels: resect_gather_kernel,
 * resect_hyp_kernel, resect_finish_kernel, gims_amd/csrc/resect.hip; tests/resect_ref.py is the NumPy float64 restatement.  All arithmetic
 * is float64.
 *   p[0] track_of  device int32 [N]: the track of every node (GIMS_AUX_BUILD_TRACKS).  NOT trusted: an entry outside 0 .. T - 1 is "no track"
 *   p[1] xyz       device double [T][3], 8-byte aligned: the point of every track (GIMS_AUX_TRIANGULATE_TRACKS)
 *   p[2] use       device uint8 [T]: non-zero = the point may serve as a correspondence
 *   p[3] kpts      device float [N][2]: the pixel (u, v) of every keypoint of every image, the images back to back
 *   p[4] cams      HOST double [m][GIMS_RESECT_CAMERA_WORDS], 8-byte aligned, read during the call like the op table itself: one record
 *                  {fx, fy, cx, cy, first node, n_k} per image to resect (an ENTRY), in the caller's order; an image may be listed twice.
 *                  Keypoint i < n_k of entry e is node first_e + i.  n_k sizes the entry's slots in the output, so it is checked (below); the
 *                  other five words are data: a record is GOOD when they are finite and fx > 0 and fy > 0, and an entry with a bad record
 *                  has no correspondence.  The records travel to the device as kernel arguments: a captured graph holds their values.
 *   p[5] out       device, 16-byte aligned, never NULL: one buffer, every region on a 256-byte boundary (al256(x) = (x + 255) & ~255), with
 *                  S = the sum of n_k over the entries, in this order:
 *                    double pose [m][12] | int32 n_corr [m] | int32 ok [m] | int32 n_inliers [m] | int32 best_hyp [m] |
 *                    int32 best_hyp_inliers [m] | int32 lo_rounds [m] | float rms_error [m] | uint8 kp_inlier [S] | float kp_error [S] |
 *                    int32 counters [8] | scratch: 56 m bytes | double [S][6] | int32 [m][iters]
 *                  that is al256(96 m) + 7 al256(4 m) + al256(S) + al256(4 S) + 256 bytes of outputs and al256(56 m) + al256(48 S) +
 *                  al256(4 m iters) bytes of scratch behind them (gims_aux_layout reports the offsets).  The slots of entry e in kp_inlier and
 *                  kp_error are [o_e, o_e + n_k), o_e = the sum of n_k over the entries in front: the entries lie back to back, a duplicated
 *                  image has slots of its own.  counters = {n_ok, n_failed, n_corr_total, n_inlier_total, 0, 0, 0, 0}.
 *   i = {m, N, T, iters | lo_iters << 16 | min_inliers << 24, seed (its 64 bits), 0}     f = {thresh (pixels), 0}
 * Correspondences of entry e.  Keypoint i gives node g = first + i (in double) and t = track_of[g].  It is a correspondence iff the record is
 *   good, 0 <= g < N, 0 <= t < T, use[t] != 0, and the three words of xyz[t] and the pixel (u, v) = kpts[g] are finite.  The dense list holds the
 *   correspondences {X = xyz[t], u, v} (u, v read as double) in ascending i; K is its length (n_corr).
 * Hypothesis h < iters, when K >= 3.  Three distinct indices below K from the sampler of gims_verify_pairs for (seed, h): state = seed ^
 *   (h * 0xD1342543DE82EF95), then repeatedly state = splitmix64(state), candidate = state mod K, kept unless already drawn.  They give (X1, X2,
 *   X3) and the unit bearings f_i = x / |x|, x = ((u - cx) / fx, (v - cy) / fy, 1).  With c_ij = f_i . f_j, a = |X1 - X2|^2, b = |X1 - X3|^2,
 *   c = |X2 - X3|^2 and the distances s_i of the points from the centre written s2 = u s1, s3 = v s1 (P3P by the law of cosines):
 *     q(u) = u^2 - 2 c12 u + 1,   N(u) = (b - c) q(u) - a (1 - u^2) = ((b - c) - a) - 2 c12 (b - c) u + ((b - c) + a) u^2,
 *     D(u) = 2 a (c23 u - c13),   v = N(u) / D(u),   and u is a real root of the quartic  P = b q D^2 - a (D^2 + N^2 - 2 c13 N D),
 *   whose five coefficients are built by polynomial products (D D, q (D D), N N, N D; out[i + j] += a[i] b[j], i outer, j inner, ascending).
 *   Its real roots, ascending: none when P_4 == 0 or a coefficient is not finite; otherwise inside the bound B = 1 + max |P_i / P_4|, for
 *   d = 1 .. 4 the roots of the (4 - d)-th derivative are sought in the intervals between -B, the roots of the derivative before it and B:
 *   an interval [x, y] holds a root iff (p(x) > 0) != (p(y) > 0), found by 80 halvings (the midpoint replaces the end whose sign it shares;
 *   the root is the last midpoint); polynomials are evaluated by Horner's rule.  Root number j (0 .. 3, ascending) gives a MODEL iff
 *   a > 0 and |e1 x (X3 - X1)|^2 > 1e-18 b (the world triangle is not degenerate; e1 below), u > 0, |D(u)| > 1e-12 a, q(u) > 0, v > 0, and
 *   every word of the result is finite.  Then s1 = sqrt(a / q(u)), Y_i = s_i f_i, and with the frame of a triangle (P1, P2, P3)
 *     e1 = (P2 - P1)^, e3 = (e1 x (P3 - P1))^, e2 = e3 x e1,  E = [e1 e2 e3] (columns):   R = E_Y E_X^T,  t = Y1 - R X1.
 * Reprojection under (R, t).  x_c = R X + t, z = x_c[2], e^2 = (fx x_c[0] / z + cx - u)^2 + (fy x_c[1] / z + cy - v)^2; INLIER iff z > 0 and
 *   e^2 <= thresh^2 (thresh^2 is the float thresh squared in double): the rule of GIMS_AUX_TRIANGULATE_TRACKS.
 * Score.  The score of a model is its number of inliers among the K correspondences.  The best model is the one of the largest score, then
 *   of the smallest h, then of the smallest root number j.  No floating-point number enters the choice.  best_hyp = its h, best_hyp_inliers =
 *   its score.
 * Stage 2, the guarded local optimisation.  The current model starts as the best model; n and c are its inlier count and the sum of e^2 over
 *   its inliers.  At most lo_iters rounds, and none while n < 4 (three correspondences fit their model): over the inliers of the current model, with y = R X, x_c = y + t, the residual r = (ru, rv) of the
 *   reprojection and its 2 x 6 Jacobian for the update R <- exp([w]x) R, t <- t + dt in the order (w, dt),
 *     au = fx / z, bu = -fx x_c[0] / z^2, av = fy / z, bv = -fy x_c[1] / z^2,
 *     Ju = (bu y1, au y2 - bu y0, -au y1, au, 0, bu),   Jv = (bv y1 - av y2, -bv y0, av y0, 0, av, bv),
 *   solve (sum J^T J) d = -(sum J^T r): Gaussian elimination on the 6 x 7 array with partial pivoting (the pivot of column c is the first row
 *   at or below c of the largest magnitude; rows are swapped; the rows below are reduced), then back substitution; the solve is REGULAR iff
 *   every pivot's magnitude is above 1e-12 times the largest diagonal entry of the matrix.  exp([w]x) = I + A [w]x + B [w]x^2, theta = |w|,
 *   A = sin(theta) / theta, B = (1 - cos(theta)) / theta^2 for theta > 1e-8, else A = 1, B = 1/2.  The round is TAKEN iff the solve is regular,
 *   every word of the candidate is finite, and the candidate's own inlier count n' and inlier cost c' have n' > n, or n' == n and c' < c
 *   with both costs rounded to float32 for this comparison (an improvement below one part in 2^24 of the cost is none, and the decision does
 *   not hang on the last bits of two float64 sums); the candidate then becomes the current model.  The first round that is not taken ends the loop; lo_rounds counts the rounds taken.
 * Final sweep.  Every correspondence is classified once under the final model: kp_inlier, kp_error = sqrt(e^2) as float (at most FLT_MAX; -1
 *   when z <= 0), n_inliers, rms_error = sqrt(sum of inlier e^2 / n_inliers).
 * ok = 1 iff K >= 3, a model exists and n_inliers >= max(min_inliers, 4) (three points fit every model of their own sample: four is the
 *   first count that says anything).  An entry with ok = 0 has NO POSE: its twelve pose words, n_inliers and rms_error are zero, the
 *   kp_inlier of all its slots 0 and their kp_error -1; best_hyp, best_hyp_inliers and lo_rounds still say what was found (-1, 0, 0 when no
 *   hypothesis gave a model).  With ok = 1, pose = {R row-major, t}, world to camera x_c = R X + t -- the convention of
 *   GIMS_AUX_TRIANGULATE_TRACKS and of the pose model; a slot whose keypoint is no correspondence has kp_inlier 0 and kp_error -1.  Every output
 *   of every entry is written by every call; no output is ever a NaN.  n_ok + n_failed = m; n_corr_total is the sum of K, n_inlier_total the
 *   sum of n_inliers.
 * GIMS_EINVAL before any HIP call, each with a message naming resect_images: m outside 0 .. 2^24; N or T outside 0 .. 2^30; i[3] negative or
 * min_inliers above 2^30 (iters is its low 16 bits, lo_iters the next 8); thresh not finite or <= 0; f[1] != 0; a NULL out; any other NULL
 * pointer while m > 0; out not 16-byte aligned, xyz or cams not 8-byte aligned, track_of or kpts not 4-byte aligned; an n_k that is not an
 * integer in 0 .. 2^30, or S above 2^30; i[5] != 0.  i[5] is reserved for selecting a later form of the function and is checked before
 * everything else: a non-zero value is refused as an unknown auxiliary function form of gims_run_ops (the message names both), whatever
 * the other arguments hold.  m == 0 is GIMS_OK after the same checks and writes the counters only.
 * Nothing outside out is written.  A fixed sequence of memset nodes, the upload of the records and three launches (two when iters == 0), the
 * same whatever the data; no host synchronisation; capturable by gims_ops_graph_create.
 * How it is computed.  gather: a workgroup per entry compacts the correspondences in order (ballots and a prefix over the waves).  hyp: a
 * workgroup of 256 per GIMS_RESECT_HB hypotheses of an entry; that many lanes solve one P3P sample each into LDS, then every thread scores one
 * correspondence per tile against the models that exist, sixteen at a time: their counters stay in registers and each model is read at a
 * wave-uniform LDS address.  finish: a workgroup per entry finds the best hypothesis, solves its sample again, runs stage 2 and the final
 * sweep.  The 27 sums of the normal equations and the inlier cost are a thread's own sum in ascending order, a butterfly over the wave, then
 * the waves in order; there are no float atomics, so the outputs of an entry are bit-identical alone or inside any batch, at any position,
 * and across runs.  Counters are integer atomics.
 *
 * GIMS_AUX_BUNDLE_ADJUST is the seventh function of this table without a stand-alone entry point, for the same reason.  It refines the free
 * cameras and the active points of the chain jointly: Levenberg-Marquardt rounds on the reprojection cost with the Schur complement over the
 * points (bundle adjustment).  This library's own specification: the reference matches one pair and has no counterpart.
 * kernels: ba_*_kernel, gims_amd/csrc/ba.hip; tests/ba_ref.py is the NumPy float64 restatement.  All arithmetic is float64, one operation
 * at a time as written here (the file is compiled without contraction into fused multiply-adds).  (Number 12 is unassigned and refused.)
 *   p[0] table  HOST int64 [GIMS_BA_TABLE_WORDS], 8-byte aligned, read during the call like the op table itself: the device addresses
 *               {indptr int32 [T + 1], obs_image int32 [n_obs], obs_keypoint int32 [n_obs], obs_use uint8 [n_obs], point_use uint8 [T], 0, 0, 0}
 *               (GIMS_AUX_BUILD_TRACKS gives the first three; obs_use and point_use are obs_inlier and status == 0 of
 *               GIMS_AUX_TRIANGULATE_TRACKS, or the caller's choice).  The three reserved words must be 0.
 *   p[1] kpts   device float [N][2]: the pixel (u, v) of every keypoint of every image, the images back to back
 *   p[2] xyz    device double [T][3], 8-byte aligned: the starting points
 *   p[3] cams   device double [n_images][GIMS_TRI_CAMERA_WORDS], 8-byte aligned: the starting cameras, the records of
 *               GIMS_AUX_TRIANGULATE_TRACKS {fx, fy, cx, cy, R row-major [9], t [3], first node, n_k}, world to camera x_c = R X + t
 *   p[4] mode   HOST int32 [n_images], read during the call: 0 ABSENT (the camera's observations are ignored), 1 FIXED, 2 FREE.  The free
 *               cameras are counted before any HIP call: n_free sizes the reduced system and the scratch.  Free camera number s in image
 *               order has SLOT s.  The modes travel to the device as kernel arguments: a captured graph holds their values.
 *   p[5] out    device, 16-byte aligned, never NULL: one buffer, every region on a 256-byte boundary (al256(x) = (x + 255) & ~255), with
 *               n = 6 n_free, in this order:
 *                 double xyz [T][3] | double cams [n_images][18] | float obs_error [n_obs] | int32 cam_obs [n_images] |
 *                 double history [iters + 1][2] | uint8 taken [iters] | int32 counters [8] |
 *                 scratch: 256 bytes of state | int32 [n_images] | int32 [n_free] | int32 [n_free + 1] | int32 [n_free] | double [T][3] |
 *                 double [n_images][18] | uint8 [T] | uint8 [n_obs] | int32 [n_obs] x 5 | double [T][9] |
 *                 double [n_obs][50] | double [T] | double [n][n] | double [n]
 *               that is al256(24 T) + al256(144 n_images) + al256(4 n_obs) + al256(4 n_images) + al256(16 (iters + 1)) + al256(iters) + 256
 *               bytes of outputs and 256 + al256(4 n_images) + 2 al256(4 n_free) + al256(4 n_free + 4) + al256(24 T) + al256(144 n_images) +
 *               al256(T) + al256(n_obs) + 5 al256(4 n_obs) + al256(72 T) + al256(400 n_obs) + al256(8 T) + al256(8 n^2) + al256(8 n) bytes of
 *               scratch behind them (gims_aux_layout reports the offsets).  The cams region has the format of p[3]: it can be handed to a later
 *               GIMS_AUX_TRIANGULATE_TRACKS op as its p[4], and xyz to a later GIMS_AUX_RESECT_IMAGES op as its p[1].
 *               counters = {n_free, n_fixed, n_held, n_points, n_active_obs, n_bad_obs, rounds_taken, status}.
 *   i = {T, n_obs, n_images, N, iters, 0}     f = {huber (pixels; 0: the squared loss), lambda0}
 * Activity.  Nothing in device memory is trusted.  A track whose indptr range descends or leaves 0 .. n_obs, or holds more than
 *   GIMS_TRI_MAX_OBS observations, is INACTIVE and touches no observation.  Observation o of another track t, (image k, keypoint i) =
 *   (obs_image, obs_keypoint)[o], is a CANDIDATE iff point_use[t] != 0, the three words of xyz[t] are finite, obs_use[o] != 0, 0 <= k <
 *   n_images, mode[k] != 0, the 18 words of camera k are finite with fx > 0 and fy > 0, 0 <= i < n_k, the node g = first_k + i (in double)
 *   lies in 0 .. N - 1 and the pixel (u, v) = kpts[g] is finite -- the rule of GIMS_AUX_TRIANGULATE_TRACKS; a value that fails its test is
 *   never used as an index.  Point t is ACTIVE iff its track has at least two candidates; an observation is ACTIVE iff it is a candidate
 *   of an active point.  cam_obs[k] = the active observations in image k.  A free camera with cam_obs < 4 is HELD: it does not move
 *   (it keeps its slot: an identity block and a zero right-hand side in the reduced system) and its observations count as those of a
 *   fixed camera.  n_free counts the free cameras that are not held, n_fixed the cameras of mode 1, n_points the active points;
 *   n_bad_obs = the observations that are not active, over the tracks with a good range and at most GIMS_TRI_MAX_OBS observations.
 * status.  Bit 1: a camera of mode 1 or 2 has a word that is not finite, or fx <= 0, or fy <= 0.  Bit 2: at the start an active
 *   observation has z <= 0, or the cost is not finite.  With status != 0 the op changes nothing: xyz and cams equal the inputs, every
 *   obs_error is -1, every history row is {0, lambda0}, taken and rounds_taken are 0; the other counters and cam_obs are as above.
 * Model.  For an active observation with y = R X, x_c = y + t, z = x_c[2]: the residual r = (ru, rv) = (fx x_c[0] / z + cx - u,
 *   fy x_c[1] / z + cy - v), e^2 = ru^2 + rv^2, and with au = fx / z, bu = -fx x_c[0] / z^2, av = fy / z, bv = -fy x_c[1] / z^2 the camera
 *   Jacobian of GIMS_AUX_RESECT_IMAGES stage 2 for the update R <- exp([w]x) R, t <- t + dt in the order (w, dt),
 *     Ju = (bu y1, au y2 - bu y0, -au y1, au, 0, bu),   Jv = (bv y1 - av y2, -bv y0, av y0, 0, av, bv),
 *   and the point Jacobian Pu[m] = au R[0][m] + bu R[2][m], Pv[m] = av R[1][m] + bv R[2][m].  With huber > 0 and e = sqrt(e^2) > huber, ru,
 *   rv and the eighteen Jacobian words are each multiplied by sqrt(huber / e) (iteratively reweighted least squares: the weight of the
 *   observation is min(1, huber / e)).  cost = the sum over the active observations of rho(e^2): rho = e^2 when huber == 0 or e <= huber,
 *   else (2 huber) e - huber huber.  The cost of a point is the sum over its active observations in ascending o; the cost is the sum of the
 *   points' costs (inactive points give 0) in this order: thread j of 256 adds the points j, j + 256, ... ascending, the 64 threads of a
 *   wave are summed by a butterfly (offsets 32, 16, .. 1), and the four waves are added in order.
 * One round, at the current state (X, R, t), lambda and cost.  Per active point, over its active observations in ascending o:
 *   V = sum (Pu Pu^T + Pv Pv^T) (each entry of the upper triangle: Pu[i] Pu[j] + Pv[i] Pv[j], added to the sum), g_p = sum (Pu ru + Pv rv);
 *   V* = V with lambda max(V_ii, 1e-6) added to each diagonal entry; V*^-1 = adj / det by the cofactor formula of
 *   GIMS_AUX_TRIANGULATE_TRACKS, every entry divided by det.  Per observation of a camera that moves (free, not held): W[c][m] = Ju[c] Pu[m] +
 *   Jv[c] Pv[m] (6 x 3) and Y = W V*^-1, Y[c][m] = W[c][0] I[0][m] + W[c][1] I[1][m] + W[c][2] I[2][m].  Per slot s that is not held, over
 *   the active observations of its image in ascending o: the 21 sums U = sum (Ju[i] Ju[j] + Jv[i] Jv[j]) and the six g_c = sum (Ju[i] ru +
 *   Jv[i] rv), each as lane l of 64 adding the observations number l, l + 64, ... of the list and a butterfly over the lanes; U* = U with
 *   lambda max(U_ii, 1e-6) added to the diagonal.  The block row s of the reduced system starts as U* in block s, zeros elsewhere, and
 *   b_s = -g_c; then for every observation o of the list in ascending order, with p its point: b_s[r] += (Y_o[r][0] g_p[0] + Y_o[r][1]
 *   g_p[1]) + Y_o[r][2] g_p[2], and for every active observation o' of p in ascending order whose camera moves, in slot k: S[6 s + r][6 k + c]
 *   -= (Y_o[r][0] W_o'[c][0] + Y_o[r][1] W_o'[c][1]) + Y_o[r][2] W_o'[c][2].  S = L L^T by Cholesky without pivoting: for j ascending, l =
 *   sqrt(S_jj), L_ij = S_ij / l for i > j, then S_ik -= L_ij L_kj for j < k <= i.  The round is REGULAR iff the det of every active point
 *   is finite and > 0 and every pivot S_jj is finite and > 0.  L y = b: for j ascending y_j = b_j / L_jj, then b_i -= L_ij y_j for i > j;
 *   L^T d = y: for j descending d_j = y_j / L_jj, then y_k -= L_jk d_j for k < j.  Per active point s = g_p, then for its active observations
 *   in ascending o whose camera moves, for c ascending: s[m] += W[c][m] d[6 k + c]; dX[m] = -((I[m][0] s[0] + I[m][1] s[1]) + I[m][2] s[2]).
 *   The candidate: X + dX; for a moving camera R' = exp([w]x) R, t' = t + dt with (w, dt) its six words of d and exp as in
 *   GIMS_AUX_RESECT_IMAGES (theta > 1e-8: A = sin(theta) / theta, B = (1 - cos(theta)) / theta^2, else 1 and 1/2).
 *   The round is TAKEN iff it is regular, every candidate word is finite, every active observation has z > 0 under the candidate, and
 *   the candidate's cost is below the current cost with both rounded to float32 for this comparison (the rule and the reason of
 *   GIMS_AUX_RESECT_IMAGES).  Taken: the candidate becomes the state, lambda <- max(lambda / 10, 1e-12).  Not taken: the state stays,
 *   lambda <- min(10 lambda, 1e12).  After GIMS_BA_MAX_REJECTS consecutive rounds that were not taken the remaining rounds do nothing
 *   (their history rows repeat the last one, their taken is 0).  history[0] = {the starting cost, lambda0}, history[r + 1] = {cost,
 *   lambda} after round r; taken[r] = 1 iff round r was taken.  The inlier set is an input (obs_use) and is not decided again: the cost
 *   is a continuous function of the parameters.  The gauge is the caller's: it is fixed by the cameras of mode 1.
 * Outputs.  xyz and cams: the final state; inactive points and absent, fixed and held cameras are copied through bit for bit (the one way
 *   a NaN reaches an output: it was in the input), as are the eight words of a free camera that are not R or t.  obs_error: sqrt(e^2) as
 *   float (at most FLT_MAX) under the final state, -1 for an observation that is not active.  Every output is written by every call.
 * GIMS_EINVAL before any HIP call, each with a message naming bundle_adjust: T, n_obs or N outside 0 .. 2^30; n_images outside 0 .. 2^24;
 * iters outside 0 .. 255; huber negative or not finite; lambda0 not finite or <= 0; a NULL out or table; kpts, xyz or one of the five
 * table addresses NULL while T > 0; cams or mode NULL while n_images > 0; out not 16-byte aligned, the table, xyz or cams not 8-byte
 * aligned, kpts, mode, indptr, obs_image or obs_keypoint not 4-byte aligned; a reserved table word that is not 0; a mode outside 0 .. 2;
 * more than GIMS_BA_MAX_FREE_CAMERAS free cameras (a 768 x 768 reduced system, 4.7 MB of scratch; a larger set needs a blocked or an
 * iterative reduced solve: the later form that i[5] is reserved for); i[5] != 0.  i[5] is checked before everything else: a non-zero value
 * is refused as an unknown auxiliary function form of gims_run_ops (the message names both), whatever the other arguments hold.  T == 0,
 * and no free camera together with no active point, are GIMS_OK: the inputs are copied through and the counters written.
 * Nothing outside out is written.  A fixed sequence of memset nodes, the upload of the slot tables and 8 + 5 iters launches (6 + 3 iters
 * when n_free == 0), the same whatever the data: all decisions live in the state block.  No host synchronisation; capturable by
 * gims_ops_graph_create.  (Track ranges that overlap are each processed; what they share holds the result of one of them.)
 * How it is computed.  The state has two buffers for points and cameras; a round writes its candidate into the one that is not current and
 * a taken round swaps them.  A thread per track forms V, g_p, V*^-1, W and Y; a wave per slot forms U, g_c and its block row of S in LDS,
 * walking a list of its observations that a count (integer atomics), a scan and an ordered fill build once per call (lane j takes
 * observation j of the walked observation's track, so the blocks of one walked observation are formed side by side); one workgroup of
 * 1024 factors S in place and solves; a thread per track substitutes back and sums its candidate cost; one workgroup sums the costs and
 * one thread decides.  There are no float atomics and no sum whose order depends on the grid: the output bytes are identical across runs.
 *
 * GIMS_AUX_BUNDLE_ADJUST_PCG is the eighth: the same adjustment for up to GIMS_BA_PCG_MAX_FREE_CAMERAS free cameras.  The
 * model, the activity rules, the status bits, the held-camera rule, the Levenberg-Marquardt schedule, the TAKEN rule, the two-buffer state
 * and the seven outputs are those of GIMS_AUX_BUNDLE_ADJUST, word for word; what differs is where the camera step d of a round comes from:
 * preconditioned conjugate gradients on the Schur complement S, which is applied and never formed, with a block-Jacobi preconditioner.
 * GIMS_AUX_BUNDLE_ADJUST itself is unchanged.  kernels: ba_pcg_*_kernel, gims_amd/csrc/ba.hip; tests/ba_pcg_ref.py is the restatement.
 *   p[], i[] and f[] as for GIMS_AUX_BUNDLE_ADJUST (i[5] is the form word: read first, must be 0), except the table, whose words 5 .. 7 are
 *               {cg_iters (1 .. GIMS_BA_PCG_MAX_CG_ITERS), the bit pattern of the double cg_tol (finite, 0 <= cg_tol < 1), 0}, and
 *   p[5] out    the seven output regions of GIMS_AUX_BUNDLE_ADJUST in their order, then
 *                 int32 cg_used [iters] | double cg_res [iters] |
 *                 scratch: 256 bytes of state | int32 [n_images] | int32 [n_free] | int32 [n_free + 1] | int32 [n_free] x 2 | double [T][3] |
 *                 double [n_images][18] | uint8 [T] | uint8 [n_obs] | int32 [n_obs] x 4 | double [T][9] | double [n_obs][50] | double [T] |
 *                 double [T][3] | double [n_free][42] | double [n_free][6] x 5
 *               every region on a 256-byte boundary: the outputs of GIMS_AUX_BUNDLE_ADJUST + al256(4 iters) + al256(8 iters) bytes of outputs
 *               and 256 + al256(4 n_images) + 3 al256(4 n_free) + al256(4 n_free + 4) + al256(24 T) + al256(144 n_images) + al256(T) +
 *               al256(n_obs) + 4 al256(4 n_obs) + al256(72 T) + al256(400 n_obs) + al256(8 T) + al256(24 T) + al256(336 n_free) +
 *               5 al256(48 n_free) bytes of scratch (gims_aux_layout reports the offsets): linear in T, n_obs, n_images and n_free,
 *               there is no n x n region.  cg_used[r] = the conjugate-gradient iterations that did work in round r, cg_res[r] =
 *               sqrt(rho_stop / rho_0) of round r; both 0 for a round that did nothing, for every round when n_free == 0, and cg_res = 0
 *               for a round that is not regular or has rho_0 = 0.
 * One round.  V, g_p, V*, V*^-1 = I, W, Y = W V*^-1 per observation, U, g_c and U* per slot are those of GIMS_AUX_BUNDLE_ADJUST.  "The
 *   slot's order" below is the order stated there for U: lane l of 64 adds the terms of the observations number l, l + 64, ... of the
 *   slot's list (the active observations of its image, ascending in o) and the lanes are summed by a butterfly (offsets 32 .. 1).
 *   Per slot s that is not held, each sum in the slot's order:
 *     B[r] = sum (Y_o[r][0] g_p[0] + Y_o[r][1] g_p[1]) + Y_o[r][2] g_p[2] (g_p of the observation's point),   b_s[r] = -g_c[r] + B[r];
 *     N[i][j] = sum (Y_o[i][0] W_o[j][0] + Y_o[i][1] W_o[j][1]) + Y_o[i][2] W_o[j][2] for i <= j (the slot's own observations only: no
 *     cross term between two observations of one track), M_s[i][j] = M_s[j][i] = U*[i][j] - N[i][j].  M_s is symmetric positive definite
 *     whenever V* is: every term Jc^T Jc - W V*^-1 W^T is positive semi-definite and the damping makes the sum definite.  M_s = L L^T by
 *     the Cholesky of GIMS_AUX_BUNDLE_ADJUST on 6 x 6 (for j ascending: l = sqrt(M_jj), L_ij = M_ij / l for i > j, M_ik -= L_ij L_kj for
 *     j < k <= i); M^-1 r: L y = r (j ascending: y_j = r_j / L_jj, then r_i -= L_ij y_j for i > j), L^T z = y (j descending: z_j = y_j /
 *     L_jj, then y_k -= L_jk z_j for k < j).
 *   A held slot is outside the system: its six words of every vector are 0, and d = 0.
 *   The product q = S v.  Per active point, s = 0, then over its active observations in ascending o whose camera moves, in slot k, for c
 *   ascending: s[m] += W_o[c][m] v[6 k + c]; y[m] = (I[m][0] s[0] + I[m][1] s[1]) + I[m][2] s[2].  Per slot that is not held: q_s[r] =
 *   ((((U*[r][0] v_s[0] + U*[r][1] v_s[1]) + U*[r][2] v_s[2]) + ...) + U*[r][5] v_s[5]) - sum (W_o[r][0] y[0] + W_o[r][1] y[1]) + W_o[r][2]
 *   y[2], y of the observation's point, the sum in the slot's order.
 *   A dot product v . w is per slot ((((v0 w0 + v1 w1) + v2 w2) + v3 w3) + v4 w4) + v5 w5, and the slots are summed by the scheme of the
 *   cost: thread j of 256 adds the slots j, j + 256, ... ascending (a held slot gives 0), a butterfly per wave, the four waves in order.
 *   x = 0, r = b, z = M^-1 r, p = z, rho_0 = rho = r . z.  With rho_0 = 0 there is no iteration and d = 0.  Iteration number it = 1 ..
 *   cg_iters: q = S p; pq = p . q; alpha = rho / pq; x <- x + alpha p; r <- r - alpha q; z = M^-1 r; rho' = r . z; the iteration STOPS iff
 *   rho' <= (cg_tol cg_tol) rho_0 or it = cg_iters; otherwise p <- z + (rho' / rho) p, rho <- rho'.  d = x, rho_stop = the last rho'.
 *   The round is REGULAR iff the det of every active point and every pivot of every M_s is finite and > 0, every pq is finite and > 0 and
 *   every rho (rho_0 and each rho') is finite and >= 0; the first value that fails ends the iteration (cg_used counts the iteration that
 *   found it), d = 0 and the round is not taken.  Back-substitution from d, the candidate, TAKEN, lambda, the stop after
 *   GIMS_BA_MAX_REJECTS rounds and the history are those of GIMS_AUX_BUNDLE_ADJUST.
 * GIMS_EINVAL before any HIP call, each with a message naming bundle_adjust: everything GIMS_AUX_BUNDLE_ADJUST refuses, with
 * GIMS_BA_PCG_MAX_FREE_CAMERAS in the place of its cap; cg_iters outside 1 .. GIMS_BA_PCG_MAX_CG_ITERS; cg_tol not finite, negative or >= 1;
 * table word 7 not 0.  The three words of this form are checked last, behind everything the two forms share.
 * Nothing outside out is written.  A fixed sequence of memset nodes, the upload of the slot tables and 8 + iters (6 + 3 cg_iters) launches:
 * init, classify, slots, fill, sort, back, decide; per round point, setup, cg-init, cg_iters x {y, S p, step}, candidate, back, decide;
 * finish -- 5 + 3 iters when n_free == 0 (init, classify, back, decide; point, back, decide; finish).  The sequence depends on iters,
 * cg_iters and n_free == 0 only: the iterations after the stop are launched and return at once, the decision lives in the state block.
 * No host synchronisation; capturable by gims_ops_graph_create.  No cooperative launch and no barrier across workgroups: workgroups
 * exchange data across kernel boundaries only.
 * How it is computed.  The lists: cam_obs is counted by integer atomics as before; one workgroup scans it into the slots' ranges; a thread
 * per observation takes a place in its slot's range from an integer cursor (any order); workgroups of 256 per slot (sixteen share a long list) then put every entry where
 * its rank among the slot's entries says, so the list ends ascending in o whatever the race was (linear in n_obs up to this ordering,
 * which costs the square of a slot's list length over 256 threads).  A wave per slot forms U*, b, M_s and its factor in registers; a
 * thread per track forms y; a wave per slot forms q_s; one workgroup of 256 does the dot products, the vector updates and M^-1, and one
 * thread of it decides.  There are no float atomics and no sum whose order depends on the grid: the output bytes are identical across
 * runs and graph replays.
 *
 * GIMS_AUX_BUNDLE_ADJUST_FOCAL is the ninth: GIMS_AUX_BUNDLE_ADJUST_PCG with the focal lengths as unknowns.  Every posed
 * image belongs to at most one FOCAL GROUP; a group has one unknown, the relative scale ds of the focal lengths of all its images: fx' =
 * fx (1 + ds), fy' = fy (1 + ds); cx, cy and the ratio fx / fy stay.  Everything not stated here is GIMS_AUX_BUNDLE_ADJUST_PCG's, word for
 * word (activity, status bits, held cameras, the lambda schedule, TAKEN with float32-rounded costs, GIMS_BA_MAX_REJECTS, cg_iters, cg_tol,
 * cg_used, cg_res, the two-buffer state); functions 13 and 14 are unchanged.  kernels: ba_focal_*_kernel, gims_amd/csrc/ba.hip;
 * tests/ba_focal_ref.py is the restatement.
 *   p[], i[] and f[] as for GIMS_AUX_BUNDLE_ADJUST_PCG (i[5] is the form word: read first, must be 0), except table word 7: the HOST
 *               address of int32 group [n_images], 4-byte aligned, read during the call like mode: -1 = the image's intrinsics stay
 *               fixed, 0 .. n_images - 1 = a group id.  n_groups = 1 + the largest id of a posed image (counted on the host before any
 *               HIP call).  The entry of an absent image is ignored.  A group without a posed image is held.
 *   p[5] out    the nine output regions of GIMS_AUX_BUNDLE_ADJUST_PCG at their offsets, then
 *                 double focal_scale [n_groups] | int32 group_obs [n_groups] |
 *                 scratch: 256 bytes of state | int32 [n_images] x 2 | int32 [n_images + 1] | int32 [n_free] | int32 [n_images] |
 *                 double [T][3] | double [n_images][18] | uint8 [T] | uint8 [n_obs] | int32 [n_obs] x 4 | double [T][9] | double [n_obs][50]
 *                 | double [T] | double [T][3] | double [n_free][42] | double [n_free][6] x 6 | int32 [n_images] x 3 | double [n_images][4] |
 *                 double [n_images][2] | double [n_obs][8] | int32 [n_groups + 1] | int32 [n_groups] | double [n_groups] | double
 *                 [n_groups][2] | double [n_groups] x 5
 *               every region on a 256-byte boundary (gims_aux_layout reports the offsets): linear in T, n_obs, n_images, n_free and
 *               n_groups.  focal_scale[g] = the product of the (1 + ds) of the rounds that were taken (1 for a held group); group_obs[g]
 *               = the active observations of the group's posed images.  In the cams region the words fx, fy of every image of a group
 *               that moves hold the refined values; every other word follows the copy-through rule of GIMS_AUX_BUNDLE_ADJUST.
 *   With every entry of group equal to -1 (n_groups = 0) the launches are those of GIMS_AUX_BUNDLE_ADJUST_PCG and the nine shared regions
 *   hold its bytes.
 * The model.  A group collects the active observations of ALL its posed images, those of fixed and held cameras included (fixing a pose
 *   fixes the gauge, not the lens).  A group is HELD iff group_obs < 4; a held group keeps its place in the system as an identity entry
 *   with a zero right-hand side.  For an active observation o of an image of a group that moves: Fu = fx x_c[0] / z, Fv = fy x_c[1] / z
 *   (the products first, as in the residual), both multiplied by the Huber factor sqrt(huber / e) when e > huber, like the other Jacobian
 *   words; G_o[m] = Fu Pu[m] + Fv Pv[m]; GI_o[m] = (G_o[0] I[0][m] + G_o[1] I[1][m]) + G_o[2] I[2][m].
 *   "The image's order": lane l of 64 adds the terms of the entries l, l + 64, ... of the image's list (its active observations ascending
 *   in o; a list exists for every posed image that is a slot or lies in a group), then a butterfly (offsets 32 .. 1).  "The group's
 *   order": the per-image sums are added by the scheme of the cost: thread j of 256 adds the group's posed images j, j + 256, ... in
 *   ascending image index, a butterfly per wave, the four waves in order.
 *   Per group that moves, each sum in the image's order and then the group's order: A = sum Fu Fu + Fv Fv, A* = A + lambda max(A, 1e-6);
 *   g_g = sum Fu ru + Fv rv; b_g = -g_g + sum (GI_o[0] g_p[0] + GI_o[1] g_p[1]) + GI_o[2] g_p[2]; M_g = A* - sum (GI_o[0] G_o[0] + GI_o[1]
 *   G_o[1]) + GI_o[2] G_o[2].  Per slot that moves and whose group moves, in the image's order: C_s[c] = sum Ju[c] Fu + Jv[c] Fv.
 *   The unknowns are [6 words per slot | 1 word per group]; S = [[U*, C], [C^T, A*]] - sum over the points of E V*^-1 E^T, where E stacks
 *   the W_o and G_o rows of the point's observations.  The product q = S v: per active point, s = 0, then over its active observations in
 *   ascending o: first, when the camera moves, for c ascending s[m] += W_o[c][m] v[6 k + c]; then, when the group moves, s[m] += G_o[m]
 *   v_g; y = I s as before.  q_s[r] = (U*[r] . v_s + C_s[r] v_g(s)) - sum W_o[r] . y (the C term only where both move; U*[r] . v_s and the
 *   sum as in function 14).  q_g = (A*_g v_g + sum over the group's images of C_s . v_s) - sum G_o . y, where C_s . v_s is the dot product
 *   of six of function 14 (0 for an image that is no moving slot) and sum G_o . y = sum (G_o[0] y[0] + G_o[1] y[1]) + G_o[2] y[2] in the
 *   image's order; both sums over the images in the group's order.  A held group has q_g = v_g.
 *   The preconditioner: M_s of function 14 unchanged, and the scalar M_g: z_g = r_g / M_g.  A dot product is the slot sum of function 14,
 *   then the group sum sum v_g w_g by the same 256-thread scheme over the groups; the two are added in that order.  The iteration is
 *   function 14's on the longer vectors.  REGULAR needs, in addition, every M_g finite and > 0.
 *   Back-substitution: per active point s = g_p, then over its active observations in ascending o: the camera term of function 14, then s[m]
 *   += G_o[m] ds_g.  The candidate of a group that moves: fx' = fx (1 + ds), fy' = fy (1 + ds) for every image of the group, scale' = scale
 *   (1 + ds); 1 + ds <= 0 or a non-finite fx' or fy' makes the round not TAKEN.  An irregular round has ds = 0.
 * GIMS_EINVAL before any HIP call, each with a message naming bundle_adjust: everything GIMS_AUX_BUNDLE_ADJUST_PCG refuses except table word
 * 7; table word 7 NULL while n_images > 0; table word 7 not 4-byte aligned; the group of a posed image outside -1 .. n_images - 1.
 * Nothing outside out is written.  With n_groups > 0: the memset nodes, the upload of the slot, list and group tables and 8 + iters
 * (10 + 4 cg_iters) + 2 launches: init, classify, groups, lists, fill, sort, back, decide; per round point, focal-point, setup, image, group,
 * cg-init, cg_iters x {y, S p, q_g, step}, candidate, focal-candidate, back, decide; finish, focal-finish -- without setup when n_free == 0
 * (poses fixed, lens and points refined: a valid call) and without lists, fill, sort, image and S p when no image is listed.  The sequence
 * depends on iters, cg_iters, n_free == 0, n_groups == 0 and on whether any image is listed, never on device data.  No host
 * synchronisation; capturable.  No cooperative launch; no float atomics; no sum whose order depends on the grid.
 *
 * GIMS_AUX_SELECT_PAIRS is the tenth function of this table without a stand-alone entry point, for the same reason.  It decides which pairs of
 * an image set are worth matching: a coarse pre-match of a few hundred int8-quantised descriptors per image, all images
 * against all images, a vote per row and the k best partners per image.  This library's own specification: the reference matches one pair and
 * has no counterpart.  kernels: pairs_*_kernel, gims_amd/csrc/pairs.hip; tests/pairs_ref.py is the restatement.  Every decision is taken in
 * integers, so every output is a function of the inputs alone.
 *   p[0] table    HOST int64 [N + 1][GIMS_PAIRS_TABLE_WORDS], 8-byte aligned, read during the call only.  Entry i < N = {address of the
 *                 descriptors of image i (const float* on the device, [n_i][D] with a row stride, 4-byte aligned; may be NULL when m_i = 0),
 *                 row stride in floats (>= D), n_i, address of the selected rows (const int32_t* on the device, m_i entries, 4-byte aligned;
 *                 NULL: rows 0 .. m_i - 1), m_i (0 .. per_image), 0, 0, 0}.  Entry N = {rq, flags, work_bytes, 0, 0, 0, 0, 0}: rq = (int) rint
 *                 ((double) ratio * (double) ratio * 65536) for the float ratio in [0, 1]; the one flag is GIMS_PAIRS_SCALE_GIVEN.
 *   p[1] votes    device int32 [N][N]: votes[i][j] = the rows of image i that vote for image j; the diagonal is 0.  Written whole.
 *   p[2] out      device int32 [3 cap], cap = min(N k, N (N - 1) / 2): pairs [cap][2], then pair_votes [cap].  The call writes the first n_pairs
 *                 entries of each; what lies behind them is left as it was.
 *   p[3] counters device int32 [8] = {n_pairs, n_rows (sum of m_i), n_short_images (m_i < 2), n_bad_rows, n_nonfinite (saturating), 0, 0, 0}
 *   p[4] work     device scratch, 16-byte aligned, of at least the table's work_bytes bytes.  With P_i = m_i rounded up to a multiple of 32,
 *                 pool = max(sum P_i, 1) rounded up to a multiple of GIMS_PAIRS_QUERY_TILE, Dp = the smallest power of two >= D and al256(x) =
 *                 (x + 255) & ~255 the call needs 256 + al256(8 * GIMS_PAIRS_TABLE_WORDS * N) + al256(4 * pool / 32) + al256(pool * Dp) +
 *                 al256(4 pool) + al256(N * N) + 2 al256(4 N) bytes.
 *   p[5] NULL (reserved).   i = {N, D, per_image, k, min_votes, 0 (the form word, read first)}   f = {scale (read with GIMS_PAIRS_SCALE_GIVEN)}
 *   1 Scale.  With GIMS_PAIRS_SCALE_GIVEN s = scale.  Otherwise maxabs = the largest |x| over the finite selected values (an integer maximum
 *     on the float bits) and s = 127.0f / maxabs in float32, 0 when maxabs is 0.  s stays in device memory.
 *   2 Quantise.  q = clamp(rintf(x * s), -127, 127) as int8: one float32 product, rounded half to even; a NaN product (0 times an s that
 *     overflowed) is 0.  A non-finite x is 0 and is counted (n_nonfinite).  A selected index outside 0 .. n_i - 1 is counted (n_bad_rows);
 *     such a row does not exist: it neither votes nor is a neighbour.  |q|^2 per row is int32.
 *   3 Two smallest.  For a row r of image i that exists and an image j != i: d^2 (r, c) = |q_r|^2 + |q_c|^2 - 2 q_r . q_c in int32 over the
 *     rows c of image j that exist; d1 <= d2 are its two smallest values as a multiset.
 *   4 Vote.  r votes for j iff image j has two rows that exist and (int64) d1 * 65536 < (int64) rq * d2.
 *   5 Select.  S[i][j] = votes[i][j] + votes[j][i].  The partners of i are the first min(k, N - 1) of {j != i: S[i][j] >= min_votes} ordered
 *     by (-S[i][j], j); the result is the union over i of (min(i, j), max(i, j)), each once, ascending; pair_votes is S of the pair.
 * GIMS_EINVAL before any HIP call, each with a message naming select_pairs: N outside 2 .. GIMS_PAIRS_MAX_IMAGES; D no multiple of 32 or
 * outside 32 .. GIMS_PAIRS_MAX_D; per_image outside 0 .. GIMS_PAIRS_MAX_ROWS; an m_i outside 0 .. per_image; k < 1; min_votes < 0; rq outside
 * 0 .. 65536; a NULL table, votes, out, counters or work; a NULL descriptor pointer with m_i > 0; a misaligned pointer; a row stride below D; a
 * non-zero reserved word (i[5], p[5], table words 5 .. 7, words 3 .. 7 and the unknown flags of entry N); a scale that is not finite and >= 0;
 * work_bytes below what the call needs.  What the descriptors and the index lists HOLD is not trusted.
 * The launches: the uploads of the table and of the image of every 32 pooled rows, three memset nodes, maxabs (without a given scale),
 * quantise, vote, select, count, scan, fill.  They are fixed by N, the m_i, D and the flag, never by device data.  No host synchronisation;
 * capturable.  Integer atomics only.
 *
 * GIMS_AUX_GUIDED_MATCH is the eleventh, for the same reason.  GUIDED MATCHING runs the descriptor match of gims_nn_match
 * again between the two keypoint sets of a verified pair, counting only partners that agree with the pair's model, and adds what it finds
 * to the matches that are already fixed.  This library's own specification: no part of the reference does this.  kernels: gd_*_kernel and
 * the gated instances of the nn_* bodies, gims_amd/csrc/nn.hip; tests/guided_ref.py is the restatement.
 *   p[0] table    HOST int64 [n_pairs][GIMS_GUIDED_TABLE_WORDS], 8-byte aligned, read during the call only.  The words of one pair:
 *                  0 A, 1 B          const float* DEVICE, [n0][d] / [n1][d], point-major, gims_nn_match's pitch and alignment rules
 *                  2 lda, 3 ldb      row pitches in floats     4 n0, 5 n1 (1 .. 32768 each; n1 = 1 is served)     6 d (a multiple of 32 in 32 .. 512)
 *                  7 kpts0, 8 kpts1  const float* DEVICE [n0][2] / [n1][2], pixels
 *                  9 model           const float* DEVICE [9], row-major       10 kind: GIMS_VERIFY_MODEL_HOMOGRAPHY (x1 ~ H x0) or _FUNDAMENTAL
 *                 11 ok              const float* DEVICE, one word (the ok column of a gims_verify_pairs record), or 0
 *                 12 prior           const int64_t* DEVICE [n0] or 0;  13 prior_mask const uint8_t* DEVICE [n0] or 0;  14 prior_scores const
 *                                    float* DEVICE [n0] or 0 (13 and 14 are read with a prior only)
 *                 15 mutual          non-zero adds the mutual test and the outputs cnn1 and matches1
 *                 16 nn1, 17 nn2 int32 [n0];  18 d1, 19 d2, 20 ratio float32 [n0];  21 n_admissible int32 [n0];  22 matches0 int64 [n0];
 *                 23 scores0 float32 [n0];  24 added0 uint8 [n0];  25 cnn1 int32 [n1] and 26 matches1 int64 [n1] (read with mutual only);
 *                 27 info int32 [8]  -- all DEVICE, caller-owned, required
 *                 28 thresh, 29 ratio, 30 max_distance: the BITS of a float32 in the low half of the word (pixels, finite, > 0; the ratio
 *                                    threshold; +inf for none)        31 reserved, 0
 *   p[1] work     device scratch, 256-byte aligned.  p[2] .. p[5] NULL (reserved).
 *   i = {n_pairs, flags (GIMS_NN_EXHAUSTIVE or 0), work_bytes, 0, 0, 0 (the form word, read first)}     f = {0, 0} (reserved)
 *   work_bytes: every region on 256 bytes (al256).  P pairs; Q problems (nx, ny): (n0, n1) per pair and with mutual also (n1, n0).  As in
 *   gims_nn_match, want = ceil(512 / sum over the problems of ceil(nx / 128)) clamped to 1 .. 8 and per problem tiles = ceil(ny / 128),
 *   tiles_per = ceil(tiles / min(want, tiles)), csplit = ceil(tiles / tiles_per).  The call needs
 *     al256(160 Q) + al256(200 P) + al256(16 P) + al256(48 Q) + al256(232 P) + al256(16 P) + al256(4 sum n1)
 *     + per pair     al256(8 n0) + al256(8 n1) + al256(4 n0) + al256(4 n1) + al256(32 n0) + al256(32 n1) + al256(n0)
 *     + per problem  al256(4 nx), for the (n1, n0) problem also 3 al256(4 nx), and without GIMS_NN_EXHAUSTIVE 2 al256(64 nx csplit) +
 *                    al256(16 nx csplit)
 *   bytes; gims_aux_layout reports it from the routine that carves it.
 * All of it is decided in float64, every product and every sum rounded on its own (no contraction), division correctly rounded; the float32
 * inputs are widened first.
 *   1 Has a model.  Iff ok is 0 (no pointer) or *ok != 0, and all nine entries of the model are finite.  Without a model no row searches:
 *     the output is the fixed rows of 2 alone and info[5] = 1.
 *   2 Fixed rows, taken columns.  Row i CLAIMS column prior[i] iff a prior is given, the mask is absent or mask[i] != 0, and 0 <= prior[i] <
 *     n1.  Row i is FIXED iff it is the lowest row that claims its column (the integer minimum over the claimants).  A claimed value other
 *     than -1 outside 0 .. n1 - 1 is counted in info[3] and never used as an index (a row the mask switches off is not read).  A claimant
 *     that lost its column is counted in info[4], is not fixed and searches like an unmatched row.  The column of a fixed row is TAKEN.
 *   3 Per-row words, computed ONCE by a prologue launch and read by every later pass.
 *     fundamental, row i of A (u, v):  la = (F00 u + F01 v) + F02, lb and lc likewise from rows 1 and 2 of F, g = la^2 + lb^2
 *     fundamental, row j of B (u', v'): ma = (F00 u' + F10 v') + F20, mb = (F01 u' + F11 v') + F21, h = ma^2 + mb^2
 *     homography, row i:  p = H (u, v, 1) in the same order of operations, a = (px / pw, py / pw); valid iff fabs(pw) > 0
 *     homography, row j:  q = C (u', v', 1), C the transposed matrix of cofactors of H (C00 = H11 H22 - H12 H21, C01 = H02 H21 - H01 H22,
 *       C02 = H01 H12 - H02 H11, C10 = H12 H20 - H10 H22, C11 = H00 H22 - H02 H20, C12 = H02 H10 - H00 H12, C20 = H10 H21 - H11 H20,
 *       C21 = H01 H20 - H00 H21, C22 = H00 H11 - H01 H10; no division by the determinant), b = (qx / qw, qy / qw); valid iff fabs(qw) > 0
 *   4 Admissible(i, j), symmetric by construction; both directions use this one definition.  Neither i fixed nor j taken, and
 *     fundamental: n = (la u' + lb v') + lc; g > 0, h > 0, n^2 <= t^2 g and n^2 <= t^2 h (the distance of each point to the other's epipolar
 *       line), t^2 = double(thresh)^2
 *     homography: both rows valid, (ax - u')^2 + (ay - v')^2 <= t^2 and (bx - u)^2 + (by - v)^2 <= t^2
 *     A comparison with a NaN is false.  n_admissible[i] is the count over all j.
 *   5 Two nearest.  S(i, j) is gims_nn_match's exact squared distance.  nn1 / nn2 are the two nearest ADMISSIBLE columns by (S, j).  One
 *     admissible column: nn2 = -1, d2 = +inf, ratio 0.  None: nn1 = -1, d1 = +inf, ratio NaN.  d1, d2, ratio float32 as in gims_nn_match.
 *   6 Match.  match = ratio < threshold && d1 <= max_distance, with mutual also cnn1[nn1[i]] == i (cnn1[j] = j's nearest admissible row
 *     of A, -1 when it has none).  A searching row: matches0 = match ? nn1 : -1, scores0 = match ? 1 - ratio : 0, added0 = match.  A fixed
 *     row: matches0 = prior[i], added0 = 0, scores0 = prior_scores[i] when given, else 1; it is not searched: nn1 = prior[i], nn2 = -1,
 *     d1 = d2 = +inf, ratio = NaN, n_admissible = 0.  With mutual matches1 is the inverse of matches0, fixed rows included: one-to-one.
 *   7 info = {rows of A re-solved exhaustively, rows of B re-solved exhaustively, n_fixed, n_bad_prior, n_dup_prior, no_model, n_added, 0}.
 * A row's outputs are bit-identical whichever way it went, and under GIMS_NN_EXHAUSTIVE.  The certificate is gims_nn_match's with one rule
 * added: a row all of whose candidate lists are short has every admissible column listed and is certified without the inequality.
 * GIMS_EINVAL before any HIP call, each with a message naming guided_match: the size and alignment rules of gims_nn_match (with n1 >= 1); an
 * unknown kind; a thresh that is not finite and > 0; a max_distance that is NaN or negative; a NULL required pointer; a non-zero reserved
 * word (i[3], i[4], p[2] .. p[5], f, word 31, the high halves of words 28 .. 30); unknown flags; a workspace below work_bytes' need.  What
 * the arrays HOLD is never trusted.
 * The launches: four table uploads, three memset nodes, claim, prologue, norms, candidate and refine (not under GIMS_NN_EXHAUSTIVE),
 * exhaustive, finish -- each ONE launch for all directions of all pairs, fixed by the sizes and flags, never by device data.  No host
 * synchronisation; capturable.  Integer atomics only. */
#define GIMS_OP_AUX 2
#define GIMS_AUX_SPLIT_SPL32 0
#define GIMS_AUX_SAGE_MEAN_SPLIT 1
#define GIMS_AUX_KENC_FIRST 2
#define GIMS_AUX_SAGE_MEAN 3
#define GIMS_AUX_KENC_FIRST_LINEAR 4
#define GIMS_AUX_LAYERNORM_ACT 5
#define GIMS_AUX_SIFT_DESCRIBE 6
#define GIMS_AUX_DIOU_NMS 7
#define GIMS_AUX_ASSEMBLE_ROWS 8
#define GIMS_AUX_BUILD_TRACKS 9
#define GIMS_TRACKS_TABLE_WORDS 8
#define GIMS_TRACKS_SCAN_TILE 2048
#define GIMS_TRACKS_SHORT_SEGMENT 32
#define GIMS_TRACKS_LONG_SEGMENT 1024
#define GIMS_TRACKS_KEEP_CONFLICTING (1 << 30)
#define GIMS_AUX_TRIANGULATE_TRACKS 10
#define GIMS_TRI_CAMERA_WORDS 18
#define GIMS_TRI_MAX_OBS 1024
#define GIMS_TRI_SHORT_TRACK 4
#define GIMS_AUX_RESECT_IMAGES 11
#define GIMS_RESECT_CAMERA_WORDS 6
#define GIMS_RESECT_HB 16
/* 12 is unassigned and stays refused as an unknown auxiliary function */
#define GIMS_AUX_BUNDLE_ADJUST 13
#define GIMS_BA_TABLE_WORDS 8
#define GIMS_BA_MAX_FREE_CAMERAS 128
#define GIMS_BA_MAX_REJECTS 5
#define GIMS_AUX_BUNDLE_ADJUST_PCG 14
#define GIMS_BA_PCG_MAX_FREE_CAMERAS 65536
#define GIMS_BA_PCG_MAX_CG_ITERS 256
/* 15 is unassigned and stays refused as an unknown auxiliary function */
#define GIMS_AUX_BUNDLE_ADJUST_FOCAL 16
#define GIMS_AUX_SELECT_PAIRS 17
#define GIMS_PAIRS_TABLE_WORDS 8
#define GIMS_PAIRS_MAX_IMAGES 8192
#define GIMS_PAIRS_MAX_ROWS 4096
#define GIMS_PAIRS_MAX_D 1024
#define GIMS_PAIRS_QUERY_TILE 128
#define GIMS_PAIRS_SCALE_GIVEN 1
#define GIMS_AUX_GUIDED_MATCH 18
#define GIMS_GUIDED_TABLE_WORDS 32
typedef struct gims_aux_args { int32_t fn, reserved; const void* p[6]; int64_t i[6]; float f[2]; } gims_aux_args;
typedef struct gims_op { int32_t kind; int32_t reserved; union { gims_linear_args lin; gims_attn_args att; gims_aux_args aux; } u; } gims_op;
int gims_run_ops(const gims_op* ops /* HOST */, int32_t n_ops, void* stream);
/* Where an auxiliary function puts every region of its caller-allocated buffer, for the sizes given: the function's own layout routine (the
 * one its launch runs) walked without a buffer.  Host arithmetic only, no HIP call: it works with no device present.  fn and sizes:
 *   GIMS_AUX_TRIANGULATE_TRACKS   {T, n_obs}                                     the buffer p[5]
 *   GIMS_AUX_RESECT_IMAGES        {m, S, iters}, S = the sum of the entries' n_k  the buffer p[5]
 *   GIMS_AUX_BUNDLE_ADJUST        {T, n_obs, n_images, iters, n_free}            the buffer p[5]
 *   GIMS_AUX_BUNDLE_ADJUST_PCG    {T, n_obs, n_images, iters, n_free}            the buffer p[5]
 *   GIMS_AUX_BUNDLE_ADJUST_FOCAL  {T, n_obs, n_images, iters, n_free, n_groups}  the buffer p[5]
 *   GIMS_AUX_DIOU_NMS             {n, n_images}                                  the workspace p[5]
 *   GIMS_AUX_BUILD_TRACKS         {N}                                            the workspace p[5]
 *   GIMS_AUX_SELECT_PAIRS         {D, N, m_0 .. m_{N-1}}                         the workspace p[4]
 *   GIMS_AUX_GUIDED_MATCH         {flags, P, (n0, n1, mutual) x P}               the workspace p[1]
 * offsets[r] receives the byte offset of region r, in the order of the function's description (every region on a 256-byte boundary, so
 * region r extends to offsets[r + 1], the last one to *bytes); *n_regions their number; *n_outputs the index of the first scratch region,
 * i.e. the number of output regions (0 for a workspace, which is scratch only); *bytes the size of the whole buffer.  offsets may be NULL
 * with capacity 0 to ask for the counts and the bytes only.  GIMS_EINVAL, with a message naming gims_aux_layout: a function that is
 * unknown or has no such buffer (GIMS_AUX_SIFT_DESCRIBE, GIMS_AUX_ASSEMBLE_ROWS); a wrong n_sizes; a size outside the range the function
 * itself accepts; a capacity below *n_regions. */
int gims_aux_layout(int32_t fn, const int64_t* h_sizes /* HOST */, int32_t n_sizes, int64_t* h_offsets /* HOST, or NULL */, int32_t capacity,
                    int32_t* n_regions, int32_t* n_outputs, size_t* bytes);
/* The same replay with a HIP event recorded on `stream` before the first op and after every op: events is a HOST array of
 * n_ops + 1 event handles from gims_events_create.  gims_events_elapsed (after the stream has been synchronised) returns the
 * n - 1 intervals between n consecutive events in milliseconds: per-kernel durations of the production path, taken on the
 * stream the kernels run on.  (Instrumentation of this build; the reference prints wall-clock stage times, gmatcher.py:226-243.) */
int gims_run_ops_timed(const gims_op* ops /* HOST */, int32_t n_ops, void* stream, void* const* events /* HOST, n_ops + 1 */);
int gims_events_create(int32_t n, void** events_out /* HOST array of n handles */);
int gims_events_elapsed(void* const* events /* HOST */, int32_t n, float* h_ms_out /* HOST, n - 1 */);
int gims_events_destroy(void* const* events /* HOST */, int32_t n);
/* The same sequence as a HIP graph: gims_ops_graph_create captures the launches of `ops` on `stream` (nothing executes),
 * gims_ops_graph_launch replays them (one graph launch: no per-kernel launch gaps), gims_ops_graph_destroy frees the graph.
 * Every op must have run once through gims_run_ops before (first-use initialisation cannot happen inside a capture), and
 * every pointer in `ops` must stay valid for as long as the graph is launched. */
int gims_ops_graph_create(const gims_op* ops /* HOST */, int32_t n_ops, void* stream, void** graph_exec_out);
int gims_ops_graph_launch(void* graph_exec, void* stream);
int gims_ops_graph_destroy(void* graph_exec);

/* ------------------------------------------------------------------------------------------------
 * Keypoint encoder front end: normalize_keypoints (gmatcher.py:26-33, with the reference's NHWC-as-NCHW
 * quirk resolved by the caller into cx, cy, scale) fused with the first Conv1d(2->c1)+BN(eval)+ReLU of
 * KeypointEncoder (gmatcher.py:87-97).  w1: [c1][2] and b1: [c1] have BatchNorm already folded in.
 * kpts: [n][2] pixel xy.  out: [n][c1].  Per-row normalisation parameters: norm[row_seg[i]] = {cx,cy,scale}.
 */
int gims_kenc_first(const float* kpts, const float* norm3 /* [n_seg][3] */, const int32_t* seg_of_row,
                    const float* w1, const float* b1, int32_t c1, float* out, int64_t n, void* stream);
/* Same without the ReLU (the use_layernorm=True variant normalises before activating). */
int gims_kenc_first_linear(const float* kpts, const float* norm3, const int32_t* seg_of_row,
                           const float* w1, const float* b1, int32_t c1, float* out, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * LayerNorm of the reference's use_layernorm=True variant + activation.
 * replaces: class LayerNorm (gmatcher.py:74-85) as MLP() inserts it between Conv1d and ReLU (gmatcher.py:19-23):
 *   y[r, :] = a2 * (x[r, :] - mean_r) / (std_r + eps) + b2   over the c channels of point r, std UNBIASED (c - 1),
 *   eps added to the std.  out (f32, may be NULL or == x) and/or out_hi/out_lo (SPL32 split planes, see gims_linear).
 * 2 <= c <= 512.  GIMS_EINVAL before any HIP call: ldx < c, ldo < c with out given, ld_split < 2 * (c rounded up to 32) with the planes given.
 */
int gims_layernorm_act(const float* x, int64_t ldx, int64_t rows, int32_t c, const float* a2, const float* b2, float eps,
                       int32_t act, float* out /* may be NULL */, int64_t ldo, uint16_t* out_hi /* may be NULL */,
                       uint16_t* out_lo, int64_t ld_split, void* stream);

/* ------------------------------------------------------------------------------------------------
 * GraphSAGE mean aggregation over the adaptive graph (CSR by destination, both edge directions):
 *   out[i, :] = mean_{j in indices[indptr[i]:indptr[i+1]]} h[j, :]     (zero for isolated nodes)
 * replaces: the message passing of dgl.nn.SAGEConv(...,'mean') (call sites gmatcher.py:149-151,158).
 * Row ids in `indices` are absolute rows of h.  c must be a multiple of 4.
 */
int gims_sage_mean(const float* h, int64_t ldh, const int32_t* indptr, const int32_t* indices,
                   int32_t n, int32_t c, float* out, int64_t ldo, void* stream);
/* The same mean written directly as SPL32 split-bf16 planes (the A-operand layout of GIMS_PREC_BF16X3 pre-split GEMMs,
 * see gims_split_spl32): hi + lo of every f32 mean, no f32 copy.  ld_spl in bf16 elements, >= 2 * c (c rounded up to 32). */
int gims_sage_mean_split(const float* h, int64_t ldh, const int32_t* indptr, const int32_t* indices,
                         int32_t n, int32_t c, uint16_t* out_spl, int64_t ld_spl, void* stream);

/* Per-pair match statistics of a batch whose outputs are concatenated (the record the multi-GPU harness all-gathers,
 * SURVEY 8(e); the reference's eval loop keeps the same numbers per pair on the host, eval_homography.py:186-236):
 *   table[p] = {pair_id, n0, n1, offset of the pair's rows in matches0 / scores0}  (int32 x 4, device memory)
 *   out[p]   = {pair_id, n0, n1, #matches (matches0 >= 0), mean matching score over the matches (0 if none)}  (f32 x 5)
 * Fixed summation order: the result is deterministic. */
int gims_pair_stats(const int64_t* matches0, const float* scores0, const int32_t* table, int32_t n_pairs, float* out, void* stream);

/* Gather rows: dst[i, :] = src[idx[i], :]  (kept-keypoint compaction, gmatcher.py:244-249).  lds, ldd >= c (GIMS_EINVAL otherwise). */
int gims_gather_rows(const float* src, int64_t lds, const int32_t* idx, int32_t n, int32_t c,
                     float* dst, int64_t ldd, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Adaptive graph construction for a BATCH of images (models/agc.py:682-709, live subset), every stage one
 * launch for all images (blockIdx.y = image):
 *   cosine similarity (382-391) -> exact percentile threshold over the strict upper triangle (367-380,
 *   439-440) -> radius pairs in float64, inclusive (435-436) filtered by sim >= thr (445-447) ->
 *   connect_isolated_nodes (476-495) -> remove_small_components (497-516) -> fast_connect_components
 *   (518-565, one round) -> sorted relabel + bidirectional CSR (dgl.from_networkx, 704).
 * Per image: kpts [n][2] f32, desc [n][d] f32 (point-major, un-normalised); outputs (device): kept[n]
 * (first n_kept entries: sorted original ids), indptr[n+1] (first n_kept+1 valid), indices[max_edges_dir]
 * in kept-relabelled ids, info[8] = {n_kept, n_dir_edges, n_coarse_edges, n_iso_added,
 * n_components_after_removal, n_link_added, threshold bits (f32), flags: bit 0 = an edge / candidate buffer overflowed (repeat with a larger
 * max_edges_dir), bit 1 = the percentile window did not hold, see below}.
 * `work` is scratch of at least gims_agc_workspace_bytes(images, n_images, flags) bytes.
 * LIMIT: 2 <= n <= gims_agc_max_keypoints() = 32768 keypoints per image (GIMS_EINVAL above it; the reference -- NumPy / SciPy -- has no
 * limit and publishes runs with up to 21 163 kept keypoints, tools/files/rgbd1/record.txt:635).  What bounds it: a pair of node ids is one
 * packed 32-bit word (i << 16 | j), the sequential isolated-node walk keeps its ordered list in LDS (135 KB of 160 KB at 32768), and the
 * workspace reserves one word per pair of the strict upper triangle (n^2 * 2 bytes: 0.9 GB per image at 21 163, 2.1 GB at 32768) -- and
 * the ROBUST flow as much again for the half similarity matrix it stores (gims_agc_workspace_bytes with GIMS_AGC_ROBUST: 1.8 GB / 4.3 GB).  Images
 * above 16384 keypoints run the component search in global memory instead of LDS (same labels).
 * Exact-distance ties in the two sequential fix-ups resolve to the lowest node index.
 * Asynchronous; read info[] after synchronising the stream.
 */
typedef struct gims_agc_image {
  const float* kpts; const float* desc; int64_t ldd; int32_t n, d;
  int32_t* kept; int32_t* indptr; int32_t* indices; int32_t max_edges_dir; int32_t* info;
} gims_agc_image;

/* flags of the two calls below.  The percentile threshold is exact in both flows (the k-th smallest of the similarities as the library evaluates
 * them: float64 dot products of the normalised f32 rows, rounded once); they differ in how the entries that can decide it are found.
 * Default: a sample of one-pass half-precision similarities predicts a window of values that holds rank k, one pass over all N^2/2 of
 * them counts what lies below the window and lists what lies inside it, and only the listed entries (and the radius candidates) are
 * evaluated exactly.  The prediction is VERIFIED on the device against a rigorous bound of the half-precision error; if it did not hold,
 * bit 1 of info[7] is set (bit 0: edge capacity) and every other output of that image -- bit 0 included -- is to be discarded: repeat the call with
 * GIMS_AGC_ROBUST, which histograms every entry instead of predicting (about 0.2 ms more per 16 images of 4096).  Images of at most 1536
 * keypoints are "sampled" in full and never report bit 1. */
#define GIMS_AGC_ROBUST 1
/* Scratch bytes of gims_agc_build(..., flags, ...): the default (window) flow never stores the N x N half similarity matrix, which is half of
 * the robust flow's workspace -- a batch of README-size images (15 k keypoints) asks for 0.5 GB per image instead of 0.9.  A call whose
 * images force the robust flow (d % 64 != 0 or d > 256; GIMS_AGC_ROBUST=1 in the environment) is sized for it whatever the flags say.
 * flags = GIMS_AGC_ROBUST is enough for either flow. */
size_t gims_agc_workspace_bytes(const gims_agc_image* h_images /* HOST array */, int32_t n_images, int32_t flags);
int32_t gims_agc_max_keypoints(void);
/* The graph parameters: n_params == 1, one (radius, percentile, min_size) for the whole batch, or n_params == n_images, h_params[i] belongs
 * to h_images[i] (still one launch per stage for the whole batch); any other n_params is GIMS_EINVAL.  `reserved` is not read (keep it 0). */
typedef struct gims_agc_params { double radius, percentile; int32_t min_size, reserved; } gims_agc_params;
int gims_agc_build(const gims_agc_image* h_images /* HOST array */, int32_t n_images, const gims_agc_params* h_params /* HOST [n_params] */,
                   int32_t n_params, int32_t flags, void* work, size_t work_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Delaunay graph construction for a BATCH of images (D-GIMS: the reference's build_graph_from_keypoints_Delaunay, models/agc.py:718-751,
 * which forward() calls instead of the adaptive build when data['delaunay'] is set), every stage one launch for all images (blockIdx.y =
 * image), no host synchronisation.  Same image descriptor as gims_agc_build; `desc` / `ldd` / `d` are not read.
 * Per image: the Delaunay triangulation of kpts [n][2] f32 as an undirected graph, written as a bidirectional CSR in ORIGINAL keypoint ids
 * (neighbours ascending): kept[n] = 0..n-1, indptr[n+1], indices[max_edges_dir]; info[8] = {n_kept = n, n_dir_edges, n_undirected_edges,
 * n_duplicates, n_hull_vertices, n_exact_fallbacks, 0, flags}.
 *   Exact duplicate coordinates: the LOWEST id of each group of identical (x, y) is the vertex, the others are isolated (degree 0).
 *   Cocircular ties: resolved by a symbolic perturbation of the lifted coordinate by id (gims_amd/csrc/delaunay_pred.h states the rule): one
 *   deterministic triangulation.  Predicates are exact (float64 filter, exact expansion fallback; n_exact_fallbacks counts the points
 *   whose star needed the fallback).
 *   flags: bit 0 = the directed edges did not fit max_edges_dir (n_dir_edges says how many there are; the CSR is void);
 *          bit 2 (GIMS_DT_INFO_DEGENERATE) = fewer than 3 distinct points, all points collinear, or a non-finite coordinate: no triangulation;
 *          bit 3 (GIMS_DT_INFO_ASYMMETRIC) = the stars did not agree (an edge present in one direction only): the result must not be used.
 * `work` is scratch of at least gims_delaunay_workspace_bytes(images, n_images) bytes (about 46 bytes per keypoint).
 * LIMIT: 1 <= n <= gims_agc_max_keypoints() = 32768 keypoints per image (GIMS_EINVAL outside).
 * Asynchronous; read info[] after synchronising the stream.
 */
#define GIMS_DT_INFO_DEGENERATE 4
#define GIMS_DT_INFO_ASYMMETRIC 8
size_t gims_delaunay_workspace_bytes(const gims_agc_image* h_images /* HOST array */, int32_t n_images);
int gims_delaunay_build(const gims_agc_image* h_images /* HOST array */, int32_t n_images, void* work, size_t work_bytes, void* stream);

/* Ingest a batch of images given in the reference's layout (descriptors channel-major (D,N), gmatcher.py:245) into
 * one row-concatenated point-major buffer: desc_out[row_off_i + n, :] = desc_i[:, n], same for keypoints and scores.
 * One launch for the whole batch (64x64 LDS-tile transpose). */
typedef struct gims_ingest_image {
  const float* kpts; const float* desc; int64_t ldd; const float* score; int32_t n, row_off;
} gims_ingest_image;

int gims_ingest_images(const gims_ingest_image* dev_images /* DEVICE array */, int32_t n_images, int32_t max_n, int32_t d,
                       float* desc_out, int64_t ldo, float* kpts_out, float* score_out /* may be NULL */, void* stream);

/* Pack the kept keypoints of a batch of images into the row-concatenated layout the rest of the path uses
 * (gmatcher.py:244-249): for image i with row offset ro_i and edge offset eo_i,
 *   feat[ro_i + r, :] = desc_i[kept_i[r], :],  kpts_out[ro_i + r] = kpts_i[kept_i[r]],  score_out likewise,
 *   seg[ro_i + r] = i,  indptr_out[ro_i + r] = indptr_i[r] + eo_i,  indices_out[eo_i + e] = indices_i[e] + ro_i
 * and indptr_out[n_rows_total] = n_edges_total. */
typedef struct gims_pack_image {
  const float* kpts; const float* desc; int64_t ldd; const float* score;
  const int32_t* kept; const int32_t* indptr; const int32_t* indices;
  int32_t n_kept, n_edges, row_off, edge_off;
  /* optional: src_row[ro_i + r] = in_off + kept_i[r], the row of kept keypoint r in an array over ALL input keypoints of the batch in which
   * image i starts at row in_off (gims_linear_args.residual_rows).  src_row is the whole batch's array; NULL = not written. */
  int32_t* src_row; int32_t in_off, reserved;
} gims_pack_image;

int gims_pack_graphs(const gims_pack_image* dev_images /* DEVICE array */, int32_t n_images, int32_t max_kept,
                     int32_t max_edges, int32_t d, float* feat, int64_t ldf, float* kpts_out, float* score_out,
                     int32_t* seg, int32_t* indptr_out, int32_t* indices_out, int32_t n_rows_total,
                     int32_t n_edges_total, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Log-domain Sinkhorn optimal transport + mutual-argmax match selection.
 * replaces: log_optimal_transport / log_sinkhorn_iterations (gmatcher.py:41-69) and the selection block
 * (gmatcher.py:284-294).  The (N+1)x(M+1) couplings matrix is never materialised: the dustbin row and
 * column (= alpha) are handled analytically, and the iteration runs in the absorbed-potential form
 *   P_ij = exp(Z_ij + u_i + v_j);  u_i += log mu_i - log sum_j P_ij;  v_j += log nu_j - log sum_i P_ij
 * which is the reference recurrence u = log mu - LSE_j(Z + v), v = log nu - LSE_i(Z + u) rewritten so
 * that one sweep over Z serves both the row update and the following column update.
 * scores: f32 [n][ld] (inner N x M block, already divided by sqrt(D)).  Problems are independent
 * (one per image pair); `work` needs gims_sinkhorn_workspace_bytes(...) bytes.
 * Outputs per problem (device): matches0 [n] int64, matches1 [m] int64, mscores0 [n] f32, mscores1 [m]
 * f32, uv: u [n+1] then v [m+1] (log-potentials, so that OT = Z + u + v - norm can be rebuilt) then one
 * status word (0 = ok, 1 = a marginal left the finite range: matches are then all -1; 2 is transient: the on-chip
 * kernel could not get all its workgroups resident and gave up -- the call then re-solves THAT problem with a
 * dependency-free kernel before the selection runs (slow, rare), so a caller never sees 2 nor -1s caused by it).
 * Two implementations of the iteration loop (same recurrence, results agree to f32 rounding):
 *   streamed  -- one launch per iteration, Z read from HBM once per iteration (any size);
 *   resident  -- ONE launch for all iterations of a group of problems: exp(Z + u + v) is held in the registers and LDS
 *                of the 256 CUs and scaled lazily by cumulative row / column factors (re-derived from Z every 50 iterations and on the last),
 *                no HBM traffic inside the loop.  Used when the matrices fit on chip (n, m <= 4096, about 134 MB of
 *                matrix per launch) and are large enough to pay (>= 6 M entries); GIMS_OT_RESIDENT=0 / 2 in the
 *                environment forces streamed / resident.  gims_sinkhorn_plan() tells which one a call will take.
 *                The on-chip kernel is the 2-D decomposition of csrc/sinkhorn2d.hip (a problem is cut into row
 *                groups, one per XCD, times 128-column blocks, one per CU; the row-sum exchange stays inside the XCD's L2, only
 *                a 0.5-KB column edge crosses XCDs; start potentials formed in the kernel).
 */
typedef struct gims_ot_problem {
  const float* scores; int64_t ld; int32_t n, m;
  int64_t* matches0; int64_t* matches1; float* mscores0; float* mscores1;
  float* uv;                                /* [n+1 + m+1 + 1] */
} gims_ot_problem;

size_t gims_sinkhorn_workspace_bytes(const gims_ot_problem* h_problems, int32_t n_problems);
/* flags of the two calls below.  GIMS_OT_STREAMED: never take an on-chip kernel -- they occupy every CU of the device for the
 * whole solve and wait on each other across workgroups, so a caller that runs several streams (or processes) on one GPU
 * concurrently must use the streamed kernels: next to another stream's kernels an on-chip solve cannot get its 256 workgroups
 * resident, gives up and is re-solved by the slow rescue path. */
#define GIMS_OT_STREAMED 1
/* 0: the call will run streamed; k > 0: resident, in k launches.  (Query only; no reference counterpart.) */
int gims_sinkhorn_plan(const gims_ot_problem* h_problems, int32_t n_problems, int32_t iters, int32_t flags);
int gims_sinkhorn_match(const gims_ot_problem* h_problems /* HOST array */, int32_t n_problems, float alpha,
                        int32_t iters, float match_threshold, void* work, size_t work_bytes, int32_t flags, void* stream);

/* Diagnostics: how many on-chip solves gave up and were re-solved by a rescue path on the CURRENT device since the process started
 * (synchronises the device; -1 on error).  A given-up solve is re-solved inside the same call -- by the streamed kernels when a
 * give-up was seen during the last 256 calls (GIMS_OT_RESCUE=1: always), else by a one-workgroup kernel -- so results never
 * depend on it; the counter lets a caller (and the tests) see that it happened.  No reference counterpart. */
int64_t gims_sinkhorn_rescues(void);

/* ------------------------------------------------------------------------------------------------
 * Per-pair evaluation after the matcher -- batched over pairs, everything stays on the device.
 * replaces: the per-pair block of eval_homography.py:186-226 --
 *   torch_find_matches(kp0, kp1, H_gt, dist_thresh=3, n_iters=3) (utils/preprocess_utils.py:98-132, with warp_keypoints
 *   :86-96 and torch_cdist :74-78), precision / recall (:207-209, 222-226), cv2.getPerspectiveTransform on the four most
 *   confident matches (:216-217), cv2.findHomography(RANSAC) (:193, 218) and the corner error (:210, 219-223,
 *   utils/common.py:477-481).  The GT matching reproduces the reference's float32 arithmetic (index sets are exact); the
 *   two OpenCV calls are restated from their documented semantics -- the RANSAC is this build's own deterministic one,
 *   OpenCV's sampler is not reproducible.  Specification (float64; also restated in oracle/eval_oracle.py):
 *     hypothesis h = 0 .. iters-1: state = seed ^ (h * 0xD1342543DE82EF95); four DISTINCT indices into the ascending list of
 *     valid matches are successive splitmix64(state) % K values (duplicates skipped); H_h = exact 4-point homography
 *     (h22 = 1); score = #matches with ||H_h p0 - p1||^2 <= thresh^2; best = highest score, lowest h on ties; then ONE
 *     least-squares refit (normal equations of the 2K x 8 DLT system) on the inliers of the best hypothesis, and the final
 *     inlier mask / count / corner error under the refit model.  The four most confident matches of the DLT are taken
 *     with ties broken by the earlier match.
 * Outputs per pair: gt0 [n0] int32 (GT partner in image 1 or -1), inlier [n0] uint8 (1 where the match of keypoint i is
 * a RANSAC inlier), record float[16] (GIMS_EVAL_* below), homographies float[18] (H_dlt then H_ransac, row-major).
 */
typedef struct gims_eval_pair {
  const float* kpts0; const float* kpts1;   /* kept keypoints [n0][2], [n1][2] (what GMatcher returns as keypoints0/1) */
  const int64_t* matches0;                  /* [n0] */
  const float* mscores0;                    /* [n0] */
  int32_t n0, n1, height, width;            /* image 0 size for the corner error */
  float h_gt[9];                            /* ground-truth homography, row-major */
  int32_t* gt0; uint8_t* inlier; float* record; float* homographies;
} gims_eval_pair;
#define GIMS_EVAL_NVALID 0      /* matches0 > -1 */
#define GIMS_EVAL_NGT 1         /* GT correspondences found */
#define GIMS_EVAL_NCORRECT 2    /* matches0[i] == gt0[i] >= 0 */
#define GIMS_EVAL_NFN 3         /* unmatched keypoints that have a GT partner */
#define GIMS_EVAL_PRECISION 4
#define GIMS_EVAL_RECALL 5
#define GIMS_EVAL_NINLIERS 6
#define GIMS_EVAL_ERR_DLT 7     /* mean corner distance, -1 when no model */
#define GIMS_EVAL_ERR_RANSAC 8
#define GIMS_EVAL_DLT_OK 9
#define GIMS_EVAL_RANSAC_OK 10
size_t gims_eval_workspace_bytes(const gims_eval_pair* h_pairs, int32_t n_pairs, int32_t ransac_iters);
int gims_eval_pairs(const gims_eval_pair* h_pairs /* HOST array */, int32_t n_pairs, float dist_thresh, int32_t n_iters,
                    float ransac_thresh, int32_t ransac_iters, uint64_t seed, void* work, size_t work_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Geometric verification without a ground truth -- batched over sets of correspondences, everything stays on the device.
 * replaces: cv2.findHomography(points0, points1, cv2.RANSAC | cv2.USAC_DEFAULT) and the count of its mask (`correct_matches`) in
 *   eval_homography.py:191, eval_matches.py:71,164 and tools/parameter_search.py:161.  Parity with OpenCV is unpinned as for
 *   gims_eval_pairs: the estimator is this build's own; its SPECIFICATION is this comment (restated in tests/verify_ref.py).
 * Inputs per set: kpts0 [n0][2], kpts1 [n1][2] float32; matches0 [n0] int64, or NULL = the identity pairing i <-> i (needs n0 == n1).
 *   The K correspondences are the rows with -1 < matches0[i] < n1, in ascending i.  Optionally h_ref / height / width (has_ref != 0) for
 *   the corner-error column.
 * Stage 1 (exactly stage 1 of gims_eval_pairs above, float64): hypotheses h = 0 .. iters-1 from the same sampler, the exact 4-point
 *   model (h22 = 1), score = #correspondences with forward reprojection error^2 <= thresh^2; a hypothesis without a finite model
 *   scores -1; best = highest score, lowest h among equals.
 * Stage 2, lo_iters == 0: the single unguarded least-squares refit of gims_eval_pairs on the inliers of the best hypothesis (raw
 *   coordinates) and the final mask under it -- the same inputs give the same model as there.
 * Stage 2, lo_iters >= 1 (local optimisation, float64): H_0 = the best 4-point model, I_0 its inliers.  For l = 1 .. lo_iters:
 *     stop if |I_{l-1}| < 4;
 *     T0, T1 = similarity normalisations of the two point sets of I_{l-1}: centroid to the origin, scale sqrt(2) / (mean distance to the
 *       centroid), scale 1 if that mean is 0;
 *     Hn = solution of the 8 x 8 normal equations (h22 = 1) over the normalised inliers, by the same elimination; stop if it fails or is
 *       not finite;
 *     H' = T1^-1 Hn T0, divided by H'[8]; stop if H'[8] is 0 or anything is not finite;
 *     I' = inliers of H';  if |I'| < |I_{l-1}|: stop and keep H_{l-1};  otherwise accept (H_l, I_l) = (H', I') and stop if I' == I_{l-1}.
 *   The inlier count never decreases; lo_iters is a cap (the default 8 is not a tuned value).
 * Outputs per set: homography [9] float32 row-major, inlier [n0] uint8 (0 on rows without a correspondence), record float[8]
 *   (GIMS_VERIFY_* below).  K < 4, iters == 0 or no hypothesis with a model: ok = 0, err_corner = -1, n_valid = K, zeros elsewhere.
 * GIMS_EINVAL: n_sets > 65535 (the sets are the grid's y dimension), iters > 2^20, lo_iters > 1024, a negative or non-finite thresh, a
 *   workspace smaller than gims_verify_workspace_bytes (checked before anything is enqueued).  Asynchronous; no host synchronisation.
 *
 * The FUNDAMENTAL-MATRIX model (model == GIMS_VERIFY_MODEL_FUNDAMENTAL; selected per set, one call may mix both models) -- what a camera
 *   that moved through a 3-D scene needs, where a homography rejects correct matches off the dominant plane.  The reference keeps the
 *   two-view utilities for it (utils/common.py:392-476: estimate_pose, compute_epipolar_error) next to its drivers.  The estimator is
 *   again this build's own and parity with OpenCV is not claimed; its SPECIFICATION is this comment (restated in tests/fundamental_ref.py).
 *   Everything is float64.  F is row-major and x1^T F x0 = 0 for x0 = (x, y, 1) of image 0, x1 = (u, v, 1) of image 1.
 *   Correspondences: gathered exactly as above.  K < 8, iters == 0 or no hypothesis with a model: ok = 0 and zeros, as above.
 *   inlier(F, x, y, u, v): a = F x0 (3), g = the first two entries of F^T x1, e = x1 . a, den = a0^2 + a1^2 + g0^2 + g1^2;
 *     inlier iff den > 0 and e^2 <= thresh^2 * den (the squared Sampson distance e^2 / den <= thresh^2, without the division).
 *   similarity(points): c = (sum of the points, in order) / n, m = (sum of the distances to c, in order) / n, s = sqrt(2) / m, or 1 when
 *     m == 0; a point p is normalised to (p - c) * s.
 *   denormalise(Fn; c0, s0, c1, s1) = T1^T Fn T0: M[r] = (Fn[r][0] s0, Fn[r][1] s0, Fn[r][2] - s0 (Fn[r][0] c0x + Fn[r][1] c0y));
 *     F[0] = s1 M[0], F[1] = s1 M[1], F[2] = M[2] - s1 (c1x M[0] + c1y M[1]).
 *   unit(F) = F / sqrt(sum of the nine squares, in order); fails when that root is 0 or anything is not finite.
 *   Stage 1: hypothesis h takes EIGHT distinct indices from the sampler's stream above, state(seed, h), continued until eight distinct
 *     values (the first four are the homography's sample).  The eight points of each image are normalised by their similarity; row k of
 *     the 8 x 9 system is (u x, u y, u, v x, v y, v, x, y, 1) of the normalised pair k.  Null vector by Gauss-Jordan elimination with
 *     complete pivoting: eight times, the pivot is the entry of largest magnitude among the rows and columns that held no pivot yet
 *     (scanned by rows, then columns; a later entry replaces an earlier one only when strictly larger), no model when that magnitude is 0
 *     or not finite; every OTHER row r (used or not) becomes row r - (A[r][pc] / pivot) * row p over all nine columns.  The column left
 *     over is the free variable: f[free] = 1, f[pc] = -A[p][free] / A[p][pc] for the eight pivots; no named entry of F is fixed.
 *     F_h = unit(denormalise(f)); no model (score -1) when anything is not finite.  No rank enforcement here.  score = #inliers of F_h;
 *     best = highest score, lowest h among equals.
 *   jacobi(S, n x n symmetric) -> the eigenvector of the smallest eigenvalue: V = I; 12 sweeps over p = 0 .. n-2, q = p+1 .. n-1; a
 *     rotation is skipped when S[p][q] is exactly 0; d = S[q][q] - S[p][p], b = 2 S[p][q], t = (d >= 0 ? b : -b) / (|d| + hypot(d, b))
 *     (no quotient that can overflow), c = 1 / sqrt(t^2 + 1), s = t c; for every k: (S[k][p], S[k][q]) <- (c S[k][p] - s S[k][q],
 *     s S[k][p] + c S[k][q]); then the rows p and q likewise; S[p][q] = S[q][p] = 0; the columns p and q of V as those of S.  The
 *     eigenvector is the column of V at the smallest diagonal entry (the first such).
 *   rank2(F): v = jacobi(F^T F); F' = unit(F - (F v) v^T); F itself when that fails.
 *   Stage 2, lo_iters == 0: the model is rank2(F_best) and the mask is taken under it.  (So every returned model has rank 2.)
 *   Stage 2, lo_iters >= 1: F_0 = F_best (as scored, not rank 2), I_0 its inliers.  For l = 1 .. lo_iters:
 *     stop if |I_{l-1}| < 8;  the two similarities of the point sets of I_{l-1};  S = the 9 x 9 matrix of the 45 sums a_i a_j over the
 *     normalised inliers, a = the row above;  Fn = jacobi(S);  F' = rank2(denormalise(Fn)) after unit(); stop if anything fails or is not
 *     finite;  I' = inliers of F';  if |I'| < |I_{l-1}|: stop and keep F_{l-1};  otherwise accept (F_l, I_l) = (F', I') and stop if
 *     I' == I_{l-1}.  When no round was accepted, the model and the mask are those of lo_iters == 0.
 *   Outputs: homography [9] receives F in float32, unit Frobenius norm, negated when its entry of largest magnitude (the first such) is
 *     negative; GIMS_VERIFY_ERR_CORNER is always -1.  has_ref != 0 with this model, or a model other than the two below, is GIMS_EINVAL
 *     (checked before anything is enqueued).  A set with model == GIMS_VERIFY_MODEL_HOMOGRAPHY computes exactly what it did before the
 *     field had a meaning.
 *
 * The calibrated RELATIVE-POSE model (model == GIMS_VERIFY_MODEL_POSE = 3; selected per set, one call may mix all three models) -- what
 *   the reference's estimate_pose (utils/common.py:392-416: cv2.findEssentialMat + cv2.recoverPose) gives a caller with calibrated
 *   cameras: an essential matrix E, the pose (R, t) with x1 ~ R x0 + t, and the inliers.  The value 2 stays refused: it was kept for an
 *   essential matrix derived from the 8-point F, and that is no estimator -- on a planar or plane-dominated scene (this project's own
 *   data) the 8-point system loses rank and its E is arbitrary, while five points determine E there.  So the model is a FIVE-POINT
 *   estimator of this build's own; parity with OpenCV is not claimed; its SPECIFICATION is this comment (restated in tests/pose_ref.py).
 *   Everything is float64 (the intrinsics and the coordinates are read as float32 and widened).
 *   Inputs: h_ref[0..7] = fx0, fy0, cx0, cy0, fx1, fy1, cx1, cy1, h_ref[8] = 0, has_ref = 0.  A focal length or centre that is not finite,
 *     a focal length <= 0, has_ref != 0, h_ref[8] != 0 or n0 >= 2^27 is GIMS_EINVAL before anything is enqueued.  Correspondences:
 *     gathered exactly as above, then normalised to camera coordinates x = (x - cx0) / fx0, y = (y - cy0) / fy0, u = (u - cx1) / fx1,
 *     v = (v - cy1) / fy1.  E is row-major and x1^T E x0 = 0 for x0 = (x, y, 1), x1 = (u, v, 1).
 *   Threshold: thresh is in pixels; the model uses tn = thresh / f_mean with the reference's own f_mean = (fx0 + fy1) / 2
 *     (utils/common.py:396) and the inlier test inlier(E, x, y, u, v) of the fundamental model with tn in the place of thresh.
 *   Stage 1: hypothesis h takes FIVE distinct indices from the sampler's stream (the first four are the homography's sample).  Row k of
 *     the 5 x 9 system is (u x, u y, u, v x, v y, v, x, y, 1).  Gauss-Jordan elimination with complete pivoting exactly as for F, five
 *     pivots; the four columns left over, ascending, are the free columns c_0 .. c_3.  Basis vector j has b_j[c_j] = 1, b_j[c_i] = 0 for
 *     the other free columns and b_j[pc] = -A[p][c_j] / A[p][pc] for the five pivots; X, Y, Z, W = b_0 .. b_3 and E = x X + y Y + z Z + W,
 *     so every entry of E is a linear form in (x, y, z, 1).  No model when a pivot is 0 or anything is not finite.
 *     The ten cubic constraints, in this order: det E = E00 (E11 E22 - E12 E21) - E01 (E10 E22 - E12 E20) + E02 (E10 E21 - E11 E20), then
 *     the nine entries of 2 (E E^T) E - tr(E E^T) E by rows; each is built by products of the linear forms (linear x linear -> the ten
 *     quadratic monomials, quadratic x linear -> the twenty cubic ones).  Their coefficients form a 10 x 20 matrix whose columns are
 *       x^3 y^3 x^2y xy^2 | x^2z x^2 | y^2z y^2 | xyz xy | xz^2 xz x | yz^2 yz y | z^3 z^2 z 1      (columns 0 .. 19).
 *     Gauss-Jordan over the columns 0 .. 9 in this order: the pivot of column c is the entry of largest magnitude of that column among
 *     the rows that held no pivot yet (the first such), the elimination fails when it is 0 or not finite; every OTHER row r becomes
 *     row r - (A[r][c] / pivot) * row p over all twenty columns.
 *     The hidden variable is PIVOTED: matrix and elimination are formed for the three orders (X, Y, Z) = (b_0, b_1, b_2), (b_0, b_2, b_1),
 *     (b_2, b_1, b_0) of the basis (W = b_3 always); the quality of an order is the smallest of its ten pivot magnitudes, -1 when its
 *     elimination fails; the order of largest quality (the first such) is the one used from here on, no model when all three fail.
 *     (With a fixed order, samples with four or five points on one plane lose the planted E by 1e-4 to 1e-2.)  With a, b = the rows of the pivots of the columns (4, 5), (6, 7), (8, 9),
 *     each divided by its pivot, a - z b has no quadratic term in (x, y): it is x p(z) + y q(z) + r(z) with (ascending powers of z)
 *       p = (a12, a11 - b12, a10 - b11, -b10), q = (a15, a14 - b15, a13 - b14, -b13), r = (a19, a18 - b19, a17 - b18, a16 - b17, -b16).
 *     The three rows form a 3 x 3 matrix B(z) of polynomials with B(z) (x, y, 1)^T = 0; its determinant, expanded along the first row, is
 *     the polynomial c_0 + c_1 z + .. + c_10 z^10.  No model when c_10 is 0 or a coefficient is not finite.
 *     Real roots: bound = 1 + max_i |c_i / c_10|.  For d = 1 .. 10, q_d = the (10 - d)-th derivative of the polynomial (coefficient i is
 *     c_{i+10-d} (i + 10 - d)! / i!); its roots are sought in the intervals between -bound, the roots of q_{d-1} (ascending) and bound:
 *     an interval [a, b] holds a root iff (q_d(a) > 0) != (q_d(b) > 0); then 80 times m = (a + b) / 2 replaces the end at which
 *     (q_d > 0) is what it is at m, and the root is the last (a + b) / 2.  Polynomials are evaluated by Horner's rule.  The roots of q_10
 *     are the real roots of the polynomial, ascending, at most ten.  (A root of even multiplicity is not found.)
 *     Each root z gives one model: of the cross products of the row pairs (0, 1), (0, 2), (1, 2) of B(z) the one whose third component
 *     is largest in magnitude (the first such) is n; x = n0 / n2, y = n1 / n2; E = unit(x X + y Y + z Z + W); the root gives no model
 *     when n2 is 0 or unit() fails.  The models of a hypothesis are numbered 0, 1, .. in ascending root order.
 *     score(h) = the largest number of inliers of one of its models, the lowest model among equals; -1 without a model.  best = highest
 *     score, lowest h among equals.  K < 5, iters == 0 or no hypothesis with a model: ok = 0 and zeros, as above.
 *   ess(E), the projection onto the essential manifold: (d, V) = the diagonal and the eigenvector matrix of jacobi(E^T E); v3 = the
 *     column of V at the smallest d (the first such), v1, v2 = the two other columns in ascending index; w_i = E v_i, s_i = |w_i|;
 *     E' = unit(w1 v1^T / s1 + w2 v2^T / s2) (singular values 1, 1, 0 up to the unit norm); E itself when s1 or s2 is 0 or unit() fails.
 *   Stage 2, lo_iters == 0: the model is ess(E_best) and the mask is taken under it.
 *   Stage 2, lo_iters >= 1: the guarded local optimisation of the fundamental model on camera coordinates -- the similarities of the
 *     inliers, the 45 sums, jacobi(S), denormalise, unit -- with ess() in the place of rank2(), the stop at fewer than 8 inliers and the
 *     same acceptance: a round is accepted only while the inlier count does not fall.  When no round was accepted the model and the
 *     mask are those of lo_iters == 0.  On plane-dominated inliers the linear 9 x 9 refit is degenerate like the 8-point system; the
 *     guard is what keeps the five-point model there (the refit's candidate loses inliers and is dropped).
 *   Stage 3, the pose of the returned E (after the sign rule below): v1, v2, v3, w1, w2, s1, s2 as in ess(E); u1 = w1 / s1, u2 = w2 / s2,
 *     u3 = u1 x u2 divided by its length; v3 is negated when (v1 x v2) . v3 < 0.  Ra = u2 v1^T - u1 v2^T + u3 v3^T and
 *     Rb = u1 v2^T - u2 v1^T + u3 v3^T (U W V^T and U W^T V^T for W = [0 -1 0; 1 0 0; 0 0 1]: det = +1); the four candidates are, in this
 *     order, (Ra, u3), (Ra, -u3), (Rb, u3), (Rb, -u3).  No pose (R, t and n_front are 0) when s1 or s2 or |u1 x u2| is 0.
 *     Triangulation of an inlier under (R, t): a = R x0; the least-squares depths of l1 x1 = l0 a + t have the numerators
 *     n0 = (x1.a)(x1.t) - (x1.x1)(a.t), n1 = (x1.t)(a.a) - (x1.a)(a.t) over D = (x1.x1)(a.a) - (x1.a)^2; the inlier votes for the
 *     candidate iff D > 0, n0 > 0 and n1 > 0 (for -t both numerators change sign).  The pose is the candidate with the most votes, the
 *     lowest index among equals; n_front is its number of votes.
 *   Outputs: the `homography` pointer of a pose set receives 24 floats: E[9] (unit Frobenius norm, negated when its entry of largest
 *     magnitude, the first such, is negative), R[9] row-major, t[3] (unit norm), n_front, the index of the best model among the models
 *     of the best hypothesis, 0.  The record keeps its seven columns; GIMS_VERIFY_ERR_CORNER is always -1.  A set with another model
 *     computes exactly the bytes it computed before this model existed.
 */
#define GIMS_VERIFY_MODEL_HOMOGRAPHY 0
#define GIMS_VERIFY_MODEL_FUNDAMENTAL 1
#define GIMS_VERIFY_MODEL_POSE 3
typedef struct gims_verify_set {
  const float* kpts0; const float* kpts1;   /* [n0][2], [n1][2] */
  const int64_t* matches0;                  /* [n0], or NULL: identity pairing */
  int32_t n0, n1, height, width;            /* image 0 size for the corner error (read with has_ref only) */
  int32_t has_ref, model;                   /* model: GIMS_VERIFY_MODEL_* */
  float h_ref[9];                           /* reference homography, row-major (read with has_ref only); model 3: the intrinsics */
  uint8_t* inlier; float* record; float* homography;     /* homography: 9 floats; model 3: 24 floats */
} gims_verify_set;
#define GIMS_VERIFY_NVALID 0            /* K */
#define GIMS_VERIFY_OK 1
#define GIMS_VERIFY_NINLIERS 2          /* under the returned model: the reference's `correct_matches` */
#define GIMS_VERIFY_BEST_HYP 3
#define GIMS_VERIFY_BEST_HYP_INLIERS 4  /* the score of the best hypothesis = |I_0| */
#define GIMS_VERIFY_LO_ROUNDS 5         /* accepted rounds of the local optimisation */
#define GIMS_VERIFY_ERR_CORNER 6        /* mean corner distance to h_ref (as GIMS_EVAL_ERR_RANSAC), -1 without h_ref or model */
size_t gims_verify_workspace_bytes(const gims_verify_set* h_sets, int32_t n_sets, int32_t iters);
int gims_verify_pairs(const gims_verify_set* h_sets /* HOST array */, int32_t n_sets, float thresh, int32_t iters, int32_t lo_iters,
                      uint64_t seed, void* work, size_t work_bytes, void* stream);

/* Rebuild the full (n+1)x(m+1) OT matrix Z + u + v - norm (gmatcher.py:47,68) -- for forward_train and tests. */
int gims_ot_matrix(const float* scores, int64_t ld, int32_t n, int32_t m, float alpha, const float* uv,
                   float* out /* [(n+1)][(m+1)] */, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training loss of GMatcher.forward_train, forward value (gmatcher.py:333-386), from the solved potentials of
 * gims_sinkhorn_match -- the OT matrix is not materialised.  Per batch element b: scores / ld / n / m / uv as in
 * gims_ot_problem, kept0 / kept1 = the sorted ORIGINAL ids of the keypoints the adaptive graph kept (data['kept_kpts*_indices']).
 * gt: [n_gt][3] int64 rows (b, i0, i1) in ORIGINAL keypoint ids, -1 = no partner (train.py:113-125).  A row is remapped
 * through the kept lists (gmatcher.py:340-367); rows with a -1 or a dropped keypoint become (b, -1, -1), which the
 * reference's tensor indexing reads as the corner cell OT[N, M] (gmatcher.py:372), and count as negatives.  Each gathered
 * log-score is clamped to [-100, 0] and negated; positives and negatives are averaged per batch element (scatter_mean,
 * empty groups give 0), then over the batch, and weighted: out3 = {loss, pos_weight * pos, neg_weight * neg}.
 * loss_vec [n_gt] f32 and tag [n_gt + 2 * n_pairs] int32 are scratch (loss_vec holds the per-row losses afterwards, tag the row
 * classes followed by the per-(batch element, sign) group sizes: gims_train_loss_grad reads both).  Deterministic. */
typedef struct gims_loss_pair {
  const float* scores; int64_t ld; int32_t n, m; const float* uv; const int32_t* kept0; const int32_t* kept1;
} gims_loss_pair;
int gims_train_loss(const gims_loss_pair* dev_pairs /* DEVICE array */, int32_t n_pairs, const int64_t* gt, int32_t n_gt, float alpha,
                    float pos_weight, float neg_weight, float* loss_vec, int32_t* tag, float* out3, void* stream);

/* Backward of that loss through the Sinkhorn iterations (first differentiable kernel): d loss / d scores and
 * d loss / d bin_score, by reverse mode through the UNROLLED iterations of log_sinkhorn_iterations (gmatcher.py:41-47) -- what
 * autograd does in the reference.
 *   gims_sinkhorn_history: a forward solve with the streamed kernels that records the potentials after every iteration:
 *     h_hist[p] (HOST array of device pointers) receives (iters + 1) slots of n + m + 2 floats (u [n+1] then v [m+1]); slot 0 is
 *     unused (u_0 = v_0 = 0), slot k holds u_k, v_k.  problems[p].uv ends with the final potentials as in gims_sinkhorn_match.
 *   gims_train_loss_grad: scatters G = d loss / d out (out = Zc + u + v - norm at the gathered cells; zero where the clamp was
 *     active, gmatcher.py:374) into ZEROED per-problem buffers dz[p] [(n+1)][(m+1)]; `tag` is gims_train_loss's scratch output.
 *   gims_sinkhorn_backward: dz[p] holds G on entry and d loss / d Zc on exit (rows 0..n-1, columns 0..m-1 = d loss / d scores,
 *     pitch m + 1); dalpha[p] = the sum over the dustbin border = that problem's share of d loss / d bin_score. */
size_t gims_sinkhorn_history_floats(int32_t n, int32_t m, int32_t iters);
int gims_sinkhorn_history(const gims_ot_problem* h_problems, int32_t n_problems, float alpha, int32_t iters, float* const* h_hist /* HOST array */,
                          void* work /* gims_sinkhorn_workspace_bytes */, size_t work_bytes, void* stream);
size_t gims_sinkhorn_backward_workspace_bytes(const gims_ot_problem* h_problems, int32_t n_problems);
int gims_sinkhorn_backward(const gims_ot_problem* h_problems, int32_t n_problems, float alpha, int32_t iters, const float* const* h_hist /* HOST array */,
                           float* const* h_dz /* HOST array */, float* dalpha /* device [n_problems] */, void* work, size_t work_bytes, void* stream);
int gims_train_loss_grad(const gims_loss_pair* dev_pairs, int32_t n_pairs, const int64_t* gt, int32_t n_gt, float alpha, const int32_t* tag,
                         float pos_weight, float neg_weight, float* const* dev_dz_ptrs /* DEVICE array */, void* stream);

/* ------------------------------------------------------------------------------------------------
 * CAR-HyNet patch descriptor: carhynet/models.py:311-399 in five entry points.  Every block runs as one workgroup per
 * patch with the patch's activation resident in LDS; between blocks an activation is either NHWC f32 ([patch][y][x][channel]) or SPL32
 * split-bf16 pixel rows (the operand layout of the next convolution).  BatchNorm (eval) is folded into weights / biases by the caller.
 *   gims_ch_conv_block_first: layer 1     -- FRN(3) + TLU(3), 3x3 convolution 3 -> 32, FRN + CoordAtt + TLU         (models.py:315-322)
 *   gims_ch_conv_block:       layers 2..6 -- 3x3 convolution (stride 1 | 2), FRN (+ CoordAtt) + TLU                 (324-355)
 *   gims_ch_sandglass:        x + SandGlass(x) behind layers 2 and 4                                                (182-235, 383-389)
 *   (layer 7, the 8x8 convolution, is gims_linear (split-bf16x3) on the flattened [patch][8*8*128] SPL32 rows of layer 6)
 *   gims_ch_l2norm:           y = x / sqrt(sum_c x^2 + eps) per row                                                 (desc_l2norm, 9-21)
 */
/* x + SandGlass(x) (models.py:182-235 with the outer residual of 383-389: 2x + conv stack) for 32x32x32 or 16x16x64 activations,
 * one workgroup per patch with the activation resident in LDS; w: HOST array of 14 device pointers (BatchNorm folded):
 * dw0 [9][c], dw0 bias [c], CoordAtt w1 [8][c], b1 [8], wh [c][8], bh [c], ww [c][8], bw [c], pw0 [16][c], pw0 bias [16],
 * pw1 [c][16], pw1 bias [c], dw1 [9][c], dw1 bias [c].  Output: SPL32 split-bf16 pixel rows. */
int gims_ch_sandglass(const float* x, int64_t patches, int32_t hw, int32_t c, const float* const* w, uint16_t* out_split, int64_t ld_split, void* stream);
/* 3x3 convolution (pad 1, stride 1 | 2) + bias + FRN (+ CoordAtt) + TLU of one CAR-HyNet layer in ONE kernel, one workgroup per patch
 * (models.py:325-360: layer2 .. layer6).  x_split: the layer's input as SPL32 split-bf16 pixel rows [patches * hin * hin][pitch ldx >= 2 cin];
 * it is read once into LDS (zero border) and the convolution runs there as an implicit GEMM on the matrix cores (split-bf16x3: hi*hi +
 * hi*lo + lo*hi, like gims_linear); the raw output never leaves the chip:  y = max((x s + b) a_w a_h, tau)  with the FRN scale
 * s = frn_weight * rsqrt(mean x^2 + eps) per (patch, channel) and CoordAtt's gates a_h [y][c], a_w [x][c] (models.py:139-153: conv1 + h_swish
 * over the h + w pooled rows of the FRN output, then conv_h / conv_w + sigmoid) is applied to the accumulators, and the result leaves as f32
 * NHWC (y) and / or SPL32 pixel rows (y_split).  gate_w: HOST array of 6 device pointers w1 [8][c] (BatchNorm folded), b1 [8], wh [c][8],
 * bh [c], ww [c][8], bw [c]; NULL: no CoordAtt.
 * w_packed: the weights [cout][cin][3][3] in MFMA fragment order, bf16: [step = (ky*3+kx) * cin/16 + ks][nb = cout/32][plane hi|lo][lane 64][8]
 * with lane = lh*32 + li holding out channel nb*32 + li, input channels 16 ks + 8 lh + (0..7) of tap (ky, kx).
 * Geometries: (hin, cin, cout, stride) = (32,32,32,1), (32,32,64,2), (16,64,64,1), (16,64,128,2), (8,128,128,1). */
int gims_ch_conv_block(const uint16_t* x_split, int64_t ldx, int64_t patches, int32_t hin, int32_t cin, int32_t cout, int32_t stride,
                       const uint16_t* w_packed, const float* bias, const float* frn_weight, const float* frn_bias, float eps,
                       const float* const* gate_w, const float* tau, float* y, uint16_t* y_split, int64_t ld_split, void* stream);
/* The FIRST layer the same way (models.py:316-323): patches [n][32][32][3] f32 -> FRN(3) + TLU(3) -> 3x3 convolution 3 -> 32 (weights packed like
 * above with the input channels zero-padded to 16) -> FRN(32) + CoordAtt + TLU, one workgroup per patch, nothing but the patch read and the result
 * written; gate_w as above. */
int gims_ch_conv_block_first(const float* patches, int64_t n, const float* frn0_weight, const float* frn0_bias, float eps0, const float* tau0,
                             const uint16_t* w_packed, const float* bias, const float* frn_weight, const float* frn_bias, float eps,
                             const float* const* gate_w, const float* tau, float* y, uint16_t* y_split, int64_t ld_split, void* stream);
int gims_ch_l2norm(const float* x, int64_t rows, int32_t c, float eps, float* y, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Patch extraction: the front-end stage between keypoint detection and CAR-HyNet,
 *   buildGaussianPyramid(img, 6, graydesc=False)  (utils/library.py:234-271)
 *   ComputePatches(k, pyramid, radius_size=64)    (utils/library.py:84-110)
 *   cv2.resize(p, (32, 32), INTER_AREA) / 255.0   (utils/common.py:884)
 * on uint8 HWC images, in OpenCV's uint8 fixed-point arithmetic as restated in gims_amd/csrc/patches.hip (PARITY UNPINNED
 * against OpenCV itself, which is not available here; bit-identical to oracle/patch_oracle.py).
 * gims_pyramid_layout: number of levels (nOctaves * 6), per-level {byte offset, h, w} inside ONE buffer of *pyr_bytes, and
 *   the scratch bytes gims_pyramid_build needs.  h_levels may be NULL to query the sizes only.
 * gims_pyramid_build: img [h][w][c] uint8 (device) -> pyr (device).  Level o*6+i: octave o, layer i; level 0 is the 2x
 *   INTER_LINEAR_EXACT upsampling of img, layer 0 of octave o > 0 the INTER_NEAREST halving of level (o-1)*6+3, every other
 *   level the uint8 GaussianBlur of its predecessor.
 * gims_patch_extract: kp4 [n][4] f32 = (x, y, size, angle) and kp_octave [n] int32 = cv2.KeyPoint.octave (packed octave /
 *   layer, utils/library.py:16-35), all on the device.  out [n][32][32][3] f32 in [0, 1] (NHWC: the input layout of the
 *   CAR-HyNet kernels).  *bad_count (device int32) = keypoints whose octave / layer lie outside the pyramid (zero patches;
 *   the reference would raise IndexError).  c must be 3. */
typedef struct gims_pyr_level { int64_t offset; int32_t h, w; } gims_pyr_level;
int gims_pyramid_layout(int32_t h, int32_t w, int32_t c, gims_pyr_level* h_levels /* HOST, may be NULL */, int32_t capacity, int32_t* n_levels,
                        size_t* pyr_bytes, size_t* scratch_bytes);
int gims_pyramid_build(const uint8_t* img, int32_t h, int32_t w, int32_t c, uint8_t* pyr, void* scratch, void* stream);
int gims_patch_extract(const uint8_t* pyr, const gims_pyr_level* dev_levels, int32_t n_levels, const float* kp4, const int32_t* kp_octave,
                       int32_t n_kp, float* out, int32_t* bad_count, void* stream);
/* The per-keypoint arithmetic of gims_patch_extract on its own: A_out [n][6] f64 = the 2x3 map ComputePatches hands to
 * cv2.warpAffine (utils/library.py:96-106, row-major a00 a01 a02 a10 a11 a12), level_out [n] = the pyramid level it warps,
 * (octave - firstOctave) * 6 + layer (utils/library.py:100; unchecked).  The same device function as inside patch extraction;
 * it exists so that this arithmetic can be pinned against the reference's own (tests/golden/patch_affine_*.npz). */
int gims_patch_affine(const float* kp4, const int32_t* kp_octave, int32_t n_kp, double* A_out, int32_t* level_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training step (SURVEY 8f, row f3 = a25): GMatcher.forward(data, mode='train') on a module in train() mode followed by
 * loss.backward() (models/gmatcher.py:309-386 under train.py:100, 136-137).  gims_amd/trainstep.py composes the entry points
 * below (with gims_agc_build, gims_sage_mean, gims_sinkhorn_match, gims_train_loss, gims_sinkhorn_history,
 * gims_train_loss_grad and gims_sinkhorn_backward) into the forward and the reverse pass behind a torch.autograd.Function
 * whose inputs are the module's parameters; activations are row-major f32 [keypoint rows][channels].
 *
 * gims_gemm_f32: for z < batch   C_z = alpha * op(A_z) op(B_z)^T + beta * C_z (+ bias[n]) (+ residual_z), then act.
 *   op(A)(m, k) = ta ? A[k * lda + m] : A[m * lda + k];  op(B)(n, k) = tb ? B[k * ldb + n] : B[n * ldb + k].
 *   X_z = X + z * s{a,b,c,r} elements.  Arithmetic: f32 operands split on the fly into two (three) bf16 parts, three (six)
 *   bf16 MFMA passes per product, f32 accumulation (`precision`).  Replaces every torch matmul / conv1d(k=1) / einsum of the step and of
 *   its autograd: nn.Conv1d forward, grad_input, grad_weight (gmatcher.py:11-24, 99-125, 202-205), attention (35-39), the
 *   score einsum (273-275).  Any m, n, k >= 0; 16-byte aligned operands with pitches that are multiples of 4 take the
 *   vector path, anything else is read element by element.  `flags` and `splits` are set by the library. */
typedef struct gims_gemm {
  const float* a; const float* b; float* c;
  const float* bias;          /* [n] or NULL */
  const float* residual;      /* [m][ldr] or NULL */
  int64_t lda, ldb, ldc, ldr;
  int64_t sa, sb, sc, sr;
  int32_t m, n, k, batch;
  int32_t ta, tb;
  int32_t act;                /* GIMS_ACT_* */
  int32_t flags;
  float alpha, beta;
  float* work;                /* optional split-K workspace (device), work_floats floats: used when the output has too few tiles */
  int64_t work_floats;        /* to fill the chip and k >= 512; partial sums are added in a fixed order.  NULL: never split */
  int32_t splits;             /* set by the library */
  int32_t precision;          /* GIMS_PREC_BF16X3 (16 mantissa bits per operand) or GIMS_PREC_BF16X6 (24 bits: the f32 class) */
} gims_gemm;
int gims_gemm_f32(const gims_gemm* g, void* stream);

/* Row segments of a batch: one segment per call of the module in the reference (all image-0 rows, all image-1 rows). */
typedef struct gims_segments { int32_t n; int32_t off[8]; int32_t rows[8]; } gims_segments;
/* nn.BatchNorm1d in train() mode after a Conv1d (gmatcher.py:17-22), optionally with the ReLU that follows it:
 * statistics per (segment, channel) over the segment's rows, biased variance for the normalisation; running_mean /
 * running_var (may be NULL) are updated segment by segment with `momentum` and the unbiased variance, exactly the sequence
 * of updates the reference's two calls per layer make.  save [segments][c][2] = (mean, 1/sqrt(var + eps)) for the backward
 * pass; work: gims_batchnorm_workspace_floats floats.  Backward: dy is the gradient of the (post-ReLU) output; the ReLU mask
 * is recomputed from x; dgamma / dbeta are the sums over all segments. */
size_t gims_batchnorm_workspace_floats(const gims_segments* sg, int32_t c);
int gims_batchnorm_train_forward(const float* x, int64_t ld, int32_t c, const gims_segments* sg, const float* gamma, const float* beta, float eps,
                                 float momentum, float* running_mean, float* running_var, float* save, float* y, int64_t ldy, int32_t relu,
                                 float* work, void* stream);
int gims_batchnorm_train_backward(const float* x, int64_t ld, const float* dy, int64_t ldd, int32_t c, const gims_segments* sg, const float* save,
                                  const float* gamma, const float* beta, int32_t relu, float* dx, int64_t ldx, float* dgamma, float* dbeta,
                                  float* work, void* stream);
/* Reverse pass of gims_layernorm_act (the reference's LayerNorm, gmatcher.py:74-85, + ReLU): dy = gradient of the (post-ReLU) output, the
 * mask is recomputed from x.  dx [rows][ldo]; g_bias / g_scale [rows][c] receive the masked dy and dy * xhat, whose column sums
 * (gims_colsum) are the gradients of b_2 and a_2. */
int gims_layernorm_backward(const float* x, int64_t ldx, const float* dy, int64_t ldd, int64_t rows, int32_t c, const float* a2, const float* b2,
                            float eps, int32_t relu, float* dx, int64_t ldo, float* g_bias, float* g_scale, void* stream);
/* Attention of the training step for all images and heads of one GNN layer, without the probability matrices (gmatcher.py:35-39 inside
 * forward_train, :309-386; replaces, per image: the scores product, gims_softmax_rows and the product with V, and in the reverse pass four products
 * and gims_softmax_rows_backward).  qkv [rows][ld]: the packed projections Q | K | V (each d = 64 * heads columns, head h in columns 64 h ..
 * 64 h + 63 of its third: gims_head_pack's layout).  problems: a HOST array; problem i attends the query rows [q_off, q_off + nq) to the source
 * rows [k_off, k_off + nk) (self: the same image, cross: the other one).
 * forward: o [rows][ldo] = softmax(scale * Q K^T) V and lse [heads][rows] = max + log(sum) of every score row (what the reverse pass needs
 * instead of P).  backward: d_qkv [rows][lddq] from d_o, o, lse (every row must be a query row of exactly one problem and a source row of exactly
 * one for d_qkv to be written completely).  The forward is exact f32 on the matrix cores (v_mfma_f32_32x32x2_f32); the reverse pass -- linear in
 * its operands -- as reverse_precision says.  Fixed summation orders.  work:
 * gims_train_attention_workspace_floats(rows, heads) floats, 16-byte aligned. */
typedef struct gims_train_attn_problem {
  int32_t q_off, nq, k_off, nk;
} gims_train_attn_problem;
typedef struct gims_train_attn_args {
  const float* qkv;
  int64_t ld, rows;
  int32_t d, heads;
  float scale;                               /* 1 / sqrt(64) */
  int32_t n_problems;
  const gims_train_attn_problem* problems;   /* host memory */
  float* o;
  int64_t ldo;
  float* lse;
  const float* d_o;                          /* backward only */
  int64_t lddo;
  float* d_qkv;                              /* backward only */
  int64_t lddq;
  float* work;
  size_t work_floats;
  int32_t reverse_precision;                 /* backward only: GIMS_TRAIN_ATTN_REVERSE_* */
} gims_train_attn_args;
#define GIMS_TRAIN_ATTN_REVERSE_F32 0     /* exact f32 products (v_mfma_f32_32x32x2_f32), like the forward */
#define GIMS_TRAIN_ATTN_REVERSE_BF16X3 1  /* operands split into two bf16 parts, three passes (v_mfma_f32_32x32x16_bf16): 16-bit-mantissa products */
size_t gims_train_attention_workspace_floats(int64_t rows, int32_t heads);
int gims_train_attention_forward(const gims_train_attn_args* args, void* stream);
int gims_train_attention_backward(const gims_train_attn_args* args, void* stream);
/* softmax over the last dimension of `batch` matrices [rows][cols] (pitch ld, matrix stride `stride`), in place
 * (gmatcher.py:37), and its backward: dp <- prob * (dp - rowsum(dp * prob)), in place on dp. */
int gims_softmax_rows(float* s, int64_t ld, int64_t rows, int32_t cols, int32_t batch, int64_t stride, void* stream);
int gims_softmax_rows_backward(const float* prob, float* dp, int64_t ld, int64_t rows, int32_t cols, int32_t batch, int64_t stride, void* stream);
/* out[ch] = beta * out[ch] + sum over rows of x[row][ch] (bias gradients), fixed summation order.  work: zero-initialised
 * once by the caller (gims_colsum_workspace_floats floats), left zeroed where it must be. */
size_t gims_colsum_workspace_floats(int64_t rows, int32_t c);
int gims_colsum(const float* x, int64_t ld, int64_t rows, int32_t c, float beta, float* out, float* work, void* stream);
#define GIMS_EW_SCALE 0      /* out = alpha * a */
#define GIMS_EW_ADD 1        /* out = a + alpha * b */
#define GIMS_EW_RELU_MASK 2  /* out = b > 0 ? a : 0   (gradient of ReLU, b = the ReLU's output) */
#define GIMS_EW_RELU 3       /* out = max(a, 0) */
#define GIMS_EW_ACC 4        /* out += alpha * a */
int gims_elementwise(int32_t op, float* out, int64_t ldo, const float* a, int64_t lda, const float* b, int64_t ldb, int64_t rows, int32_t cols,
                     float alpha, void* stream);
/* dst[i0*d0 + i1*d1 + i2*d2] (= | +=) src[i0*s0 + i1*s1 + i2*s2] over [n0][n1][n2]: the reference's interleaved heads
 * (channel = d * heads + h, gmatcher.py:108-113) <-> contiguous heads, for weights on the way in and gradients on the way out. */
int gims_permute3(float* dst, const float* src, int32_t n0, int32_t n1, int32_t n2, int64_t d0, int64_t d1, int64_t d2, int64_t s0, int64_t s1,
                  int64_t s2, int32_t accumulate, void* stream);
/* Every head-interleave permutation of one attention layer in one launch.  proj_w / proj_b: HOST arrays of 3 device pointers (the q, k, v
 * projections in the reference's layout, [d][d] and [d]); merge_w [d][d].  to_params = 0: pack them into wqkv [3d][d], bqkv [3d] (rows grouped by
 * head) and wm [d][d] (columns grouped by head); to_params = 1: the reverse map (weight gradients back to the parameters' layout). */
int gims_head_pack(float* const* proj_w, float* const* proj_b, float* merge_w, float* wqkv, float* bqkv, float* wm, int32_t d, int32_t heads,
                   int32_t to_params, void* stream);
/* gradient of gims_sage_mean with respect to its input: out_j = sum over neighbours i of j of g_i / deg_i (symmetric CSR). */
int gims_sage_mean_transposed(const float* g, int64_t ldg, const int32_t* indptr, const int32_t* indices, int32_t n, int32_t c, float* out,
                              int64_t ldo, void* stream);
/* normalize_keypoints (gmatcher.py:26-33) as a tensor: out [n][2] = (kpts - norm3[seg][0..1]) / norm3[seg][2]. */
int gims_normalize_keypoints(const float* kpts, const float* norm3, const int32_t* seg_of_row, int64_t n, float* out, void* stream);

/* ---- optimizer step of the training loop (train.py:52-57 builds torch.optim.Adam over three parameter groups -- BatchNorm weights +
 * bin_score / other weights with weight decay / biases --, train.py:138 calls optimizer.step()) ----
 * One fused multi-tensor Adam step over HOST tables of device pointers (contiguous float32 tensors): ~count/80 launches for the
 * whole model instead of one list-kernel per operation and 64-tensor bucket.  Arithmetic = torch's _single_tensor_adam (amsgrad =
 * False, maximize = False), operation by operation in float32; the step-dependent scalars (lr / (1 - beta1^step), sqrt(1 - beta2^step))
 * are formed in double and rounded once.  `step` is the 1-based count AFTER this step's increment, per group (torch keeps it per
 * parameter; all parameters of a group that are stepped together share it).  Tensors with n = 0 are skipped. */
typedef struct gims_adam_tensor { float* param; const float* grad; float* exp_avg; float* exp_avg_sq; int64_t n; int32_t group; int32_t reserved; } gims_adam_tensor;
typedef struct gims_adam_group { double lr, beta1, beta2, eps, weight_decay; int64_t step; } gims_adam_group;
int gims_adam_step(const gims_adam_tensor* tensors, int32_t count, const gims_adam_group* groups, int32_t n_groups /* <= 8 */, void* stream);
/* The same for opt_type: sgd (train.py:55 builds optim.SGD(pg0, lr, momentum=0.9, nesterov=True)): torch's _single_tensor_sgd (maximize =
 * False) in float32, every `x + alpha * y` one fused multiply-add, the scalars (-lr, 1 - dampening) formed in double and rounded once.
 * first != 0: this tensor's momentum buffer holds nothing yet -- it is written (buf = g + wd * p), never read.  momentum_buffer may be
 * null only in a group whose momentum is 0.  Both calls check their arguments before any HIP call; count == 0 returns GIMS_OK. */
typedef struct gims_sgd_tensor { float* param; const float* grad; float* momentum_buffer; int64_t n; int32_t group; int32_t first; } gims_sgd_tensor;
typedef struct gims_sgd_group { double lr, momentum, dampening, weight_decay; int32_t nesterov; int32_t reserved; } gims_sgd_group;
int gims_sgd_step(const gims_sgd_tensor* tensors, int32_t count, const gims_sgd_group* groups, int32_t n_groups /* 1..8 */, void* stream);
/* ModelEMA.update (utils/common.py:1005-1015: `v *= d; v += (1 - d) * msd[k]` per floating state-dict entry) over a HOST table:
 * ema = fadd(fmul(ema, (float)decay), fmul((float)(1.0 - decay), model)), three separately rounded operations as torch's two statements
 * are; ~count/80 launches.  decay in [0, 1]; ema and model of one entry must be different tensors. */
typedef struct gims_ema_tensor { float* ema; const float* model; int64_t n; } gims_ema_tensor;
int gims_ema_update(const gims_ema_tensor* tensors, int32_t count, double decay, void* stream);

/* ---- SIFT keypoint detection (gims_amd/csrc/sift.hip): OpenCV 4.x SIFT_create(0, 3, 0.001, 80, 1.6).detect,
 * restated for uint8 BGR [n][h][w][3] or gray [n][h][w][1] images of one size, every image of a batch in the same launches.
 * gims_sift_layout (host only): octave sizes, float offsets of the Gaussian (6 per octave) and DoG (5) levels inside ONE image's
 *   pyramid of image_floats floats, the blur sigmas, kernel sizes and half kernels (kernel[i][j] = tap j from the centre).
 * gims_sift_pyramid: img -> pyr [n][image_floats] (scratch: [n][scratch_floats]); a test hook, gims_sift_detect runs it too.
 * gims_sift_detect: pyramid + extrema + refinement + orientation.  cand: int32 [cand_cap][4]; *counter (device) = the number of
 *   3x3x3 extrema, which may exceed cand_cap (then the caller grows the buffers and calls again).  Slots: cand_cap * GIMS_SIFT_SLOTS
 *   entries, SoA -- slot_f32 [5][S] (x, y, size, angle, response before the firstOctave rescale), slot_i32 [2][S] (packed octave,
 *   image; image = n_images marks an empty slot), slot_keys int64 [3][S]: stable-sort by key 0, then 1, then 2, then image to get
 *   removeDuplicatedSorted's order (x, y ascending, size descending, angle ascending, response descending, octave descending).
 * gims_sift_compact: with pos == NULL writes keep [n] (the first of each run of equal image / x / y / size / angle, in perm order);
 *   with pos = inclusive prefix sum of keep, writes the kept keypoints with the firstOctave = -1 rescale and counts[image] += 1. */
#define GIMS_SIFT_MAX_OCTAVES 16
#define GIMS_SIFT_MAX_RADIUS 16
#define GIMS_SIFT_SLOTS 18
typedef struct gims_sift_info {
  int32_t h, w, n_octaves, reserved;
  int64_t image_floats, scratch_floats;
  int32_t oct_h[GIMS_SIFT_MAX_OCTAVES], oct_w[GIMS_SIFT_MAX_OCTAVES];
  int64_t gauss_offset[GIMS_SIFT_MAX_OCTAVES], dog_offset[GIMS_SIFT_MAX_OCTAVES];
  double sigma[6];
  int32_t ksize[6];
  float kernel[6][GIMS_SIFT_MAX_RADIUS + 1];
} gims_sift_info;
int gims_sift_layout(int32_t h, int32_t w, gims_sift_info* info /* HOST */);
int gims_sift_pyramid(const uint8_t* img, int32_t n_images, int32_t h, int32_t w, int32_t c, float* pyr, float* scratch, void* stream);
int gims_sift_detect(const uint8_t* img, int32_t n_images, int32_t h, int32_t w, int32_t c, float* pyr, float* scratch, int32_t* cand,
                     int32_t cand_cap, int32_t* counter, float* slot_f32, int64_t* slot_keys, int32_t* slot_i32, void* stream);
int gims_sift_compact(const int64_t* perm, int64_t n, int32_t n_images, int32_t cand_cap, float* slot_f32, int64_t* slot_keys, int32_t* slot_i32,
                      int32_t* keep, const int64_t* pos, float* pt, float* size, float* angle, float* response, int32_t* octave, int32_t* counts,
                      void* stream);

/* ---- Training data from images (gims_amd/csrc/warp.hip, eval.hip): the reference's COCO_loader / train.py data path.
 * gims_warp_perspective: cv2.warpPerspective(src, M, (dw, dh)), INTER_LINEAR, BORDER_CONSTANT 0, for uint8 [n][sh][sw][c] -> [n][dh][dw][c],
 *   c = 1 or 3; m: HOST float64 [n][9] forward matrices (inverted here like cv::invert(M, DECOMP_LU): determinant / cofactor path; singular -> 0); work: device, >= 72 * n bytes, 16-aligned.
 * gims_resize: cv2.resize(src, (dw, dh), interpolation) for GIMS_INTER_LINEAR / GIMS_INTER_AREA, same layout (OpenCV's path choice:
 *   copy, area-fast, general area, linear with area-mode coefficients).
 * gims_train_labels: torch_find_matches(kpts0, kpts1, H, dist_thresh, n_iters) for n_pairs pairs and the match_indexes rows of
 *   train.py:118-125 -- rows int64 [sum(n0 + n1)][3] (capacity), filled from row 0 pair after pair: [k, i0, i1] (i1 ascending within an
 *   iteration, iteration after iteration), [k, miss0, -1], [k, -1, miss1]; *total (device int64) = the number of rows written.
 *   homographies: DEVICE float32 [n_pairs][9].  Keypoints: DEVICE float32 [n][2]. */
#define GIMS_INTER_LINEAR 1
#define GIMS_INTER_AREA 3
typedef struct gims_label_pair { const float* kpts0; const float* kpts1; int32_t n0, n1; } gims_label_pair;
int gims_warp_perspective(const uint8_t* src, int32_t n, int32_t sh, int32_t sw, int32_t c, const double* m /* HOST */, uint8_t* dst, int32_t dh,
                          int32_t dw, double* work, void* stream);
int gims_resize(const uint8_t* src, int32_t n, int32_t sh, int32_t sw, int32_t c, uint8_t* dst, int32_t dh, int32_t dw, int32_t interpolation,
                void* stream);
size_t gims_train_labels_workspace_bytes(const gims_label_pair* h_pairs /* HOST array */, int32_t n_pairs);
int gims_train_labels(const gims_label_pair* h_pairs /* HOST array */, int32_t n_pairs, const float* homographies, float dist_thresh,
                      int32_t n_iters, int64_t* rows, int64_t* total, void* work, size_t work_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Classical descriptor baselines (gims_amd/csrc/nn.hip): the nearest-neighbour distance ratio test and its
 * mutual-nearest variant, batched over pairs, nothing of size n0 x n1 stored.
 * replaces: calculate_nndr / calculate_mnn (eval_matches.py:13-67: torch.cdist + a full torch.sort of every row).
 * Semantics (fixed; tests/nn_ref.py restates them in NumPy):
 *   inputs   A [n0][d], B [n1][d] float32, finite, row pitches lda / ldb (elements, multiples of 4; pointers 16-byte aligned);
 *            d a multiple of 32 in [32, 512] (128 and 256 are the tested ones); 1 <= n0, 2 <= n1, both <= 32768 = gims_agc_max_keypoints;
 *            mutual != 0 also needs n0 >= 2 (the reference indexes a second neighbour of every row of B).
 *   distance d(i,j) = sqrt(S(i,j)),  S(i,j) = sum_k (double(a_ik) - double(b_jk))^2  in float64, in this fixed order: 64 partial sums,
 *            partial sum l takes k = l, l + 64, l + 128, ... ascending (square rounded, then added: no fused multiply-add); the 64
 *            partial sums are then combined by a butterfly: v_l <- v_l + v_(l xor 32), then xor 16, 8, 4, 2, 1.  This is the EXACT
 *            distance; every decision is taken on it.  Distances are ordered by S (the float64 square root is monotone in it).
 *   per row i of A: nn1[i], nn2[i] = the nearest and second-nearest row of B by exact distance, an exact tie goes to the LOWEST index;
 *            d1, d2 = those distances, sqrt in float64 then rounded to float32; ratio[i] = d1 / d2 in float32 (IEEE: 0/0 = NaN, which
 *            is no match); match[i] = ratio[i] < threshold (threshold as float32).
 *   mutual:  for each row j of B, cnn1[j] = its exact nearest row of A (lowest index on ties);  match[i] &= (cnn1[nn1[i]] == i).
 *   derived: matches0[i] = match ? nn1[i] : -1;  scores0[i] = match ? 1 - ratio[i] : 0;  mutual only: matches1[j] = the i matched to j, or -1.
 * How: an exact-f32 MFMA pass keeps, per row and per column slice, the 4 smallest approximate scores |b_j|^2 - 2 a_i.b_j in registers;
 * one wave per row re-evaluates the candidates exactly and CERTIFIES the row against an a-priori bound of the approximation error
 * (every column that is no candidate is then strictly farther than nn2); a row that cannot be certified is re-solved exactly against
 * all of B inside the same call.  Results are bit-identical whichever way a row went, and from run to run (no float atomics).
 * info[4] = {rows of A re-solved exhaustively, rows of B re-solved exhaustively (mutual only), 0, 0}.
 * debug (may be NULL; [n0][4] float32, test hook of the candidate pass): {eps_i (the bound, rounded up), max over ALL candidates of row i
 * of |approximate - exact score| (rounded up), the approximate score the candidate pass gave column nn1[i] (NaN if nn1[i] was no
 * candidate), T_i = the smallest of the per-list largest kept scores}; rows re-solved exhaustively included (their candidates are
 * still measured).  Not written under GIMS_NN_EXHAUSTIVE.
 * flags: GIMS_NN_EXHAUSTIVE sends every row through the exhaustive float64 path (tests, A/B runs).
 * `work`: scratch of gims_nn_workspace_bytes(pairs, n_pairs, flags) bytes, 256-byte aligned.  Asynchronous; no host synchronisation.
 */
typedef struct gims_nn_pair {
  const float* a; const float* b; int64_t lda, ldb;
  int32_t n0, n1, d, mutual;
  float threshold; int32_t reserved;
  int32_t* nn1; int32_t* nn2; float* d1; float* d2; float* ratio; uint8_t* match;   /* [n0] */
  int64_t* matches0; float* scores0;                                                /* [n0] */
  int32_t* cnn1; int64_t* matches1;                                                 /* [n1]; read only when mutual; cnn1 may be NULL */
  int32_t* info;                                                                    /* [4] */
  float* debug;                                                                     /* [n0][4] or NULL */
} gims_nn_pair;
#define GIMS_NN_EXHAUSTIVE 1
size_t gims_nn_workspace_bytes(const gims_nn_pair* h_pairs /* HOST array */, int32_t n_pairs, int32_t flags);   /* 0 on bad arguments */
int gims_nn_match(const gims_nn_pair* h_pairs /* HOST array */, int32_t n_pairs, int32_t flags, void* work, size_t work_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Colour augmentation of the training images (gims_amd/csrc/augment.hip): brightness / contrast, motion blur and
 * Gaussian noise for a batch of uint8 [n][h][w][c] images, c = 1 or 3, into a SEPARATE output of the same shape, one augmentation launch
 * for the batch (after the upload of the plans, below), every image under its own plan.
 * replaces: the albumentations Compose of utils/dataset.py:23-29 (RandomBrightness / RandomContrast, MotionBlur / GaussNoise).  This is
 * the build's OWN, fully specified restatement of the documented behaviour of those transforms (like the RANSAC above): neither
 * albumentations nor OpenCV is available to pin it to, and their random streams could not be reproduced anyway.  tests/aug_ref.py
 * restates the specification in NumPy; the device equals it bit for bit.
 * A plan has up to three parts, applied in this order:
 *   (a) LUT (use_lut != 0): p = lut[src].  Applied on the fly to every source pixel that (b) or (c) reads; alone, dst = lut[src].
 *   (b) motion blur (ksize 3, 5 or 7; 0: none): cv2.filter2D(img, -1, K) restated.  K = kernel[0 .. ksize*ksize), row-major.
 *       Correlation (K is not flipped), anchor at the centre r = ksize / 2:  out(y, x, ch) = sum over (i, j) of K[i][j] * p(Y(y + i - r),
 *       X(x + j - r), ch) with the border BORDER_REFLECT_101 by OpenCV's borderInterpolate loop: for len == 1 the index is 0, otherwise
 *       repeat { q = -q if q < 0;  q = 2 * (len - 1) - q if q >= len } until 0 <= q < len (an image narrower than r bounces several
 *       times).  Arithmetic per pixel and channel: acc = 0.f, then acc = fmaf(K[i][j], (float)p, acc) for every tap with K[i][j] != 0
 *       in row-major tap order (i outer, j inner); out = saturate_cast<uchar>(acc): round half to even, then clamp to [0, 255].
 *   (c) Gaussian noise (sigma > 0; <= 0: none): v = fmaf(sigma, z, (float)p);  out = (uint8)trunc(min(max(v, 0), 255)) -- truncation,
 *       what np.clip(...).astype(uint8) does.  Every channel of every pixel has its own z, from a counter-based generator (no state, the
 *       same result under any launch geometry): e = (y * w + x) * c + ch, the element's index inside its image;
 *         s0 = key ^ (e * 0x9E3779B97F4A7C15)  (uint64, wrapping);  s1 = splitmix64(s0), s2 = splitmix64(s1), s3 = splitmix64(s2) with
 *         splitmix64(x): x += 0x9E3779B97F4A7C15; x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9; x = (x ^ (x >> 27)) * 0x94D049BB133111EB;
 *         return x ^ (x >> 31)  (the function of the RANSAC sampler above, chained the same way);
 *         S = the sum of the twelve 16-bit lanes of s1, s2, s3 (0 .. 786420);  z = (float)(S - 393210) / 65536.f.
 *       Integer arithmetic and two exact float32 operations: z is the same on every machine.  Unit variance to 2e-10 (1 - 2^-32), excess
 *       kurtosis -0.1, support +-6.
 *   (b) and (c) never occur in one plan (the reference's OneOf picks one); a plan with none of the three copies the image.
 * plans: HOST array of n plans, copied into `work` on the stream through kernel arguments (like gims_label_pair / gims_eval_pair tables):
 *   one small upload launch per 8 plans ahead of the one augmentation launch.  A batch whose plans are all empty is one device copy.
 * work: device scratch of gims_color_aug_workspace_bytes(n) bytes, 16-byte aligned.  Asynchronous; no host synchronisation.
 * sigma: noise is on when sigma > 0; a NaN sigma therefore means no noise (the comparison is false), like any sigma <= 0.
 * GIMS_EINVAL: c not 1 or 3, ksize not in {0, 3, 5, 7}, blur and noise in one plan, sigma = +infinity, dst overlapping src (the blur reads
 * neighbours), h * w * c >= 2^31, n > 65535 (the batch is the grid's y dimension), a missing, misaligned or too small workspace.
 * n == 0 is GIMS_OK and touches nothing. */
typedef struct gims_aug_plan {
  uint8_t lut[256];
  float kernel[49];            /* ksize x ksize, row-major, in the first ksize * ksize entries */
  int32_t use_lut, ksize;      /* ksize 0: no blur */
  float sigma;                 /* <= 0: no noise */
  uint64_t key;                /* noise key of this image (offset 464; the struct is 472 bytes with no padding) */
} gims_aug_plan;
size_t gims_color_aug_workspace_bytes(int32_t n);
int gims_color_aug(const uint8_t* src, int32_t n, int32_t h, int32_t w, int32_t c, const gims_aug_plan* plans /* HOST array */, uint8_t* dst,
                   void* work, size_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GIMS_HIP_H */
