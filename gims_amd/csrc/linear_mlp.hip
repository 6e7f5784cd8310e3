// One layer's MLP in one launch (GIMS_OP_MLP of gims_run_ops, include/gims_hip.h):
//
//   out = residual + W1 relu(W0 [a0 | a1] + b0) + b1        (the last two `mlp` launches of a layer, gmatcher.py:141-142)
//
// on pre-split SPL32 operands, for the descriptor width D = 256 (k = hidden = 512, n = 256).  The 512-wide hidden activation never
// leaves the REGISTERS: both GEMMs run as D^T = W A^T (linear.hip), so the accumulators of the first hold hid^T with one row per lane
// column -- after bias, ReLU and the hi/lo split that is the B operand of the second GEMM's MFMAs, provided W1's K axis is stored in
// the order in which a lane holds its 16 accumulator values of a 32-channel block (position 16 s + 8 (lane >> 5) + j holds channel
// (r & 3) + 8 (r >> 2) + 4 (lane >> 5), r = 8 s + j: GMatcher._packed permutes W1 so).  attention8_bf16_kernel feeds P to its PV
// product the same way.
//
// Workgroup: 128 rows, 8 waves = 4 row blocks of 32 (rb) x 2 hidden groups (hg).
//   phase 1  hid^T = W0 [a0 | a1]^T in two halves of 256 hidden channels, each a full K = 512 loop over 48-KiB stages (A 16 KiB + W0 32 KiB);
//            wave (rb, hg) owns hidden channels half * 256 + hg * 128 + [0, 128) of its 32 rows: 64 accumulator registers per half, turned
//            into 32 + 32 packed hi / lo registers at the end of the half.  The K order and the order of the three products per K step are
//            those of linear_x3p_tile, and so is the arithmetic of bias, ReLU and split: the hidden values are bit for bit what the MLP0
//            launch writes.
//   phase 2  out^T = W1 hid^T in four slices of 64 output channels (32 accumulator registers next to the 128 B-fragment registers).  A
//            32-KiB stage carries two 32-channel hidden blocks of W1 for EACH hidden group, so all eight waves multiply in every stage;
//            the two waves of a row block add their partial sums through LDS, transposed as in linear_x3p_tile's epilogue, and each stores
//            half of the rows: bias, residual, f32 and SPL32 lines, whole 128-byte lines per row.  The stores of a slice are issued in
//            the first stage of the next one, its residual is fetched a stage ahead.
// Operands travel L2 -> LDS by LDS-DMA with the source-side swizzle of linear.hip; two stage slots, one workgroup barrier per stage.
#include "common.h"

namespace gims {
namespace {

constexpr int MF_D = 256, MF_K = 2 * MF_D, MF_HID = 2 * MF_D;      // the one shape served
constexpr int MF_TM = 128;                                         // rows per workgroup
constexpr int MF_A_TILE = MF_TM * 64;                              // bf16 elements: 128 rows x (32 hi | 32 lo)
constexpr int MF_P1_STAGE = MF_A_TILE + 256 * 64;                  // + 256 hidden rows of W0: 48 KiB
constexpr int MF_P2_SUB = 64 * 64;                                 // 64 output rows x one hidden block of W1
constexpr int MF_P2_STAGE = 4 * MF_P2_SUB;                         // [hidden group][block e][64 rows]: 32 KiB
constexpr int MF_EP_PITCH = 64 + 4;                                // floats per row of a wave's transpose slice
constexpr int MF_EP_OFF = 2 * MF_P2_STAGE * 2;                     // bytes: the slices sit behind the two phase-2 stage slots
constexpr int MF_BIAS_OFF = MF_EP_OFF + 8 * 32 * MF_EP_PITCH * 4;  // bytes: b0 | b1, 3n floats, staged once per workgroup
constexpr int MF_LDS_BYTES = MF_BIAS_OFF + (MF_HID + MF_D) * 4;
static_assert(MF_LDS_BYTES >= 2 * MF_P1_STAGE * 2 && MF_LDS_BYTES <= 160 * 1024, "both rings fit");

__device__ __forceinline__ void mf_wait_all() { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); }
__device__ __forceinline__ int mf_off(int row, int chunk) { return row * 64 + ((chunk ^ ((row >> 1) & 7)) << 3); }
__device__ __forceinline__ void mf_dma(const char* g, uint16_t* dst) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g, (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
}
__device__ __forceinline__ bf16x8 mf_pack8(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  const u32x4 v = {a, b, c, d};
  return __builtin_bit_cast(bf16x8, v);
}

}  // namespace

__global__ __launch_bounds__(512) void mlp_fused_x3_kernel(gims_linear_args p) {
  extern __shared__ __attribute__((aligned(16))) uint16_t smem[];
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int rb = wave >> 1, hg = wave & 1;
  const int li = lane & 31, lh = lane >> 5;
  const int m0 = (int)blockIdx.x * MF_TM;
  const int drow = lane >> 3, dpos = lane & 7;                     // LDS-DMA: a 1-KiB piece is 8 rows of 8 chunks

  // ---- DMA duties.  Phase 1: 48 pieces per stage [16 of A | 32 of W0]: every wave moves A pieces 2 w, 2 w + 1 and W0 pieces 4 w .. 4 w + 3;
  // phase 2: 32 pieces, four per wave.  A lane's chunk inside its row is swizzled at the source: piece parity flips bit 2 of the rotation.
  const uint32_t ch0 = 16u * (uint32_t)(dpos ^ (drow >> 1)), ch1 = ch0 ^ 64u;
  uint32_t voffa0[2], voffa1[2];                                  // rows of A clamped to the last valid one
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = 8 * (2 * wave + i) + drow, rmax = p.m - m0 - 1;
    const uint32_t rl = (uint32_t)(row < rmax ? row : rmax);
    voffa0[i] = rl * (uint32_t)p.lda0 * 2u + (i ? ch1 : ch0);
    voffa1[i] = rl * (uint32_t)p.lda1 * 2u + (i ? ch1 : ch0);
  }
  // W0 / W1 pieces: the wave's four pieces are rows 8 i + drow behind a wave-uniform base: 32-bit lane offsets like A's, `opaque` at the
  // point of use -- base + offset is loop-invariant up to the K term and would otherwise be kept as a 64-bit pointer per lane and piece
  auto opaque = [](uint32_t v) __attribute__((always_inline)) { asm volatile("" : "+v"(v)); return v; };
  uint32_t voffw[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) voffw[i] = (uint32_t)(8 * i + drow) * (uint32_t)p.ldw * 2u + ((i & 1) ? ch1 : ch0);
  auto issue1 = [&](int half, int kt) {
    const int k = kt * 32;
    const bool second = k >= MF_D;
    const int akk = second ? k - MF_D : k;
    const char* ab = (const char*)(second ? p.a1 : p.a0) + ((int64_t)m0 * (second ? p.lda1 : p.lda0) + 2 * akk) * 2;
    const char* wb = (const char*)p.w + ((int64_t)(half * 256 + 32 * wave) * p.ldw + 2 * k) * 2;
    uint16_t* dst = smem + (kt & 1) * MF_P1_STAGE;
#pragma unroll
    for (int i = 0; i < 2; ++i) mf_dma(ab + (second ? voffa1[i] : voffa0[i]), dst + (2 * wave + i) * 512);
#pragma unroll
    for (int i = 0; i < 4; ++i) mf_dma(wb + opaque(voffw[i]), dst + MF_A_TILE + (4 * wave + i) * 512);
  };
  auto issue2 = [&](int slice, int ts) {
    // this wave's four pieces lie in sub-tile u = wave >> 1 = (hidden group, block e): W1 rows slice * 64 + [0, 64), hidden block hb
    const int g = wave >> 2, q = 2 * ts + ((wave >> 1) & 1);
    const int hb = (q >> 2) * 8 + g * 4 + (q & 3);
    const int r0 = MF_HID + slice * 64 + 32 * (wave & 1);
    const char* wb = (const char*)p.w + ((int64_t)r0 * p.ldw + 64 * hb) * 2;
    uint16_t* dst = smem + (ts & 1) * MF_P2_STAGE + wave * 4 * 512;
#pragma unroll
    for (int i = 0; i < 4; ++i) mf_dma(wb + opaque(voffw[i]), dst + i * 512);
  };

  bf16x8 Bh[8][2], Bl[8][2];        // hid^T of this wave: [local hidden block q = half * 4 + j][K step] as MFMA B fragments

  // ------------------------------------------------------------------------------------------ phase 1
  const uint32_t frag0 = (uint32_t)(mf_off(li, lh) * 2);            // byte offset of (row li, chunk lh) in a tile of 128-byte rows
  issue1(0, 0);
  // both biases go through LDS (visible behind the first stage's barrier): the conversions below then wait for LDS, not for L2
  float* const bias_s = (float*)((char*)smem + MF_BIAS_OFF);
  if (t < (MF_HID + MF_D) / 4) *(float4*)(bias_s + 4 * t) = *(const float4*)(p.bias + 4 * t);
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    f32x16 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    for (int kt = 0; kt < 16; ++kt) {
      mf_wait_all();
      __builtin_amdgcn_s_barrier();
      if (kt + 1 < 16) issue1(half, kt + 1);
      else if (half == 0) issue1(1, 0);
      else issue2(0, 0);
      // fragment addresses: row * 128 bytes + swizzled chunk.  The chunk index is lh | 2 s | 4 lo, so every address of a row is ONE lane
      // base (chunk lh) XOR a constant; made opaque per stage, or the eight bases would be kept in registers across the loop
      const uint32_t fa = opaque(frag0) + (uint32_t)((kt & 1) * MF_P1_STAGE * 2 + rb * 32 * 128);
      const uint32_t fw = opaque(frag0) + (uint32_t)((kt & 1) * MF_P1_STAGE * 2 + MF_A_TILE * 2 + hg * 128 * 128);
      auto frag = [&](uint32_t base, int row32, int chunk) __attribute__((always_inline)) {
        return *(const bf16x8*)((const char*)smem + ((base ^ (uint32_t)(chunk << 4)) + (uint32_t)(row32 * 32 * 128)));
      };
      // Two groups of two hidden blocks, each: reads of K step 0 -> its lo*hi and hi*lo products -> reads of step 1 -> hi*hi of step 0 ->
      // step 1 (per accumulator the order of linear_x3p_tile).  Reads are pinned ahead of the MFMAs that consume them; a group at a
      // time keeps the fragments at 48 registers next to the 64 accumulators and the 64 fragment registers of the first half.
      bf16x8 ah[2], al[2];
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        bf16x8 wh[2][2], wl[2][2];
        auto rd = [&](int s) __attribute__((always_inline)) {
          if (g == 0) ah[s] = frag(fa, 0, 2 * s);
#pragma unroll
          for (int i = 0; i < 2; ++i) wl[s][i] = frag(fw, 2 * g + i, 4 + 2 * s);
          if (g == 0) al[s] = frag(fa, 0, 4 + 2 * s);
#pragma unroll
          for (int i = 0; i < 2; ++i) wh[s][i] = frag(fw, 2 * g + i, 2 * s);
        };
        auto lo_terms = [&](int s) __attribute__((always_inline)) {
#pragma unroll
          for (int i = 0; i < 2; ++i) acc[2 * g + i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl[s][i], ah[s], acc[2 * g + i], 0, 0, 0);
#pragma unroll
          for (int i = 0; i < 2; ++i) acc[2 * g + i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh[s][i], al[s], acc[2 * g + i], 0, 0, 0);
        };
        auto hi_term = [&](int s) __attribute__((always_inline)) {
#pragma unroll
          for (int i = 0; i < 2; ++i) acc[2 * g + i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh[s][i], ah[s], acc[2 * g + i], 0, 0, 0);
        };
        rd(0);
        __builtin_amdgcn_sched_barrier(0);
        lo_terms(0);
        __builtin_amdgcn_sched_barrier(0);
        rd(1);
        __builtin_amdgcn_sched_barrier(0);
        hi_term(0);
        lo_terms(1);
        hi_term(1);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // bias, ReLU, hi/lo split (the arithmetic of linear_x3p_tile's epilogue): the accumulators become B fragments
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float* bp = bias_s + (half * 8 + hg * 4 + j) * 32 + 4 * lh;
      float v[16];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 b = *(const float4*)(bp + 8 * g);
        v[4 * g] = fmaxf(acc[j][4 * g] + b.x, 0.f);
        v[4 * g + 1] = fmaxf(acc[j][4 * g + 1] + b.y, 0.f);
        v[4 * g + 2] = fmaxf(acc[j][4 * g + 2] + b.z, 0.f);
        v[4 * g + 3] = fmaxf(acc[j][4 * g + 3] + b.w, 0.f);
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        uint32_t h[4], l[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          h[e] = pack_bf2(v[8 * s + 2 * e], v[8 * s + 2 * e + 1]);
          l[e] = pack_bf2(v[8 * s + 2 * e] - __uint_as_float(h[e] << 16), v[8 * s + 2 * e + 1] - __uint_as_float(h[e] & 0xffff0000u));
        }
        Bh[half * 4 + j][s] = mf_pack8(h[0], h[1], h[2], h[3]);
        Bl[half * 4 + j][s] = mf_pack8(l[0], l[1], l[2], l[3]);
      }
      __builtin_amdgcn_sched_barrier(0);               // one block at a time: 16 accumulator registers become 16 fragment registers
    }
  }

  // ------------------------------------------------------------------------------------------ phase 2
  // (the lane index is passed through an empty asm so that nothing phase 2 derives from it is computed -- and kept -- ahead of phase 1)
  int lane2 = lane;
  asm volatile("" : "+v"(lane2));
  const int li2 = lane2 & 31, lh2 = lane2 >> 5;
  float* const ep_all = (float*)((char*)smem + MF_EP_OFF);
  float* const ep = ep_all + wave * (32 * MF_EP_PITCH);                        // this wave's partial sums, [32 rows][64 channels]
  const float* const ep0 = ep_all + (rb * 2) * (32 * MF_EP_PITCH);             // ... and those of the row block's two hidden groups
  const float* const ep1 = ep0 + 32 * MF_EP_PITCH;
  const int c8 = (lane2 & 7) * 8, rsub = lane2 >> 3;                             // read-back: 8 lanes per row, 8 rows per access
  float4 res[2][2];
  auto load_res = [&](int slice) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int row = m0 + rb * 32 + rsub + 8 * (2 * hg + q);
      const bool ok = p.residual && row < p.m;
#pragma unroll
      for (int h = 0; h < 2; ++h)
        res[q][h] = ok ? *(const float4*)(p.residual + (int64_t)row * p.ldc + slice * 64 + c8 + 4 * h) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto store_slice = [&](int slice) {
    const int col = slice * 64 + c8;
    const float4 b0 = *(const float4*)(bias_s + MF_HID + col), b1 = *(const float4*)(bias_s + MF_HID + col + 4);
    const int scol = spl_col(col);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int rl = rsub + 8 * (2 * hg + q), row = m0 + rb * 32 + rl;
      const float4 x0 = *(const float4*)(ep0 + rl * MF_EP_PITCH + c8), x1 = *(const float4*)(ep0 + rl * MF_EP_PITCH + c8 + 4);
      const float4 y0 = *(const float4*)(ep1 + rl * MF_EP_PITCH + c8), y1 = *(const float4*)(ep1 + rl * MF_EP_PITCH + c8 + 4);
      if (row >= p.m) continue;
      float v[8] = {(x0.x + y0.x) + b0.x, (x0.y + y0.y) + b0.y, (x0.z + y0.z) + b0.z, (x0.w + y0.w) + b0.w,
                    (x1.x + y1.x) + b1.x, (x1.y + y1.y) + b1.y, (x1.z + y1.z) + b1.z, (x1.w + y1.w) + b1.w};
      v[0] += res[q][0].x; v[1] += res[q][0].y; v[2] += res[q][0].z; v[3] += res[q][0].w;
      v[4] += res[q][1].x; v[5] += res[q][1].y; v[6] += res[q][1].z; v[7] += res[q][1].w;
      float* o = p.out_f32 + (int64_t)row * p.ldc + col;
      *(float4*)o = make_float4(v[0], v[1], v[2], v[3]);
      *(float4*)(o + 4) = make_float4(v[4], v[5], v[6], v[7]);
      uint32_t h[4], l[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        h[e] = pack_bf2(v[2 * e], v[2 * e + 1]);
        l[e] = pack_bf2(v[2 * e] - __uint_as_float(h[e] << 16), v[2 * e + 1] - __uint_as_float(h[e] & 0xffff0000u));
      }
      uint16_t* oh = p.out_hi + (int64_t)row * p.ld_split + scol;
      *(uint4*)oh = make_uint4(h[0], h[1], h[2], h[3]);
      *(uint4*)(oh + 32) = make_uint4(l[0], l[1], l[2], l[3]);
    }
  };

  for (int slice = 0; slice < 4; ++slice) {
    f32x16 acc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
#pragma unroll
    for (int ts = 0; ts < 4; ++ts) {
      mf_wait_all();                                   // own DMA pieces landed, own partial sums (previous slice) written
      __builtin_amdgcn_s_barrier();
      if (ts + 1 < 4) issue2(slice, ts + 1);
      else if (slice + 1 < 4) issue2(slice + 1, 0);
      if (ts == 0 && slice > 0) store_slice(slice - 1);
      if (ts == 3) load_res(slice);
      const uint16_t* st = smem + (ts & 1) * MF_P2_STAGE + (hg * 2) * MF_P2_SUB;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const uint16_t* sw = st + e * MF_P2_SUB;
        const int q = 2 * ts + e;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          bf16x8 wh[2], wl[2];
#pragma unroll
          for (int ob = 0; ob < 2; ++ob) {
            wl[ob] = *(const bf16x8*)(sw + mf_off(ob * 32 + li2, 4 + 2 * s + lh2));
            wh[ob] = *(const bf16x8*)(sw + mf_off(ob * 32 + li2, 2 * s + lh2));
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int ob = 0; ob < 2; ++ob) acc[ob] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl[ob], Bh[q][s], acc[ob], 0, 0, 0);
#pragma unroll
          for (int ob = 0; ob < 2; ++ob) acc[ob] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh[ob], Bl[q][s], acc[ob], 0, 0, 0);
#pragma unroll
          for (int ob = 0; ob < 2; ++ob) acc[ob] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh[ob], Bh[q][s], acc[ob], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // partial sums of this wave, transposed: lane (li, lh) holds channels 8 g + 4 lh + [0, 4) of row li per 32-channel block.  The slices
    // were last read in the first stage of this slice, three barriers ago.
#pragma unroll
    for (int ob = 0; ob < 2; ++ob)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *(float4*)(ep + li2 * MF_EP_PITCH + ob * 32 + 8 * g + 4 * lh2) = make_float4(acc[ob][4 * g], acc[ob][4 * g + 1], acc[ob][4 * g + 2], acc[ob][4 * g + 3]);
  }
  mf_wait_all();
  __builtin_amdgcn_s_barrier();
  store_slice(3);
}

// GIMS_OP_MLP of gims_run_ops: every check precedes the launch
int mlp_fused_launch(const gims_linear_args& a, hipStream_t s) {
  GIMS_CHECK_ARG(a.m > 0 && a.n == MF_D && a.k == MF_K && a.k0 == MF_D, "mlp_fused: serves n = %d, k = %d, k0 = %d (got m=%d n=%d k=%d k0=%d)", MF_D, MF_K, MF_D,
                 a.m, a.n, a.k, a.k0);
  GIMS_CHECK_ARG(a.a0 && a.a1 && a.w && a.bias && a.out_f32 && a.out_hi, "mlp_fused: null operand or output");
  GIMS_CHECK_ARG(a.a0_lo && a.a1_lo && a.w_lo && a.precision == GIMS_PREC_BF16X3, "mlp_fused: pre-split SPL32 operands, GIMS_PREC_BF16X3");
  GIMS_CHECK_ARG(a.act == GIMS_ACT_RELU && a.scale == 1.f && a.flags == 0 && !a.out_bf16 && !a.guard.stat && !a.range_stat && a.probe_delay == 0 &&
                 !a.residual_rows, "mlp_fused: act = GIMS_ACT_RELU, scale = 1, no flags, no out_bf16, no guard, no range_stat, no residual_rows");
  GIMS_CHECK_ARG((a.lda0 % 64) == 0 && (a.lda1 % 64) == 0 && (a.ldw % 64) == 0 && a.lda0 >= 2 * MF_D && a.lda1 >= 2 * MF_D && a.ldw >= 2 * MF_K,
                 "mlp_fused: SPL32 operands have row pitch >= 2*K, a multiple of 64 elements");
  GIMS_CHECK_ARG(a.lda0 < (1 << 22) && a.lda1 < (1 << 22) && a.ldw < (1 << 22), "mlp_fused: row pitch too large (32-bit tile-relative offsets)");
  GIMS_CHECK_ARG((((uintptr_t)a.a0 | (uintptr_t)a.a1 | (uintptr_t)a.w) & 127) == 0, "mlp_fused: SPL32 operands must be 128-byte aligned");
  GIMS_CHECK_ARG((a.ldc % 4) == 0 && a.ldc >= MF_D && (a.ld_split % 8) == 0 && a.ld_split >= 2 * MF_D && a.out_lo == a.out_hi + 32,
                 "mlp_fused: ldc >= n, a multiple of 4; ld_split >= 2n, a multiple of 8; out_lo = out_hi + 32");
  GIMS_CHECK_ARG((((uintptr_t)a.out_f32 | (uintptr_t)a.out_hi | (uintptr_t)a.residual | (uintptr_t)a.bias) & 15) == 0,
                 "mlp_fused: bias, residual and outputs must be 16-byte aligned");
  GIMS_LDS_ATTR((const void*)mlp_fused_x3_kernel, MF_LDS_BYTES);
  hipLaunchKernelGGL(mlp_fused_x3_kernel, dim3(cdiv(a.m, MF_TM)), dim3(512), MF_LDS_BYTES, s, a);
  GIMS_LAUNCH_CHECK();
  return GIMS_OK;
}

}  // namespace gims
