// Image-set matching: GIMS_AUX_ASSEMBLE_ROWS of gims_run_ops fills the residual stream of a batch of pairs, f32 `desc` and its
// SPL32 copy `dpl`, from per-image stores of encoded rows in ONE launch.  include/gims_hip.h has the contract; tests/features_ref.py is the NumPy
// restatement.  A pure streaming kernel: 4 bytes read, 4 + 4 written per element.
#include "common.h"

namespace gims {

constexpr int ASM_THREADS = 256;      // 4 waves
// (a source address comes out of the table as an integer: say that it is global memory, or the rows are read with flat loads)
typedef __attribute__((address_space(1))) f32x4 global_f32x4;
constexpr int ASM_ROWS = 4;         // consecutive destination rows per wave: one segment search serves them while they stay inside the segment

// The segment that holds destination row r, as its source row address, or nullptr (a gap, or a row of no segment).  tab: [n_seg][4] =
// {source address, source pitch in floats, rows, first destination row}, ascending by first destination row.  Everything here is wave-uniform
// (r comes from a readfirstlane'd wave index), so the search is scalar loads and scalar compares.
__device__ __forceinline__ const float* asm_locate(const int64_t* __restrict__ tab, int n_seg, int64_t r, int& hint) {
  int j = hint;
  if (j < 0 || !(tab[4 * (int64_t)j + 3] <= r && (j + 1 == n_seg || tab[4 * (int64_t)(j + 1) + 3] > r))) {
    // the last segment whose first destination row is <= r
    int lo = 0, hi = n_seg;           // invariant: start[lo - 1] <= r < start[hi]
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (tab[4 * (int64_t)mid + 3] <= r) lo = mid + 1; else hi = mid;
    }
    j = lo - 1;
  }
  hint = j;
  // segments without rows hold nothing: the one in front may still hold r (equal first rows sort in any order)
  while (j >= 0 && tab[4 * (int64_t)j + 2] <= 0) --j;
  if (j < 0) return nullptr;
  const int64_t* e = tab + 4 * (int64_t)j;
  const int64_t local = r - e[3];
  if (local < 0 || local >= e[2]) return nullptr;
  return (const float*)(uintptr_t)e[0] + local * e[1];
}

// One wave per ASM_ROWS destination rows; a lane takes 16 bytes of a row per step (k = 256: one step, 64 lanes x 16 B = the row).  Its four f32
// leave as one 16-byte store, its four hi and four lo bf16 as two 8-byte stores (four channels never straddle a 32-channel block).
__global__ __launch_bounds__(ASM_THREADS) void assemble_rows_kernel(const int64_t* __restrict__ tab, int n_seg, int64_t n_rows, int k,
                                                                    float* __restrict__ out, int64_t ld_out, uint16_t* __restrict__ split,
                                                                    int64_t ld_split) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * (ASM_THREADS / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t r0 = wave * ASM_ROWS;
  const float* src[ASM_ROWS];
  int hint = -1;
#pragma unroll
  for (int u = 0; u < ASM_ROWS; ++u) src[u] = r0 + u < n_rows ? asm_locate(tab, n_seg, r0 + u, hint) : nullptr;
  for (int c = 4 * lane; c < k; c += 256) {
    f32x4 v[ASM_ROWS];
#pragma unroll
    for (int u = 0; u < ASM_ROWS; ++u)
      if (src[u]) v[u] = *(const global_f32x4*)(uintptr_t)(src[u] + c);
#pragma unroll
    for (int u = 0; u < ASM_ROWS; ++u) {
      if (!src[u]) continue;
      const int64_t r = r0 + u;
      if (out) *(f32x4*)(out + r * ld_out + c) = v[u];
      if (split) {
        uint16_t h[4], l[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          h[q] = f2bf(v[u][q]);
          l[q] = f2bf(v[u][q] - bf2f(h[q]));
        }
        uint16_t* d = split + r * ld_split + spl_col(c);
        *(uint2*)d = make_uint2((uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16));
        *(uint2*)(d + 32) = make_uint2((uint32_t)l[0] | ((uint32_t)l[1] << 16), (uint32_t)l[2] | ((uint32_t)l[3] << 16));
      }
    }
  }
}

// GIMS_AUX_ASSEMBLE_ROWS of gims_run_ops (include/gims_hip.h): every argument check precedes the first HIP call
int assemble_rows_aux(const gims_aux_args& x, hipStream_t st) {
  const int64_t n_seg = x.i[0], n_rows = x.i[1], k = x.i[2], ld_out = x.i[3], ld_split = x.i[4];
  float* out = (float*)x.p[1];
  uint16_t* split = (uint16_t*)x.p[2];
  // i[5] is where a later form of this function would be selected: it is read FIRST, because under another form the other words need not mean
  // what they mean here -- to this version such a call asks for an auxiliary function it does not know, and is refused as one
  GIMS_CHECK_ARG(x.i[5] == 0, "gims_run_ops: unknown auxiliary function form: assemble_rows with i[5] = %lld (i[5] is reserved and must be 0)",
                 (long long)x.i[5]);
  GIMS_CHECK_ARG(n_seg >= 0 && n_seg <= INT32_MAX, "assemble_rows: n_seg = %lld is out of range (0 .. 2^31 - 1)", (long long)n_seg);
  GIMS_CHECK_ARG(n_rows >= 0 && n_rows <= INT32_MAX, "assemble_rows: n_rows = %lld is out of range (0 .. 2^31 - 1)", (long long)n_rows);
  GIMS_CHECK_ARG(k > 0 && k % 32 == 0 && k < (1 << 21), "assemble_rows: k = %lld must be a positive multiple of 32", (long long)k);
  GIMS_CHECK_ARG(out || split, "assemble_rows: out and out_split are both NULL");
  GIMS_CHECK_ARG(x.p[0] || n_seg == 0, "assemble_rows: the segment table is NULL while n_seg = %lld", (long long)n_seg);
  GIMS_CHECK_ARG(((uintptr_t)x.p[0] & 7) == 0, "assemble_rows: the segment table must be 8-byte aligned");
  GIMS_CHECK_ARG(!out || ld_out >= k, "assemble_rows: ld_out = %lld is below k = %lld", (long long)ld_out, (long long)k);
  GIMS_CHECK_ARG(!split || ld_split >= 2 * k, "assemble_rows: ld_split = %lld is below 2 k = %lld", (long long)ld_split, (long long)(2 * k));
  // what gims_linear asks of its pre-split operands and of the f32 stream next to them
  GIMS_CHECK_ARG(!out || (((uintptr_t)out & 15) == 0 && ld_out % 4 == 0), "assemble_rows: out must be 16-byte aligned, ld_out a multiple of 4 (alignment)");
  GIMS_CHECK_ARG(!split || (((uintptr_t)split & 127) == 0 && ld_split % 64 == 0 && ld_split < (1 << 22)),
                 "assemble_rows: out_split must be 128-byte aligned, ld_split a multiple of 64 below 2^22 (alignment)");
  if (n_seg == 0 || n_rows == 0) return GIMS_OK;
  const int64_t rows_per_block = (int64_t)ASM_ROWS * (ASM_THREADS / 64);
  assemble_rows_kernel<<<(unsigned)((n_rows + rows_per_block - 1) / rows_per_block), ASM_THREADS, 0, st>>>((const int64_t*)x.p[0], (int)n_seg, n_rows,
                                                                                                          (int)k, out, ld_out, split, ld_split);
  GIMS_LAUNCH_CHECK();
  return GIMS_OK;
}

}  // namespace gims
