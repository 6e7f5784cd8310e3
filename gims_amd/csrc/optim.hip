// Fused multi-tensor weight updates: what the reference's training loop does between loss.backward() and the next pair, for ALL tensors
// of the model in a handful of launches -- the optimizer step (train.py:52-57 builds torch.optim.Adam or, for opt_type: sgd,
// optim.SGD(momentum=0.9, nesterov=True) over three parameter groups, :138 calls optimizer.step()) and the EMA weight update
// (train.py:141, utils/common.py:1005-1015).
// HBM-bound elementwise work (Adam: per element 4 reads (p, g, m, v) + 3 writes (p, m, v) of 4 bytes); nothing to tile, nothing for the
// matrix cores -- the point is one launch per ~90 tensors instead of torch's ~90 launches + list marshalling per step (3 ms of host
// time per 29-ms step at 282 tensors).  multi_tensor_apply is the shared part: a by-value block of up to 80 tensors, the prefix table
// of 4096-element chunks, the ballot lookup of the owning tensor, the 16-byte f32x4 path with a scalar tail; an operation is a functor
// over RW read-modify-write streams and one stream that is read once (nontemporal).
// Adam follows torch's single-tensor Adam (torch/optim/adam.py, _single_tensor_adam, non-amsgrad, maximize = False, float32 op-math),
// operation by operation:
//     g' = g + wd * p                         (weight_decay != 0)
//     m  = m + (g' - m) * (1 - beta1)         (Tensor.lerp_, weight < 0.5 branch)
//     v  = v * beta2 + (1 - beta2) * g' * g'  (mul_ then addcmul_)
//     p  = p - step_size * m / (sqrt(v) / sqrt(1 - beta2^t) + eps),   step_size = lr / (1 - beta1^t)
// with the step-dependent scalars formed on the host in double and rounded to float once, as torch's scalar arguments are.
// SGD follows torch's _single_tensor_sgd (torch/optim/sgd.py, maximize = False):
//     g'  = g + wd * p                                  (weight_decay != 0)
//     buf = g'                                          (momentum != 0, first step of this tensor: the buffer is written, never read)
//     buf = buf * momentum + (1 - dampening) * g'       (momentum != 0, later steps: mul_ then add_(alpha))
//     g'' = g' + momentum * buf (nesterov) | buf (momentum != 0) | g' (momentum == 0)
//     p   = p + (-lr) * g''
// Every `x + alpha * y` of SGD is ONE fused multiply-add (sgd_axpy): torch's add(alpha) functor is `a + alpha * b` in one device
// expression, which the device compiler contracts -- this form reproduces torch.optim.SGD(foreach=False) bit for bit on gfx950
// (tests/test_optim_sgd_ema_gpu.py prints the difference: 0); the two-rounding form does not.
// EMA is the reference's two statements `v *= d; v += (1 - d) * msd[k]`: three separately rounded operations, no contraction.
#include "common.h"

namespace gims {

constexpr int MT_MAX_TENSORS = 80;     // per launch; Adam: 80 * 36 + 81 * 4 + 8 * 28 bytes of kernel arguments (< 4 KB)
constexpr int MT_MAX_GROUPS = 8;
constexpr int MT_CHUNK = 4096;         // elements per workgroup (256 threads x 4 float4)

// The tensors of one launch: RW streams that are read, updated and written back, and one stream that is only read, once.
template <int RW>
struct MultiTensorLaunch {
  float* rw[RW][MT_MAX_TENSORS];
  const float* ro[MT_MAX_TENSORS];
  int first_chunk[MT_MAX_TENSORS + 1];   // prefix sum of chunk counts
  int n[MT_MAX_TENSORS];
  unsigned char tag[MT_MAX_TENSORS];     // the operation's own per-tensor byte (its hyper-parameter group, flags)
  int count;
};

// One workgroup per 4096-element chunk.  Op supplies: RW; Hyper and hyper(tag) (what one tensor's elements share); live(r, h) (false:
// stream r of this tensor is absent -- its pointer may be null, nothing is loaded or stored); one(x[RW], g, h), the per-element update.
template <class Op>
__device__ __forceinline__ void multi_tensor_apply(const MultiTensorLaunch<Op::RW>& a, const Op& op) {
  constexpr int RW = Op::RW;
  __shared__ int s_t;
  if (threadIdx.x < 64) {                       // which tensor owns this chunk: ballot over the prefix table
    const int b = (int)blockIdx.x;
    int t = -1;
    for (int base = 0; base < a.count && t < 0; base += 64) {
      const int i = base + (int)threadIdx.x;
      const bool mine = i < a.count && b >= a.first_chunk[i] && b < a.first_chunk[i + 1];
      const unsigned long long mask = __ballot(mine);
      if (mask) t = base + __ffsll((long long)mask) - 1;
    }
    if (threadIdx.x == 0) s_t = t;
  }
  __syncthreads();
  const int t = s_t;
  if (t < 0) return;
  const typename Op::Hyper h = op.hyper(a.tag[t]);
  const int n = a.n[t];
  const int64_t base = (int64_t)((int)blockIdx.x - a.first_chunk[t]) * MT_CHUNK;
  const float* g = a.ro[t];
  float* x[RW];
  bool live[RW];
  uintptr_t bits = reinterpret_cast<uintptr_t>(g);
#pragma unroll
  for (int r = 0; r < RW; ++r) {
    live[r] = Op::live(r, h);
    x[r] = a.rw[r][t];
    if (live[r]) bits |= reinterpret_cast<uintptr_t>(x[r]);
  }
  const bool vec = (bits & 15) == 0;
#pragma unroll
  for (int k = 0; k < MT_CHUNK / 1024; ++k) {
    const int64_t i = base + (int64_t)k * 1024 + 4 * (int)threadIdx.x;
    if (i >= n) break;
    if (vec && i + 4 <= n) {
      f32x4 xx[RW];
#pragma unroll
      for (int r = 0; r < RW; ++r) xx[r] = live[r] ? *reinterpret_cast<const f32x4*>(x[r] + i) : f32x4{0.f, 0.f, 0.f, 0.f};
      const f32x4 gg = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g + i));
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float xe[RW];
#pragma unroll
        for (int r = 0; r < RW; ++r) xe[r] = xx[r][e];
        Op::one(xe, gg[e], h);
#pragma unroll
        for (int r = 0; r < RW; ++r) xx[r][e] = xe[r];
      }
#pragma unroll
      for (int r = 0; r < RW; ++r)
        if (live[r]) *reinterpret_cast<f32x4*>(x[r] + i) = xx[r];
    } else {
      for (int e = 0; e < 4 && i + e < n; ++e) {
        float xe[RW];
#pragma unroll
        for (int r = 0; r < RW; ++r) xe[r] = live[r] ? x[r][i + e] : 0.f;
        Op::one(xe, g[i + e], h);
#pragma unroll
        for (int r = 0; r < RW; ++r)
          if (live[r]) x[r][i + e] = xe[r];
      }
    }
  }
}

// ---- Adam: streams p, m, v; read once: g; tag = group
struct AdamGroup { float step_size, bc2_sqrt, beta2, eps, wd, one_m_beta1, one_m_beta2; };   // 1 - beta formed in double, like torch's scalars

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const AdamGroup& h) {
  // no contraction across torch's separately rounded operations
  if (h.wd != 0.f) g = __fadd_rn(g, __fmul_rn(h.wd, p));
  m = __fadd_rn(m, __fmul_rn(__fsub_rn(g, m), h.one_m_beta1));
  v = __fmul_rn(v, h.beta2);
  v = __fadd_rn(v, __fmul_rn(__fmul_rn(h.one_m_beta2, g), g));      // addcmul_: input + value * t1 * t2
  const float denom = __fadd_rn(__fdiv_rn(__fsqrt_rn(v), h.bc2_sqrt), h.eps);
  p = __fadd_rn(p, __fmul_rn(-h.step_size, __fdiv_rn(m, denom)));   // addcdiv_: input + value * (t1 / t2)
}


struct AdamOp {
  static constexpr int RW = 3;
  typedef AdamGroup Hyper;
  AdamGroup grp[MT_MAX_GROUPS];
  __device__ __forceinline__ Hyper hyper(int tag) const { return grp[tag]; }
  static __device__ __forceinline__ bool live(int, const Hyper&) { return true; }
  static __device__ __forceinline__ void one(float (&x)[3], float g, const Hyper& h) { adam_one(x[0], g, x[1], x[2], h); }
};

__global__ __launch_bounds__(256) void adam_kernel(const MultiTensorLaunch<3> a, const AdamOp op) { multi_tensor_apply(a, op); }

// ---- SGD: streams p, momentum buffer (absent when the group's momentum is 0); read once: g; tag = group | first << 3
struct SgdGroup { float neg_lr, momentum, one_m_damp, wd; int nesterov, first; };

__device__ __forceinline__ float sgd_axpy(float a, float alpha, float b) { return __fmaf_rn(alpha, b, a); }   // a + alpha * b, one rounding

struct SgdOp {
  static constexpr int RW = 2;
  typedef SgdGroup Hyper;
  SgdGroup grp[MT_MAX_GROUPS];
  __device__ __forceinline__ Hyper hyper(int tag) const {
    Hyper h = grp[tag & 7];
    h.first = tag >> 3;
    return h;
  }
  static __device__ __forceinline__ bool live(int r, const Hyper& h) { return r == 0 || h.momentum != 0.f; }
  static __device__ __forceinline__ void one(float (&x)[2], float g, const Hyper& h) {
    const float p = x[0];
    if (h.wd != 0.f) g = sgd_axpy(g, h.wd, p);
    if (h.momentum != 0.f) {
      const float buf = h.first ? g : sgd_axpy(__fmul_rn(x[1], h.momentum), h.one_m_damp, g);
      x[1] = buf;
      g = h.nesterov ? sgd_axpy(g, h.momentum, buf) : buf;
    }
    x[0] = sgd_axpy(p, h.neg_lr, g);
  }
};

__global__ __launch_bounds__(256) void sgd_kernel(const MultiTensorLaunch<2> a, const SgdOp op) { multi_tensor_apply(a, op); }

// ---- EMA: stream ema; read once: model
struct EmaOp {
  static constexpr int RW = 1;
  struct Hyper { float d, one_m_d; };
  Hyper h;
  __device__ __forceinline__ Hyper hyper(int) const { return h; }
  static __device__ __forceinline__ bool live(int, const Hyper&) { return true; }
  static __device__ __forceinline__ void one(float (&x)[1], float m, const Hyper& h) {
#pragma clang fp contract(off)   // __fmul_rn / __fadd_rn are plain * and + to the compiler, which would fuse them
    const float a = x[0] * h.d, b = h.one_m_d * m;
    x[0] = a + b;
  }
};

__global__ __launch_bounds__(256) void ema_kernel(const MultiTensorLaunch<1> a, const EmaOp op) { multi_tensor_apply(a, op); }

// Host side of every operation: pack the next up to 80 non-empty tensors (row(k, rw, ro, n, tag) describes tensor k) and launch.
template <int RW, class Row, class Launch>
static int multi_tensor_run(int32_t count, Row row, Launch launch) {
  MultiTensorLaunch<RW> a;
  int k = 0;
  while (k < count) {
    int c = 0, chunks = 0;
    for (; k < count && c < MT_MAX_TENSORS; ++k) {
      float* rw[RW];
      const float* ro;
      int64_t n;
      unsigned char tag;
      row(k, rw, ro, n, tag);
      if (n == 0) continue;
      for (int r = 0; r < RW; ++r) a.rw[r][c] = rw[r];
      a.ro[c] = ro; a.n[c] = (int)n; a.tag[c] = tag;
      a.first_chunk[c] = chunks;
      chunks += cdiv(n, MT_CHUNK);
      ++c;
    }
    if (c == 0) break;
    a.first_chunk[c] = chunks;
    a.count = c;
    launch(a, chunks);
    GIMS_LAUNCH_CHECK();
  }
  return GIMS_OK;
}

}  // namespace gims

using namespace gims;

extern "C" int gims_adam_step(const gims_adam_tensor* tensors, int32_t count, const gims_adam_group* groups, int32_t n_groups, void* stream) {
  GIMS_CHECK_ARG(count >= 0 && n_groups >= 0 && n_groups <= MT_MAX_GROUPS, "gims_adam_step: %d groups (at most %d)", n_groups, MT_MAX_GROUPS);
  if (count == 0) return GIMS_OK;
  GIMS_CHECK_ARG(tensors && groups && n_groups > 0, "gims_adam_step: null table");
  AdamGroup hg[MT_MAX_GROUPS];
  for (int k = 0; k < n_groups; ++k) {
    const gims_adam_group& g = groups[k];
    GIMS_CHECK_ARG(g.step >= 1 && g.beta1 >= 0.0 && g.beta1 < 1.0 && g.beta2 >= 0.0 && g.beta2 < 1.0 && g.eps >= 0.0 && g.lr >= 0.0 && g.weight_decay >= 0.0,
                   "gims_adam_step: group %d: step %lld lr %g betas (%g, %g) eps %g weight_decay %g", k, (long long)g.step, g.lr, g.beta1, g.beta2, g.eps,
                   g.weight_decay);
    const double bc1 = 1.0 - pow(g.beta1, (double)g.step), bc2 = 1.0 - pow(g.beta2, (double)g.step);
    hg[k].step_size = (float)(g.lr / bc1);
    hg[k].bc2_sqrt = (float)sqrt(bc2);
    hg[k].beta2 = (float)g.beta2;
    hg[k].eps = (float)g.eps;
    hg[k].wd = (float)g.weight_decay;
    hg[k].one_m_beta1 = (float)(1.0 - g.beta1);
    hg[k].one_m_beta2 = (float)(1.0 - g.beta2);
  }
  for (int k = 0; k < count; ++k) {
    GIMS_CHECK_ARG(tensors[k].n >= 0 && tensors[k].n < ((int64_t)1 << 31), "gims_adam_step: tensor %d has %lld elements", k, (long long)tensors[k].n);
    GIMS_CHECK_ARG(tensors[k].n == 0 || (tensors[k].param && tensors[k].grad && tensors[k].exp_avg && tensors[k].exp_avg_sq), "gims_adam_step: tensor %d: null pointer", k);
    GIMS_CHECK_ARG(tensors[k].group >= 0 && tensors[k].group < n_groups, "gims_adam_step: tensor %d names group %d of %d", k, tensors[k].group, n_groups);
  }
  AdamOp op;
  for (int k = 0; k < n_groups; ++k) op.grp[k] = hg[k];
  return multi_tensor_run<3>(
      count,
      [&](int k, float** rw, const float*& ro, int64_t& n, unsigned char& tag) {
        rw[0] = tensors[k].param; rw[1] = tensors[k].exp_avg; rw[2] = tensors[k].exp_avg_sq;
        ro = tensors[k].grad; n = tensors[k].n; tag = (unsigned char)tensors[k].group;
      },
      [&](const MultiTensorLaunch<3>& a, int chunks) { hipLaunchKernelGGL(adam_kernel, dim3((unsigned)chunks), dim3(256), 0, (hipStream_t)stream, a, op); });
}

extern "C" int gims_sgd_step(const gims_sgd_tensor* tensors, int32_t count, const gims_sgd_group* groups, int32_t n_groups, void* stream) {
  GIMS_CHECK_ARG(count >= 0, "gims_sgd_step: %d tensors", count);
  if (count == 0) return GIMS_OK;
  GIMS_CHECK_ARG(tensors && groups, "gims_sgd_step: null table");
  GIMS_CHECK_ARG(n_groups >= 1 && n_groups <= MT_MAX_GROUPS, "gims_sgd_step: %d groups (1 to %d)", n_groups, MT_MAX_GROUPS);
  SgdOp op;
  for (int k = 0; k < n_groups; ++k) {
    const gims_sgd_group& g = groups[k];
    GIMS_CHECK_ARG(g.lr >= 0.0 && g.momentum >= 0.0 && g.weight_decay >= 0.0 && g.dampening == g.dampening,
                   "gims_sgd_step: group %d: lr %g momentum %g dampening %g weight_decay %g", k, g.lr, g.momentum, g.dampening, g.weight_decay);
    GIMS_CHECK_ARG(!g.nesterov || (g.momentum > 0.0 && g.dampening == 0.0), "gims_sgd_step: group %d: nesterov needs a momentum and zero dampening (momentum %g dampening %g)",
                   k, g.momentum, g.dampening);
    op.grp[k].neg_lr = (float)(-g.lr);
    op.grp[k].momentum = (float)g.momentum;
    op.grp[k].one_m_damp = (float)(1.0 - g.dampening);
    op.grp[k].wd = (float)g.weight_decay;
    op.grp[k].nesterov = g.nesterov != 0;
    op.grp[k].first = 0;
  }
  for (int k = 0; k < count; ++k) {
    const gims_sgd_tensor& t = tensors[k];
    GIMS_CHECK_ARG(t.n >= 0 && t.n < ((int64_t)1 << 31), "gims_sgd_step: tensor %d has %lld elements", k, (long long)t.n);
    GIMS_CHECK_ARG(t.group >= 0 && t.group < n_groups, "gims_sgd_step: tensor %d names group %d of %d", k, t.group, n_groups);
    // the kernel decides on the float: a momentum that rounds to 0 runs without a buffer
    GIMS_CHECK_ARG(t.n == 0 || (t.param && t.grad && (t.momentum_buffer || op.grp[t.group].momentum == 0.f)), "gims_sgd_step: tensor %d: null pointer", k);
  }
  return multi_tensor_run<2>(
      count,
      [&](int k, float** rw, const float*& ro, int64_t& n, unsigned char& tag) {
        rw[0] = tensors[k].param; rw[1] = tensors[k].momentum_buffer;
        ro = tensors[k].grad; n = tensors[k].n; tag = (unsigned char)(tensors[k].group | (tensors[k].first != 0 ? 8 : 0));
      },
      [&](const MultiTensorLaunch<2>& a, int chunks) { hipLaunchKernelGGL(sgd_kernel, dim3((unsigned)chunks), dim3(256), 0, (hipStream_t)stream, a, op); });
}

extern "C" int gims_ema_update(const gims_ema_tensor* tensors, int32_t count, double decay, void* stream) {
  GIMS_CHECK_ARG(count >= 0, "gims_ema_update: %d tensors", count);
  if (count == 0) return GIMS_OK;
  GIMS_CHECK_ARG(tensors, "gims_ema_update: null table");
  GIMS_CHECK_ARG(decay >= 0.0 && decay <= 1.0, "gims_ema_update: decay %g outside [0, 1]", decay);
  for (int k = 0; k < count; ++k) {
    const gims_ema_tensor& t = tensors[k];
    GIMS_CHECK_ARG(t.n >= 0 && t.n < ((int64_t)1 << 31), "gims_ema_update: tensor %d has %lld elements", k, (long long)t.n);
    GIMS_CHECK_ARG(t.n == 0 || (t.ema && t.model), "gims_ema_update: tensor %d: null pointer", k);
    GIMS_CHECK_ARG(t.n == 0 || t.ema != t.model, "gims_ema_update: tensor %d: ema and model are the same tensor", k);
  }
  EmaOp op;
  op.h.d = (float)decay;
  op.h.one_m_d = (float)(1.0 - decay);
  return multi_tensor_run<1>(
      count,
      [&](int k, float** rw, const float*& ro, int64_t& n, unsigned char& tag) {
        rw[0] = tensors[k].ema; ro = tensors[k].model; n = tensors[k].n; tag = 0;
      },
      [&](const MultiTensorLaunch<1>& a, int chunks) { hipLaunchKernelGGL(ema_kernel, dim3((unsigned)chunks), dim3(256), 0, (hipStream_t)stream, a, op); });
}
