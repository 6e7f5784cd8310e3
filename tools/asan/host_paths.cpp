// Host-side AddressSanitizer harness ("compile-time -fsanitize=address for host C++").  CPU container
// only -- never on the GPU pool.  The library's HOST code (argument validation, workspace / plan / layout arithmetic, table
// builders, error strings, the replay loop) is compiled with -fsanitize=address (device code untouched: -fno-gpu-sanitize)
// and driven through every entry point that can run without a GPU: calls either return before touching HIP (GIMS_EINVAL,
// size queries) or fail cleanly inside the runtime (GIMS_EHIP: no device here).  ASan aborts on any heap / stack / global
// overflow, use-after-free or leak it sees on the way.    Build + run: tools/asan/run.sh
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/gims_hip.h"

namespace gims {   // the internal interface of sinkhorn2d.hip as csrc/common.h declares it: the on-chip Sinkhorn layout is chosen only on a
// device with 256 compute units, so its carving mode is reached here directly
struct OtR2Host { const float* z; int64_t ld; int n, m; float* u; float* v; float* status; float norm, log_mu_bin, log_nu_bin; };
struct OtR2Plan { bool ok; int nx, nc, ppg, ngroups; size_t bytes; };
OtR2Plan ot_res2_plan(const OtR2Host* pr, int np, int iters);
int ot_res2_run(const OtR2Plan& P, const OtR2Host* hp, int np, float alpha, int iters, int init_inside, char* base, hipStream_t s);
}  // namespace gims

static int checks = 0;
#define EXPECT(cond) do { ++checks; if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s  (last error: %s)\n", __FILE__, __LINE__, #cond, gims_last_error()); exit(1); } } while (0)

int main() {
  EXPECT(gims_abi_version() == GIMS_ABI_VERSION);
  // ---- Sinkhorn: size / plan arithmetic over ragged problem lists (host vectors, per-problem loops)
  std::vector<gims_ot_problem> pr;
  for (int i = 0; i < 40; ++i) {
    gims_ot_problem q; memset(&q, 0, sizeof(q));
    q.n = 600 + 7 * i; q.m = 640 - 5 * i; q.ld = (q.m + 3) / 4 * 4;
    pr.push_back(q);
  }
  EXPECT(gims_sinkhorn_workspace_bytes(pr.data(), (int)pr.size()) > 0);
  EXPECT(gims_sinkhorn_workspace_bytes(nullptr, 3) == 0);
  EXPECT(gims_sinkhorn_plan(pr.data(), (int)pr.size(), 100, 0) >= 0);
  for (int n : {1, 31, 1024, 4096, 5000, 16384}) {
    gims_ot_problem q; memset(&q, 0, sizeof(q)); q.n = n; q.m = n; q.ld = (n + 3) / 4 * 4;
    EXPECT(gims_sinkhorn_workspace_bytes(&q, 1) > 0);
    EXPECT(gims_sinkhorn_plan(&q, 1, 100, 0) >= 0);
  }
  EXPECT(gims_sinkhorn_match(nullptr, 1, 1.f, 10, 0.2f, nullptr, 0, 0, nullptr) == GIMS_EINVAL);
  EXPECT(gims_sinkhorn_match(pr.data(), (int)pr.size(), 1.f, -1, 0.2f, (void*)0x1000, 1 << 20, 0, nullptr) == GIMS_EINVAL);
  EXPECT(strlen(gims_last_error()) > 0);
  // ---- adaptive graph: workspace arithmetic, validation
  std::vector<gims_agc_image> im(5);
  for (size_t i = 0; i < im.size(); ++i) { memset(&im[i], 0, sizeof(im[i])); im[i].n = 100 + 900 * (int)i; im[i].d = 256; im[i].ldd = 256; im[i].max_edges_dir = 64 * im[i].n; }
  EXPECT(gims_agc_workspace_bytes(im.data(), (int)im.size(), GIMS_AGC_ROBUST) > 0);
  const gims_agc_params one = {15.0, 2.0, 7, 0};
  EXPECT(gims_agc_build(nullptr, 0, &one, 1, 0, nullptr, 0, nullptr) != GIMS_OK);
  {   // flags, the keypoint limit by name, workspace arithmetic at the largest published size and at the limit
    EXPECT(gims_agc_max_keypoints() == 32768);
    EXPECT(gims_agc_build(nullptr, 0, &one, 1, GIMS_AGC_ROBUST, nullptr, 0, nullptr) != GIMS_OK);
    gims_agc_image big; memset(&big, 0, sizeof(big));
    big.d = 256; big.ldd = 256;
    for (int n : {2, 16384, 16385, 21163, 32768}) {
      big.n = n; big.max_edges_dir = 64 * n;
      const size_t wb = gims_agc_workspace_bytes(&big, 1, GIMS_AGC_ROBUST);
      EXPECT(wb > (size_t)n * (size_t)(n - 1) * 2);                                   // one word per pair of the strict upper triangle is in there
    }
    big.n = 32769; big.max_edges_dir = 64;                                             // over the limit: refused with the limit in the message
    big.kpts = (const float*)0x1000; big.desc = (const float*)0x2000; big.kept = (int32_t*)0x3000; big.indptr = (int32_t*)0x4000;
    big.indices = (int32_t*)0x5000; big.info = (int32_t*)0x6000;
    EXPECT(gims_agc_build(&big, 1, &one, 1, 0, (void*)0x7000, (size_t)1 << 40, nullptr) == GIMS_EINVAL);
    EXPECT(strstr(gims_last_error(), "32768") != nullptr);
    big.n = 100; big.d = 48;                                                           // descriptor width not a multiple of 32
    EXPECT(gims_agc_build(&big, 1, &one, 1, 0, (void*)0x7000, (size_t)1 << 40, nullptr) == GIMS_EINVAL);
    big.d = 256;                                                                       // a workspace that is too small
    EXPECT(gims_agc_build(&big, 1, &one, 1, GIMS_AGC_ROBUST, (void*)0x7000, 64, nullptr) == GIMS_EINVAL);
    // per-flow workspace sizes -- the default flow does not hold the half N x N matrix; a descriptor width that forces the robust flow
    // is sized for it whatever the flags say; a workspace sized for the default flow is refused by a robust build
    for (int n : {1000, 21163}) {
      big.n = n; big.d = 256; big.max_edges_dir = 64 * n;
      const size_t w0 = gims_agc_workspace_bytes(&big, 1, 0), w1 = gims_agc_workspace_bytes(&big, 1, GIMS_AGC_ROBUST);
      EXPECT(w1 >= w0 + (size_t)n * (size_t)n * 2 && w0 > (size_t)n * (size_t)(n - 1) * 2);      // the flags argument decides the half N x N matrix
    }
    big.n = 1000; big.d = 96; big.max_edges_dir = 64000;
    EXPECT(gims_agc_workspace_bytes(&big, 1, 0) == gims_agc_workspace_bytes(&big, 1, GIMS_AGC_ROBUST));
    big.d = 256;
    EXPECT(gims_agc_build(&big, 1, &one, 1, GIMS_AGC_ROBUST, (void*)0x7000, gims_agc_workspace_bytes(&big, 1, 0), nullptr) == GIMS_EINVAL);
    EXPECT(gims_agc_workspace_bytes(nullptr, 0, 0) == 0);
  }
  {   // guarded launches (gims_attn_guard) -- validation only
    gims_attn_args aa; memset(&aa, 0, sizeof(aa));
    EXPECT(gims_attention(nullptr, nullptr) == GIMS_EINVAL);
    EXPECT(gims_attention(&aa, nullptr) == GIMS_EINVAL);
    aa.qkv = (const uint16_t*)0x1000; aa.ld = 1536; aa.k_col = 256; aa.v_col = 512; aa.problems = (const gims_attn_problem*)0x2000; aa.n_problems = 1;
    aa.max_n_q = 64; aa.n_heads = 4; aa.out = (float*)0x3000; aa.ld_out = 256;
    aa.guard.stat = (uint64_t*)0x4000; aa.guard.kind = GIMS_GUARD_PEAKED; aa.guard.n_heads = 4;
    EXPECT(gims_attention(&aa, nullptr) == GIMS_EINVAL);                            // a guard without GIMS_ATTN_X3
    aa.flags = GIMS_ATTN_X3; aa.guard.kind = 7;
    EXPECT(gims_attention(&aa, nullptr) == GIMS_EINVAL);                            // unknown guard kind
    aa.guard.kind = GIMS_GUARD_RANGE; aa.guard.n_heads = 16;
    EXPECT(gims_attention(&aa, nullptr) == GIMS_EINVAL);                            // more heads than one wave evaluates
    gims_linear_args lg; memset(&lg, 0, sizeof(lg));
    lg.a0 = (const float*)0x1000; lg.w = (const void*)0x2000; lg.out_f32 = (float*)0x3000; lg.m = lg.n = lg.k = lg.k0 = 64; lg.lda0 = lg.ldw = lg.ldc = 64;
    lg.guard.stat = (uint64_t*)0x4000; lg.guard.kind = GIMS_GUARD_PEAKED; lg.guard.n_heads = 4;
    EXPECT(gims_linear(&lg, nullptr) == GIMS_EINVAL);                                  // a guard on a launch without pre-split operands
  }
  {   // round 5: training attention (gims_train_attention_*) -- argument validation and workspace arithmetic (no launch)
    EXPECT(gims_train_attention_workspace_floats(0, 4) == 0);
    EXPECT(gims_train_attention_workspace_floats(4096, 4) >= (size_t)4096 * 4 * (1 + 3 * 64));
    EXPECT(gims_train_attention_workspace_floats(3, 3) % 4 == 0 || gims_train_attention_workspace_floats(3, 3) > 9);      // D block rounded to 16 bytes
    std::vector<gims_train_attn_problem> tp(40);
    for (int i = 0; i < 40; ++i) { tp[i].q_off = 100 * i; tp[i].nq = 100; tp[i].k_off = 100 * (i ^ 1); tp[i].nk = 100; }
    gims_train_attn_args ta; memset(&ta, 0, sizeof(ta));
    EXPECT(gims_train_attention_forward(nullptr, nullptr) == GIMS_EINVAL);
    EXPECT(gims_train_attention_forward(&ta, nullptr) == GIMS_EINVAL);
    ta.qkv = (const float*)0x10000; ta.ld = 768; ta.rows = 4000; ta.d = 256; ta.heads = 4; ta.scale = 0.125f; ta.n_problems = 40; ta.problems = tp.data();
    ta.o = (float*)0x20000; ta.ldo = 256; ta.lse = (float*)0x30000;
    ta.heads = 8;
    EXPECT(gims_train_attention_forward(&ta, nullptr) == GIMS_EINVAL);                 // head dimension 32
    ta.heads = 4; ta.ld = 767;
    EXPECT(gims_train_attention_forward(&ta, nullptr) == GIMS_EINVAL);                 // pitch
    ta.ld = 768; tp[38].nk = 101;
    EXPECT(gims_train_attention_forward(&ta, nullptr) == GIMS_EINVAL);                 // sources beyond the rows
    EXPECT(strstr(gims_last_error(), "problem 38") != nullptr);
    tp[38].nk = 100; tp[7].nq = 0;
    EXPECT(gims_train_attention_forward(&ta, nullptr) == GIMS_EINVAL);                 // an empty problem
    tp[7].nq = 100;
    EXPECT(gims_train_attention_forward(&ta, nullptr) == GIMS_EINVAL);                 // several key ranges and no workspace
    ta.work = (float*)0x40004;
    EXPECT(gims_train_attention_forward(&ta, nullptr) == GIMS_EINVAL);                 // misaligned workspace
    ta.work = (float*)0x40000; ta.work_floats = 16;
    EXPECT(gims_train_attention_forward(&ta, nullptr) == GIMS_EINVAL);                 // too small
    ta.work_floats = gims_train_attention_workspace_floats(ta.rows, ta.heads);
    EXPECT(gims_train_attention_backward(&ta, nullptr) == GIMS_EINVAL);                // no gradient tensors
    ta.d_o = (const float*)0x50000; ta.lddo = 256; ta.d_qkv = (float*)0x60000; ta.lddq = 768; ta.reverse_precision = 5;
    EXPECT(gims_train_attention_backward(&ta, nullptr) == GIMS_EINVAL);                // unknown reverse precision
  }
  // ---- evaluation: workspace arithmetic
  std::vector<gims_eval_pair> ep(3);
  for (size_t i = 0; i < ep.size(); ++i) { memset(&ep[i], 0, sizeof(ep[i])); ep[i].n0 = 500 + (int)i; ep[i].n1 = 400; ep[i].height = 480; ep[i].width = 640; }
  EXPECT(gims_eval_workspace_bytes(ep.data(), (int)ep.size(), 2000) > 0);
  EXPECT(gims_eval_pairs(nullptr, 0, 3.f, 3, 3.f, 100, 1, nullptr, 0, nullptr) != GIMS_OK);
  // ---- pyramid layout (host loops over octaves / levels, caller-provided table with exact and short capacity)
  int32_t nl = 0; size_t pb = 0, sb = 0;
  EXPECT(gims_pyramid_layout(480, 640, 3, nullptr, 0, &nl, &pb, &sb) == GIMS_OK && nl > 0 && nl % 6 == 0 && pb > 0 && sb > 0);
  std::vector<gims_pyr_level> lv(nl);
  EXPECT(gims_pyramid_layout(480, 640, 3, lv.data(), nl, &nl, &pb, &sb) == GIMS_OK);
  EXPECT(lv[0].h == 960 && lv[0].w == 1280 && lv[6].h == 480 && (size_t)lv[nl - 1].offset < pb);
  EXPECT(gims_pyramid_layout(480, 640, 3, lv.data(), nl - 1, &nl, &pb, &sb) == GIMS_EINVAL);
  EXPECT(gims_pyramid_layout(0, 640, 3, nullptr, 0, &nl, &pb, &sb) == GIMS_EINVAL);
  for (int h : {1, 2, 3, 7, 33, 75, 1201}) {          // tiny images have no octave at all: a clean GIMS_EINVAL
    const int rc = gims_pyramid_layout(h, 2 * h + 1, 3, nullptr, 0, &nl, &pb, &sb);
    EXPECT(rc == GIMS_OK || (h < 3 && rc == GIMS_EINVAL));
  }
  EXPECT(gims_pyramid_build(nullptr, 10, 10, 3, nullptr, nullptr, nullptr) == GIMS_EINVAL);
  EXPECT(gims_patch_extract(nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr) == GIMS_EINVAL);
  // ---- replay loop: empty table, unknown op kind, a linear op that fails validation
  EXPECT(gims_run_ops(nullptr, 0, nullptr) == GIMS_EINVAL);
  std::vector<gims_op> ops(3);
  memset(ops.data(), 0, sizeof(gims_op) * ops.size());
  EXPECT(gims_run_ops(ops.data(), 0, nullptr) == GIMS_OK);
  ops[0].kind = 7;
  EXPECT(gims_run_ops(ops.data(), 1, nullptr) == GIMS_EINVAL);
  ops[0].kind = GIMS_OP_LINEAR;                       // all-null linear arguments
  EXPECT(gims_run_ops(ops.data(), 3, nullptr) != GIMS_OK);
  ops[0].kind = GIMS_OP_ATTENTION;
  EXPECT(gims_run_ops(ops.data(), 3, nullptr) != GIMS_OK);
  EXPECT(gims_run_ops_timed(ops.data(), 1, nullptr, nullptr) == GIMS_EINVAL);
  // ---- validation of the remaining entry points (every call returns before touching memory it was not given)
  gims_linear_args la; memset(&la, 0, sizeof(la));
  EXPECT(gims_linear(&la, nullptr) != GIMS_OK);
  EXPECT(gims_linear(nullptr, nullptr) != GIMS_OK);
  EXPECT(gims_linear_batch(nullptr, 0, 0, 0, GIMS_PREC_F32, nullptr) != GIMS_OK);
  {   // the launch counters (host-side state only)
    uint64_t cnt[8] = {9, 9, 9, 9, 9, 9, 9, 9};
    EXPECT(gims_attention_launch_counts(cnt, 8, 1) == GIMS_OK && cnt[GIMS_ATTN_KERNEL_KINDS] == 0 && cnt[7] == 0);
    EXPECT(gims_attention_launch_counts(cnt, 3, 0) == GIMS_OK && cnt[0] == 0 && cnt[2] == 0);
    EXPECT(gims_attention_launch_counts(nullptr, 4, 0) == GIMS_EINVAL && gims_attention_launch_counts(nullptr, 0, 0) == GIMS_OK);
    gims_attn_args aa; memset(&aa, 0, sizeof(aa));                                    // a guard without GIMS_ATTN_X3 is refused before anything is launched
    aa.qkv = (const uint16_t*)0x1000; aa.ld = 1536; aa.k_col = 256; aa.v_col = 512; aa.problems = (const gims_attn_problem*)0x2000; aa.n_problems = 1;
    aa.max_n_q = 64; aa.n_heads = 4; aa.out = (float*)0x3000; aa.ld_out = 256; aa.guard.stat = (uint64_t*)0x4000; aa.guard.kind = GIMS_GUARD_PEAKED;
    aa.guard.n_heads = 4; aa.guard.max_thr = 0.5;
    EXPECT(gims_attention(&aa, nullptr) == GIMS_EINVAL);
    memset(&aa.guard, 0, sizeof(aa.guard)); aa.ld = 768; aa.stat = (uint64_t*)0x4004;
    EXPECT(gims_attention(&aa, nullptr) == GIMS_EINVAL && strstr(gims_last_error(), "stat"));      // misaligned statistics accumulator
  }
  EXPECT(gims_patch_affine(nullptr, nullptr, 3, nullptr, nullptr, nullptr) == GIMS_EINVAL);
  EXPECT(gims_patch_affine(nullptr, nullptr, 0, nullptr, nullptr, nullptr) == GIMS_OK);          // nothing to do
  EXPECT(gims_sinkhorn_plan(pr.data(), (int)pr.size(), 100, GIMS_OT_STREAMED) == 0);           // streamed on request, whatever the sizes
  EXPECT(gims_sinkhorn_match(nullptr, 0, 1.f, 10, 0.2f, nullptr, 0, GIMS_OT_STREAMED, nullptr) == GIMS_EINVAL);
  EXPECT(gims_train_loss(nullptr, 0, nullptr, 0, 1.f, 0.45f, 1.f, nullptr, nullptr, nullptr, nullptr) == GIMS_EINVAL);
  EXPECT(gims_ingest_images(nullptr, 0, 0, 0, nullptr, 0, nullptr, nullptr, nullptr) == GIMS_EINVAL);
  EXPECT(gims_pack_graphs(nullptr, 0, 0, 0, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr) == GIMS_EINVAL);
  EXPECT(gims_events_create(0, nullptr) == GIMS_EINVAL);
  EXPECT(gims_ops_graph_create(nullptr, 0, nullptr, nullptr) == GIMS_EINVAL);
  // ---- training-step entry points: size queries over ragged shapes, argument checks, the split-K / alignment planning of gims_gemm_f32
  {
    gims_gemm g; memset(&g, 0, sizeof(g));
    EXPECT(gims_gemm_f32(&g, nullptr) == GIMS_EINVAL);
    EXPECT(gims_gemm_f32(nullptr, nullptr) == GIMS_EINVAL);
    g.a = (const float*)0x1000; g.b = (const float*)0x2000; g.c = (float*)0x3000; g.m = 5; g.n = 7; g.k = 3; g.batch = 1; g.lda = 2; g.ldb = 3; g.ldc = 7;
    g.precision = GIMS_PREC_BF16X6;
    EXPECT(gims_gemm_f32(&g, nullptr) == GIMS_EINVAL);            // lda smaller than the row it strides
    g.lda = 3; g.precision = GIMS_PREC_F32;
    EXPECT(gims_gemm_f32(&g, nullptr) == GIMS_EINVAL);            // unsupported precision
    gims_segments sg; memset(&sg, 0, sizeof(sg));
    EXPECT(gims_batchnorm_workspace_floats(&sg, 32) == 0);
    sg.n = 8;
    for (int i = 0; i < 8; ++i) { sg.off[i] = 300 * i; sg.rows[i] = 1 + 37 * i; }
    EXPECT(gims_batchnorm_workspace_floats(&sg, 512) > 0);
    sg.n = 9;
    EXPECT(gims_batchnorm_workspace_floats(&sg, 512) == 0);
    EXPECT(gims_batchnorm_train_forward((const float*)0x1000, 512, 512, &sg, (const float*)0x1000, (const float*)0x1000, 1e-5f, 0.1f, nullptr, nullptr,
                                        (float*)0x1000, (float*)0x1000, 512, 1, (float*)0x1000, nullptr) == GIMS_EINVAL);
    EXPECT(gims_colsum_workspace_floats(4097, 768) == 64 + (size_t)33 * 768);
    EXPECT(gims_colsum((const float*)0x1001, 512, 10, 512, 0.f, (float*)0x1000, (float*)0x1000, nullptr) == GIMS_EINVAL);   // unaligned
    EXPECT(gims_softmax_rows(nullptr, 0, 1, 1, 1, 0, nullptr) == GIMS_EINVAL);
    EXPECT(gims_layernorm_backward(nullptr, 0, nullptr, 0, 1, 600, nullptr, nullptr, 1e-6f, 1, nullptr, 0, nullptr, nullptr, nullptr) == GIMS_EINVAL);
    EXPECT(gims_head_pack(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 256, 4, 0, nullptr) == GIMS_EINVAL);
    EXPECT(gims_sage_mean_transposed(nullptr, 0, nullptr, nullptr, 1, 30, nullptr, 0, nullptr) == GIMS_EINVAL);
    for (int n : {1, 63, 2048, 4097}) {
      gims_ot_problem q; memset(&q, 0, sizeof(q)); q.n = n; q.m = n + 3; q.ld = (q.m + 3) / 4 * 4;
      EXPECT(gims_sinkhorn_backward_workspace_bytes(&q, 1) > 0);
      EXPECT(gims_sinkhorn_history_floats(q.n, q.m, 100) == (size_t)101 * (size_t)(q.n + q.m + 2));
    }
    EXPECT(gims_sinkhorn_backward_workspace_bytes(nullptr, 2) == 0);
    EXPECT(gims_sinkhorn_backward(nullptr, 0, 1.f, 10, nullptr, nullptr, nullptr, nullptr, 0, nullptr) == GIMS_EINVAL);
    EXPECT(gims_sinkhorn_history(nullptr, 0, 1.f, 10, nullptr, nullptr, 0, nullptr) == GIMS_EINVAL);
  }
  {   // ---- fused Adam (round 3): table validation, and the multi-launch split of > 80 tensors
    gims_adam_group g; memset(&g, 0, sizeof(g));
    g.lr = 1e-3; g.beta1 = 0.9; g.beta2 = 0.999; g.eps = 1e-8; g.weight_decay = 0.0; g.step = 1;
    gims_adam_tensor t1; memset(&t1, 0, sizeof(t1));
    EXPECT(gims_adam_step(nullptr, 0, nullptr, 0, nullptr) == GIMS_OK);                 // nothing to do
    EXPECT(gims_adam_step(&t1, 1, &g, 9, nullptr) == GIMS_EINVAL);                      // more than 8 hyper-parameter sets
    t1.n = 16; t1.group = 0;
    EXPECT(gims_adam_step(&t1, 1, &g, 1, nullptr) == GIMS_EINVAL);                      // null tensor pointers
    t1.param = (float*)0x1000; t1.grad = (const float*)0x2000; t1.exp_avg = (float*)0x3000; t1.exp_avg_sq = (float*)0x4000; t1.group = 1;
    EXPECT(gims_adam_step(&t1, 1, &g, 1, nullptr) == GIMS_EINVAL);                      // group index out of range
    t1.group = 0; g.step = 0;
    EXPECT(gims_adam_step(&t1, 1, &g, 1, nullptr) == GIMS_EINVAL);                      // step counts from 1
    g.step = 3; g.beta2 = 1.0;
    EXPECT(gims_adam_step(&t1, 1, &g, 1, nullptr) == GIMS_EINVAL);                      // beta2 < 1
    g.beta2 = 0.999; t1.n = (int64_t)1 << 31;
    EXPECT(gims_adam_step(&t1, 1, &g, 1, nullptr) == GIMS_EINVAL);                      // element count beyond 2^31
    std::vector<gims_adam_tensor> many(300, t1);                                        // host-side chunking over 80-tensor launches; every launch
    for (size_t i = 0; i < many.size(); ++i) many[i].n = (i % 7 == 0) ? 0 : 5 + (int64_t)i;   // fails cleanly here (no device), empty tensors skipped
    const int rc_adam = gims_adam_step(many.data(), (int32_t)many.size(), &g, 1, nullptr);
    EXPECT(rc_adam == GIMS_OK || rc_adam == GIMS_EHIP);
  }
  {   // ---- the per-keypoint affine map on its own (round 3): empty input is a no-op, bad pointers are refused
    const int rc0 = gims_patch_affine(nullptr, nullptr, 0, nullptr, nullptr, nullptr);
    EXPECT(rc0 == GIMS_OK || rc0 == GIMS_EINVAL);
    EXPECT(gims_patch_affine(nullptr, nullptr, 5, nullptr, nullptr, nullptr) == GIMS_EINVAL);
  }
  {   // ---- workspace layouts (csrc/common.h: WsLayout): every layout routine in sizing mode (the queries, over ragged lists on and around a
      // 256-byte boundary) and in carving mode (the entry points with fake non-null pointers and an adequate work_bytes: every pointer is
      // computed, then the call fails cleanly in the runtime -- no device here), and the refusal of a workspace one byte short
    const int shp[5][2] = {{1, 2}, {63, 65}, {64, 64}, {257, 4097}, {700, 650}};
    char* const work = (char*)0x10000000;
    auto fake = [](uintptr_t v) { return (void*)v; };
    auto carved = [](int rc) { return rc == GIMS_EHIP || rc == GIMS_OK; };
    std::vector<gims_ot_problem> ot(5);
    std::vector<gims_eval_pair> ev(5);
    std::vector<gims_label_pair> lb(5);
    std::vector<gims_nn_pair> nn(5);
    std::vector<gims_agc_image> gi(5);
    std::vector<gims_agc_params> gp(5);
    std::vector<float*> hist(5, (float*)fake(0x70000)), dz(5, (float*)fake(0x80000));
    for (int i = 0; i < 5; ++i) {
      const int a = shp[i][0], b = shp[i][1];
      memset(&ot[i], 0, sizeof(ot[i])); memset(&ev[i], 0, sizeof(ev[i])); memset(&nn[i], 0, sizeof(nn[i])); memset(&gi[i], 0, sizeof(gi[i]));
      ot[i].scores = (const float*)fake(0x1000); ot[i].ld = (b + 3) / 4 * 4; ot[i].n = a; ot[i].m = b;
      ot[i].matches0 = (int64_t*)fake(0x2000); ot[i].matches1 = (int64_t*)fake(0x3000); ot[i].mscores0 = (float*)fake(0x4000);
      ot[i].mscores1 = (float*)fake(0x5000); ot[i].uv = (float*)fake(0x6000);
      ev[i].kpts0 = (const float*)fake(0x1000); ev[i].kpts1 = (const float*)fake(0x2000); ev[i].matches0 = (const int64_t*)fake(0x3000);
      ev[i].mscores0 = (const float*)fake(0x4000); ev[i].n0 = a; ev[i].n1 = b; ev[i].height = 480; ev[i].width = 640;
      ev[i].gt0 = (int32_t*)fake(0x5000); ev[i].inlier = (uint8_t*)fake(0x6000); ev[i].record = (float*)fake(0x7000); ev[i].homographies = (float*)fake(0x8000);
      lb[i].kpts0 = (const float*)fake(0x1000); lb[i].kpts1 = (const float*)fake(0x2000); lb[i].n0 = a; lb[i].n1 = b;
      nn[i].a = (const float*)fake(0x1000); nn[i].b = (const float*)fake(0x2000); nn[i].lda = nn[i].ldb = 64; nn[i].n0 = a + 1; nn[i].n1 = b; nn[i].d = 64;
      nn[i].mutual = i & 1; nn[i].threshold = 0.8f;
      nn[i].nn1 = nn[i].nn2 = (int32_t*)fake(0x3000); nn[i].d1 = nn[i].d2 = nn[i].ratio = nn[i].scores0 = (float*)fake(0x4000);
      nn[i].match = (uint8_t*)fake(0x5000); nn[i].matches0 = nn[i].matches1 = (int64_t*)fake(0x6000); nn[i].info = (int32_t*)fake(0x7000);
      gi[i].kpts = (const float*)fake(0x1000); gi[i].desc = (const float*)fake(0x2000); gi[i].ldd = 128; gi[i].n = a + 1; gi[i].d = 128;
      gi[i].kept = (int32_t*)fake(0x3000); gi[i].indptr = (int32_t*)fake(0x4000); gi[i].indices = (int32_t*)fake(0x5000); gi[i].max_edges_dir = 64 * (a + 1) + 7;
      gi[i].info = (int32_t*)fake(0x6000);
      gp[i].radius = 15.0; gp[i].percentile = 2.0; gp[i].min_size = 7; gp[i].reserved = 0;
    }
    size_t need;
    for (int it : {0, 1, 65, 3000}) {
      EXPECT((need = gims_eval_workspace_bytes(ev.data(), 5, it)) > 0 && need % 256 == 0);
      EXPECT(carved(gims_eval_pairs(ev.data(), 5, 3.f, 3, 3.f, it, 1, work, need, nullptr)));
      EXPECT(gims_eval_pairs(ev.data(), 5, 3.f, 3, 3.f, it, 1, work, need - 1, nullptr) == GIMS_EINVAL && strstr(gims_last_error(), "gims_eval_pairs"));
    }
    EXPECT((need = gims_train_labels_workspace_bytes(lb.data(), 5)) > 0 && need % 256 == 0);
    EXPECT(carved(gims_train_labels(lb.data(), 5, (const float*)fake(0x7000), 3.f, 3, (int64_t*)fake(0x8000), (int64_t*)fake(0x9000), work, need, nullptr)));
    EXPECT(gims_train_labels(lb.data(), 5, (const float*)fake(0x7000), 3.f, 3, (int64_t*)fake(0x8000), (int64_t*)fake(0x9000), work, need - 1, nullptr) == GIMS_EINVAL &&
           strstr(gims_last_error(), "gims_train_labels"));
    for (int np : {1, 5}) {
      EXPECT((need = gims_sinkhorn_workspace_bytes(ot.data(), np)) > 0 && need % 256 == 0);
      for (int flags : {0, (int)GIMS_OT_STREAMED}) EXPECT(carved(gims_sinkhorn_match(ot.data(), np, 1.f, 10, 0.2f, work, need, flags, nullptr)));
      EXPECT(gims_sinkhorn_match(ot.data(), np, 1.f, 10, 0.2f, work, need - 1, 0, nullptr) == GIMS_EINVAL && strstr(gims_last_error(), "gims_sinkhorn_match"));
      EXPECT(carved(gims_sinkhorn_history(ot.data(), np, 1.f, 3, hist.data(), work, need, nullptr)));
      EXPECT(gims_sinkhorn_history(ot.data(), np, 1.f, 3, hist.data(), work, need - 1, nullptr) == GIMS_EINVAL && strstr(gims_last_error(), "gims_sinkhorn_history"));
      EXPECT((need = gims_sinkhorn_backward_workspace_bytes(ot.data(), np)) > 0 && need % 256 == 0);
      for (int it : {3, 128, 129}) EXPECT(carved(gims_sinkhorn_backward(ot.data(), np, 1.f, it, hist.data(), dz.data(), (float*)fake(0x9000), work, need, nullptr)));
      EXPECT(gims_sinkhorn_backward(ot.data(), np, 1.f, 3, hist.data(), dz.data(), (float*)fake(0x9000), work, need - 1, nullptr) == GIMS_EINVAL &&
             strstr(gims_last_error(), "gims_sinkhorn_backward"));
    }
    {   // the on-chip Sinkhorn layout: several geometry classes in one list (sizing), then the carve of every class
      std::vector<gims::OtR2Host> h2;
      for (int i = 0; i < 5; ++i) {
        if (ot[i].m > 4096) continue;
        h2.push_back(gims::OtR2Host{ot[i].scores, ot[i].ld, ot[i].n, ot[i].m, ot[i].uv, ot[i].uv, ot[i].uv, -1.f, -1.f, -1.f});
      }
      h2.push_back(gims::OtR2Host{ot[0].scores, 2000, 2000, 1990, ot[0].uv, ot[0].uv, ot[0].uv, -1.f, -1.f, -1.f});
      const gims::OtR2Plan plan = gims::ot_res2_plan(h2.data(), (int)h2.size(), 10);
      EXPECT(plan.ok && plan.ngroups >= 3 && plan.bytes > 0 && plan.bytes % 256 == 0);
      EXPECT(gims::ot_res2_run(plan, h2.data(), (int)h2.size(), 1.f, 10, 1, work, nullptr) == GIMS_EHIP);
    }
    for (int flags : {0, (int)GIMS_AGC_ROBUST}) {
      EXPECT((need = gims_agc_workspace_bytes(gi.data(), 5, flags)) > 0 && need % 256 == 0);
      for (int n_params : {1, 5}) EXPECT(carved(gims_agc_build(gi.data(), 5, gp.data(), n_params, flags, work, need, nullptr)));
      EXPECT(gims_agc_build(gi.data(), 5, gp.data(), 5, flags, work, need - 1, nullptr) == GIMS_EINVAL && strstr(gims_last_error(), "gims_agc_build"));
    }
    for (int n_params : {0, 2, 6}) EXPECT(gims_agc_build(gi.data(), 5, gp.data(), n_params, 0, work, need, nullptr) == GIMS_EINVAL && strstr(gims_last_error(), "n_params"));
    EXPECT(gims_agc_build(gi.data(), 5, nullptr, 5, 0, work, need, nullptr) == GIMS_EINVAL && strstr(gims_last_error(), "n_params"));
    EXPECT((need = gims_delaunay_workspace_bytes(gi.data(), 5)) > 0 && need % 256 == 0);
    EXPECT(carved(gims_delaunay_build(gi.data(), 5, work, need, nullptr)));
    EXPECT(gims_delaunay_build(gi.data(), 5, work, need - 1, nullptr) == GIMS_EINVAL && strstr(gims_last_error(), "gims_delaunay_build"));
    for (int flags : {0, (int)GIMS_NN_EXHAUSTIVE}) {
      EXPECT((need = gims_nn_workspace_bytes(nn.data(), 5, flags)) > 0 && need % 256 == 0);
      EXPECT(carved(gims_nn_match(nn.data(), 5, flags, work, need, nullptr)));
      EXPECT(gims_nn_match(nn.data(), 5, flags, work, need - 1, nullptr) == GIMS_EINVAL && strstr(gims_last_error(), "gims_nn_match"));
    }
    {   // gims_aux_layout: the layout routines of the auxiliary functions with the recorder attached, counts only and with the offsets
      struct { int fn; std::vector<int64_t> sizes; } aux[] = {
          {GIMS_AUX_TRIANGULATE_TRACKS, {257, 1300}}, {GIMS_AUX_RESECT_IMAGES, {3, 1350, 65}}, {GIMS_AUX_BUNDLE_ADJUST, {257, 1300, 7, 20, 5}},
          {GIMS_AUX_BUNDLE_ADJUST_PCG, {257, 1300, 7, 20, 65536}}, {GIMS_AUX_BUNDLE_ADJUST_FOCAL, {257, 1300, 7, 20, 5, 3}}, {GIMS_AUX_DIOU_NMS, {700, 5}},
          {GIMS_AUX_BUILD_TRACKS, {3000000}}, {GIMS_AUX_SELECT_PAIRS, {96, 3, 33, 0, 64}}, {GIMS_AUX_GUIDED_MATCH, {0, 2, 257, 4097, 1, 700, 650, 0}},
          {GIMS_AUX_GUIDED_MATCH, {GIMS_NN_EXHAUSTIVE, 1, 1, 1, 1}}};
      for (auto& q : aux) {
        int32_t nr = 0, no = 0;
        size_t bytes = 0;
        EXPECT(gims_aux_layout(q.fn, q.sizes.data(), (int)q.sizes.size(), nullptr, 0, &nr, &no, &bytes) == GIMS_OK && nr > 0 && no <= nr && bytes % 256 == 0);
        std::vector<int64_t> off((size_t)nr);
        EXPECT(gims_aux_layout(q.fn, q.sizes.data(), (int)q.sizes.size(), off.data(), nr, &nr, &no, &bytes) == GIMS_OK && off[0] == 0 &&
               (size_t)off[(size_t)nr - 1] < bytes);
        EXPECT(gims_aux_layout(q.fn, q.sizes.data(), (int)q.sizes.size(), off.data(), nr - 1, &nr, &no, &bytes) == GIMS_EINVAL);
        EXPECT(gims_aux_layout(q.fn, q.sizes.data(), (int)q.sizes.size() - 1, nullptr, 0, &nr, &no, &bytes) == GIMS_EINVAL && strstr(gims_last_error(), "gims_aux_layout"));
      }
      int32_t nr = 0, no = 0;
      int64_t one = 1;
      EXPECT(gims_aux_layout(GIMS_AUX_SIFT_DESCRIBE, &one, 1, nullptr, 0, &nr, &no, &need) == GIMS_EINVAL && strstr(gims_last_error(), "gims_aux_layout"));
    }
  }
  // ---- a call that reaches the HIP runtime: no device in this container -> a clean GIMS_EHIP / error string, no crash
  char host_table[64] = {0};
  const int rc = gims_upload_table(host_table, sizeof(host_table), (void*)0x1000, nullptr);
  EXPECT(rc == GIMS_OK || rc == GIMS_EHIP || rc == GIMS_EINVAL);
  printf("asan host harness: %d checks passed\n", checks);
  return 0;
}
