// Host-side AddressSanitizer harness for GIMS_AUX_BUILD_TRACKS (gims_amd/csrc/tracks.hip), in the manner of host_paths.cpp: CPU container only.
// The op's host code -- the argument checks, the workspace layout arithmetic, the dispatch in gims_run_ops -- is driven through every call
// that returns before the first HIP call (GIMS_EINVAL); the pointers are fake and never dereferenced.    Build + run: tools/asan/run.sh
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/gims_hip.h"

static int checks = 0;
#define EXPECT(cond) do { ++checks; if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s  (last error: %s)\n", __FILE__, __LINE__, #cond, gims_last_error()); exit(1); } } while (0)

static size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
static size_t work_bytes(size_t n) {          // the header's formula
  const size_t h = n / 1024 > GIMS_TRACKS_LONG_SEGMENT ? n / 1024 : GIMS_TRACKS_LONG_SEGMENT;
  return 12 * al256(4 * n) + al256(4 * (n / GIMS_TRACKS_SCAN_TILE + 2)) + al256(4 * (n / (h + 1) + 1) * (n / GIMS_TRACKS_SCAN_TILE + 1)) + 256;
}

static gims_op good(int64_t n) {
  gims_op o;
  memset(&o, 0, sizeof(o));
  o.kind = GIMS_OP_AUX;
  o.u.aux.fn = GIMS_AUX_BUILD_TRACKS;
  for (int k = 0; k < 6; ++k) o.u.aux.p[k] = (const void*)(uintptr_t)(0x10000 * (k + 1));
  o.u.aux.i[0] = 3; o.u.aux.i[1] = 4; o.u.aux.i[2] = n; o.u.aux.i[3] = 2; o.u.aux.i[4] = (int64_t)work_bytes((size_t)n);
  return o;
}

static void refused(gims_op o, const char* word) {
  EXPECT(gims_run_ops(&o, 1, nullptr) == GIMS_EINVAL);
  EXPECT(strstr(gims_last_error(), "build_tracks") != nullptr);
  EXPECT(strstr(gims_last_error(), word) != nullptr);
}

int main() {
  EXPECT(gims_abi_version() == GIMS_ABI_VERSION);
  for (int64_t n : {(int64_t)1, (int64_t)12, (int64_t)2049, (int64_t)204800, (int64_t)2000000, (int64_t)1 << 30}) {
    gims_op o = good(n);
    o.u.aux.i[4] -= 1;                        // one byte below the formula is refused, so the library computes the same number
    refused(o, "work_bytes");
    o = good(n); o.u.aux.p[4] = (const void*)(uintptr_t)0x50002;          // ... and with the full size the next check is reached
    refused(o, "4-byte aligned");
  }
  gims_op o = good(5000);
  o.u.aux.i[0] = -1; refused(o, "n_pairs");
  o = good(5000); o.u.aux.i[1] = 0; refused(o, "n_images");
  o = good(5000); o.u.aux.i[2] = ((int64_t)1 << 30) + 1; refused(o, "N = ");
  o = good(5000); o.u.aux.i[3] = 1; refused(o, "min_length");
  o = good(5000); o.u.aux.i[3] = 2 | ((int64_t)1 << 40); refused(o, "min_length");
  o = good(5000); o.u.aux.i[3] = 2 | GIMS_TRACKS_KEEP_CONFLICTING; o.u.aux.p[5] = nullptr; refused(o, "workspace is NULL");
  o = good(5000); o.u.aux.f[0] = NAN; refused(o, "NaN");
  o = good(5000); o.u.aux.p[0] = nullptr; refused(o, "pair table is NULL");
  o = good(5000); o.u.aux.p[0] = (const void*)(uintptr_t)0x10004; refused(o, "8-byte aligned");
  o = good(5000); o.u.aux.p[5] = (const void*)(uintptr_t)0x60008; refused(o, "16-byte aligned");
  o = good(5000); o.u.aux.i[5] = 7; refused(o, "unknown auxiliary function form");
  o = good(0); o.u.aux.p[2] = nullptr; o.u.aux.p[5] = nullptr; o.u.aux.i[4] = 0; o.u.aux.p[3] = nullptr; refused(o, "NULL");
  printf("tracks_paths: %d checks passed\n", checks);
  return 0;
}
