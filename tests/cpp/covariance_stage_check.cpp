// covariance_stage_check.cpp -- the staging plan of hsm_covariance_batch (hector_slam_amd/csrc/stage_layout.h
// covariance_batch_stage) against its layout written out term by term, with the copies the plan asks for: poses, end points and
// (a CSR batch) offsets in, the four outputs out -- an output the caller does not ask for, and the offsets of a shared scan, are a
// region of no bytes that is copied neither way and takes no room.  Every case is compared exactly; prints one JSON line, exits 1
// on a mismatch.
#include <stdio.h>

#include "stage_layout.h"

using namespace hsm_host;

static size_t al(size_t x) { return (x + 255) & ~(size_t)255; }
static long long cases = 0, mismatches = 0;

static void same(size_t got, size_t want, const char* what, int batch, size_t total, int mask) {
  ++cases;
  if (got == want) return;
  if (++mismatches <= 20) fprintf(stderr, "%s (%d, %zu, mask %d): %zu, written out %zu\n", what, batch, total, mask, got, want);
}

// mask: bit 0 CSR offsets, bits 1 .. 4 the outputs cov_world, cov_map, lh7, likelihood
static void check(int batch, size_t total, int mask) {
  static float poses, pts, cw, cm, l7, lh;  // (addresses only)
  static int offs;
  const int* o = (mask & 1) ? &offs : nullptr;
  float* out[4] = {(mask & 2) ? &cw : nullptr, (mask & 4) ? &cm : nullptr, (mask & 8) ? &l7 : nullptr, (mask & 16) ? &lh : nullptr};
  const CovarianceBatchStage s = covariance_batch_stage(batch, total, &poses, &pts, o, out[0], out[1], out[2], out[3]);
  const size_t b = (size_t)batch * sizeof(float);
  const size_t bytes[7] = {3 * b, total * 2 * sizeof(float), o ? ((size_t)batch + 1) * sizeof(int) : 0,
                           out[0] ? 9 * b : 0, out[1] ? 9 * b : 0, out[2] ? 7 * b : 0, out[3] ? b : 0};
  size_t off[8];
  off[0] = 0;
  for (int i = 0; i < 7; ++i) off[i + 1] = off[i] + al(bytes[i]);
  const size_t got[7] = {s.poses, s.pts, s.offs, s.cov_world, s.cov_map, s.lh7, s.lh};
  const char* names[7] = {"poses", "pts", "offs", "cov_world", "cov_map", "lh7", "lh"};
  for (int i = 0; i < 7; ++i) same(got[i], off[i], names[i], batch, total, mask);
  same(s.plan.total(), off[7], "total", batch, total, mask);
  same((size_t)s.plan.n, 7, "regions", batch, total, mask);
  const void* src[7] = {&poses, &pts, o, nullptr, nullptr, nullptr, nullptr};
  const void* dst[7] = {nullptr, nullptr, nullptr, out[0], out[1], out[2], out[3]};
  for (int i = 0; i < 7 && i < s.plan.n; ++i) {
    same(s.plan.r[i].off, off[i], "region offset", batch, total, mask);
    same(s.plan.r[i].bytes, bytes[i], "region bytes", batch, total, mask);
    same(s.plan.r[i].src == src[i], 1, "region source", batch, total, mask);
    same(s.plan.r[i].dst == dst[i], 1, "region destination", batch, total, mask);
  }
  // every region starts on a 256-byte boundary and none overlaps the next
  for (int i = 0; i + 1 < s.plan.n; ++i) {
    same(s.plan.r[i].off % 256, 0, "alignment", batch, total, mask);
    same(s.plan.r[i].off + s.plan.r[i].bytes <= s.plan.r[i + 1].off, 1, "no overlap", batch, total, mask);
  }
}

int main() {
  const int batches[] = {1, 2, 3, 7, 21, 22, 37, 64, 85, 4096};  // 64 x 4 B, 21 x 3 x 4 B + 4: either side of a 256-byte multiple
  const size_t totals[] = {0, 1, 31, 32, 33, 181, 1081, (size_t)4096 * 1081};
  for (int b : batches)
    for (size_t t : totals)
      for (int mask = 2; mask < 32; ++mask)
        if (mask & 30) check(b, t, mask);
  printf("{\"cases\": %lld, \"mismatches\": %lld}\n", cases, mismatches);
  return mismatches ? 1 : 0;
}
