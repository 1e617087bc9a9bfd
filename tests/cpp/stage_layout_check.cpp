// stage_layout_check.cpp -- hector_slam_amd/csrc/stage_layout.h against the sums the host runtime wrote out by hand before
// the header existed: the workspace of hsm_match_batch_ranges_device, the staging blocks of hsm_match_batch /
// hsm_match_score_batch (device and pinned form; with and without score, residual, ranking and its optional arrays) and the
// growth rule of every grow-on-demand buffer.  Every case is compared exactly; prints one JSON line, exits 1 on a mismatch.
#include <stdio.h>

#include <vector>

#include "stage_layout.h"

using namespace hsm_host;

static size_t al(size_t x) { return (x + 255) & ~(size_t)255; }
static long long cases = 0, mismatches = 0;

static void same(size_t got, size_t want, const char* what, long long a, long long b, long long c) {
  ++cases;
  if (got == want) return;
  if (++mismatches <= 20) fprintf(stderr, "%s (%lld, %lld, %lld): %zu, written out %zu\n", what, a, b, c, got, want);
}

static void check_ranges(int batch, int n) {
  const bool refused = batch < 0 || n < 0 || n > HSM_MAX_UPDATE_BEAMS || (size_t)batch * (size_t)n > (size_t)INT_MAX;
  RangesLayout L;
  const bool ok = ranges_layout(batch, n, &L);
  same(ok, !refused, "ranges_layout accepts", batch, n, 0);
  if (refused || !ok) return;
  const size_t bn = (size_t)batch * (size_t)n;
  const size_t counts = 0;
  const size_t offsets = counts + al((size_t)batch * sizeof(int));
  const size_t copy = offsets + al(((size_t)batch + 1) * sizeof(int));
  const size_t pts = copy + al(bn * sizeof(float));
  const size_t total = pts + al((bn > 0 ? bn : 1) * 2 * sizeof(float));
  same(L.counts, counts, "ranges counts", batch, n, 0);
  same(L.offsets, offsets, "ranges offsets", batch, n, 0);
  same(L.copy, copy, "ranges copy", batch, n, 0);
  same(L.pts, pts, "ranges pts", batch, n, 0);
  same(L.total, total, "ranges total", batch, n, 0);
}

// flags: 1 score, 2 residual, 4 ranking, 8 group offsets, 16 winner score, 32 winner pose, 64 CSR offsets (device form only)
static void check_batch(size_t batch, size_t total_pts, size_t G, int flags, bool pinned) {
  const bool sr = flags & 1;
  if (!sr) G = 0;
  if (!(flags & 4)) G = 0;
  const size_t b_begin = batch * 3 * sizeof(float);
  const size_t b_pts = total_pts * 2 * sizeof(float);
  const size_t b_offs = (flags & 64) && !pinned ? (batch + 1) * sizeof(int) : 0;
  const size_t b_pose = b_begin, b_cov = batch * 9 * sizeof(float);
  const size_t b_lh = sr ? batch * sizeof(float) : 0, b_res = sr && (flags & 2) ? b_lh : 0;
  const size_t b_goffs = G > 0 && (flags & 8) ? (G + 1) * sizeof(int) : 0;
  const size_t b_idx = G * sizeof(int), b_bscore = G > 0 && (flags & 16) ? G * sizeof(float) : 0;
  const size_t b_bpose = G > 0 && (flags & 32) ? G * 3 * sizeof(float) : 0;
  const size_t o_res = al(b_lh), o_goffs = o_res + al(b_res), o_idx = o_goffs + al(b_goffs), o_bscore = o_idx + al(b_idx);
  const size_t o_bpose = o_bscore + al(b_bscore), b_extra = o_bpose + al(b_bpose);
  size_t pts, offs = 0, pose, cov, x, total;
  if (pinned) {
    pose = al(b_begin);
    cov = al(b_begin) + al(b_pose);
    pts = al(b_begin) + al(b_pose) + al(b_cov);
    x = al(b_begin) + al(b_pose) + al(b_cov) + al(b_pts);
    total = x + b_extra;
  } else {
    pts = al(b_begin);
    offs = al(b_begin) + al(b_pts);
    pose = al(b_begin) + al(b_pts) + al(b_offs);
    cov = al(b_begin) + al(b_pts) + al(b_offs) + al(b_pose);
    x = al(b_begin) + al(b_pts) + al(b_offs) + al(b_pose) + al(b_cov);
    total = al(b_begin) + al(b_pts) + al(b_offs) + al(b_pose) + al(b_cov) + b_extra;
  }
  BatchBytes b = {b_begin, b_pts, b_offs, b_cov, b_lh, b_res, b_goffs, b_idx, b_bscore, b_bpose};
  const BatchLayout L = batch_layout(b, pinned);
  const long long key = flags + (pinned ? 1000 : 0);
  same(L.pts, pts, "batch pts", batch, total_pts, key);
  if (!pinned) same(L.offs, offs, "batch offs", batch, total_pts, key);
  same(L.pose, pose, "batch pose", batch, total_pts, key);
  same(L.cov, cov, "batch cov", batch, total_pts, key);
  same(L.lh, x, "batch likelihood", batch, total_pts, key);
  same(L.res, x + o_res, "batch residual", batch, total_pts, key);
  same(L.goffs, x + o_goffs, "batch group offsets", batch, total_pts, key);
  same(L.idx, x + o_idx, "batch winner index", batch, total_pts, key);
  same(L.bscore, x + o_bscore, "batch winner score", batch, total_pts, key);
  same(L.bpose, x + o_bpose, "batch winner pose", batch, total_pts, key);
  same(L.total, total, "batch total", batch, total_pts, key);
}

static void check_growth(size_t n) {
  // exact: d_batch, d_rbatch, d_occ, the speculative-carry scratch, the group blocks
  same(grown_capacity(n, kExact), n, "exact", n, 0, 0);
  // +50 %: h_copy_pinned, h_hyp_pinned, d_upd_stage, d_cells, d_beam_recs
  same(grown_capacity(n, kHalfMore), n + n / 2, "+50 %", n, 0, 0);
  // +50 %, floor 4096 elements: d_scan, d_retained, d_retained_alt, h_scan_pinned, h_upd_pinned
  same(grown_capacity(n, kScanGrowth), n < 4096 ? 4096 : n + n / 2, "+50 % floor 4096", n, 0, 0);
  // floor 2048: the ingest trio;  floor 64: d_upd_batches
  same(grown_capacity(n, {2048, 50}), n < 2048 ? 2048 : n + n / 2, "floor 2048", n, 0, 0);
  same(grown_capacity(n, {64, 50}), n < 64 ? 64 : n + n / 2, "floor 64", n, 0, 0);
  // multiples of 4096 ints (the permutation buffers): the caller rounds, the buffer allocates exactly that
  same(grown_capacity((n + 4095) / 4096 * 4096, kExact), (n + 4095) / 4096 * 4096, "multiples of 4096", n, 0, 0);
}

int main() {
  // sizes around the 256-byte multiples of every element size in play (4, 8, 12, 36 bytes), and the ends of the ranges
  std::vector<long long> sizes = {0, 1, 2, 3, 5, 7, 21, 22, 31, 32, 33, 63, 64, 65, 85, 86, 127, 128, 129, 255, 256, 257, 1023, 1024,
                                  1025, 1081, 2047, 2048, 2049, 4095, 4096, 4097, 6143, 6144, 16384, 65535, 65536, 65537, 1048575};
  for (long long v = 1; v <= 40; ++v)  // one byte either side of a multiple for 4-byte elements needs every count near 64 k
    for (long long d = -1; d <= 1; ++d) sizes.push_back(64 * v + d);
  for (long long s : sizes) {
    same(stage_align((size_t)s), al((size_t)s), "round-up", s, 0, 0);
    for (long long d = -1; d <= 1; ++d) {  // one byte either side of a 256-byte multiple, as a size and as a carved region
      const size_t bytes = (size_t)(256 * (s + 1) + d);
      same(stage_align(bytes), al(bytes), "round-up", s, d, 0);
      Carver c;
      same(c.take(bytes), 0, "carver first", s, d, 0);
      same(c.take((size_t)s), al(bytes), "carver second", s, d, 0);
      same(c.take(1), al(bytes) + al((size_t)s), "carver third", s, d, 0);
      same(c.total(), al(bytes) + al((size_t)s) + al(1), "carver total", s, d, 0);
    }
    check_growth((size_t)s);
  }
  // the public workspace size: every pair of the grid, n up to HSM_MAX_UPDATE_BEAMS and one beyond, refused products, negatives
  std::vector<long long> ns = sizes;
  for (long long v : {(long long)HSM_MAX_UPDATE_BEAMS - 1, (long long)HSM_MAX_UPDATE_BEAMS, (long long)HSM_MAX_UPDATE_BEAMS + 1, -1LL})
    ns.push_back(v);
  std::vector<long long> batches = sizes;
  for (long long v : {-1LL, 2047LL, 2048LL, 2049LL, (long long)INT_MAX / HSM_MAX_UPDATE_BEAMS, (long long)INT_MAX / HSM_MAX_UPDATE_BEAMS + 1,
                      (long long)INT_MAX - 1, (long long)INT_MAX})
    batches.push_back(v);
  for (long long bt : batches)
    for (long long n : ns) check_ranges((int)bt, (int)n);
  check_ranges(INT_MAX, 1);  // the largest product the entry accepts, and the first it refuses
  check_ranges(46341, 46341);
  check_ranges(2048, HSM_MAX_UPDATE_BEAMS);
  check_ranges(2049, HSM_MAX_UPDATE_BEAMS);
  // the host batch blocks
  for (long long bt : sizes)
    for (long long pts : {0LL, 1LL, 31LL, 32LL, 33LL, 1081LL, (long long)HSM_MAX_UPDATE_BEAMS, bt * 181})
      for (long long G : {0LL, 1LL, 63LL, 64LL, 65LL, bt})
        for (int flags = 0; flags < 128; ++flags) {
          check_batch((size_t)bt, (size_t)pts, (size_t)G, flags, false);
          if (!(flags & 64)) check_batch((size_t)bt, (size_t)pts, (size_t)G, flags, true);
        }
  printf("{\"cases\": %lld, \"mismatches\": %lld}\n", cases, mismatches);
  return mismatches ? 1 : 0;
}
