// stage_layout.h -- the arithmetic of the host runtime's staging blocks: how much a grow-on-demand buffer allocates and where the
// 256-byte aligned regions of one allocation start.  Plain C++ (no HIP header): tests/cpp/stage_layout_check.cpp compiles it with
// the host compiler and holds it to the written-out sums (tests/test_stage_layout.py).
#pragma once
#include <limits.h>
#include <stddef.h>

#include "hector_mi355/capi.h"

namespace hsm_host {

constexpr size_t stage_align(size_t x) { return (x + 255) & ~(size_t)255; }

// regions of one allocation, in order: take(bytes) is the offset of the next one
struct Carver {
  size_t off = 0;
  size_t take(size_t bytes) {
    const size_t o = off;
    off += stage_align(bytes);
    return o;
  }
  size_t total() const { return off; }
};

// what a buffer allocates when it has to grow to `need` (any unit): `floor` for a smaller need, else need + slack_pct %
struct Growth {
  size_t floor;
  unsigned slack_pct;
};
constexpr Growth kExact = {0, 0}, kHalfMore = {0, 50}, kScanGrowth = {4096, 50};
constexpr size_t grown_capacity(size_t need, Growth g) { return need < g.floor ? g.floor : need + need * g.slack_pct / 100; }

// workspace of hsm_match_batch_ranges_device, byte offsets: counts[B] | offsets[B + 1] | copy of the ranges[B * n] |
// endpoints[max(B * n, 1)].  The endpoint region keeps one element when every scan is empty: the matcher clamps an empty scan's
// loads to element 0 (gn_match_exact.h).  false = sizes the entry refuses.
struct RangesLayout {
  size_t counts, offsets, copy, pts, total;
};

inline bool ranges_layout(int batch, int n, RangesLayout* L) {
  if (batch < 0 || n < 0 || n > HSM_MAX_UPDATE_BEAMS || (size_t)batch * (size_t)n > (size_t)INT_MAX) return false;
  const size_t bn = (size_t)batch * (size_t)n;
  Carver c;
  L->counts = c.take((size_t)batch * sizeof(int));
  L->offsets = c.take(((size_t)batch + 1) * sizeof(int));
  L->copy = c.take(bn * sizeof(float));
  L->pts = c.take((bn > 0 ? bn : 1) * 2 * sizeof(float));
  L->total = c.total();
  return true;
}

// workspace of hsm_slam_ranges_tf_device, byte offsets: counts[count] | offsets[count + 1] | origos[count * 2] |
// endpoints[max(count * n, 1)] -- the outputs of the tf conversion, which the scan loop reads where they lie.  false = sizes the
// entry refuses (those of the conversion).
struct SlamRangesTfLayout {
  size_t counts, offsets, origos, pts, total;
};

inline bool slam_ranges_tf_layout(int count, int n, SlamRangesTfLayout* L) {
  if (count < 0 || n < 0 || n > HSM_MAX_UPDATE_BEAMS || (size_t)count * (size_t)n > (size_t)INT_MAX) return false;
  const size_t cn = (size_t)count * (size_t)n;
  Carver c;
  L->counts = c.take((size_t)count * sizeof(int));
  L->offsets = c.take(((size_t)count + 1) * sizeof(int));
  L->origos = c.take((size_t)count * 2 * sizeof(float));
  L->pts = c.take((cn > 0 ? cn : 1) * 2 * sizeof(float));
  L->total = c.total();
  return true;
}

// staging block of hsm_match_batch / hsm_match_score_batch.  Sizes in bytes, 0 for an array the call does not have (pose = begin).
struct BatchBytes {
  size_t begin, pts, offs, cov;
  size_t lh, res, goffs, idx, bscore, bpose;  // the score's and the ranking's arrays
};
// byte offsets; the start poses are at 0.  device block: begin | pts | offs | pose | cov, pinned block of the shared-scan form:
// begin | pose | cov | pts; behind either: likelihood | residual | group offsets | winner index | winner score | winner pose
struct BatchLayout {
  size_t pts, offs, pose, cov, lh, res, goffs, idx, bscore, bpose, total;
};

inline BatchLayout batch_layout(const BatchBytes& b, bool pinned) {
  Carver c;
  BatchLayout L;
  c.take(b.begin);
  if (!pinned) L.pts = c.take(b.pts), L.offs = c.take(b.offs);
  L.pose = c.take(b.begin);
  L.cov = c.take(b.cov);
  if (pinned) L.pts = c.take(b.pts), L.offs = c.take(b.offs);
  L.lh = c.take(b.lh);
  L.res = c.take(b.res);
  L.goffs = c.take(b.goffs);
  L.idx = c.take(b.idx);
  L.bscore = c.take(b.bscore);
  L.bpose = c.take(b.bpose);
  L.total = c.total();
  return L;
}

}  // namespace hsm_host
