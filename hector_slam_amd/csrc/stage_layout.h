// stage_layout.h -- the arithmetic of the host runtime's staging blocks: how much a grow-on-demand buffer allocates and where the
// 256-byte aligned regions of one allocation start.  Plain C++ (no HIP header): tests/cpp/stage_layout_check.cpp compiles it with
// the host compiler and holds it to the written-out sums (tests/test_stage_layout.py).
#pragma once
#include <assert.h>
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

// The staging block of a host-array entry: its regions in the order they are carved, each with the host array that is copied
// into it before the launches (src), the host array that receives it after them (dst), both (an in/out array) or neither (device
// scratch).  A null array or an empty region is not copied; the copies are queued in the order of the list (hsm_ctx.h stage_copy_in /
// stage_copy_out).
struct StageRegion {
  size_t off, bytes;
  const void* src;
  void* dst;
};

struct StagePlan {
  static constexpr int kMaxRegions = 12;
  StageRegion r[kMaxRegions];
  int n = 0;
  Carver c;
  size_t add(size_t bytes, const void* src = nullptr, void* dst = nullptr) { return view(c.take(bytes), bytes, src, dst); }
  // a copy into or out of part of a region carved before: it takes no room
  size_t view(size_t off, size_t bytes, const void* src, void* dst) {
    assert(n < kMaxRegions);
    r[n++] = {off, bytes, src, dst};
    return off;
  }
  size_t total() const { return c.total(); }
};

// hsm_update_by_scans (d_upd_stage): end points[total_pts] | poses[count * 3] | offsets[count + 1]
struct UpdateScansStage {
  StagePlan plan;
  size_t pts, poses, offs;
};

inline UpdateScansStage update_scans_stage(int count, size_t total_pts, const float* poses, const float* pts, const int* offsets) {
  UpdateScansStage s;
  s.pts = s.plan.add(total_pts * 2 * sizeof(float), pts);
  s.poses = s.plan.add((size_t)count * 3 * sizeof(float), poses);
  s.offs = s.plan.add(((size_t)count + 1) * sizeof(int), offsets);
  return s;
}

// hsm_match_batch / hsm_match_score_batch.  A CSR batch (d_batch): start poses | end points | offsets | poses | covariances; the
// pinned, device-mapped block of the shared-scan form (h_hyp_pinned), whose end points alone are copied on: start poses | poses |
// covariances | end points; behind either: likelihood | residual | group offsets | winner index | winner score | winner pose.
// The covariances (carved with or without the caller's array) and the winner poses go in and out: an empty scan and a group
// without a winner leave the caller's.  The score's and the ranking's arrays the call does not have are not carved.
struct MatchBatchStage {
  StagePlan plan;
  size_t begin, pts, offs, pose, cov, lh, res, goffs, idx, bscore, bpose;
};

inline MatchBatchStage match_batch_stage(int batch, size_t total_pts, int groups, bool pinned, const float* begin, const float* pts,
                                         const int* offsets, float* out_pose, float* out_cov, float* out_lh, float* out_res,
                                         const int* group_offsets, int* out_index, float* out_score, float* out_best_pose) {
  const size_t b = (size_t)batch * sizeof(float), g = (size_t)groups;
  MatchBatchStage s;
  const auto scan = [&] {
    s.pts = s.plan.add(total_pts * 2 * sizeof(float), pts);
    s.offs = s.plan.add(offsets ? ((size_t)batch + 1) * sizeof(int) : 0, offsets);
  };
  s.begin = s.plan.add(3 * b, begin);
  if (!pinned) scan();
  s.pose = s.plan.add(3 * b, nullptr, out_pose);
  s.cov = s.plan.add(9 * b, out_cov, out_cov);
  if (pinned) scan();
  s.lh = s.plan.add(out_lh ? b : 0, nullptr, out_lh);
  s.res = s.plan.add(out_res ? b : 0, nullptr, out_res);
  s.goffs = s.plan.add(g && group_offsets ? (g + 1) * sizeof(int) : 0, group_offsets);
  s.idx = s.plan.add(g * sizeof(int), nullptr, out_index);
  s.bscore = s.plan.add(out_score ? g * sizeof(float) : 0, nullptr, out_score);
  s.bpose = s.plan.add(out_best_pose ? g * 3 * sizeof(float) : 0, out_best_pose, out_best_pose);
  return s;
}

// hsm_match_batch_ranges (d_rbatch): start poses | poses | covariances | counts | raw ranges | the device call's workspace.
// The covariances go in and out: the matcher leaves an empty scan's as it was.
struct RangesStage {
  StagePlan plan;
  size_t begin, pose, cov, counts, ranges, ws;
};

inline RangesStage ranges_stage(int batch, int n, size_t ws_bytes, const float* begin, const float* ranges, float* out_pose,
                                float* out_cov, int* out_counts) {
  const size_t b3 = (size_t)batch * 3 * sizeof(float);
  RangesStage s;
  s.begin = s.plan.add(b3, begin);
  s.pose = s.plan.add(b3, nullptr, out_pose);
  s.cov = s.plan.add((size_t)batch * 9 * sizeof(float), nullptr, out_cov);
  s.counts = s.plan.add((size_t)batch * sizeof(int), nullptr, out_counts);
  s.ranges = s.plan.add((size_t)batch * (size_t)n * sizeof(float), ranges);
  s.ws = s.plan.add(ws_bytes);
  s.plan.view(s.cov, (size_t)batch * 9 * sizeof(float), out_cov, nullptr);  // (in as well, behind the other copies in)
  return s;
}

// hsm_likelihood_states / hsm_residual_states (d_batch): end points[n] | states[batch * 3] | likelihoods[batch] | residuals[batch]
struct ScoreStatesStage {
  StagePlan plan;
  size_t pts, states, lh, res;
};

inline ScoreStatesStage score_states_stage(int batch, int n, const float* states, const float* pts, float* out_lh, float* out_res) {
  ScoreStatesStage s;
  s.pts = s.plan.add((size_t)n * 2 * sizeof(float), pts);
  s.states = s.plan.add((size_t)batch * 3 * sizeof(float), states);
  s.lh = s.plan.add((size_t)batch * sizeof(float), nullptr, out_lh);
  s.res = s.plan.add((size_t)batch * sizeof(float), nullptr, out_res);
  return s;
}

// hsm_covariance_for_poses (d_batch): end points[n] | poses[batch * 3] | map-frame covariances[batch * 9] | world-frame
// covariances[batch * 9] | the seven sigma-point likelihoods[batch * 7]
struct PoseCovarianceStage {
  StagePlan plan;
  size_t pts, poses, cov_map, cov_world, lh7;
};

inline PoseCovarianceStage pose_covariance_stage(int batch, int n, const float* poses, const float* pts, float* out_cov_map,
                                                 float* out_cov_world, float* out_lh7) {
  PoseCovarianceStage s;
  s.pts = s.plan.add((size_t)n * 2 * sizeof(float), pts);
  s.poses = s.plan.add((size_t)batch * 3 * sizeof(float), poses);
  s.cov_map = s.plan.add((size_t)batch * 9 * sizeof(float), nullptr, out_cov_map);
  s.cov_world = s.plan.add((size_t)batch * 9 * sizeof(float), nullptr, out_cov_world);
  s.lh7 = s.plan.add((size_t)batch * 7 * sizeof(float), nullptr, out_lh7);
  return s;
}

// hsm_covariance_batch (d_batch): world poses[batch * 3] | end points[total_pts] | offsets[batch + 1] (a CSR batch; not carved
// for a shared scan) | world-frame covariances[batch * 9] | map-frame covariances[batch * 9] | the seven sigma-point
// likelihoods[batch * 7] | the pose's likelihood[batch].  An output the caller does not ask for is not carved: the kernel gets none.
struct CovarianceBatchStage {
  StagePlan plan;
  size_t poses, pts, offs, cov_world, cov_map, lh7, lh;
};

inline CovarianceBatchStage covariance_batch_stage(int batch, size_t total_pts, const float* poses, const float* pts,
                                                   const int* offsets, float* out_cov_world, float* out_cov_map, float* out_lh7,
                                                   float* out_lh) {
  const size_t b = (size_t)batch * sizeof(float);
  CovarianceBatchStage s;
  s.poses = s.plan.add(3 * b, poses);
  s.pts = s.plan.add(total_pts * 2 * sizeof(float), pts);
  s.offs = s.plan.add(offsets ? ((size_t)batch + 1) * sizeof(int) : 0, offsets);
  s.cov_world = s.plan.add(out_cov_world ? 9 * b : 0, nullptr, out_cov_world);
  s.cov_map = s.plan.add(out_cov_map ? 9 * b : 0, nullptr, out_cov_map);
  s.lh7 = s.plan.add(out_lh7 ? 7 * b : 0, nullptr, out_lh7);
  s.lh = s.plan.add(out_lh ? b : 0, nullptr, out_lh);
  return s;
}

// hsm_ray_distances (d_batch): ray begins[n * 2] | ray ends[n * 2] | distances[n] | hit points[n * 2].  The hit points go in and
// out: a ray without a hit leaves the caller's values.
struct RayDistancesStage {
  StagePlan plan;
  size_t begin, end, dist, hit;
};

inline RayDistancesStage ray_distances_stage(int n, const float* begin, const float* end, float* out_dist, float* out_hit) {
  const size_t n2 = (size_t)n * 2 * sizeof(float);
  RayDistancesStage s;
  s.begin = s.plan.add(n2, begin);
  s.end = s.plan.add(n2, end);
  s.dist = s.plan.add((size_t)n * sizeof(float), nullptr, out_dist);
  s.hit = s.plan.add(n2, out_hit, out_hit);
  return s;
}

// hsm_cast_scans (d_batch): sensor poses[batch * 3] | beam angles[n] | ranges[batch * n] | hit points[batch * n * 2].  The hit
// points go in and out like hsm_ray_distances's; without the caller's array the region is not carved and the kernel gets none.
struct CastScansStage {
  StagePlan plan;
  size_t poses, angles, ranges, hit;
};

inline CastScansStage cast_scans_stage(int batch, int n, const float* poses, const float* angles, float* out_ranges, float* out_hit) {
  const size_t bn = (size_t)batch * (size_t)n;
  CastScansStage s;
  s.poses = s.plan.add((size_t)batch * 3 * sizeof(float), poses);
  s.angles = s.plan.add((size_t)n * sizeof(float), angles);
  s.ranges = s.plan.add(bn * sizeof(float), nullptr, out_ranges);
  s.hit = s.plan.add(out_hit ? bn * 2 * sizeof(float) : 0, out_hit, out_hit);
  return s;
}

// hsm_match_batch_ranges_tf (d_rbatch): transforms[batch or 1][12] | start poses | poses | covariances | counts | origos |
// offsets[batch + 1] | raw ranges | endpoints[max(batch * n, 1)]
struct RangesTfStage {
  StagePlan plan;
  size_t tf, begin, pose, cov, counts, origo, offs, ranges, pts;
};

inline RangesTfStage ranges_tf_stage(int batch, int n, bool shared_tf, const double* tf_rows, const float* begin,
                                     const float* ranges, float* out_pose, float* out_cov, int* out_counts, float* out_origo) {
  const size_t bn = (size_t)batch * (size_t)n, b3 = (size_t)batch * 3 * sizeof(float), b_int = (size_t)batch * sizeof(int);
  RangesTfStage s;
  s.tf = s.plan.add((shared_tf ? 1 : (size_t)batch) * 12 * sizeof(double), tf_rows);
  s.begin = s.plan.add(b3, begin);
  s.pose = s.plan.add(b3, nullptr, out_pose);
  s.cov = s.plan.add((size_t)batch * 9 * sizeof(float), nullptr, out_cov);
  s.counts = s.plan.add(b_int, nullptr, out_counts);
  s.origo = s.plan.add((size_t)batch * 2 * sizeof(float), nullptr, out_origo);
  s.offs = s.plan.add(b_int + sizeof(int));
  s.ranges = s.plan.add(bn * sizeof(float), ranges);
  s.pts = s.plan.add((bn > 0 ? bn : 1) * 2 * sizeof(float));
  s.plan.view(s.cov, (size_t)batch * 9 * sizeof(float), out_cov, nullptr);  // (in as well, behind the other copies in)
  return s;
}

// hsm_slam_ranges_tf (d_rbatch): transforms[count or 1][12] | start pose | hint deltas | force | poses | covariances | applied |
// counts | raw ranges | the device call's workspace `L`, whose origos are copied out where they lie
struct SlamRangesTfStage {
  StagePlan plan;
  size_t tf, start, deltas, force, pose, cov, applied, counts, ranges, ws;
};

inline SlamRangesTfStage slam_ranges_tf_stage(int count, int n, bool shared_tf, const SlamRangesTfLayout& L, const double* tf_rows,
                                              const float* start_pose, const float* hint_deltas, const unsigned char* force,
                                              const float* ranges, float* out_pose, float* out_cov, int* out_applied,
                                              int* out_counts, float* out_origo) {
  const size_t b3 = (size_t)count * 3 * sizeof(float), b_int = (size_t)count * sizeof(int);
  SlamRangesTfStage s;
  s.tf = s.plan.add((shared_tf ? 1 : (size_t)count) * 12 * sizeof(double), tf_rows);
  s.start = s.plan.add(3 * sizeof(float), start_pose);
  s.deltas = s.plan.add(b3, hint_deltas);
  s.force = s.plan.add((size_t)count, force);
  s.pose = s.plan.add(b3, nullptr, out_pose);
  s.cov = s.plan.add((size_t)count * 9 * sizeof(float), nullptr, out_cov);
  s.applied = s.plan.add(b_int, nullptr, out_applied);
  s.counts = s.plan.add(b_int, nullptr, out_counts);
  s.ranges = s.plan.add((size_t)count * (size_t)n * sizeof(float), ranges);
  s.ws = s.plan.add(L.total);
  s.plan.view(s.cov, (size_t)count * 9 * sizeof(float), out_cov, nullptr);  // (in as well, behind the other copies in)
  s.plan.view(s.ws + L.origos, (size_t)count * 2 * sizeof(float), nullptr, out_origo);
  return s;
}

// hsm_score_window (d_batch): centre pose | end points[n] | likelihoods[window] | residuals[window].  An output the caller does
// not ask for is not carved: the kernel gets none.
struct ScoreWindowStage {
  StagePlan plan;
  size_t center, pts, lh, res;
};

inline ScoreWindowStage score_window_stage(size_t window, int n, const float* center, const float* pts, float* out_lh, float* out_res) {
  ScoreWindowStage s;
  s.center = s.plan.add(3 * sizeof(float), center);
  s.pts = s.plan.add((size_t)n * 2 * sizeof(float), pts);
  s.lh = s.plan.add(out_lh ? window * sizeof(float) : 0, nullptr, out_lh);
  s.res = s.plan.add(out_res ? window * sizeof(float) : 0, nullptr, out_res);
  return s;
}

// hsm_relocalize (d_batch): centre pose | end points[n] | the device call's workspace | candidate poses[k * 3] | candidate
// covariances[k * 9] | candidate likelihoods[k] | best pose | best score | best index.  The covariances and the best pose go in
// and out: an empty scan leaves the caller's matrices, a search without a winner the caller's pose.
struct RelocalizeStage {
  StagePlan plan;
  size_t center, pts, ws, pose, cov, lh, bpose, bscore, bidx;
};

inline RelocalizeStage relocalize_stage(int k, int n, size_t ws_bytes, const float* center, const float* pts, float* out_cand_pose,
                                        float* out_cand_cov, float* out_cand_lh, float* out_best_pose, float* out_best_score,
                                        int* out_best_index) {
  const size_t kf = (size_t)k * sizeof(float);
  RelocalizeStage s;
  s.center = s.plan.add(3 * sizeof(float), center);
  s.pts = s.plan.add((size_t)n * 2 * sizeof(float), pts);
  s.ws = s.plan.add(ws_bytes);
  s.pose = s.plan.add(3 * kf, nullptr, out_cand_pose);
  s.cov = s.plan.add(out_cand_cov ? 9 * kf : 0, out_cand_cov, out_cand_cov);
  s.lh = s.plan.add(kf, nullptr, out_cand_lh);
  s.bpose = s.plan.add(3 * sizeof(float), out_best_pose, out_best_pose);
  s.bscore = s.plan.add(out_best_score ? sizeof(float) : 0, nullptr, out_best_score);
  s.bidx = s.plan.add(sizeof(int), nullptr, out_best_index);
  return s;
}

// hsm_relocalize_batch (d_batch): centre poses[batch * 3] | end points[total_pts] | offsets[batch + 1] (a CSR batch; not carved
// for a shared scan) | the device call's workspace | candidate poses[batch * k * 3] | candidate covariances[batch * k * 9] |
// candidate likelihoods[batch * k] | candidates' window indices[batch * k] | best poses[batch * 3] | best scores[batch] | best
// indices[batch].  The covariances and the best poses go in and out, as hsm_relocalize's; the arrays the caller does not ask for
// are not carved.
struct RelocalizeBatchStage {
  StagePlan plan;
  size_t centers, pts, offs, ws, pose, cov, lh, cidx, bpose, bscore, bidx;
};

inline RelocalizeBatchStage relocalize_batch_stage(int batch, int k, size_t total_pts, size_t ws_bytes, const float* centers,
                                                   const float* pts, const int* offsets, float* out_cand_pose, float* out_cand_cov,
                                                   float* out_cand_lh, int* out_cand_index, float* out_best_pose,
                                                   float* out_best_score, int* out_best_index) {
  const size_t b = (size_t)batch * sizeof(float), bk = b * (size_t)k;
  RelocalizeBatchStage s;
  s.centers = s.plan.add(3 * b, centers);
  s.pts = s.plan.add(total_pts * 2 * sizeof(float), pts);
  s.offs = s.plan.add(offsets ? ((size_t)batch + 1) * sizeof(int) : 0, offsets);
  s.ws = s.plan.add(ws_bytes);
  s.pose = s.plan.add(3 * bk, nullptr, out_cand_pose);
  s.cov = s.plan.add(out_cand_cov ? 9 * bk : 0, out_cand_cov, out_cand_cov);
  s.lh = s.plan.add(bk, nullptr, out_cand_lh);
  s.cidx = s.plan.add(out_cand_index ? bk : 0, nullptr, out_cand_index);
  s.bpose = s.plan.add(3 * b, out_best_pose, out_best_pose);
  s.bscore = s.plan.add(out_best_score ? b : 0, nullptr, out_best_score);
  s.bidx = s.plan.add(b, nullptr, out_best_index);
  return s;
}

// hsm_occupied_points (d_batch): points[max_points] | counts[2] | the device call's workspace.  Only the counts are copied out
// by the plan: the entry copies the points the counts name once it has them, so that the caller's array is touched no further.
struct OccupiedPointsStage {
  StagePlan plan;
  size_t pts, counts, ws;
};

inline OccupiedPointsStage occupied_points_stage(int max_points, size_t ws_bytes, int* out_count) {
  OccupiedPointsStage s;
  s.pts = s.plan.add((size_t)max_points * 2 * sizeof(float));
  s.counts = s.plan.add(2 * sizeof(int), nullptr, out_count);
  s.ws = s.plan.add(ws_bytes);
  return s;
}

// hsm_map_tiles (d_batch): poses[batch * 3] | tiles[batch * tile bytes] | boxes[batch * 4].  Without the caller's array the boxes
// are not carved and the kernel gets none.
struct MapTilesStage {
  StagePlan plan;
  size_t poses, tiles, boxes;
};

inline MapTilesStage map_tiles_stage(int batch, size_t tile_bytes, const float* poses, unsigned char* out_tiles, int* out_boxes) {
  MapTilesStage s;
  s.poses = s.plan.add((size_t)batch * 3 * sizeof(float), poses);
  s.tiles = s.plan.add((size_t)batch * tile_bytes, nullptr, out_tiles);
  s.boxes = s.plan.add(out_boxes ? (size_t)batch * 4 * sizeof(int) : 0, nullptr, out_boxes);
  return s;
}

// hsm_align_map (the destination's d_batch): the guess as the window's centre | points[max_points] | counts[2] | the
// extraction's workspace | the relocalisation's workspace, whose k window indices are copied out where they lie (`kindex_at`
// inside it) | candidate poses[k * 3] | candidate covariances[k * 9] | candidate likelihoods[k] | best pose, seeded with the guess
// | best score | best index.  The counts come down in the middle of the chain, not with the plan.
struct AlignMapStage {
  StagePlan plan;
  size_t center, pts, counts, xws, ws, pose, cov, lh, bpose, bscore, bidx;
};

inline AlignMapStage align_map_stage(int k, int max_points, size_t xws_bytes, size_t ws_bytes, size_t kindex_at, const float* guess,
                                     int* out_kindex, float* out_cand_cov, float* out_best_pose, float* out_best_score,
                                     int* out_best_index) {
  const size_t kf = (size_t)k * sizeof(float);
  AlignMapStage s;
  s.center = s.plan.add(3 * sizeof(float), guess);
  s.pts = s.plan.add((size_t)max_points * 2 * sizeof(float));
  s.counts = s.plan.add(2 * sizeof(int));
  s.xws = s.plan.add(xws_bytes);
  s.ws = s.plan.add(ws_bytes);
  s.pose = s.plan.add(3 * kf);
  s.cov = s.plan.add(9 * kf, nullptr, out_cand_cov);
  s.lh = s.plan.add(kf);
  s.bpose = s.plan.add(3 * sizeof(float), guess, out_best_pose);
  s.bscore = s.plan.add(sizeof(float), nullptr, out_best_score);
  s.bidx = s.plan.add(sizeof(int), nullptr, out_best_index);
  s.plan.view(s.ws + kindex_at, (size_t)k * sizeof(int), nullptr, out_kindex);
  return s;
}

}  // namespace hsm_host
