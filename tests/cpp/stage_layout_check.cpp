// stage_layout_check.cpp -- hector_slam_amd/csrc/stage_layout.h against the sums the host runtime wrote out by hand before
// the header existed: the workspace of hsm_match_batch_ranges_device, the staging blocks of hsm_match_batch /
// hsm_match_score_batch (device and pinned form; with and without score, residual, ranking and its optional arrays) and the
// growth rule of every grow-on-demand buffer; and the staging plans of the host-array entries built on StagePlan
// (hsm_match_batch / hsm_match_score_batch themselves, hsm_update_by_scans, hsm_match_batch_ranges, hsm_match_batch_ranges_tf,
// hsm_slam_ranges_tf, the probes hsm_likelihood_states / hsm_residual_states, hsm_covariance_for_poses, hsm_ray_distances, and the
// window entries hsm_score_window, hsm_relocalize) against each entry's layout written out term by term, with the copies a plan
// asks for.  Every case is compared exactly; prints one JSON line, exits 1 on a mismatch.
#include <stdio.h>

#include <utility>
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

static const float kF[1] = {0};  // any non-null host array
static const double kD[1] = {0};
static const int kI[1] = {0};
static const unsigned char kU[1] = {0};

// the copies of a plan: region `off` is copied in from `src` / out to `dst` over `bytes`, and nothing else is
struct WantCopy {
  size_t off, bytes;
  const void* src;
  const void* dst;
};
static void check_copies(const StagePlan& p, const std::vector<WantCopy>& want, const char* what, long long a, long long b, long long c) {
  size_t in = 0, out = 0, want_in = 0, want_out = 0;
  for (const WantCopy& w : want) {
    const bool does_in = w.src && w.bytes, does_out = w.dst && w.bytes;
    want_in += does_in;
    want_out += does_out;
    bool found_in = !does_in, found_out = !does_out;
    for (int i = 0; i < p.n; ++i) {
      const StageRegion& r = p.r[i];
      if (does_in && r.src == w.src && r.off == w.off && r.bytes == w.bytes) found_in = true;
      if (does_out && r.dst == w.dst && r.off == w.off && r.bytes == w.bytes) found_out = true;
    }
    same(found_in && found_out, true, what, a, b, c);
  }
  for (int i = 0; i < p.n; ++i) in += p.r[i].src && p.r[i].bytes, out += p.r[i].dst && p.r[i].bytes;
  same(in, want_in, what, a, b, c);
  same(out, want_out, what, a, b, c);
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
  // the arrays of the call the flags describe (hsm_match_score_batch wants the likelihoods, and the winner index of a ranking)
  float pose_out[1], cov_io[1], lh[1], res[1], bscore[1], bpose_io[1];
  int idx[1];
  const int* offsets = b_offs ? kI : nullptr;
  float* out_lh = sr ? lh : nullptr;
  float* out_res = sr && (flags & 2) ? res : nullptr;
  const int* group_offsets = sr && (flags & 8) ? kI + 0 : nullptr;
  int* out_index = G > 0 ? idx : nullptr;
  float* out_score = sr && (flags & 16) ? bscore : nullptr;
  float* out_best_pose = sr && (flags & 32) ? bpose_io : nullptr;
  const MatchBatchStage L = match_batch_stage((int)batch, total_pts, (int)G, pinned, kF, kF + 0, offsets, pose_out, cov_io, out_lh,
                                              out_res, group_offsets, out_index, out_score, out_best_pose);
  const long long key = flags + (pinned ? 1000 : 0);
  same(L.begin, 0, "batch begin", batch, total_pts, key);
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
  same(L.plan.total(), total, "batch total", batch, total_pts, key);
  // start poses, end points, offsets and group offsets in; poses, likelihood, residual, winner index and score out; covariances
  // and winner poses both ways; an array the call does not have, neither
  check_copies(L.plan, {{0, b_begin, kF, nullptr}, {pts, b_pts, kF, nullptr}, {offs, b_offs, offsets, nullptr},
                        {pose, b_pose, nullptr, pose_out}, {cov, b_cov, cov_io, cov_io}, {x, b_lh, nullptr, out_lh},
                        {x + o_res, b_res, nullptr, out_res}, {x + o_goffs, b_goffs, group_offsets, nullptr},
                        {x + o_idx, b_idx, nullptr, out_index}, {x + o_bscore, b_bscore, nullptr, out_score},
                        {x + o_bpose, b_bpose, out_best_pose, out_best_pose}},
               "batch copies", batch, total_pts, key);
  // the copies are queued in the order of the list: that of the block, so begin, pts, offs, cov, group offsets, winner pose go in
  for (int i = 0; i + 1 < L.plan.n; ++i) same(L.plan.r[i].off <= L.plan.r[i + 1].off, true, "batch copy order", batch, total_pts, key);
  // ... and without the caller's covariances the region keeps its room and is copied neither way
  const MatchBatchStage N = match_batch_stage((int)batch, total_pts, (int)G, pinned, kF, kF + 0, offsets, pose_out, nullptr, out_lh,
                                              out_res, group_offsets, out_index, out_score, out_best_pose);
  same(N.cov, cov, "batch cov, not asked for", batch, total_pts, key);
  same(N.plan.total(), total, "batch total, cov not asked for", batch, total_pts, key);
  check_copies(N.plan, {{0, b_begin, kF, nullptr}, {pts, b_pts, kF, nullptr}, {offs, b_offs, offsets, nullptr},
                        {pose, b_pose, nullptr, pose_out}, {x, b_lh, nullptr, out_lh}, {x + o_res, b_res, nullptr, out_res},
                        {x + o_goffs, b_goffs, group_offsets, nullptr}, {x + o_idx, b_idx, nullptr, out_index},
                        {x + o_bscore, b_bscore, nullptr, out_score}, {x + o_bpose, b_bpose, out_best_pose, out_best_pose}},
               "batch copies, cov not asked for", batch, total_pts, key);
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

// ---- the staging plans of the host-array entries: offsets and totals written out term by term, as the entries carved them by hand
// before StagePlan; and which regions are copied in and out (null array or empty region: no copy) ----
// flags: 1 pts, 2 offsets
static void check_update_scans_stage(int count, size_t total, int flags) {
  const float* pts = flags & 1 ? kF : nullptr;
  const int* offsets = flags & 2 ? kI : nullptr;
  const size_t b_pts = total * 2 * sizeof(float), b_poses = (size_t)count * 3 * sizeof(float), b_offs = ((size_t)count + 1) * sizeof(int);
  const UpdateScansStage s = update_scans_stage(count, total, kF, pts, offsets);
  same(s.pts, 0, "update stage pts", count, total, flags);
  same(s.poses, al(b_pts), "update stage poses", count, total, flags);
  same(s.offs, al(b_pts) + al(b_poses), "update stage offsets", count, total, flags);
  same(s.plan.total(), al(b_pts) + al(b_poses) + al(b_offs), "update stage total", count, total, flags);
  check_copies(s.plan, {{0, b_pts, pts, nullptr}, {al(b_pts), b_poses, kF, nullptr}, {al(b_pts) + al(b_poses), b_offs, offsets, nullptr}},
               "update stage copies", count, total, flags);
}

// flags: 1 out_cov, 2 out_counts, 4 ranges
static void check_ranges_stage(int batch, int n, int flags) {
  RangesLayout L;
  if (!ranges_layout(batch, n, &L)) return;
  float cov[1], pose[1];
  int counts[1];
  float* out_cov = flags & 1 ? cov : nullptr;
  int* out_counts = flags & 2 ? counts : nullptr;
  const float* ranges = flags & 4 ? kF : nullptr;
  const size_t b_begin = (size_t)batch * 3 * sizeof(float), b_cov = (size_t)batch * 9 * sizeof(float);
  const size_t b_counts = (size_t)batch * sizeof(int), b_ranges = (size_t)batch * n * sizeof(float);
  const size_t o_pose = al(b_begin), o_cov = al(b_begin) + al(b_begin), o_counts = al(b_begin) + al(b_begin) + al(b_cov);
  const size_t o_ranges = al(b_begin) + al(b_begin) + al(b_cov) + al(b_counts);
  const size_t o_ws = al(b_begin) + al(b_begin) + al(b_cov) + al(b_counts) + al(b_ranges);
  const RangesStage s = ranges_stage(batch, n, L.total, kF, ranges, pose, out_cov, out_counts);
  same(s.begin, 0, "ranges stage begin", batch, n, flags);
  same(s.pose, o_pose, "ranges stage pose", batch, n, flags);
  same(s.cov, o_cov, "ranges stage cov", batch, n, flags);
  same(s.counts, o_counts, "ranges stage counts", batch, n, flags);
  same(s.ranges, o_ranges, "ranges stage ranges", batch, n, flags);
  same(s.ws, o_ws, "ranges stage workspace", batch, n, flags);
  same(s.plan.total(), o_ws + al(L.total), "ranges stage total", batch, n, flags);
  check_copies(s.plan, {{0, b_begin, kF, nullptr}, {o_pose, b_begin, nullptr, pose}, {o_cov, b_cov, out_cov, out_cov},
                        {o_counts, b_counts, nullptr, out_counts}, {o_ranges, b_ranges, ranges, nullptr}},
               "ranges stage copies", batch, n, flags);
}

// flags: 1 out_cov, 2 out_counts, 4 ranges, 8 out_origo, 16 shared_tf
static void check_ranges_tf_stage(int batch, int n, int flags) {
  if (batch < 0 || n < 0 || n > HSM_MAX_UPDATE_BEAMS || (size_t)batch * (size_t)n > (size_t)INT_MAX) return;
  float cov[1], pose[1], origo[1];
  int counts[1];
  float* out_cov = flags & 1 ? cov : nullptr;
  int* out_counts = flags & 2 ? counts : nullptr;
  const float* ranges = flags & 4 ? kF : nullptr;
  float* out_origo = flags & 8 ? origo : nullptr;
  const bool shared_tf = flags & 16;
  const size_t bn = (size_t)batch * n;
  const size_t b_begin = (size_t)batch * 3 * sizeof(float), b_cov = (size_t)batch * 9 * sizeof(float);
  const size_t b_counts = (size_t)batch * sizeof(int), b_ranges = bn * sizeof(float);
  const size_t b_tf = (shared_tf ? 1 : (size_t)batch) * 12 * sizeof(double), b_origo = (size_t)batch * 2 * sizeof(float);
  const size_t o_begin = al(b_tf), o_pose = al(b_tf) + al(b_begin), o_cov = al(b_tf) + al(b_begin) + al(b_begin);
  const size_t o_counts = al(b_tf) + al(b_begin) + al(b_begin) + al(b_cov);
  const size_t o_origo = al(b_tf) + al(b_begin) + al(b_begin) + al(b_cov) + al(b_counts);
  const size_t o_offs = al(b_tf) + al(b_begin) + al(b_begin) + al(b_cov) + al(b_counts) + al(b_origo);
  const size_t o_ranges = al(b_tf) + al(b_begin) + al(b_begin) + al(b_cov) + al(b_counts) + al(b_origo) + al(b_counts + sizeof(int));
  const size_t o_pts = o_ranges + al(b_ranges);
  const size_t total = o_pts + al((bn > 0 ? bn : 1) * 2 * sizeof(float));
  const RangesTfStage s = ranges_tf_stage(batch, n, shared_tf, kD, kF, ranges, pose, out_cov, out_counts, out_origo);
  same(s.tf, 0, "ranges tf stage tf", batch, n, flags);
  same(s.begin, o_begin, "ranges tf stage begin", batch, n, flags);
  same(s.pose, o_pose, "ranges tf stage pose", batch, n, flags);
  same(s.cov, o_cov, "ranges tf stage cov", batch, n, flags);
  same(s.counts, o_counts, "ranges tf stage counts", batch, n, flags);
  same(s.origo, o_origo, "ranges tf stage origo", batch, n, flags);
  same(s.offs, o_offs, "ranges tf stage offsets", batch, n, flags);
  same(s.ranges, o_ranges, "ranges tf stage ranges", batch, n, flags);
  same(s.pts, o_pts, "ranges tf stage pts", batch, n, flags);
  same(s.plan.total(), total, "ranges tf stage total", batch, n, flags);
  check_copies(s.plan, {{0, b_tf, kD, nullptr}, {o_begin, b_begin, kF, nullptr}, {o_pose, b_begin, nullptr, pose},
                        {o_cov, b_cov, out_cov, out_cov}, {o_counts, b_counts, nullptr, out_counts},
                        {o_origo, b_origo, nullptr, out_origo}, {o_ranges, b_ranges, ranges, nullptr}},
               "ranges tf stage copies", batch, n, flags);
}

// flags: 1 out_cov, 2 out_counts, 4 ranges, 8 out_origo, 16 shared_tf, 32 start_pose, 64 hint_deltas, 128 force, 256 out_applied
static void check_slam_ranges_tf_stage(int count, int n, int flags) {
  SlamRangesTfLayout L;
  if (!slam_ranges_tf_layout(count, n, &L)) return;
  float cov[1], pose[1], origo[1];
  int counts[1], applied[1];
  float* out_cov = flags & 1 ? cov : nullptr;
  int* out_counts = flags & 2 ? counts : nullptr;
  const float* ranges = flags & 4 ? kF : nullptr;
  float* out_origo = flags & 8 ? origo : nullptr;
  const bool shared_tf = flags & 16;
  const float* start = flags & 32 ? kF : nullptr;
  const float* deltas = flags & 64 ? kF + 0 : nullptr;
  const unsigned char* force = flags & 128 ? kU : nullptr;
  int* out_applied = flags & 256 ? applied : nullptr;
  const size_t b3 = (size_t)count * 3 * sizeof(float), b_cov = (size_t)count * 9 * sizeof(float);
  const size_t b_int = (size_t)count * sizeof(int), b_ranges = (size_t)count * n * sizeof(float);
  const size_t b_tf = (shared_tf ? 1 : (size_t)count) * 12 * sizeof(double), b_origo = (size_t)count * 2 * sizeof(float);
  const size_t o_start = al(b_tf), o_deltas = al(b_tf) + al(3 * sizeof(float)), o_force = al(b_tf) + al(3 * sizeof(float)) + al(b3);
  const size_t o_pose = al(b_tf) + al(3 * sizeof(float)) + al(b3) + al((size_t)count);
  const size_t o_cov = al(b_tf) + al(3 * sizeof(float)) + al(b3) + al((size_t)count) + al(b3);
  const size_t o_applied = al(b_tf) + al(3 * sizeof(float)) + al(b3) + al((size_t)count) + al(b3) + al(b_cov);
  const size_t o_counts = al(b_tf) + al(3 * sizeof(float)) + al(b3) + al((size_t)count) + al(b3) + al(b_cov) + al(b_int);
  const size_t o_ranges = al(b_tf) + al(3 * sizeof(float)) + al(b3) + al((size_t)count) + al(b3) + al(b_cov) + al(b_int) + al(b_int);
  const size_t o_ws = o_ranges + al(b_ranges);
  const SlamRangesTfStage s = slam_ranges_tf_stage(count, n, shared_tf, L, kD, start, deltas, force, ranges, pose, out_cov, out_applied,
                                                   out_counts, out_origo);
  same(s.tf, 0, "slam stage tf", count, n, flags);
  same(s.start, o_start, "slam stage start", count, n, flags);
  same(s.deltas, o_deltas, "slam stage deltas", count, n, flags);
  same(s.force, o_force, "slam stage force", count, n, flags);
  same(s.pose, o_pose, "slam stage pose", count, n, flags);
  same(s.cov, o_cov, "slam stage cov", count, n, flags);
  same(s.applied, o_applied, "slam stage applied", count, n, flags);
  same(s.counts, o_counts, "slam stage counts", count, n, flags);
  same(s.ranges, o_ranges, "slam stage ranges", count, n, flags);
  same(s.ws, o_ws, "slam stage workspace", count, n, flags);
  same(s.plan.total(), o_ws + al(L.total), "slam stage total", count, n, flags);
  check_copies(s.plan, {{0, b_tf, kD, nullptr}, {o_start, 3 * sizeof(float), start, nullptr}, {o_deltas, b3, deltas, nullptr},
                        {o_force, (size_t)count, force, nullptr}, {o_pose, b3, nullptr, pose}, {o_cov, b_cov, out_cov, out_cov},
                        {o_applied, b_int, nullptr, out_applied}, {o_counts, b_int, nullptr, out_counts},
                        {o_ranges, b_ranges, ranges, nullptr}, {o_ws + L.origos, b_origo, nullptr, out_origo}},
               "slam stage copies", count, n, flags);
}

// flags: 1 out_lh, 2 out_residual, 4 pts
static void check_score_states_stage(int batch, int n, int flags) {
  float lh[1], res[1];
  float* out_lh = flags & 1 ? lh : nullptr;
  float* out_res = flags & 2 ? res : nullptr;
  const float* pts = flags & 4 ? kF : nullptr;
  const size_t b_pts = (size_t)n * 2 * sizeof(float), b_states = (size_t)batch * 3 * sizeof(float), b_one = (size_t)batch * sizeof(float);
  const ScoreStatesStage s = score_states_stage(batch, n, kF, pts, out_lh, out_res);
  same(s.pts, 0, "score stage pts", batch, n, flags);
  same(s.states, al(b_pts), "score stage states", batch, n, flags);
  same(s.lh, al(b_pts) + al(b_states), "score stage likelihood", batch, n, flags);
  same(s.res, al(b_pts) + al(b_states) + al(b_one), "score stage residual", batch, n, flags);
  same(s.plan.total(), al(b_pts) + al(b_states) + al(b_one) + al(b_one), "score stage total", batch, n, flags);
  check_copies(s.plan, {{0, b_pts, pts, nullptr}, {al(b_pts), b_states, kF, nullptr}, {al(b_pts) + al(b_states), b_one, nullptr, out_lh},
                        {al(b_pts) + al(b_states) + al(b_one), b_one, nullptr, out_res}},
               "score stage copies", batch, n, flags);
}

// flags: 1 out_cov_map, 2 out_cov_world, 4 out_lh7, 8 pts
static void check_pose_covariance_stage(int batch, int n, int flags) {
  float cm[1], cw[1], l7[1];
  float* out_map = flags & 1 ? cm : nullptr;
  float* out_world = flags & 2 ? cw : nullptr;
  float* out_lh7 = flags & 4 ? l7 : nullptr;
  const float* pts = flags & 8 ? kF : nullptr;
  const size_t b_pts = (size_t)n * 2 * sizeof(float), b_poses = (size_t)batch * 3 * sizeof(float);
  const size_t b_cov = (size_t)batch * 9 * sizeof(float), b_lh7 = (size_t)batch * 7 * sizeof(float);
  const size_t o_poses = al(b_pts), o_map = al(b_pts) + al(b_poses), o_world = al(b_pts) + al(b_poses) + al(b_cov);
  const size_t o_lh7 = al(b_pts) + al(b_poses) + al(b_cov) + al(b_cov);
  const PoseCovarianceStage s = pose_covariance_stage(batch, n, kF, pts, out_map, out_world, out_lh7);
  same(s.pts, 0, "covariance stage pts", batch, n, flags);
  same(s.poses, o_poses, "covariance stage poses", batch, n, flags);
  same(s.cov_map, o_map, "covariance stage map frame", batch, n, flags);
  same(s.cov_world, o_world, "covariance stage world frame", batch, n, flags);
  same(s.lh7, o_lh7, "covariance stage likelihoods", batch, n, flags);
  same(s.plan.total(), o_lh7 + al(b_lh7), "covariance stage total", batch, n, flags);
  check_copies(s.plan, {{0, b_pts, pts, nullptr}, {o_poses, b_poses, kF, nullptr}, {o_map, b_cov, nullptr, out_map},
                        {o_world, b_cov, nullptr, out_world}, {o_lh7, b_lh7, nullptr, out_lh7}},
               "covariance stage copies", batch, n, flags);
}

// flags: 1 out_hit (in and out)
static void check_ray_distances_stage(int n, int flags) {
  float dist[1], hit[1];
  float* out_hit = flags & 1 ? hit : nullptr;
  const size_t b2 = (size_t)n * 2 * sizeof(float), b1 = (size_t)n * sizeof(float);
  const RayDistancesStage s = ray_distances_stage(n, kF, kF + 0, dist, out_hit);
  same(s.begin, 0, "ray stage begin", n, flags, 0);
  same(s.end, al(b2), "ray stage end", n, flags, 0);
  same(s.dist, al(b2) + al(b2), "ray stage distances", n, flags, 0);
  same(s.hit, al(b2) + al(b2) + al(b1), "ray stage hits", n, flags, 0);
  same(s.plan.total(), al(b2) + al(b2) + al(b1) + al(b2), "ray stage total", n, flags, 0);
  // (begin and end are one host array here: two copies in of it, told apart by their offsets)
  check_copies(s.plan, {{0, b2, kF, nullptr}, {al(b2), b2, kF, nullptr}, {al(b2) + al(b2), b1, nullptr, dist},
                        {al(b2) + al(b2) + al(b1), b2, out_hit, out_hit}},
               "ray stage copies", n, flags, 0);
}

// flags: 1 out_lh, 2 out_residual, 4 pts
static void check_score_window_stage(size_t window, int n, int flags) {
  float lh[1], res[1];
  float* out_lh = flags & 1 ? lh : nullptr;
  float* out_res = flags & 2 ? res : nullptr;
  const float* pts = flags & 4 ? kF + 0 : nullptr;
  const size_t b_center = 3 * sizeof(float), b_pts = (size_t)n * 2 * sizeof(float);
  const size_t b_lh = out_lh ? window * sizeof(float) : 0, b_res = out_res ? window * sizeof(float) : 0;
  const ScoreWindowStage s = score_window_stage(window, n, kF, pts, out_lh, out_res);
  same(s.center, 0, "window stage centre", window, n, flags);
  same(s.pts, al(b_center), "window stage pts", window, n, flags);
  same(s.lh, al(b_center) + al(b_pts), "window stage likelihood", window, n, flags);
  same(s.res, al(b_center) + al(b_pts) + al(b_lh), "window stage residual", window, n, flags);
  same(s.plan.total(), al(b_center) + al(b_pts) + al(b_lh) + al(b_res), "window stage total", window, n, flags);
  check_copies(s.plan, {{0, b_center, kF, nullptr}, {al(b_center), b_pts, pts, nullptr}, {al(b_center) + al(b_pts), b_lh, nullptr, out_lh},
                        {al(b_center) + al(b_pts) + al(b_lh), b_res, nullptr, out_res}},
               "window stage copies", window, n, flags);
}

// flags: 1 out_cand_cov (in and out), 2 out_best_score, 4 pts
static void check_relocalize_stage(int k, int n, size_t ws_bytes, int flags) {
  float pose[1], cov[1], lh[1], bpose[1], bscore[1];
  int bidx[1];
  float* out_cov = flags & 1 ? cov : nullptr;
  float* out_bscore = flags & 2 ? bscore : nullptr;
  const float* pts = flags & 4 ? kF + 0 : nullptr;
  const size_t b_center = 3 * sizeof(float), b_pts = (size_t)n * 2 * sizeof(float), b_pose = (size_t)k * 3 * sizeof(float);
  const size_t b_cov = out_cov ? (size_t)k * 9 * sizeof(float) : 0, b_lh = (size_t)k * sizeof(float), b_bpose = 3 * sizeof(float);
  const size_t b_bscore = out_bscore ? sizeof(float) : 0, b_bidx = sizeof(int);
  const size_t o_pts = al(b_center), o_ws = al(b_center) + al(b_pts), o_pose = al(b_center) + al(b_pts) + al(ws_bytes);
  const size_t o_cov = al(b_center) + al(b_pts) + al(ws_bytes) + al(b_pose);
  const size_t o_lh = al(b_center) + al(b_pts) + al(ws_bytes) + al(b_pose) + al(b_cov);
  const size_t o_bpose = al(b_center) + al(b_pts) + al(ws_bytes) + al(b_pose) + al(b_cov) + al(b_lh);
  const size_t o_bscore = al(b_center) + al(b_pts) + al(ws_bytes) + al(b_pose) + al(b_cov) + al(b_lh) + al(b_bpose);
  const size_t o_bidx = al(b_center) + al(b_pts) + al(ws_bytes) + al(b_pose) + al(b_cov) + al(b_lh) + al(b_bpose) + al(b_bscore);
  const RelocalizeStage s = relocalize_stage(k, n, ws_bytes, kF, pts, pose, out_cov, lh, bpose, out_bscore, bidx);
  const long long key = flags + 1000 * (long long)ws_bytes;
  same(s.center, 0, "relocalize stage centre", k, n, key);
  same(s.pts, o_pts, "relocalize stage pts", k, n, key);
  same(s.ws, o_ws, "relocalize stage workspace", k, n, key);
  same(s.pose, o_pose, "relocalize stage poses", k, n, key);
  same(s.cov, o_cov, "relocalize stage covariances", k, n, key);
  same(s.lh, o_lh, "relocalize stage likelihoods", k, n, key);
  same(s.bpose, o_bpose, "relocalize stage best pose", k, n, key);
  same(s.bscore, o_bscore, "relocalize stage best score", k, n, key);
  same(s.bidx, o_bidx, "relocalize stage best index", k, n, key);
  same(s.plan.total(), o_bidx + al(b_bidx), "relocalize stage total", k, n, key);
  check_copies(s.plan, {{0, b_center, kF, nullptr}, {o_pts, b_pts, pts, nullptr}, {o_pose, b_pose, nullptr, pose},
                        {o_cov, b_cov, out_cov, out_cov}, {o_lh, b_lh, nullptr, lh}, {o_bpose, b_bpose, bpose, bpose},
                        {o_bscore, b_bscore, nullptr, out_bscore}, {o_bidx, b_bidx, nullptr, bidx}},
               "relocalize stage copies", k, n, key);
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
  // the staging plans: counts and n of 0 and 1, and one element either side of every 256-byte multiple an element size in play
  // reaches (4-byte elements at 64, 8 at 32, 12 at 64, 36 at 64, 96 at 8, 1 at 256); every optional array present and absent
  const std::vector<long long> stage_sizes = {0, 1, 2, 7, 8, 9, 21, 22, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1081};
  for (long long cnt : stage_sizes) {
    for (long long t : stage_sizes)
      for (int flags = 0; flags < 4; ++flags) check_update_scans_stage((int)cnt, (size_t)t, flags);
    for (long long n : stage_sizes) {
      for (int flags = 0; flags < 8; ++flags) check_ranges_stage((int)cnt, (int)n, flags);
      for (int flags = 0; flags < 32; ++flags) check_ranges_tf_stage((int)cnt, (int)n, flags);
      for (int flags = 0; flags < 512; ++flags) check_slam_ranges_tf_stage((int)cnt, (int)n, flags);
    }
  }
  // the probes' plans: empty, one element, odd sizes below a 256-byte multiple, and sizes that cross one in every region
  for (const auto& bn : {std::pair<int, int>{0, 0}, {1, 1}, {3, 7}, {65, 129}}) {
    for (int flags = 0; flags < 8; ++flags) check_score_states_stage(bn.first, bn.second, flags);
    for (int flags = 0; flags < 16; ++flags) check_pose_covariance_stage(bn.first, bn.second, flags);
  }
  for (int n : {0, 1, 65})
    for (int flags = 0; flags < 2; ++flags) check_ray_distances_stage(n, flags);
  // the window entries' plans: windows of one pose, either side of a 256-byte multiple and of the lane form's 65536; k from 1 to
  // HSM_MAX_TOPK either side of the multiples 12-, 36- and 4-byte elements reach; a workspace of any size, aligned or not
  for (int n : {0, 1, 32, 33, 1081})
    for (int flags = 0; flags < 8; ++flags) {
      for (size_t window : {(size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)1089, (size_t)65536, (size_t)INT_MAX})
        check_score_window_stage(window, n, flags);
      for (int k : {1, 7, 8, 21, 22, 63, HSM_MAX_TOPK})
        for (size_t ws : {(size_t)0, (size_t)8, (size_t)255, (size_t)256, (size_t)257, (size_t)4356 + 1024, (size_t)INT_MAX * 4 + 4096})
          check_relocalize_stage(k, n, ws, flags);
    }
  printf("{\"cases\": %lld, \"mismatches\": %lld}\n", cases, mismatches);
  return mismatches ? 1 : 0;
}
