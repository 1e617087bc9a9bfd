// match.hip -- the matcher's front door: every hsm_match* entry, the score, covariance, select and match-score entries, the plan of a launch
// (match_plan.h) and its record, and the single-scan path with its staging.  Kernels launched here: the one-workgroup-per-scan and
// multi-workgroup forms of gn_match_dense.h and gn_match_spec.h, and score_kernels.h; the batch / team forms are dispatched to
// match_exact_cached.hip and match_teams.hip through the launch entries hsm_ctx.h declares, whose kernels this unit does not see.
// What it needs of the core runtime (hector_mi355.hip: the context, the level views, the stream ordering, the error text) is
// declared in hsm_ctx.h and hsm_host.h, and so are the bundles a batched call travels as, filled once by its extern "C" entry:
// ScanBatch, MatchOut, ScoringStep, Ranking.  match_batch_device_nolock is the match, match_chain_nolock the one chain match ->
// scoring step -> winners behind the match-score, match-covariance, host and relocalisation entries.
#include <hip/hip_runtime.h>
#include <math.h>
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <chrono>
#include <mutex>
#include <string>
#include <vector>

#include "gn_match_dense.h"
#include "gn_match_spec.h"
#include "gn_step.h"
#include "hector_mi355/capi.h"
#include "hsm_ctx.h"
#include "hsm_host.h"
#include "score_kernels.h"

namespace {

using namespace hsm;
using namespace hsm_host;

static_assert(hsm_plan::kQuad == kLayoutQuad && hsm_plan::kPlane == kLayoutPlane && hsm_plan::kExactGroupRounds == kExactGroupRounds &&
                  hsm_plan::kDenseRound == kDenseRound && hsm_plan::kSpec1MaxBeams == kSpec1MaxBeams,
              "match_plan.h restates match_types.h / gn_step.h / gn_match_dense.h / gn_match_spec.h");
static_assert(hsm_plan::kParityFast == HSM_PARITY_FAST && hsm_plan::kParityExact == HSM_PARITY_EXACT && hsm_plan::kParityRelaxed == HSM_PARITY_RELAXED,
              "match_plan.h restates capi.h");

using hsm_plan::Family;
using hsm_plan::MatchSite;
using hsm_plan::plan_match;

// the site of a match launch (match_plan.h): the context's knobs and the call's shape.  The staging of a single scan and its
// launch both come here, so that they plan the same form.  `stream`: only the opt-in speculative-carry form asks whether it is
// being captured, so nobody else pays for the question.
MatchSite match_site(const hsm_ctx* h, int batch, int max_n, int n_bound, bool batched, bool trace, hipStream_t stream) {
  MatchSite s;
  static_cast<hsm_plan::MatchKnobs&>(s) = h->cfg.match;
  s.batch = batch, s.max_n = max_n, s.n_bound = n_bound;
  s.exact = wants_exact(h), s.relaxed = h->cfg.parity.relaxed, s.layout = h->cfg.layout;
  s.batched = batched, s.trace = trace, s.clock_probe = h->batch.clock_probe != nullptr;
  s.capturing = h->cfg.match.exact_spec && stream_capturing(stream);
  s.compute_units = h->compute_units, s.level0_cells = h->levels[0].cells();
  s.coop_skip = h->single.coop_skip > 0;
  return s;
}
MatchSite single_scan_site(const hsm_ctx* h, int n, bool trace = false) { return match_site(h, 1, n, n, false, trace, h->stream); }

// what hsm_last_launch_config / _kernel / _parity report: the plan that was launched
void record_launch(hsm_ctx* h, const MatchPlan& plan) {
  for (int i = 0; i < 6; ++i) h->last.last_cfg[i] = plan.record[i];
  h->last.last_kernel = plan.name;
  h->last.last_parity = plan.parity;
}
// ... and behind a sampler kernel (with_sampler_form): its name and the summation order the context ran it in
void record_sampler_launch(hsm_ctx* h, const char* kernel) {
  h->last.last_kernel = kernel;
  h->last.last_parity = wants_exact(h) ? HSM_PARITY_EXACT : (h->cfg.parity.relaxed ? HSM_PARITY_RELAXED : HSM_PARITY_FAST);
}

// the one-workgroup-per-scan forms of this unit: Family::kExactDense, kSpec (gn_match_dense.h, gn_match_spec.h: `batch` workgroups) and
// kSpec1 (one scan)
int launch_workgroup_form(hsm_ctx* h, MatchParams P, MatchPlan& plan, const MatchSite& site, hipStream_t stream) {
  if (plan.family == Family::kSpec) {
    // The product scratch is the launching stream's own (two streams' launches would write the same rows at once).  A launch into a
    // graph capture was planned in the literal form, which needs no scratch: a graph never reads a block that an eager launch grows
    // (frees), and nothing is allocated or synchronised while the caller captures.  A ninth stream falls to it here.
    hsm_ctx::SpecScratch* sb = nullptr;
    for (hsm_ctx::SpecScratch& b : h->batch.spec_scratch)
      if (b.s == stream) sb = &b;
    if (!sb && h->batch.spec_scratch.size() < 8) {
      h->batch.spec_scratch.push_back({stream, {}});
      sb = &h->batch.spec_scratch.back();
    }
    if (!sb) {
      MatchSite literal = site;
      literal.exact_spec = false;
      plan = plan_match(literal);
    } else {
      const size_t stride = spec_scratch_float4s_bound(P.n_bound);  // enough for every n <= n_bound
      const size_t need = stride * (size_t)P.batch;
      if (!sb->d.holds(need)) HIP_TRY(hipStreamSynchronize(stream));  // (a launch of this stream in flight may still read the old block)
      if (int rc = sb->d.reserve(need)) return rc;
      P.spec_scratch = (float*)sb->d.p;
      P.spec_stride = (unsigned)stride;
      P.spec_stats = h->batch.d_spec_stats;
    }
  }
#define HSM_LAUNCH_WG(KERNEL)                                                              \
  do {                                                                                     \
    if (plan.layout == kLayoutPlane)                                                       \
      hipLaunchKernelGGL((KERNEL<kLayoutPlane>), dim3(plan.grid), dim3(plan.block), 0, stream, P); \
    else                                                                                   \
      hipLaunchKernelGGL((KERNEL<kLayoutQuad>), dim3(plan.grid), dim3(plan.block), 0, stream, P);  \
  } while (0)
  if (plan.family == Family::kSpec) HSM_LAUNCH_WG(gn_match_spec_kernel);
  else if (plan.family == Family::kExactDense) HSM_LAUNCH_WG(gn_match_exact_dense_kernel);
  else HSM_LAUNCH_WG(gn_match_spec1_kernel);
#undef HSM_LAUNCH_WG
  HIP_TRY(hipGetLastError());
  return HSM_OK;
}

// launches `plan` (any family but the cooperative one, which match_single launches itself) and records it
int launch_plan(hsm_ctx* h, MatchParams P, const MatchSite& site, MatchPlan plan, hipStream_t stream) {
  if (plan.wants_perm)
    if (int rc = ensure_batch_perm(h, P, stream)) return rc;  // (hsm_set_batch_order)
  int rc;
  switch (plan.family) {
    case Family::kExactDense:
    case Family::kSpec:
    case Family::kSpec1: rc = launch_workgroup_form(h, P, plan, site, stream); break;
    case Family::kExactCached:
    case Family::kExactCachedCw:
      if (plan.tail_batch > 0) {
        // the whole generations, and behind them the part-filled last one in its own launch
        MatchParams A = P, B = P;
        A.batch = P.batch - plan.tail_batch, B.batch = plan.tail_batch;
        if (P.perm) {  // (a permuted batch: the second launch takes the rest of the permutation, its scan indices stay absolute)
          B.perm = P.perm + A.batch;
        } else {
          B.begin_world = P.begin_world + 3 * (size_t)A.batch;
          if (P.offsets) B.offsets = P.offsets + A.batch;  // (absolute offsets into pts: the pointer moves, pts stays)
          B.out_pose = P.out_pose + 3 * (size_t)A.batch;
          if (P.out_cov) B.out_cov = P.out_cov + 9 * (size_t)A.batch;
        }
        B.clock_probe = nullptr;  // (scan 0's probe belongs to the first launch)
        A.xp.world = 0;           // (neither part carries the pose exchange: plan_split_part)
        B.xp.world = 0;
        rc = launch_exact_cached_form(h, A, hsm_plan::plan_split_part(site, plan.tail_batch, false), stream);
        if (rc == HSM_OK) rc = launch_exact_cached_form(h, B, hsm_plan::plan_split_part(site, plan.tail_batch, true), stream);
      } else {
        rc = launch_exact_cached_form(h, P, plan, stream);
      }
      break;
    default: rc = launch_team_form(h, P, plan, stream); break;
  }
  if (rc == HSM_OK) record_launch(h, plan);
  return rc;
}

int launch_match(hsm_ctx* h, const MatchParams& P, int max_n, hipStream_t stream) {
  h->last.last_sorted = false;  // (the forms that take a permuted batch set it: ensure_batch_perm)
  MatchSite site = match_site(h, P.batch, max_n, P.n_bound, P.begin_world != nullptr, P.trace != nullptr, stream);
  site.exchange = P.xp.world > 0, site.exchange_wait_blocks = P.xp.wait_blocks;
  site.coop_skip = true;  // (the cooperative form is match_single's to launch: here its scan goes to one workgroup)
  return launch_plan(h, P, site, plan_match(site), stream);
}

// the schedule of MapRepMultiMap::matchData (MapRepMultiMap.h:116-132): coarse levels
// maxIterations = 3, level 0 maxIterations = 5, each plus the unconditional first step.  `batched`: the batched entries, where
// the test hook hsm_debug_set_schedule may restrict the schedule to one level (every level's view stays filled: the batch
// order reads level 0's)
void fill_schedule(const hsm_ctx* h, MatchParams& P, bool batched = false) {
  const int nl = (int)h->levels.size();
  for (int l = 0; l < nl; ++l) P.lv[l] = level_view(h->levels[l], level_factor(l), l == 0 ? 6 : 4);
  P.first_level = nl - 1;
  P.last_level = 0;
  if (batched && h->batch.sched_level >= 0 && h->batch.sched_level < nl) {
    P.lv[h->batch.sched_level].gn_steps = h->batch.sched_steps;
    P.first_level = P.last_level = h->batch.sched_level;
  }
}

// The refusals of a scoring step on its own (a chain has its combined check): the level first.  The covariance entries name
// themselves in every text, the level's and the null context's too; the score's answer those as valid_level does
int scoring_level_check(const hsm_ctx* h, const ScoringStep& S) {
  if (!S.covariance) return valid_level(h, S.level);
  if (!h) return fail_at(HSM_ERR_INVALID, S.who, ": null context");
  if (S.level < 0 || S.level >= (int)h->levels.size()) return fail_at(HSM_ERR_INVALID, S.who, ": level out of range");
  return HSM_OK;
}
int scoring_step_check(const hsm_ctx* h, const ScoringStep& S, const ScanBatch& B) {
  if (int rc = scoring_level_check(h, S)) return rc;
  if (B.bad_shape() || S.no_output() || (B.batch > 0 && !B.d_poses) || B.points_missing())
    return fail_at(HSM_ERR_INVALID, S.who, ": bad argument");
  return HSM_OK;
}

// The weighting step behind a batched match, or the covariance estimate: B (world pose, scan) pairs on S.level in one launch of
// score_batch_kernel or covariance_batch_kernel (score_kernels.h), a wavefront per pair.  A reader of the map like the batched
// match and bracketed like it; no workspace, no state.  Arguments checked
int scoring_step_launch(hsm_ctx* h, const ScoringStep& S, const ScanBatch& B, void* stream) {
  if (B.batch == 0) return HSM_OK;
  if (int rc = select_device(h)) return rc;
  hipStream_t s = (hipStream_t)stream;
  MapReader reader;
  if (int rc = reader.begin(h, s, S.covariance ? S.who : "hsm_score_batch_device")) return rc;
  const Level& Lv = h->levels[S.level];
  const LevelView v = level_view(Lv, level_factor(S.level), 1);
  const float2* pts = reinterpret_cast<const float2*>(B.d_pts);
  const int grid = (B.batch + 3) / 4, n = B.kernel_shared_n();
  if (!S.covariance)
    with_sampler_form(h, [&](auto lay, auto ex) {
      hipLaunchKernelGGL((score_batch_kernel<lay(), ex()>), dim3(grid), dim3(256), 0, s, v, B.d_poses, B.batch, pts, B.d_offsets, n,
                         S.score.d_likelihood, S.score.d_residual);
    });
  else
    with_sampler_form(h, [&](auto lay, auto ex) {
      hipLaunchKernelGGL((covariance_batch_kernel<lay(), ex()>), dim3(grid), dim3(256), 0, s, v, B.d_poses, B.batch, pts, B.d_offsets, n,
                         Lv.cell_length, S.cov.d_cov_world, S.cov.d_cov_map, S.cov.d_lh7, S.cov.d_likelihood);
    });
  HIP_TRY(hipGetLastError());
  reader.queued();
  record_sampler_launch(h, S.covariance ? "covariance_batch_kernel" : "score_batch_kernel");
  return HSM_OK;
}

// Groups of at most this many entries (or, with CSR groups whose sizes only the device knows, launches of at least this many
// groups) take one wavefront per group, the others one workgroup per group.  Either shape gives the same result.
constexpr int kSelectWaveGroupMax = 1024;

// the winner of every group of R by `d_scores`, its pose out of `d_poses_world`; reads no map: stream order is all it needs
int select_best_device_nolock(hsm_ctx* h, const Ranking& R, const float* d_scores, const float* d_poses_world, void* stream) {
  if (R.groups < 0 || (!R.group_offsets && R.group_size < 0) || !R.out_index || (R.out_best_pose && !d_poses_world) ||
      (!d_scores && R.groups > 0 && (R.group_offsets || R.group_size > 0)) ||
      (!R.group_offsets && R.groups > 0 && (long long)R.groups * R.group_size > INT_MAX))
    return fail(HSM_ERR_INVALID, "hsm_select_best_device: bad argument");
  if (R.groups == 0) return HSM_OK;
  if (int rc = select_device(h)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const bool wave_per_group = R.group_offsets ? R.groups >= kSelectWaveGroupMax : R.group_size <= kSelectWaveGroupMax;
  if (wave_per_group)
    hipLaunchKernelGGL((select_best_kernel<true>), dim3((R.groups + 3) / 4), dim3(256), 0, s, R.groups, R.group_offsets, R.group_size,
                       d_scores, d_poses_world, R.out_index, R.out_score, R.out_best_pose);
  else
    hipLaunchKernelGGL((select_best_kernel<false>), dim3(R.groups), dim3(256), 0, s, R.groups, R.group_offsets, R.group_size,
                       d_scores, d_poses_world, R.out_index, R.out_score, R.out_best_pose);
  HIP_TRY(hipGetLastError());
  return HSM_OK;
}

}  // namespace

// The batched match.  B.shared_n doubles as the sizing HINT for CSR input, whose per-scan lengths only the device knows (callers
// pass the typical beams per scan, 0 = unknown).  It only picks the kernel form: every form handles scans longer than the hint
// (the beams beyond the register/LDS-resident ones stream from memory).
int hsm_host::match_batch_device_nolock(hsm_ctx* h, const ScanBatch& B, const MatchOut& M, void* stream) {
  if (B.bad_shape() || !B.d_poses || !M.d_out_pose) return fail(HSM_ERR_INVALID, "hsm_match_batch_device: bad argument");
  if (B.batch == 0) return HSM_OK;
  if (int rc = select_device(h)) return rc;
  MatchParams P;
  memset(&P, 0, sizeof P);
  fill_schedule(h, P, true);
  P.batch = B.batch;
  P.begin_world = B.d_poses;
  P.pts = reinterpret_cast<const float2*>(B.d_pts);
  P.offsets = B.d_offsets;
  P.shared_n = B.shared_n;
  P.out_pose = M.d_out_pose;
  P.out_cov = M.d_out_cov;
  // a true bound of the scan lengths, where the host has one: a shared scan's length, or what the caller computed from host offsets
  P.n_bound = B.d_offsets ? M.n_bound : B.shared_n;
  if (M.xp) P.xp = *M.xp;
  h->batch.fused_exchange_done = false;
  // workgroup -> XCD mapping (beam_sample.h, xcd_block): chunks dealt to the XCDs in turn balance the data-dependent
  // per-scan time; maps whose touched region outgrows the L2s keep one contiguous eighth of the batch per XCD
  const bool outgrows = hsm_plan::level0_outgrows_l2(h->levels[0].cells());
  P.xcd_chunk = outgrows ? 0 : h->cfg.batch.xcd_chunk;
  P.wg_sync = h->cfg.batch.wg_sync >= 0 ? h->cfg.batch.wg_sync : (outgrows ? 1 : 0);
  P.clock_probe = h->batch.clock_probe;
  const int hint = B.shared_n > 0 ? B.shared_n : 1081;
  hipStream_t s = (hipStream_t)stream;
  MapReader reader;
  if (int rc = reader.begin(h, s, "hsm_match_batch_device")) return rc;
  if (int rc = launch_match(h, P, hint, s)) return rc;
  reader.queued();
  return HSM_OK;
}

// match -> `step` (the score or the covariance estimate) at the matched poses -> (R.groups > 0) the winner of every group by the
// pose's own likelihood, queued on `stream` under one lock.  Every argument is checked before the first launch, so a bad one
// queues nothing.
int hsm_host::match_chain_nolock(hsm_ctx* h, const ScanBatch& B, const MatchOut& M, const ScoringStep& step, const Ranking& R,
                                 void* stream) {
  if (int rc = scoring_level_check(h, step)) return rc;
  if (B.bad_shape() || !B.d_poses || !M.d_out_pose || step.no_output() || B.points_missing() ||
      R.bad_ranking(B.batch, step.likelihood()))
    return fail_at(HSM_ERR_INVALID, step.who, ": bad argument");
  if (int rc = match_batch_device_nolock(h, B, M, stream)) return rc;
  // the sizing hint of a CSR match means nothing to the scoring step: its kernel reads every scan's length from the offsets
  if (int rc = scoring_step_launch(h, step, B.at(M.d_out_pose), stream)) return rc;
  if (R.groups == 0) return HSM_OK;
  return select_best_device_nolock(h, R, step.likelihood(), M.d_out_pose, stream);
}

extern "C" {

// what hsm_match_score_batch asks for on top of hsm_match_batch (host pointers)
struct BatchScoreReq {
  int level;
  ScoreOut out;  // the residuals may be null
  Ranking rank;
};

// hsm_match_batch, and with `sr` hsm_match_score_batch: host arrays in (`B`, `M`: host pointers), one device call on the context's
// stream, results out
static int match_batch_host(hsm_ctx* h, const ScanBatch& B, const MatchOut& M, const BatchScoreReq* sr, const char* who) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  if (B.batch < 0 || !B.d_poses || !M.d_out_pose) return fail(HSM_ERR_INVALID, who);
  static const BatchScoreReq kNoScore = {};
  const BatchScoreReq& r = sr ? *sr : kNoScore;
  const Ranking& R = r.rank;
  const int batch = B.batch, G = R.groups;
  const int* scan_offsets = B.d_offsets;
  if (sr) {
    if (int rc = valid_level(h, r.level)) return rc;
    if (!r.out.d_likelihood || R.bad_ranking(batch, r.out.d_likelihood)) return fail(HSM_ERR_INVALID, who);
    if (G > 0 && R.group_offsets)
      for (int g = 0; g < G; ++g)
        if (R.group_offsets[g] < 0 || R.group_offsets[g] > R.group_offsets[g + 1] || R.group_offsets[g + 1] > batch)
          return fail(HSM_ERR_INVALID, who);
  }
  if (batch == 0) return HSM_OK;
  const int shared_n = B.shared_n > 0 ? B.shared_n : 0;
  const size_t total = scan_offsets ? (size_t)scan_offsets[batch] : (size_t)shared_n;
  if (total > 0 && !B.d_pts) return fail(HSM_ERR_INVALID, who);
  const MatchBatchStage st = match_batch_stage(batch, total, G, !scan_offsets, B.d_poses, B.d_pts, scan_offsets, M.d_out_pose, M.d_out_cov,
                                               r.out.d_likelihood, r.out.d_residual, R.group_offsets, R.out_index, R.out_score,
                                               R.out_best_pose);
  // the launches behind the copies in: x = the device address of the block, d_pts = that of the end points
  auto launch = [&](char* x, const float* d_pts, int n_or_hint, int n_bound) {
    const ScanBatch D{batch, staged<float>(x, st.begin), d_pts, staged<int>(x, st.offs, scan_offsets), n_or_hint};
    const MatchOut O{staged<float>(x, st.pose), staged<float>(x, st.cov, M.d_out_cov), n_bound};
    if (!sr) return match_batch_device_nolock(h, D, O, h->stream);
    const ScoringStep step{r.level, {staged<float>(x, st.lh), staged<float>(x, st.res, r.out.d_residual)}};
    const Ranking DR{G, staged<int>(x, st.goffs, R.group_offsets), R.group_size, staged<int>(x, st.idx),
                     staged<float>(x, st.bscore, R.out_score), staged<float>(x, st.bpose, R.out_best_pose)};
    return match_chain_nolock(h, D, O, step, DR, h->stream);
  };
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  if (!scan_offsets) {
    // Pose hypotheses of ONE scan (a particle filter's weighting step: BASELINE configs[2]): 12 bytes in and 12 (+36) bytes out
    // per hypothesis.  The start poses and the results live in pinned, device-mapped host memory -- every wavefront reads its
    // start pose once and writes its result once, so they cross PCIe exactly once without a copy command in front of or behind the
    // launch -- and only the scan (which every wavefront reads) is copied to the device.  4096 hypotheses of a 1081-beam scan:
    // one 8.6 KB copy + the launch, against three copies, the launch and two more copies of the general path below.
    // (With a score behind the match, its wavefront reads the matched pose back once and writes 4 or 8 bytes; the ranking reads
    // every likelihood once.)
    Buf<char>& hyp = h->batch.h_hyp_pinned;
    if (!hyp.holds(st.plan.total())) HIP_TRY(hipStreamSynchronize(h->stream));
    if (int rc = hyp.reserve(st.plan.total(), kHalfMore)) return rc;
    stage_fill_host(st.plan, hyp);
    char* dp = nullptr;
    HIP_TRY(hipHostGetDevicePointer((void**)&dp, hyp, 0));
    if (int rc = h->d_scan.reserve(total, kScanGrowth)) return rc;
    if (total) HIP_TRY(hipMemcpyAsync(h->d_scan, hyp + st.pts, total * sizeof(float2), hipMemcpyHostToDevice, h->stream));
    if (int rc = launch(dp, (const float*)h->d_scan.p, shared_n, 0)) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    stage_drain_host(st.plan, hyp);
    return HSM_OK;
  }
  if (int rc = h->d_batch.reserve(st.plan.total())) return rc;
  char* base = h->d_batch;
  if (int rc = stage_copy_in(st.plan, base, h->stream)) return rc;
  int hint = 0;
  for (int i = 0; i < batch; ++i) {
    const int ni = scan_offsets[i + 1] - scan_offsets[i];
    if (ni > hint) hint = ni;
  }
  if (int rc = launch(base, staged<float>(base, st.pts), hint, hint)) return rc;
  if (int rc = stage_copy_out(st.plan, base, h->stream)) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  return HSM_OK;
}

int hsm_match_batch_device(hsm_ctx* h, int batch, const float* d_begin_world, const float* d_pts_xy,
                           const int* d_scan_offsets, int shared_n, float* d_out_pose, float* d_out_cov,
                           void* stream) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  std::lock_guard<std::mutex> lk(h->mu);
  return match_batch_device_nolock(h, {batch, d_begin_world, d_pts_xy, d_scan_offsets, shared_n}, {d_out_pose, d_out_cov}, stream);
}

int hsm_match_batch_device_gather(hsm_ctx* h, int batch, const float* d_begin_world, const float* d_pts_xy,
                                  const int* d_scan_offsets, int shared_n, float* d_out_pose, float* d_out_cov,
                                  hsm_exchange* x, int first_row, int lag, float* d_out_all, void* stream) {
  if (!h || !x) return fail(HSM_ERR_INVALID, "null context / exchange");
  if (batch <= 0) return fail(HSM_ERR_INVALID, "hsm_match_batch_device_gather: every rank posts a non-empty shard");
  std::lock_guard<std::mutex> lk(h->mu);
  // The exchange step of this match: carried by the matcher launch itself where the form can (the exact-order batch forms: every
  // wavefront posts its pose from the kernel's epilogue, extra workgroups at the end of the grid unpack the epoch `lag` matches
  // back -- no launch of its own, nothing between two matcher launches), else one launch of the stand-alone exchange kernel behind it.
  ExchangeFused f;
  if (int rc = hsm_host::exchange_fused_begin(x, first_row, batch, lag, d_out_all, &f)) return rc;
  if (int rc = match_batch_device_nolock(h, {batch, d_begin_world, d_pts_xy, d_scan_offsets, shared_n}, {d_out_pose, d_out_cov, 0, &f},
                                         stream))
    return rc;
  if (h->batch.fused_exchange_done) {
    hsm_host::exchange_fused_commit(x, f);
    return HSM_OK;
  }
  return hsm_exchange_post_wait(x, d_out_pose, first_row, batch, lag, d_out_all, stream);
}

int hsm_score_batch_device(hsm_ctx* h, int level, int batch, const float* d_poses_world, const float* d_pts_xy,
                           const int* d_scan_offsets, int shared_n, float* d_out_likelihood, float* d_out_residual,
                           void* stream) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  std::lock_guard<std::mutex> lk(h->mu);
  const ScanBatch B{batch, d_poses_world, d_pts_xy, d_scan_offsets, shared_n};
  const ScoringStep step{level, {d_out_likelihood, d_out_residual}, {}, false, "hsm_score_batch_device"};
  if (int rc = scoring_step_check(h, step, B)) return rc;
  return scoring_step_launch(h, step, B, stream);
}

int hsm_covariance_batch_device(hsm_ctx* h, int level, int batch, const float* d_poses_world, const float* d_pts_xy,
                                const int* d_scan_offsets, int shared_n, float* d_out_cov_world, float* d_out_cov_map,
                                float* d_out_lh7, float* d_out_likelihood, void* stream) {
  if (!h) return fail(HSM_ERR_INVALID, "hsm_covariance_batch_device: null context");
  std::lock_guard<std::mutex> lk(h->mu);
  const ScanBatch B{batch, d_poses_world, d_pts_xy, d_scan_offsets, shared_n};
  const ScoringStep step{level, {}, {d_out_cov_world, d_out_cov_map, d_out_lh7, d_out_likelihood}, true, "hsm_covariance_batch_device"};
  if (int rc = scoring_step_check(h, step, B)) return rc;
  return scoring_step_launch(h, step, B, stream);
}

int hsm_select_best_device(hsm_ctx* h, int groups, const int* d_group_offsets, int group_size, const float* d_scores,
                           const float* d_poses_world, int* d_out_index, float* d_out_score, float* d_out_pose_world,
                           void* stream) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  std::lock_guard<std::mutex> lk(h->mu);
  return select_best_device_nolock(h, {groups, d_group_offsets, group_size, d_out_index, d_out_score, d_out_pose_world}, d_scores,
                                   d_poses_world, stream);
}

int hsm_match_score_batch_device(hsm_ctx* h, int batch, const float* d_begin_world, const float* d_pts_xy,
                                 const int* d_scan_offsets, int shared_n, float* d_out_pose, float* d_out_cov, int score_level,
                                 float* d_out_likelihood, float* d_out_residual, int groups, const int* d_group_offsets,
                                 int group_size, int* d_out_index, float* d_out_score, float* d_out_best_pose, void* stream) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  std::lock_guard<std::mutex> lk(h->mu);
  return match_chain_nolock(h, {batch, d_begin_world, d_pts_xy, d_scan_offsets, shared_n}, {d_out_pose, d_out_cov},
                            {score_level, {d_out_likelihood, d_out_residual}},
                            {groups, d_group_offsets, group_size, d_out_index, d_out_score, d_out_best_pose}, stream);
}

int hsm_match_cov_batch_device(hsm_ctx* h, int batch, const float* d_begin_world, const float* d_pts_xy, const int* d_scan_offsets,
                               int shared_n, float* d_out_pose, float* d_out_cov, int cov_level, float* d_out_cov_world,
                               float* d_out_cov_map, float* d_out_lh7, float* d_out_likelihood, int groups,
                               const int* d_group_offsets, int group_size, int* d_out_index, float* d_out_score,
                               float* d_out_best_pose, void* stream) {
  static const char* const who = "hsm_match_cov_batch_device";
  if (!h) return fail_at(HSM_ERR_INVALID, who, ": null context");
  std::lock_guard<std::mutex> lk(h->mu);
  return match_chain_nolock(h, {batch, d_begin_world, d_pts_xy, d_scan_offsets, shared_n}, {d_out_pose, d_out_cov},
                            {cov_level, {}, {d_out_cov_world, d_out_cov_map, d_out_lh7, d_out_likelihood}, true, who},
                            {groups, d_group_offsets, group_size, d_out_index, d_out_score, d_out_best_pose}, stream);
}

// host arrays in, covariance_batch_kernel on the context's stream, results out; synchronous
int hsm_covariance_batch(hsm_ctx* h, int level, int batch, const float* poses_world, const float* pts_xy, const int* scan_offsets,
                         int shared_n, float* out_cov_world, float* out_cov_map, float* out_lh7, float* out_likelihood) {
  static const char* const who = "hsm_covariance_batch";
  const ScanBatch B{batch, poses_world, pts_xy, scan_offsets, shared_n};
  if (int rc = scoring_step_check(h, {level, {}, {out_cov_world, out_cov_map, out_lh7, out_likelihood}, true, who}, B)) return rc;
  if (batch == 0) return HSM_OK;
  if (scan_offsets) {
    if (scan_offsets[0] != 0) return fail_at(HSM_ERR_INVALID, who, ": bad argument");
    for (int i = 0; i < batch; ++i)
      if (scan_offsets[i + 1] < scan_offsets[i]) return fail_at(HSM_ERR_INVALID, who, ": bad argument");
  }
  const size_t total = scan_offsets ? (size_t)scan_offsets[batch] : (size_t)shared_n;
  if (total > 0 && !pts_xy) return fail_at(HSM_ERR_INVALID, who, ": bad argument");
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  const CovarianceBatchStage st = covariance_batch_stage(batch, total, poses_world, pts_xy, scan_offsets, out_cov_world, out_cov_map,
                                                         out_lh7, out_likelihood);
  if (int rc = h->d_batch.reserve(st.plan.total())) return rc;
  char* base = h->d_batch;
  if (int rc = stage_copy_in(st.plan, base, h->stream)) return rc;
  const ScanBatch D{batch, staged<float>(base, st.poses), staged<float>(base, st.pts), staged<int>(base, st.offs, scan_offsets),
                    B.kernel_shared_n()};
  const CovOut d_out{staged<float>(base, st.cov_world, out_cov_world), staged<float>(base, st.cov_map, out_cov_map),
                     staged<float>(base, st.lh7, out_lh7), staged<float>(base, st.lh, out_likelihood)};
  if (int rc = scoring_step_launch(h, {level, {}, d_out, true, who}, D, h->stream)) return rc;
  if (int rc = stage_copy_out(st.plan, base, h->stream)) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  return HSM_OK;
}

int hsm_match_batch(hsm_ctx* h, int batch, const float* begin_world, const float* pts_xy,
                    const int* scan_offsets, int shared_n, float* out_pose, float* out_cov) {
  return match_batch_host(h, {batch, begin_world, pts_xy, scan_offsets, shared_n}, {out_pose, out_cov}, nullptr,
                          "hsm_match_batch: bad argument");
}

int hsm_match_score_batch(hsm_ctx* h, int batch, const float* begin_world, const float* pts_xy, const int* scan_offsets,
                          int shared_n, float* out_pose, float* out_cov, int score_level, float* out_likelihood,
                          float* out_residual, int groups, const int* group_offsets, int group_size, int* out_index,
                          float* out_score, float* out_best_pose) {
  const BatchScoreReq sr = {score_level, {out_likelihood, out_residual},
                            {groups, group_offsets, group_size, out_index, out_score, out_best_pose}};
  return match_batch_host(h, {batch, begin_world, pts_xy, scan_offsets, shared_n}, {out_pose, out_cov}, &sr,
                          "hsm_match_score_batch: bad argument");
}

// One scan on the levels selected in P.  `pts` is a device-accessible pointer (device memory or pinned
// mapped host memory), level-0 units.  Latency path of the ROS node: ONE kernel launch and one stream
// synchronise -- the start estimate travels in the kernel arguments and the kernel writes pose, H and
// the optional hook trace straight into the pinned h_small block.
// Completion of a single-scan match.  The kernel's last act is a system-scope release store of `seq` into
// the pinned result block, AFTER pose / cov / trace: polling that word returns the results a few
// microseconds before the end-of-kernel signal would (the queue's completion interrupt path is most of
// what hipStreamSynchronize waits for on a 25 us kernel).  Bounded: after 2 ms without the word the normal
// stream synchronisation takes over, which also surfaces a faulted kernel.  Later work on the stream
// stays ordered behind the kernel as usual.
static int wait_single_scan(hsm_ctx* h, unsigned seq) {
  if (h->cfg.single.spin_wait) {
    volatile unsigned* flag = reinterpret_cast<volatile unsigned*>(h->single.h_small + kDoneFlagOff);
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned it = 1;; ++it) {
      if (*flag == seq) {
        std::atomic_thread_fence(std::memory_order_acquire);
        return HSM_OK;
      }
      __builtin_ia32_pause();
      if ((it & 0xfff) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
    }
  }
  HIP_TRY(hipStreamSynchronize(h->stream));
  return HSM_OK;
}

static int match_single(hsm_ctx* h, MatchParams& P, const float begin_world[3], const float2* pts, int n,
                        float out_pose_world[3], float cov[9], float* trace = nullptr, int trace_steps = 0) {
  float* hs = h->single.h_small;
  float* hs_dev = nullptr;
  HIP_TRY(hipHostGetDevicePointer((void**)&hs_dev, hs, 0));
  P.batch = 1;
  P.begin_world = nullptr;
  P.begin_inline[0] = begin_world[0];
  P.begin_inline[1] = begin_world[1];
  P.begin_inline[2] = begin_world[2];
  P.pts = pts;
  P.offsets = nullptr;
  P.shared_n = n;
  P.n_bound = n;
  P.out_pose = hs_dev + 3;
  P.out_cov = hs_dev + 6;
  P.trace = trace_steps > 0 ? hs_dev + kTraceOff : nullptr;
  const unsigned seq = ++h->single.done_seq;
  P.done_flag = h->cfg.single.spin_wait ? reinterpret_cast<unsigned*>(hs_dev + kDoneFlagOff) : nullptr;
  P.done_seq = seq;
  P.err_flag = reinterpret_cast<unsigned*>(hs_dev + kErrFlagOff);
  P.coop_mute_block = h->single.coop_mute_block;
  P.clock_probe = h->batch.clock_probe;
  // which form: the site the scan was staged for (stage_scan), now with the trace
  MatchSite site = single_scan_site(h, n, trace_steps > 0);
  site.coop_skip = false;
  MatchPlan plan = plan_match(site);
  if (plan.family == Family::kCoop && h->single.coop_skip > 0) {  // backing off after an exchange timeout: this match goes straight to the one-workgroup form
    --h->single.coop_skip;
    site.coop_skip = true;
    plan = plan_match(site);
  }
  const bool coop_tried = plan.family == Family::kCoop;
  if (coop_tried) {
    // one dense scan spread over K workgroups of one launch (match_plan.h has the measurements)
    const int K = plan.grid;
    float* partials = h->single.d_partials;
    unsigned* bar_counter = reinterpret_cast<unsigned*>(h->single.d_partials + 2 * 64 * 12);
    unsigned bar_base = h->single.coop_bar_base;
    void* args[] = {(void*)&P, (void*)&partials, (void*)&bar_counter, (void*)&bar_base};
    const void* fn = h->cfg.layout == kLayoutPlane ? (const void*)gn_match_coop_kernel<kLayoutPlane, false>
                                                : (const void*)gn_match_coop_kernel<kLayoutQuad, false>;
    // The tagged-record exchange (default) has no grid barrier: a workgroup that is not resident yet only delays the others'
    // polls, which are bounded (a record that never arrives turns into an error return, err_flag) -- so it is an ORDINARY
    // launch: K <= 64 workgroups of 256 lanes are co-resident on an idle 256-CU device, and on a busy one they become so as
    // soon as other kernels retire.  (Round 3 launched it through hipLaunchCooperativeKernel: that goes through the
    // device's cooperative queue -- a slower launch, and a process that has used it segfaults in the runtime's exit
    // handlers when it runs under rocprofv3, profiles/r04/README.md.)  The counter-barrier form (HSM_COOP_TAGGED=0) spins
    // without a bound and keeps the cooperative launch's co-residency guarantee.
    hipError_t le;
    if (h->cfg.single.coop_tagged) {
      if (h->cfg.layout == kLayoutPlane)
        hipLaunchKernelGGL((gn_match_coop_kernel<kLayoutPlane, true>), dim3(K), dim3(256), 0, h->stream, P, partials, bar_counter, bar_base);
      else
        hipLaunchKernelGGL((gn_match_coop_kernel<kLayoutQuad, true>), dim3(K), dim3(256), 0, h->stream, P, partials, bar_counter, bar_base);
      le = hipGetLastError();
    } else {
      le = hipLaunchCooperativeKernel(fn, dim3(K), dim3(256), args, 0, h->stream);
    }
    if (le == hipSuccess) {
      unsigned steps = 0;
      for (int l = P.first_level; l >= P.last_level; --l) steps += (unsigned)P.lv[l].gn_steps;
      h->single.coop_bar_base += (unsigned)K * steps;  // one arrival per workgroup per GN step
      record_launch(h, plan);
    } else {
      // the runtime could not guarantee co-residency (device busy with other work): the one-workgroup
      // matcher computes the same thing on one CU
      (void)hipGetLastError();
      if (int rc = launch_match(h, P, n, h->stream)) return rc;
    }
  } else if (int rc = launch_match(h, P, n, h->stream)) {  // (plans the same site again, with the cooperative form ruled out)
    return rc;
  }
  if (int rc = wait_single_scan(h, seq)) return rc;
  h->upd.queued_update = false;  // the match kernel was the last thing on `stream`, and it has completed
  if (*reinterpret_cast<volatile unsigned*>(hs + kErrFlagOff) == seq) {
    // The multi-workgroup matcher's tagged exchange gave up waiting for a record: its K workgroups were not co-resident for
    // ~2^22 polls (a device shared with another process, or a long kernel of another stream holding the CUs -- an ordinary
    // launch carries no co-residency guarantee).  No pose was written.  The scan is matched again by the one-workgroup
    // matcher, which needs no other workgroup to make progress -- same sums in a different tree, so the caller gets a pose
    // within the fast mode's bar instead of an error (round-4 advisor); hsm_last_launch_config() then reports that form.
    const unsigned seq2 = ++h->single.done_seq;
    P.done_seq = seq2;
    if (int rc = launch_match(h, P, n, h->stream)) return rc;
    if (int rc = wait_single_scan(h, seq2)) return rc;
    ++h->single.coop_fallbacks;
    h->single.coop_backoff = h->single.coop_backoff ? (h->single.coop_backoff < 1024 ? 2 * h->single.coop_backoff : 1024) : 1;
    h->single.coop_skip = h->single.coop_backoff;
    {
      char b[200];
      snprintf(b, sizeof b, "hsm_match: the multi-workgroup matcher's exchange timed out (device shared or busy); re-ran on one workgroup, "
               "skipping that form for the next %u dense matches", h->single.coop_skip);
      set_error_text(b);  // (not an error return: the pose is valid; the text tells who asks why a match took long)
    }
    if (*reinterpret_cast<volatile unsigned*>(hs + kErrFlagOff) == seq2)
      return fail(HSM_ERR_HIP, "hsm_match: exchange timeout flagged by the one-workgroup matcher (cannot happen: it has no exchange)");
  }
  else if (coop_tried)
    h->single.coop_backoff = 0;  // an exchange completed: the device is ours again
  for (int i = 0; i < trace_steps * 12; ++i) trace[i] = hs[kTraceOff + i];
  out_pose_world[0] = hs[3];
  out_pose_world[1] = hs[4];
  out_pose_world[2] = hs[5];
  if (n != 0 && cov)
    for (int i = 0; i < 9; ++i) cov[i] = hs[6 + i];
  return HSM_OK;
}

// stage a host scan where the matcher can read it: pinned mapped host memory when the form planned for it reads it once
// (MatchPlan::reads_scan_once: no H2D copy command in front of the kernel), device memory otherwise
static int stage_scan(hsm_ctx* h, const float* pts_xy, int n, Buf<float2>& d_buf, const float2** out) {
  if (plan_match(single_scan_site(h, n)).reads_scan_once) {
    if (int rc = h->single.h_scan_pinned.reserve(n > 0 ? n : 1, kScanGrowth)) return rc;  // (1: also the empty first scan of a fresh context)
    if (n > 0) memcpy(h->single.h_scan_pinned, pts_xy, (size_t)n * sizeof(float2));
    float2* dev = nullptr;
    HIP_TRY(hipHostGetDevicePointer((void**)&dev, h->single.h_scan_pinned, 0));
    *out = dev;
    return HSM_OK;
  }
  if (int rc = d_buf.reserve((size_t)n, kScanGrowth)) return rc;
  if (n > 0) HIP_TRY(hipMemcpyAsync(d_buf, pts_xy, (size_t)n * sizeof(float2), hipMemcpyHostToDevice, h->stream));
  *out = d_buf;
  return HSM_OK;
}

// The retained scan of matchData when it has to live in device memory (dense scans, exact order): uploaded on the copy
// stream into the buffer the update kernels of the scan BEFORE are not reading, so that the copy runs while those kernels
// still occupy `stream` (in a match + update loop the upload of scan t + 1 used to wait behind the update of scan t: ~10 us of
// every configs[4] step).  Safe with two buffers: the kernels that read buffer A (match t, update t) are all ordered before
// match t + 1 on `stream`, and hsm_match returns only when match t + 1 has completed -- so when the upload of scan t + 2 is
// issued into A nothing reads it any more.  The staging block is pinned (a pageable hipMemcpyAsync would block the host
// until everything queued on its stream has completed) and free again for the same reason.
static int stage_scan_overlapped(hsm_ctx* h, const float* pts_xy, int n, const float2** out) {
  if (!h->single.copy_stream) {
    HIP_TRY(hipStreamCreateWithFlags(&h->single.copy_stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&h->single.copy_evt, hipEventDisableTiming));
  }
  std::swap(h->retained.d_retained, h->single.d_retained_alt);
  if (int rc = h->retained.d_retained.reserve((size_t)n, kScanGrowth)) return rc;
  if (!h->single.h_copy_pinned.holds((size_t)n)) HIP_TRY(hipStreamSynchronize(h->single.copy_stream));
  if (int rc = h->single.h_copy_pinned.reserve((size_t)n, kHalfMore)) return rc;
  memcpy(h->single.h_copy_pinned, pts_xy, (size_t)n * sizeof(float2));
  HIP_TRY(hipMemcpyAsync(h->retained.d_retained, h->single.h_copy_pinned, (size_t)n * sizeof(float2), hipMemcpyHostToDevice, h->single.copy_stream));
  HIP_TRY(hipEventRecord(h->single.copy_evt, h->single.copy_stream));
  HIP_TRY(hipStreamWaitEvent(h->stream, h->single.copy_evt, 0));
  *out = h->retained.d_retained;
  return HSM_OK;
}

// the containers of matchData: DataContainer::setFrom keeps scaled copies for the coarse levels (MapRepMultiMap.h:127);
// here: one level-0 copy, scaled by 2^-level on use
static void retain_scan(hsm_ctx* h, const float* pts_xy, int n, const float origo[2]) {
  if (h->levels.size() <= 1) return;
  h->retained.retained_pts.assign(pts_xy, pts_xy + 2 * (size_t)n);
  h->retained.retained_origo[0] = origo ? origo[0] : 0.0f;
  h->retained.retained_origo[1] = origo ? origo[1] : 0.0f;
  h->retained.retained_valid = true;
}

static int match_impl(hsm_ctx* h, const float begin_world[3], const float* pts_xy, int n, const float origo[2],
                      float out_pose_world[3], float cov[9], float* trace, int trace_steps,
                      const float2* d_prestaged = nullptr);

int hsm_match(hsm_ctx* h, const float begin_world[3], const float* pts_xy, int n, const float origo[2],
              float out_pose_world[3], float cov[9]) {
  return match_impl(h, begin_world, pts_xy, n, origo, out_pose_world, cov, nullptr, 0);
}

int hsm_match_trace(hsm_ctx* h, const float begin_world[3], const float* pts_xy, int n, const float origo[2],
                    float out_pose_world[3], float cov[9], float* trace, int trace_cap_steps, int* steps_written) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  const int steps = hsm_gn_iterations_per_match(h);
  if (!trace || !steps_written || trace_cap_steps < steps)
    return fail(HSM_ERR_INVALID, "hsm_match_trace: trace buffer smaller than hsm_gn_iterations_per_match()");
  *steps_written = n > 0 ? steps : 0;
  return match_impl(h, begin_world, pts_xy, n, origo, out_pose_world, cov, trace, n > 0 ? steps : 0);
}

static int match_impl(hsm_ctx* h, const float begin_world[3], const float* pts_xy, int n, const float origo[2],
                      float out_pose_world[3], float cov[9], float* trace, int trace_steps,
                      const float2* d_prestaged) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  if (!begin_world || !out_pose_world || n < 0 || (n > 0 && !pts_xy))
    return fail(HSM_ERR_INVALID, "hsm_match: bad argument");
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  retain_scan(h, pts_xy, n, origo);
  const float2* pts = d_prestaged;
  if (!pts) {
    // (the same rule as stage_scan's: scans the matcher reads once stay in pinned host memory)
    const bool to_device = !plan_match(single_scan_site(h, n)).reads_scan_once;
    // ... and only behind an update that was queued and not waited for (the match + update loop): on an idle stream the
    // extra hop through the copy stream's event costs ~10 us of latency and hides nothing (asking the runtime with
    // hipStreamQuery costs half of what the overlap gains: 0.1855 against 0.179 ms per configs[4] step)
    if (to_device && h->cfg.single.overlap_upload && n > 0 && h->upd.queued_update) {
      if (int rc = stage_scan_overlapped(h, pts_xy, n, &pts)) return rc;
    } else if (int rc = stage_scan(h, pts_xy, n, h->retained.d_retained, &pts)) {
      return rc;
    }
  }
  // the device copy of the retained scan is (re)uploaded lazily by the next update when the
  // matcher read the scan from pinned host memory
  h->retained.d_retained_current = h->levels.size() > 1 && pts == h->retained.d_retained;
  MatchParams P;
  memset(&P, 0, sizeof P);
  fill_schedule(h, P);
  return match_single(h, P, begin_world, pts, n, out_pose_world, cov, trace, trace_steps);
}

int hsm_match_level(hsm_ctx* h, int level, const float begin_world[3], const float* pts_level_xy, int n,
                    int max_iterations, float out_pose_world[3], float cov[9]) {
  if (int rc = valid_level(h, level)) return rc;
  if (!begin_world || !out_pose_world || n < 0 || max_iterations < 0 || (n > 0 && !pts_level_xy))
    return fail(HSM_ERR_INVALID, "hsm_match_level: bad argument");
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  const float2* pts = nullptr;
  if (int rc = stage_scan(h, pts_level_xy, n, h->d_scan, &pts)) return rc;
  MatchParams P;
  memset(&P, 0, sizeof P);
  P.lv[level] = level_view(h->levels[level], 1.0f, 1 + max_iterations);
  P.first_level = level;
  P.last_level = level;
  return match_single(h, P, begin_world, pts, n, out_pose_world, cov);
}

int hsm_match_ingested(hsm_ctx* h, const float begin_world[3], float out_pose_world[3], float cov[9]) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  if (h->ingest.ingest_n < 0) return fail(HSM_ERR_INVALID, "hsm_match_ingested: no scan ingested");
  static const float dummy[2] = {0.0f, 0.0f};
  const float* hp = h->ingest.ingest_n > 0 ? h->ingest.h_ingest.data() : dummy;
  return match_impl(h, begin_world, hp, h->ingest.ingest_n, h->ingest.ingest_origo, out_pose_world, cov, nullptr, 0, h->ingest.d_ingest);
}

int hsm_retain_scan(hsm_ctx* h, const float* pts_xy, int n, const float origo[2]) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  if (n < 0 || (n > 0 && !pts_xy)) return fail(HSM_ERR_INVALID, "hsm_retain_scan: bad argument");
  std::lock_guard<std::mutex> lk(h->mu);
  retain_scan(h, pts_xy, n, origo);
  h->retained.d_retained_current = false;  // (never true on a one-level map)
  return HSM_OK;
}

}  // extern "C"
