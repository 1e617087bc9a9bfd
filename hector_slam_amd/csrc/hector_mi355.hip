// hector_mi355.hip -- host runtime + C ABI (include/hector_mi355/capi.h) of the
// MI355X-native hector_mapping scan matcher.  Kernels: gn_match.h, map_update.h; the batch / team matcher forms are
// launched from match_exact_cached.hip and match_teams.hip, the probes and test hooks are in probes.hip, the multi-GPU group in
// group.hip, raw-scan conversion in ingest.hip, the occupancy exports in occupancy.hip (hsm_ctx.h says which unit holds what).
//
// The context mirrors hectorslam::MapRepMultiMap (HSL/slam_main/MapRepMultiMap.h): a
// pyramid of levels, each with its grid (log-odds + update stamps), its world<->map
// transforms (HSL/map/GridMapBase.h:265-280) and the update counters of
// OccGridMapBase (HSL/map/OccGridMapBase.h:264-266).  All planes live in HBM; the
// host keeps only scalars.  There is no CPU compute path.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see build.py).
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

#include "gn_match.h"
#include "gn_match_spec.h"
#include "hector_mi355/capi.h"
#include "hsm_ctx.h"
#include "hsm_host.h"
#include "map_update.h"

namespace {

using namespace hsm;
using namespace hsm_host;

thread_local std::string g_last_error;

}  // namespace

// every object of the library reports through this per-thread text (hsm_host.h)
int hsm_host::fail(int code, const char* what, hipError_t e) {
  char buf[512];
  if (e != hipSuccess)
    snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
  else
    snprintf(buf, sizeof buf, "%s", what);
  g_last_error = buf;
  return code;
}

int hsm_host::fail_at(int code, const char* who, const char* text, hipError_t e) {
  char buf[512];
  snprintf(buf, sizeof buf, "%s%s", who, text);
  return fail(code, buf, e);
}

void hsm_host::set_error_text(const char* text) { g_last_error = text; }

namespace {

float prob_to_log_odds(float prob) {  // GridMapLogOdds.h:196-200 (float log overload)
  float odds = prob / (1.0f - prob);
  return logf(odds);
}

// GridMapBase::setMapTransformation (GridMapBase.h:265-280) with Eigen's evaluation
// order: mapTworld = Scaling(s,s) * Translation(off); worldTmap = mapTworld.inverse()
void set_map_transformation(Level& L, float offx, float offy, float cell_length) {
  L.cell_length = cell_length;
  L.scale_to_map = 1.0f / cell_length;
  const float s = L.scale_to_map;
  Affine2 m;
  m.l00 = s;
  m.l10 = 0.0f;
  m.l01 = 0.0f;
  m.l11 = s;
  m.t0 = s * offx;
  m.t1 = s * offy;
  L.mapTworld = m;
  const float det = m.l00 * m.l11 - m.l10 * m.l01;
  const float invdet = 1.0f / det;
  Affine2 w;
  w.l00 = m.l11 * invdet;
  w.l10 = -m.l10 * invdet;
  w.l01 = -m.l01 * invdet;
  w.l11 = m.l00 * invdet;
  w.t0 = (-w.l00) * m.t0 + (-w.l01) * m.t1;
  w.t1 = (-w.l10) * m.t0 + (-w.l11) * m.t1;
  L.worldTmap = w;
}

}  // namespace

// (declared in hsm_ctx.h: the other units use these too)
namespace hsm_host {

LevelRW level_rw(const Level& L) {
  LevelRW v;
  v.logodds = L.d_logodds;
  v.update_index = L.d_update_index;
  v.prob = L.d_prob;
  v.quad = L.d_quad;
  v.key_free = L.d_key_free;
  v.key_occ = L.d_key_occ;
  v.occ_bits = L.d_occ_bits;
  v.free_bytes = L.d_free_bytes;
  v.sx = L.sx;
  v.sy = L.sy;
  v.tiles_x = L.tiles_x();
  v.kf_tiles_x = key_free_tiles_x(L.sx);
  v.quad_texels = L.quad_texels();
  return v;
}

LevelView level_view(const Level& L, float pt_scale, int gn_steps) {
  LevelView v;
  v.quad = L.d_quad;
  v.prob = L.d_prob;
  v.sx = L.sx;
  v.sy = L.sy;
  v.tiles_x = L.tiles_x();
  v.quad_texels = L.quad_texels();
  v.limx = L.limx;
  v.limy = L.limy;
  v.mapTworld = L.mapTworld;
  v.worldTmap = L.worldTmap;
  v.pt_scale = pt_scale;
  v.gn_steps = gn_steps;
  return v;
}

int grid_for(size_t n, int block) {
  size_t g = (n + block - 1) / block;
  if (g > 256 * 8) g = 256 * 8;  // grid-stride the rest (guide, Guideline 11)
  if (g < 1) g = 1;
  return (int)g;
}

int rebuild_probability(hsm_ctx* h, Level& L) {
  hipLaunchKernelGGL(rebuild_prob_kernel, dim3(grid_for(L.cells())), dim3(256), 0, h->stream, level_rw(L));
  if (L.d_quad)
    hipLaunchKernelGGL(rebuild_quad_kernel, dim3(grid_for(L.cells())), dim3(256), 0, h->stream, level_rw(L));
  HIP_TRY(hipGetLastError());
  return HSM_OK;
}

// HSM_PARITY_AUTO (the default): EVERY match -- batched, single scan, dense scan, and the likelihood / covariance / Hessian
// entry points -- takes the reference's summation order: bit-identical to the reference CPU matcher on every entry point.
// History: round 3 chose exact order only on maps of more than 2^23 cells (a rule fitted to BASELINE's own scenes); round 4's scene
// sweep (tools/parity_scene_sweep.py, profiles/r04/parity_scene_sweep.jsonl) found the fast tree beyond 1e-4 m of the reference in
// every scene family for some set-up -- wherever the reference's own Gauss-Newton iteration has not settled -- and no property of
// the map or the batch known at launch separates those scans, so every batch went exact; single scans kept the tree on the evidence
// of 256 scans per family, of which the corridor family already failed (0.83 within 1e-4 m).  Round 5: the same argument holds for
// one scan as for 4096, so the default does not try there either.  HSM_PARITY_FAST / _RELAXED stay opt-in for callers who trade
// the guarantee for speed (profiles/r05/README.md has the prices: batch +34 % / +45 %, single 1081-beam scan ~35 vs ~95 us).
// AUTO and HSM_PARITY_EXACT launch the same kernels today; the distinction kept in the API is one of contract: AUTO promises the
// reference's BITS by whatever form delivers them, EXACT names the reference's order of additions.
// The effective order is an INPUT of the plan (MatchSite::exact) -- the context's flags are never changed by a launch
// (hsm_parity() reads them without the mutex) -- and is recorded for hsm_last_launch_parity().
bool wants_exact(const hsm_ctx* h) { return h->exact || h->auto_parity; }

// every cell of the level may have changed (create, reset, upload): host mirrors and the published grid take all of it
void whole_level_changed(Level& L, bool mirror) {
  const int all[4] = {0, 0, L.sx - 1, L.sy - 1};
  for (int k = 0; k < 4; ++k) {
    if (mirror) L.dirty[k] = all[k];
    L.pub[k] = all[k];
  }
}

int valid_level(const hsm_ctx* h, int level) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  if (level < 0 || level >= (int)h->levels.size()) return fail(HSM_ERR_INVALID, "level out of range");
  return HSM_OK;
}

int select_device(const hsm_ctx* h) {
  HIP_TRY(hipSetDevice(h->device));
  return HSM_OK;
}

}  // namespace hsm_host

namespace {

int fill_level(hsm_ctx* h, Level& L) {  // GridMapBase::clear + LogOddsCell::resetGridCell
  hipLaunchKernelGGL(fill_level_kernel, dim3(grid_for(L.cells())), dim3(256), 0, h->stream, level_rw(L),
                     0.0f, -1);
  HIP_TRY(hipGetLastError());
  return HSM_OK;
}

void free_level(Level& L, TeardownLog* log = nullptr) {
  TEARDOWN(log, hipFree(L.d_logodds));
  TEARDOWN(log, hipFree(L.d_update_index));
  TEARDOWN(log, hipFree(L.d_prob));
  TEARDOWN(log, hipFree(L.d_quad));
  TEARDOWN(log, hipFree(L.d_key_free));
  TEARDOWN(log, hipFree(L.d_key_occ));
  TEARDOWN(log, hipFree(L.d_occ_bits));
  TEARDOWN(log, hipFree(L.d_free_bytes));
  L = Level();
}

static_assert(hsm_plan::kQuad == kLayoutQuad && hsm_plan::kPlane == kLayoutPlane && hsm_plan::kExactGroupRounds == kExactGroupRounds &&
                  hsm_plan::kDenseRound == kDenseRound && hsm_plan::kSpec1MaxBeams == kSpec1MaxBeams,
              "match_plan.h restates gn_match.h / gn_match_spec.h");
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
  s.batch = batch, s.max_n = max_n, s.n_bound = n_bound;
  s.exact = wants_exact(h), s.relaxed = h->relaxed, s.layout = h->layout;
  s.batched = batched, s.trace = trace, s.clock_probe = h->clock_probe != nullptr;
  s.capturing = h->exact_spec && stream_capturing(stream);
  s.compute_units = h->compute_units, s.level0_cells = h->levels[0].cells();
  s.wps_override = h->wps_override, s.bpl_override = h->bpl_override;
  s.texel_cache = h->texel_cache, s.exact_cached = h->exact_cached;
  s.exact_chain_wave = h->exact_chain_wave != 0, s.exact_split_tail = h->exact_split_tail != 0;
  s.exact_dense = h->exact_dense, s.exact_dense_min = h->exact_dense_min;
  s.exact_spec = h->exact_spec, s.exact_spec1 = h->exact_spec1;
  s.spb_large = h->spb_large, s.coop_min_beams = h->coop_min_beams, s.coop_skip = h->coop_skip > 0;
  return s;
}
MatchSite single_scan_site(const hsm_ctx* h, int n, bool trace = false) { return match_site(h, 1, n, n, false, trace, h->stream); }

// what hsm_last_launch_config / _kernel / _parity report: the plan that was launched
void record_launch(hsm_ctx* h, const MatchPlan& plan) {
  for (int i = 0; i < 6; ++i) h->last_cfg[i] = plan.record[i];
  h->last_kernel = plan.name;
  h->last_parity = plan.parity;
}

// the one-workgroup-per-scan forms of this unit: Family::kExactDense, kSpec (gn_match.h, gn_match_spec.h: `batch` workgroups) and
// kSpec1 (one scan)
int launch_workgroup_form(hsm_ctx* h, MatchParams P, MatchPlan& plan, const MatchSite& site, hipStream_t stream) {
  if (plan.family == Family::kSpec) {
    // The product scratch is the launching stream's own (two streams' launches would write the same rows at once).  A launch into a
    // graph capture was planned in the literal form, which needs no scratch: a graph never reads a block that an eager launch grows
    // (frees), and nothing is allocated or synchronised while the caller captures.  A ninth stream falls to it here.
    hsm_ctx::SpecScratch* sb = nullptr;
    for (hsm_ctx::SpecScratch& b : h->spec_scratch)
      if (b.s == stream) sb = &b;
    if (!sb && h->spec_scratch.size() < 8) {
      h->spec_scratch.push_back({stream, {}});
      sb = &h->spec_scratch.back();
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
      P.spec_stats = h->d_spec_stats;
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
  h->last_sorted = false;  // (the forms that take a permuted batch set it: ensure_batch_perm)
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
  for (int l = 0; l < nl; ++l) {
    // static_cast<float>(1.0 / pow(2.0, level)) -- a power of two, exact in fp32
    const float factor = (float)(1.0 / pow(2.0, (double)l));
    P.lv[l] = level_view(h->levels[l], factor, l == 0 ? 6 : 4);
  }
  P.first_level = nl - 1;
  P.last_level = 0;
  if (batched && h->sched_level >= 0 && h->sched_level < nl) {
    P.lv[h->sched_level].gn_steps = h->sched_steps;
    P.first_level = P.last_level = h->sched_level;
  }
}

// acc = the hull of acc and b ({x0, y0, x1, y1} inclusive, empty where x1 < x0); b is not empty
void box_widen(int acc[4], const int b[4]) {
  if (acc[2] < acc[0]) {
    for (int k = 0; k < 4; ++k) acc[k] = b[k];
    return;
  }
  if (b[0] < acc[0]) acc[0] = b[0];
  if (b[1] < acc[1]) acc[1] = b[1];
  if (b[2] > acc[2]) acc[2] = b[2];
  if (b[3] > acc[3]) acc[3] = b[3];
}

// OccGridMapBase::updateByScan on one level (OccGridMapBase.h:121-168), host side, in two steps so that the GPU can
// start on the scan while the host is still busy:
//   prepare_level()  counters, the pose transform, the begin cell and everything the MARK pass needs -> batch.lv[]
//                    (every level with n > 0; the box fields are left empty)
//   -- the mark pass of all levels is launched here --
//   level_bbox()     the cell box of everything the scan can touch (what the dense APPLY / texel passes run over):
//                    computed on the host from the host copy of the endpoints while the mark pass runs, or derived
//                    from a finer level's box (see below)
// pts are LEVEL-0 endpoints on the device; pt_scale/origo bring them to this level.
struct LevelPrep {
  int level = -1;
  int slot = -1;          // index in batch.lv, -1 = nothing to launch for this level (empty scan)
  const float* h_pts = nullptr;
  int n = 0;
  bool derivable = false;  // set by level_bbox(): coarser levels of the same container may derive their box from this one
};

// The marks of an update -- mark bytes (dense scans), end-cell bitmap bits (keyed form) -- are cleared by the apply pass of the
// SAME update and carry no generation tag.  If that pass never ran over them (a HIP error between the two launches, or a box
// the host found empty) they would be applied by a later scan as spurious free / occupied updates.  The level remembers that
// a mark pass is outstanding; the next update on it then clears both mark planes first and widens the rows the key-wrap
// clear covers to the whole level (the failed update's keys carry an older generation and are ignored as such).
int scrub_marks(hsm_ctx* h, Level& L) {
  HIP_TRY(hipMemsetAsync(L.d_free_bytes, 0, mark_plane_bytes(L.sx, L.sy), h->stream));
  HIP_TRY(hipMemsetAsync(L.d_occ_bits, 0, ((L.cells() + 31) / 32 + 1) * sizeof(unsigned int), h->stream));
  L.key_rows[0] = 0;
  L.key_rows[1] = L.sy - 1;
  L.marks_pending = false;
  return HSM_OK;
}

int prepare_level(hsm_ctx* h, UpdateBatch& batch, LevelPrep& prep, int level, const float pose_world[3],
                  const float2* d_pts, const float* h_pts, int n, float pt_scale, const float origo_level[2]) {
  Level& L = h->levels[level];
  prep.level = level;
  prep.slot = -1;
  prep.h_pts = h_pts;
  prep.n = n;
  L.curr_mark_free = L.curr_update_index + 1;
  L.curr_mark_occ = L.curr_update_index + 2;
  if (L.stamps_ahead()) batch.stamped = 1;  // a restored stamp >= this scan's free mark
  float mx, my;
  affine_apply_host(L.mapTworld, pose_world[0], pose_world[1], mx, my);  // getMapCoordsPose
  const float mth = pose_world[2];
  // Translation2f(mapPose.xy) * Rotation2Df(mapPose.theta): host float sin/cos like the reference
  Affine2 T;
  const float sinA = sinf(mth), cosA = cosf(mth);
  T.l00 = cosA;
  T.l01 = -sinA;
  T.l10 = sinA;
  T.l11 = cosA;
  T.t0 = mx;
  T.t1 = my;
  float bx, by;
  affine_apply_host(T, origo_level[0], origo_level[1], bx, by);
  L.bbox[0] = L.bbox[1] = 0;
  L.bbox[2] = L.bbox[3] = -1;
  if (n > 0) {
    if (n > HSM_MAX_UPDATE_BEAMS) return fail(HSM_ERR_TOO_LARGE, "update_by_scan: more than HSM_MAX_UPDATE_BEAMS beams");
    if (L.marks_pending)
      if (int rc = scrub_marks(h, L)) return rc;
    if (++L.serial > kSerialMax) {
      // key generation wrapped (every 4095 updates of a level): clear the rows that carry keys -- the union of the update
      // boxes since the last clear, not the whole planes (an 8192^2 level would be a 512 MB memset in the middle of a
      // 40 Hz update stream)
      if (L.key_rows[1] >= L.key_rows[0]) {
        const size_t y0 = (size_t)L.key_rows[0], y1 = (size_t)L.key_rows[1];
        HIP_TRY(hipMemsetAsync(L.d_key_occ + y0 * L.sx, 0, (y1 - y0 + 1) * L.sx * sizeof(unsigned int), h->stream));
        const size_t row_words = (size_t)key_free_tiles_x(L.sx) * 32u;  // one row of 8x4-cell tiles
        HIP_TRY(hipMemsetAsync(L.d_key_free + (y0 >> 2) * row_words, 0, ((y1 >> 2) - (y0 >> 2) + 1) * row_words * sizeof(unsigned int), h->stream));
      }
      L.key_rows[0] = 0;
      L.key_rows[1] = -1;
      L.serial = 1;
    }
    UpdateParams P;
    P.lv = level_rw(L);
    P.pose = T;
    P.pts = d_pts;
    P.n = n;
    P.pt_scale = pt_scale;
    P.bx = (int)(bx + 0.5f);
    P.by = (int)(by + 0.5f);
    P.serial = L.serial;
    P.log_odds_free = L.log_odds_free;
    P.log_odds_occ = L.log_odds_occ;
    P.mark_free = L.curr_mark_free;
    P.mark_occ = L.curr_mark_occ;
    P.x0 = P.y0 = 0;
    P.x1 = P.y1 = -1;  // empty box until level_bbox(): the dense passes skip the level
    P.recs = nullptr;  // dense scans: set by launch_update_mark()
    prep.slot = batch.nlev;
    batch.lv[batch.nlev++] = P;
    L.marks_pending = true;  // until the apply pass over this level's box is queued (update_applied)
  }
  L.last_update_index++;     // setUpdated(), GridMapBase.h:343
  L.curr_update_index += 3;  // OccGridMapBase.h:167
  return HSM_OK;
}

// Box of level prep.level.  `finer` != nullptr: the level sees the SAME container as the finer level `finer`
// describes, scaled by a power of two -- then every fp32 value of this level's endpoint arithmetic is exactly the
// finer level's value times 2^-k (products and sums of exactly scaled operands), so cell = (int)(e * 2^-k + 0.5)
// with the finer cell (int)(e + 0.5) in [x0, x1] lies in [(x0 >> k) - 1, (x1 >> k) + 1]: a conservative box without
// touching the endpoints again (a superset only costs the dense passes a few rows of untouched cells).
//   The derivation needs the finer level to have SEEN every beam the coarser one accepts.  The low map edge breaks that:
//   (int) truncates towards zero, so level 0 keeps an end point e (cell units, before the + 0.5) with e > -1.5 while
//   level k keeps e * 2^-k > -1.5, i.e. e > -1.5 * 2^k -- a beam (or the begin cell) just outside the low x / y edge of
//   level 0 is dropped there and valid on the coarser levels (the high edge only gets stricter with k).  level 0's own
//   pass therefore records whether it rejected anything on the low side (prep.derivable); if so the coarser levels walk
//   the end points themselves.
void level_bbox(hsm_ctx* h, UpdateBatch& batch, LevelPrep& prep, const UpdateParams* finer, int shift) {
  prep.derivable = false;
  if (prep.slot < 0) return;
  Level& L = h->levels[prep.level];
  UpdateParams& P = batch.lv[prep.slot];
  const int bxi = P.bx, byi = P.by;
  const bool begin_in = bxi >= 0 && bxi < L.sx && byi >= 0 && byi < L.sy;
  int x0 = L.sx, y0 = L.sy, x1 = -1, y1 = -1;
  if (begin_in && finer) {
    if (finer->x1 >= finer->x0) {
      x0 = (finer->x0 >> shift) - 1;
      y0 = (finer->y0 >> shift) - 1;
      x1 = (finer->x1 >> shift) + 1;
      y1 = (finer->y1 >> shift) + 1;
      if (x0 < 0) x0 = 0;
      if (y0 < 0) y0 = 0;
      if (x1 > L.sx - 1) x1 = L.sx - 1;
      if (y1 > L.sy - 1) y1 = L.sy - 1;
    }
  } else if (begin_in) {
    // every in-map end cell (a Bresenham line stays inside the box of its end points).  Same fp32 expressions as
    // beam_line(); pure index work.  (Beams that end in the begin cell are skipped by the kernels; the begin cell is
    // in the box anyway.)
    const float fsx = (float)L.sx + 2.0f, fsy = (float)L.sy + 2.0f;
    const float* h_pts = prep.h_pts;
    const float pt_scale = P.pt_scale;
    bool low_reject = false;  // a beam this level drops at its low x / y edge (a coarser level may keep it)
    for (int i = 0; i < prep.n; ++i) {
      float ex, ey;
      affine_apply_host(P.pose, h_pts[2 * i] * pt_scale, h_pts[2 * i + 1] * pt_scale, ex, ey);
      ex += 0.5f;
      ey += 0.5f;
      low_reject |= (ex <= -1.0f) | (ey <= -1.0f);
      if (!(ex > -2.0f && ex < fsx && ey > -2.0f && ey < fsy)) continue;
      const int exi = (int)ex, eyi = (int)ey;
      if (exi < 0 || exi >= L.sx || eyi < 0 || eyi >= L.sy) continue;
      if (exi < x0) x0 = exi;
      if (exi > x1) x1 = exi;
      if (eyi < y0) y0 = eyi;
      if (eyi > y1) y1 = eyi;
    }
    prep.derivable = !low_reject;
  }
  if (x1 >= 0) {  // at least one beam ends inside the map
    L.bbox[0] = P.x0 = x0 < bxi ? x0 : bxi;
    L.bbox[1] = P.y0 = y0 < byi ? y0 : byi;
    L.bbox[2] = P.x1 = x1 > bxi ? x1 : bxi;
    L.bbox[3] = P.y1 = y1 > byi ? y1 : byi;
    if (L.key_rows[1] < L.key_rows[0]) {
      L.key_rows[0] = L.bbox[1];
      L.key_rows[1] = L.bbox[3];
    } else {
      if (L.bbox[1] < L.key_rows[0]) L.key_rows[0] = L.bbox[1];
      if (L.bbox[3] > L.key_rows[1]) L.key_rows[1] = L.bbox[3];
    }
    box_widen(L.dirty, L.bbox);
    box_widen(L.pub, L.bbox);
  }
}

// dense scans (>= merged_mark_max beams) take the byte-map form of the update (map_update.h), on every map width since round 4;
// env HSM_DENSE_BITS=0 keeps them on the keyed one-launch mark pass of the small scans
bool use_dense_bits(const hsm_ctx* h, const UpdateBatch& batch, int max_n) {
  if (!h->dense_bits || max_n < h->merged_mark_max) return false;
  for (int i = 0; i < batch.nlev; ++i)
    if (batch.lv[i].lv.free_bytes == nullptr) return false;
  return true;
}

// pass 1 of map_update.h for all levels of the batch (grid.y = level): needs no box
int launch_update_mark(hsm_ctx* h, UpdateBatch& batch) {
  if (batch.nlev == 0) return HSM_OK;
  int max_n = 0;
  for (int i = 0; i < batch.nlev; ++i)
    if (batch.lv[i].n > max_n) max_n = batch.lv[i].n;
  const unsigned ny = (unsigned)batch.nlev;
  if (use_dense_bits(h, batch, max_n)) {
    // per-beam records: written by the end-cell pass, read by the line walk (one block of max_n records per level)
    if (!h->d_beam_recs.holds((size_t)max_n * HSM_MAX_LEVELS))
      if (int rc = h->d_beam_recs.reserve(grown_capacity((size_t)max_n, kHalfMore) * HSM_MAX_LEVELS)) return rc;
    const size_t per_level = h->d_beam_recs.count() / HSM_MAX_LEVELS;
    for (int i = 0; i < batch.nlev; ++i) batch.lv[i].recs = h->d_beam_recs + (size_t)i * per_level;
    hipLaunchKernelGGL(update_mark_occ_dense_kernel, dim3((max_n + 255) / 256, ny), dim3(256), 0, h->stream, batch);
    // x extent a multiple of 8: workgroup b of every level then runs on XCD b % 8 (the kernel's beam -> XCD mapping)
    hipLaunchKernelGGL(update_mark_free_dense_kernel, dim3(mark_dense_blocks(max_n), ny), dim3(256), 0, h->stream, batch);
    HIP_TRY(hipGetLastError());
    return HSM_OK;
  }
  // small scans (and HSM_DENSE_BITS=0): end-cell marks and line walks in ONE launch (keyed atomics, map_update.h) -- one
  // dependent launch less
  const unsigned occ_blocks = (unsigned)(max_n + 255) / 256;
  hipLaunchKernelGGL(update_mark_kernel, dim3(occ_blocks + (max_n + 3) / 4, ny), dim3(256), 0, h->stream, batch, occ_blocks);
  HIP_TRY(hipGetLastError());
  return HSM_OK;
}

// passes 2 (+ 3) over the boxes level_bbox() filled in; levels with an empty box return at once
int launch_update_apply(hsm_ctx* h, const UpdateBatch& batch) {
  size_t max_box = 0;
  for (int i = 0; i < batch.nlev; ++i) {
    const UpdateParams& P = batch.lv[i];
    if (P.x1 < P.x0) continue;
    const size_t box = (size_t)(P.x1 - P.x0 + 2) * (size_t)(P.y1 - P.y0 + 2);
    if (box > max_box) max_box = box;
  }
  if (max_box == 0) return HSM_OK;
  const unsigned ny = (unsigned)batch.nlev;
  int max_n = 0;
  for (int i = 0; i < batch.nlev; ++i)
    if (batch.lv[i].n > max_n) max_n = batch.lv[i].n;
  if (use_dense_bits(h, batch, max_n)) {
    // one wavefront per block of 256 cells of the widened box (32 x 8 cells: two 16 x 8 mark tiles; map_update.h)
    const int g = grid_for(max_box / 4 + 4096);
    auto dense = h->layout == kLayoutQuad ? (batch.stamped ? update_apply_dense_kernel<true, true> : update_apply_dense_kernel<true, false>)
                                          : (batch.stamped ? update_apply_dense_kernel<false, true> : update_apply_dense_kernel<false, false>);
    hipLaunchKernelGGL(dense, dim3(g, ny), dim3(256), 0, h->stream, batch);
    HIP_TRY(hipGetLastError());
    return HSM_OK;
  }
  if (h->layout == kLayoutQuad && max_n < h->scatter_texels_max) {
    // the apply pass writes the texels itself: one dependent launch less for the launch-bound small scans (1081 beams,
    // 3 levels: complete 39 -> 34.5 us) and one dense pass less for the big ones (16 k beams on 8192^2: 0.51 -> 0.45 ms)
    auto apply = batch.stamped ? update_apply_kernel<true, true> : update_apply_kernel<true, false>;
    hipLaunchKernelGGL(apply, dim3(grid_for(max_box), ny), dim3(256), 0, h->stream, batch);
  } else {
    auto apply = batch.stamped ? update_apply_kernel<false, true> : update_apply_kernel<false, false>;
    hipLaunchKernelGGL(apply, dim3(grid_for(max_box), ny), dim3(256), 0, h->stream, batch);
    if (h->layout == kLayoutQuad)
      hipLaunchKernelGGL(update_texels_kernel, dim3(grid_for(max_box), ny), dim3(256), 0, h->stream, batch);
  }
  HIP_TRY(hipGetLastError());
  return HSM_OK;
}

// the apply pass of this level is queued behind its mark pass: its marks will be cleared.  A level whose box the host found
// EMPTY has no apply pass and needs none: the box is the hull of every in-map end cell, computed by level_bbox() from the same
// fp32 expressions the mark kernels evaluate (beam_line), and a beam whose end cell -- or the begin cell -- lies outside the map
// is dropped whole on the device as in the reference (OccGridMapBase.h:176-188); the non-empty case already relies on that
// equality (a mark outside the host's box would never be applied either).  Until round 4 such a level stayed "pending" and the
// NEXT update scrubbed both mark planes and widened the key rows to the whole level -- tens of MB of memset per level and update
// for as long as the robot stood outside a coarse level, or every scan was empty (round-4 advisor).  What remains pending is the
// case the flag exists for: a HIP error between the mark launch and the apply launch (the caller sees the error; the next
// update on the level scrubs first).
void update_applied(hsm_ctx* h, const UpdateBatch& batch, const LevelPrep& prep) {
  if (prep.slot < 0) return;
  h->levels[prep.level].marks_pending = false;
}

}  // namespace

namespace hsm_host {

// for map_shift.hip: hsm_create's transforms of a level for other offsets, and the clear of marks a failed update left behind
void set_level_transformation(Level& L, float offx, float offy, float cell_length) { set_map_transformation(L, offx, offy, cell_length); }
int scrub_pending_marks(hsm_ctx* h, Level& L) { return scrub_marks(h, L); }

// every writer of the map queues behind a batch match that a caller-owned stream may still be running, and
// bumps the epoch the next such match orders itself behind
int order_after_foreign_match(hsm_ctx* h) {
  // Refused, before anything is queued, while a caller's stream that this context has matched on is being captured into a graph:
  // a marker recorded on that stream would go into the capture, and the context's stream, waiting for it, would join the capture.
  for (const hsm_ctx::ForeignStream& f : h->foreign)
    if (stream_capturing(f.s))
      return fail(HSM_ERR_INVALID, "map update while a caller's stream that this context matches on is being captured into a graph: "
                                   "end the capture first (the caller orders replays against updates)");
  for (hsm_ctx::ForeignStream& f : h->foreign) {
    if (!f.pending) continue;
    // everything the caller has queued on that stream up to now (a superset of our matches); the wait captures
    // the event's state at this call, so one event serves all streams in turn
    if (!h->evt_foreign) HIP_TRY(hipEventCreateWithFlags(&h->evt_foreign, hipEventDisableTiming));
    if (hipEventRecord(h->evt_foreign, f.s) == hipSuccess) {
      HIP_TRY(hipStreamWaitEvent(h->stream, h->evt_foreign, 0));
    } else {  // the caller destroyed the stream meanwhile: its work has been flushed or is covered by a device sync
      (void)hipGetLastError();
      HIP_TRY(hipDeviceSynchronize());
    }
    f.pending = false;
  }
  if (h->foreign.size() > 16) h->foreign.clear();  // nothing pending any more: forget streams callers may have destroyed
  ++h->upd_epoch;
  return HSM_OK;
}

// Device-side updates (hsm_update_by_scans_device) leave their cell boxes on the device: the host never sees their poses.  Whoever
// needs Level::bbox / Level::dirty -- the box getters, and every host-side writer of them -- first waits for the context's stream
// and merges slot 0 (the running dirty boxes) and slot 1 (the last scan's boxes) of d_upd_boxes: one 256-byte copy.  Callers test
// upd_boxes_outstanding themselves, so a context that never took a device-side update pays one branch.
int merge_device_boxes(hsm_ctx* h) {
  if (int rc = select_device(h)) return rc;
  int host[2 * kMaxLevels * 4];
  HIP_TRY(hipMemcpyAsync(host, h->d_upd_boxes, sizeof host, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  hipLaunchKernelGGL(update_boxes_clear_kernel, dim3(1), dim3(64), 0, h->stream, h->d_upd_boxes, kMaxLevels);
  HIP_TRY(hipGetLastError());
  for (size_t l = 0; l < h->levels.size(); ++l) {
    Level& L = h->levels[l];
    const int* run = host + 4 * l;
    const int* last = host + 4 * (kMaxLevels + l);
    if (last[2] >= last[0]) {
      for (int k = 0; k < 4; ++k) L.bbox[k] = last[k];
    } else {
      L.bbox[0] = L.bbox[1] = 0;
      L.bbox[2] = L.bbox[3] = -1;
    }
    if (run[2] >= run[0]) box_widen(L.dirty, run);
  }
  h->upd_boxes_outstanding = false;
  return HSM_OK;
}

// Gated updates (hsm_update_by_scans_device_gated, hsm_slam_scans_device) count the scans they integrate on the device: the
// host never sees their decisions.  Whoever needs the levels' update counters on the host -- prepare_level, the ungated
// hsm_update_by_scans_device, hsm_update_index, reset and upload -- first waits for the context's stream, fetches the count and
// folds it in: OccGridMapBase.h:123-124, :167 and setUpdated() (GridMapBase.h:343) that many times.  Callers test
// gate_outstanding themselves, so a context that never made a gated call pays one branch.  *state: the block as fetched.
int fold_gate_counters(hsm_ctx* h, GateState* state) {
  if (int rc = select_device(h)) return rc;
  GateState host;
  HIP_TRY(hipMemcpyAsync(&host, h->d_gate, sizeof host, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (state) *state = host;
  const int applied = host.pending;
  if (applied > 0) {
    HIP_TRY(hipMemsetAsync(&h->d_gate->pending, 0, sizeof(int), h->stream));  // ahead of every later gated call
    for (Level& L : h->levels) {
      L.curr_mark_free = L.curr_update_index + 3 * (applied - 1) + 1;
      L.curr_mark_occ = L.curr_update_index + 3 * (applied - 1) + 2;
      L.curr_update_index += 3 * applied;
      L.last_update_index += applied;
    }
    h->gate_applied_total += applied;
    if (state) state->pending = 0;
  }
  h->gate_outstanding = false;
  return HSM_OK;
}

// the context's stream behind the caller's: the inputs are complete where `s` stands now
int wait_for_caller_inputs(hsm_ctx* h, hipStream_t s) {
  if (s == h->stream) return HSM_OK;
  if (!h->evt_inputs) HIP_TRY(hipEventCreateWithFlags(&h->evt_inputs, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(h->evt_inputs, s));
  HIP_TRY(hipStreamWaitEvent(h->stream, h->evt_inputs, 0));
  return HSM_OK;
}

// the refusals of a scan-log call, before anything is queued: `s` or a stream this context has matched on is being captured
int slam_refuse_capture(hsm_ctx* h, hipStream_t s, const char* who) {
  if (stream_capturing(s))
    return fail_at(HSM_ERR_INVALID, who, ": `stream` is being captured into a graph (map updates are not captured)");
  for (const hsm_ctx::ForeignStream& f : h->foreign)  // (order_after_foreign_match)
    if (stream_capturing(f.s))
      return fail_at(HSM_ERR_INVALID, who, ": a caller's stream that this context matches on is being captured into a graph");
  return HSM_OK;
}

// the caller's stream behind the context's (the results are complete where the context's stream stands now)
int slam_caller_waits(hsm_ctx* h, hipStream_t s) {
  if (s == h->stream) return HSM_OK;
  if (!h->evt_slam_done) HIP_TRY(hipEventCreateWithFlags(&h->evt_slam_done, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(h->evt_slam_done, h->stream));
  HIP_TRY(hipStreamWaitEvent(s, h->evt_slam_done, 0));
  return HSM_OK;
}

}  // namespace hsm_host

namespace {

// the UpdateBatch blocks and cell boxes of `count` scans (hsm_ctx::d_upd_batches / d_upd_boxes)
int ensure_update_scans(hsm_ctx* h, size_t count) {
  if (h->d_upd_boxes && h->d_upd_batches.holds(count)) return HSM_OK;
  if (h->upd_boxes_outstanding)  // the running boxes live in the block that is about to go
    if (int rc = merge_device_boxes(h)) return rc;
  if (int rc = h->d_upd_boxes.drop()) return rc;  // (both go before either comes back: the box block stands for the pair)
  if (int rc = h->d_upd_batches.drop()) return rc;
  const size_t want = grown_capacity(count, {64, 50});
  if (int rc = h->d_upd_batches.reserve(want)) return rc;
  if (int rc = h->d_upd_boxes.reserve((want + 2) * kMaxLevels * 4)) return rc;
  hipLaunchKernelGGL(update_boxes_clear_kernel, dim3(1), dim3(64), 0, h->stream, h->d_upd_boxes, 2 * kMaxLevels);
  HIP_TRY(hipGetLastError());
  return HSM_OK;
}

// the key planes of a whole level back to zero: the key generation of a device-side update wrapped.  The WHOLE level, not the
// rows that carry keys: those rows are known on the device only, and a wrap is one scan in 4095.
int clear_key_planes(hsm_ctx* h, Level& L) {
  HIP_TRY(hipMemsetAsync(L.d_key_occ, 0, L.cells() * sizeof(unsigned int), h->stream));
  HIP_TRY(hipMemsetAsync(L.d_key_free, 0, key_free_cells(L.sx, L.sy) * sizeof(unsigned int), h->stream));
  return HSM_OK;
}

int reset_update_gate(hsm_ctx* h) {
  hipLaunchKernelGGL(update_gate_reset_kernel, dim3(1), dim3(64), 0, h->stream, h->d_gate);
  HIP_TRY(hipGetLastError());
  return HSM_OK;
}

}  // namespace

// Orders a launch on `s` that READS the map (a batched match, a batched score, the rays of rays.hip) against the map updates,
// which are queued on the context's own stream.  *mark = the stream's record where the launch has to be remembered for the next
// update (`(*mark)->pending = true` once it is queued), nullptr where nothing is to be remembered (the context's own stream; a
// capture).
int hsm_host::order_map_reader(hsm_ctx* h, hipStream_t s, const char* who, hsm_ctx::ForeignStream** mark) {
  *mark = nullptr;
  if (s == h->stream) return HSM_OK;
  // A caller-owned stream is not ordered against the context's own one, on which map updates are queued
  // (hsm_update_by_scan returns before they ran): order the launch behind the updates queued so far, and
  // leave a marker the next update waits for, so that it does not rewrite the map under a running reader.
  hsm_ctx::ForeignStream* fs = nullptr;
  for (hsm_ctx::ForeignStream& f : h->foreign)
    if (f.s == s) fs = &f;
  if (!fs) {
    h->foreign.push_back({s, 0ull, false});
    fs = &h->foreign.back();
  }
  if (stream_capturing(s)) {
    // A launch into a graph capture runs at the caller's replays, not now: it neither records that the stream is ordered behind
    // the updates nor leaves a marker for the next update (either would describe work only the graph holds).  The updates queued
    // so far are waited for on the host instead -- a wait node on an event recorded outside the capture would order the graph
    // but not the stream's later eager launches.  Later updates and the replays are ordered by the caller; while the capture
    // lasts, updates are refused (order_after_foreign_match).
    hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
    HIP_TRY(hipThreadExchangeStreamCaptureMode(&mode));
    const hipError_t e = hipStreamSynchronize(h->stream);
    (void)hipThreadExchangeStreamCaptureMode(&mode);
    if (e != hipSuccess) return fail_at(HSM_ERR_HIP, who, ": waiting for the queued map updates at capture", e);
    return HSM_OK;
  }
  // (what test_queued_updates_are_ordered_against_caller_streams holds)
  if (fs->ordered_epoch != h->upd_epoch) {  // THIS stream has not been ordered behind the latest map writes yet
    if (!h->evt_updates) HIP_TRY(hipEventCreateWithFlags(&h->evt_updates, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(h->evt_updates, h->stream));
    HIP_TRY(hipStreamWaitEvent(s, h->evt_updates, 0));
    fs->ordered_epoch = h->upd_epoch;
  }
  // no marker here (an event record between back-to-back launches costs 2-3 us of kernel time each): the
  // next writer of the map records one on every stream with a pending reader (order_after_foreign_match)
  *mark = fs;
  return HSM_OK;
}

int hsm_host::match_batch_device_nolock(hsm_ctx* h, int batch, const float* d_begin_world, const float* d_pts_xy,
                                        const int* d_scan_offsets, int shared_n, float* d_out_pose,
                                        float* d_out_cov, void* stream, int n_bound, const ExchangeFused* xp) {
  if (batch < 0 || !d_begin_world || !d_out_pose || (!d_scan_offsets && shared_n < 0))
    return fail(HSM_ERR_INVALID, "hsm_match_batch_device: bad argument");
  if (batch == 0) return HSM_OK;
  if (int rc = select_device(h)) return rc;
  MatchParams P;
  memset(&P, 0, sizeof P);
  fill_schedule(h, P, true);
  P.batch = batch;
  P.begin_world = d_begin_world;
  P.pts = reinterpret_cast<const float2*>(d_pts_xy);
  P.offsets = d_scan_offsets;
  P.shared_n = shared_n;
  P.out_pose = d_out_pose;
  P.out_cov = d_out_cov;
  // a true bound of the scan lengths, where the host has one: a shared scan's length, or what the caller computed from host offsets
  P.n_bound = d_scan_offsets ? n_bound : shared_n;
  if (xp) P.xp = *xp;
  h->fused_exchange_done = false;
  // workgroup -> XCD mapping (gn_match.h, xcd_block): chunks dealt to the XCDs in turn balance the data-dependent
  // per-scan time; maps whose touched region outgrows the L2s keep one contiguous eighth of the batch per XCD
  const bool outgrows = hsm_plan::level0_outgrows_l2(h->levels[0].cells());
  P.xcd_chunk = outgrows ? 0 : h->xcd_chunk;
  P.wg_sync = h->wg_sync >= 0 ? h->wg_sync : (outgrows ? 1 : 0);
  P.clock_probe = h->clock_probe;
  // per-scan length is only known on the device for CSR input; shared_n doubles as the sizing HINT there
  // (callers pass the typical beams per scan, 0 = unknown).  It only picks the kernel form: every form handles
  // scans longer than the hint (the beams beyond the register/LDS-resident ones stream from memory).
  const int hint = shared_n > 0 ? shared_n : 1081;
  hipStream_t s = (hipStream_t)stream;
  hsm_ctx::ForeignStream* fs = nullptr;
  if (int rc = order_map_reader(h, s, "hsm_match_batch_device", &fs)) return rc;
  if (int rc = launch_match(h, P, hint, s)) return rc;
  if (fs) fs->pending = true;
  return HSM_OK;
}

extern "C" {

const char* hsm_last_error(void) { return g_last_error.c_str(); }
const char* hsm_version(void) { return "hector_mi355 0.1 (gfx950)"; }

int hsm_create(float map_resolution, int size_x, int size_y, unsigned levels, float start_x, float start_y,
               const hsm_opts* opts, hsm_ctx** out) {
  if (!out) return fail(HSM_ERR_INVALID, "hsm_create: out is null");
  *out = nullptr;
  if (levels < 1 || levels > HSM_MAX_LEVELS || size_x < 2 || size_y < 2 || !(map_resolution > 0.0f))
    return fail(HSM_ERR_INVALID, "hsm_create: bad map geometry");
  // the samplers address texels with a 32-bit byte offset (16 B per cell) and 24-bit multiplies
  if (size_x >= (1 << 24) || size_y >= (1 << 24) || ((size_t)size_x + 3) * ((size_t)size_y + 1) >= ((size_t)1 << 28))
    return fail(HSM_ERR_TOO_LARGE, "hsm_create: map larger than 2^28 cells");
  if ((size_x >> (levels - 1)) < 2 || (size_y >> (levels - 1)) < 2)
    return fail(HSM_ERR_INVALID, "hsm_create: too many levels for this map size");
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev < 1)
    return fail(HSM_ERR_NO_DEVICE, "hsm_create: no HIP device (this library has no CPU path)", e);
  hsm_ctx* h = new hsm_ctx();
  if (opts && opts->device >= 0) {
    h->device = opts->device;
  } else {
    if (hipGetDevice(&h->device) != hipSuccess) h->device = 0;
  }
  if (h->device >= ndev) {
    delete h;
    return fail(HSM_ERR_INVALID, "hsm_create: device ordinal out of range");
  }
  {  // (a partition of the device -- CPX mode -- reports its own CU count; 256 on a whole MI355X)
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) == hipSuccess && cus > 0) h->compute_units = cus;
  }
  int layout = opts ? opts->layout : HSM_LAYOUT_AUTO;
  if (layout == HSM_LAYOUT_AUTO) {
    const char* env = getenv("HSM_LAYOUT");
    layout = (env && strcmp(env, "plane") == 0) ? HSM_LAYOUT_PLANE : HSM_LAYOUT_QUAD;
  }
  h->layout = layout == HSM_LAYOUT_PLANE ? kLayoutPlane : kLayoutQuad;
  int wps = opts ? opts->waves_per_scan : 0;
  if (wps == 0) {
    const char* env = getenv("HSM_WPS");
    if (env) wps = atoi(env);
  }
  if (wps != 0 && wps != 1 && wps != 2 && wps != 4 && wps != 8 && wps != 16) {
    delete h;
    return fail(HSM_ERR_INVALID, "hsm_create: waves_per_scan must be 0,1,2,4,8,16");
  }
  h->wps_override = wps;
  if (const char* env = getenv("HSM_BPL")) h->bpl_override = atoi(env) == 0 ? 0 : -1;
  if (const char* env = getenv("HSM_COOP_MIN")) h->coop_min_beams = atoi(env);
  if (const char* env = getenv("HSM_COOP_TAGGED")) h->coop_tagged = atoi(env) != 0;
  if (const char* env = getenv("HSM_SPIN_WAIT")) h->spin_wait = atoi(env) != 0;
  if (const char* env = getenv("HSM_ASYNC_UPDATE")) h->async_update = atoi(env) != 0;
  if (const char* env = getenv("HSM_OVERLAP_UPLOAD")) h->overlap_upload = atoi(env) != 0;
  if (const char* env = getenv("HSM_TEXEL_CACHE")) h->texel_cache = atoi(env) != 0;
  if (const char* env = getenv("HSM_UPDATE_ZEROCOPY_MAX")) h->update_zero_copy_max = atoi(env);
  if (const char* env = getenv("HSM_PARITY")) {
    // only the four documented words change the mode; anything else ("Exact", "1", a typo) must not silently select the
    // fast tree: the context is refused
    const bool is_exact = strcmp(env, "exact") == 0, is_relaxed = strcmp(env, "relaxed") == 0, is_auto = strcmp(env, "auto") == 0;
    if (!is_exact && !is_relaxed && !is_auto && strcmp(env, "fast") != 0) {
      delete h;
      return fail(HSM_ERR_INVALID, "hsm_create: HSM_PARITY must be one of auto, fast, exact, relaxed");
    }
    h->exact = is_exact;
    h->relaxed = is_relaxed;
    h->auto_parity = is_auto;
  }
  if (const char* env = getenv("HSM_BATCH_ORDER")) {
    if (strcmp(env, "auto") == 0) h->batch_order = HSM_ORDER_AUTO;
    else if (strcmp(env, "given") == 0) h->batch_order = HSM_ORDER_GIVEN;
    else if (strcmp(env, "morton") == 0) h->batch_order = HSM_ORDER_MORTON;
    else {
      delete h;
      return fail(HSM_ERR_INVALID, "hsm_create: HSM_BATCH_ORDER must be one of auto, given, morton");
    }
  }
  if (const char* env = getenv("HSM_BATCH_ORDER_MIN")) h->batch_order_min = atoi(env);
  if (const char* env = getenv("HSM_BATCH_ORDER_REFRESH")) h->batch_order_refresh = atoi(env) > 0 ? atoi(env) : 1;
  if (const char* env = getenv("HSM_MERGED_MARK_MAX")) h->merged_mark_max = atoi(env);
  if (const char* env = getenv("HSM_SCATTER_TEXELS_MAX")) h->scatter_texels_max = atoi(env);
  if (const char* env = getenv("HSM_DENSE_BITS")) h->dense_bits = atoi(env) != 0;
  if (const char* env = getenv("HSM_EXACT_CACHED")) h->exact_cached = atoi(env) != 0;
  if (const char* env = getenv("HSM_EXACT_DENSE")) h->exact_dense = atoi(env) != 0;
  if (const char* env = getenv("HSM_EXACT_SPEC")) h->exact_spec = atoi(env) != 0;
  if (const char* env = getenv("HSM_EXACT_SPEC1")) h->exact_spec1 = atoi(env) != 0;
  if (const char* env = getenv("HSM_EXACT_DENSE_MIN")) h->exact_dense_min = atoi(env);
  if (const char* env = getenv("HSM_EXACT_CHAIN_WAVE")) h->exact_chain_wave = atoi(env);
  if (const char* env = getenv("HSM_EXACT_SPLIT_TAIL")) h->exact_split_tail = atoi(env);
  if (const char* env = getenv("HSM_WG_SYNC")) h->wg_sync = atoi(env) != 0;
  if (const char* env = getenv("HSM_SPB_LARGE")) h->spb_large = atoi(env) == 8 ? 8 : 4;
  if (const char* env = getenv("HSM_XCD_CHUNK")) h->xcd_chunk = atoi(env) > 0 ? atoi(env) : 0;
  if (const char* env = getenv("HSM_CAST_FORM")) h->cast_form = !strcmp(env, "wave") ? 0 : (!strcmp(env, "lane") ? 1 : -1);
  if (const char* env = getenv("HSM_WINDOW_FORM")) h->window_form = !strcmp(env, "wave") ? 0 : (!strcmp(env, "lane") ? 1 : -1);
  if (const char* env = getenv("HSM_XCD_CHUNK_EXACT")) h->xcd_chunk_exact = atoi(env) > 0 ? atoi(env) : 0;
  if (const char* env = getenv("HSM_COPY_STAGE")) h->copy_stage = atoi(env) != 0;

#define CREATE_TRY(expr)                                   \
  do {                                                     \
    hipError_t e__ = (expr);                               \
    if (e__ != hipSuccess) {                               \
      int rc__ = fail(HSM_ERR_HIP, #expr, e__);            \
      hsm_destroy(h);                                      \
      return rc__;                                         \
    }                                                      \
  } while (0)

  CREATE_TRY(hipSetDevice(h->device));
  CREATE_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  CREATE_TRY(hipMalloc((void**)&h->d_small, kSmallFloats * sizeof(float)));
  CREATE_TRY(hipMalloc((void**)&h->d_partials, 2 * 64 * 12 * sizeof(float) + 64));  // [2][64] records of 3 x {p,p,p,tag}; + the grid-barrier counter
  CREATE_TRY(hipMemset(h->d_partials, 0, 2 * 64 * 12 * sizeof(float) + 64));
  CREATE_TRY(hipHostMalloc((void**)&h->h_small, kSmallFloats * sizeof(float),
                           hipHostMallocMapped | hipHostMallocCoherent));
  memset(h->h_small, 0, kSmallFloats * sizeof(float));
  CREATE_TRY(hipMalloc((void**)&h->d_gate, sizeof(GateState)));
  CREATE_TRY(hipMemsetAsync(h->d_gate, 0, sizeof(GateState), h->stream));
  hipLaunchKernelGGL(update_gate_reset_kernel, dim3(1), dim3(64), 0, h->stream, h->d_gate);
  CREATE_TRY(hipGetLastError());
  CREATE_TRY(hipMalloc((void**)&h->d_pub_boxes, 3 * kMaxLevels * 4 * sizeof(int)));
  hipLaunchKernelGGL(update_boxes_clear_kernel, dim3(1), dim3(64), 0, h->stream, h->d_pub_boxes, 2 * kMaxLevels);
  CREATE_TRY(hipGetLastError());

  // MapRepMultiMap ctor (MapRepMultiMap.h:48-72)
  int rx = size_x, ry = size_y;
  const float total_x = map_resolution * (float)size_x;
  const float mid_offset_x = total_x * start_x;
  const float total_y = map_resolution * (float)size_y;
  const float mid_offset_y = total_y * start_y;
  h->levels.resize(levels);
  h->start[0] = start_x;
  h->start[1] = start_y;
  for (unsigned i = 0; i < levels; ++i) {
    Level& L = h->levels[i];
    L.sx = rx;
    L.sy = ry;
    L.limx = (float)rx - 2.0f;  // MapDimensionProperties::setMapCellDims (:70-74)
    L.limy = (float)ry - 2.0f;
    set_map_transformation(L, mid_offset_x, mid_offset_y, map_resolution);
    L.log_odds_free = prob_to_log_odds(0.4f);  // GridMapLogOdds.h:117-118
    L.log_odds_occ = prob_to_log_odds(0.6f);
    const size_t n = L.cells();
    CREATE_TRY(hipMalloc((void**)&L.d_logodds, n * sizeof(float)));
    CREATE_TRY(hipMalloc((void**)&L.d_update_index, n * sizeof(int)));
    // the samplers point out-of-map beams at an all-zero footprint stored BEHIND the planes
    // (gn_match.h sample_fetch): one extra texel, resp. sizeX + 2 extra cells, zeroed once here
    CREATE_TRY(hipMalloc((void**)&L.d_prob, (n + (size_t)rx + 2) * sizeof(float)));
    CREATE_TRY(hipMemsetAsync(L.d_prob + n, 0, ((size_t)rx + 2) * sizeof(float), h->stream));
    if (h->layout == kLayoutQuad) {
      // HSM_LAYOUT_PLANE samples the probability plane directly (4 gathers per beam) and keeps NO texel plane:
      // 16 B/cell less memory and one dense pass less per update -- the better trade for update-heavy use
      // (single dense scans); the quad layout is the better one for batched matching
      CREATE_TRY(hipMalloc((void**)&L.d_quad, ((size_t)L.quad_texels() + 1) * sizeof(float4)));
      CREATE_TRY(hipMemsetAsync(L.d_quad + L.quad_texels(), 0, sizeof(float4), h->stream));
    }
    CREATE_TRY(hipMalloc((void**)&L.d_key_free, key_free_cells(L.sx, L.sy) * sizeof(unsigned int)));
    CREATE_TRY(hipMalloc((void**)&L.d_key_occ, n * sizeof(unsigned int)));
    CREATE_TRY(hipMemsetAsync(L.d_key_free, 0, key_free_cells(L.sx, L.sy) * sizeof(unsigned int), h->stream));
    CREATE_TRY(hipMemsetAsync(L.d_key_occ, 0, n * sizeof(unsigned int), h->stream));
    CREATE_TRY(hipMalloc((void**)&L.d_occ_bits, ((n + 31) / 32 + 1) * sizeof(unsigned int)));
    CREATE_TRY(hipMemsetAsync(L.d_occ_bits, 0, ((n + 31) / 32 + 1) * sizeof(unsigned int), h->stream));
    CREATE_TRY(hipMalloc((void**)&L.d_free_bytes, mark_plane_bytes(L.sx, L.sy)));
    CREATE_TRY(hipMemsetAsync(L.d_free_bytes, 0, mark_plane_bytes(L.sx, L.sy), h->stream));
    if (fill_level(h, L) != HSM_OK) {
      hsm_destroy(h);
      return HSM_ERR_HIP;
    }
    whole_level_changed(L, false);  // the first export of a level is all of it (a mirror starts from the same cleared map: not dirty)
    CREATE_TRY(hipMemcpyAsync(h->d_pub_boxes + (2 * kMaxLevels + i) * 4, L.pub, sizeof L.pub, hipMemcpyHostToDevice, h->stream));
    rx /= 2;
    ry /= 2;
    map_resolution *= 2.0f;
  }
  CREATE_TRY(hipStreamSynchronize(h->stream));
#undef CREATE_TRY
  *out = h;
  return HSM_OK;
}

void hsm_destroy(hsm_ctx* h) {
  if (!h) return;
  TeardownLog log_, *log = &log_;
  TEARDOWN(log, hipSetDevice(h->device));
  if (h->stream) TEARDOWN(log, hipStreamSynchronize(h->stream));
  if (h->copy_stream) TEARDOWN(log, hipStreamSynchronize(h->copy_stream));
  for (Level& L : h->levels) free_level(L, log);
  for (GrowBuf* b : h->bufs) b->release(log);  // every grow-on-demand block of the context (hsm_ctx.h)
  for (hsm_ctx::SpecScratch& b : h->spec_scratch) b.d.release(log);
  for (hsm_ctx::PermBuf& b : h->perm_bufs) b.d.release(log);
  for (hsm_ctx::RangesGeometry& g : h->ranges_geoms) TEARDOWN(log, hipFree(g.d));
  for (hsm_ctx::RangesTfGeometry& g : h->ranges_tf_geoms) TEARDOWN(log, hipFree(g.d));
  TEARDOWN(log, hipFree(h->d_spec_stats));
  TEARDOWN(log, hipFree(h->d_small));
  TEARDOWN(log, hipFree(h->d_partials));
  TEARDOWN(log, hipFree(h->d_gate));
  TEARDOWN(log, hipFree(h->d_pub_boxes));
  if (h->h_small) TEARDOWN(log, hipHostFree(h->h_small));
  for (hipEvent_t e : {h->copy_evt, h->evt_updates, h->evt_foreign, h->evt_inputs, h->evt_slam_done, h->upd_evt[0], h->upd_evt[1],
                       h->evt_copy_read, h->evt_copy_src})
    if (e) TEARDOWN(log, hipEventDestroy(e));
  if (h->copy_stream) TEARDOWN(log, hipStreamDestroy(h->copy_stream));
  if (h->stream) TEARDOWN(log, hipStreamDestroy(h->stream));
  delete h;
  if (!log_.first.empty()) {
    g_last_error = "hsm_destroy: " + log_.first;
    (void)hipGetLastError();  // consumed here, not by the next caller's launch check
  }
}

int hsm_reset(hsm_ctx* h) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  if (h->upd_boxes_outstanding)
    if (int rc = merge_device_boxes(h)) return rc;
  if (h->gate_outstanding)
    if (int rc = fold_gate_counters(h)) return rc;
  if (int rc = order_after_foreign_match(h)) return rc;
  if (int rc = reset_update_gate(h)) return rc;
  for (Level& L : h->levels) {
    if (int rc = fill_level(h, L)) return rc;
    L.uploaded_stamp_max = -1;  // every stamp is -1 again
    whole_level_changed(L);
  }
  HIP_TRY(hipStreamSynchronize(h->stream));
  return HSM_OK;
}

int hsm_levels(const hsm_ctx* h) { return h ? (int)h->levels.size() : 0; }
float hsm_scale_to_map(const hsm_ctx* h) { return h ? h->levels[0].scale_to_map : 0.0f; }

int hsm_set_update_factor_free(hsm_ctx* h, float f) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  std::lock_guard<std::mutex> lk(h->mu);
  for (Level& L : h->levels) L.log_odds_free = prob_to_log_odds(f);
  return HSM_OK;
}
int hsm_set_update_factor_occupied(hsm_ctx* h, float f) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  std::lock_guard<std::mutex> lk(h->mu);
  for (Level& L : h->levels) L.log_odds_occ = prob_to_log_odds(f);
  return HSM_OK;
}
int hsm_on_map_updated(hsm_ctx* h) { return h ? HSM_OK : fail(HSM_ERR_INVALID, "null context"); }

int hsm_set_parity(hsm_ctx* h, int mode) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  if (mode != HSM_PARITY_FAST && mode != HSM_PARITY_EXACT && mode != HSM_PARITY_RELAXED && mode != HSM_PARITY_AUTO)
    return fail(HSM_ERR_INVALID, "hsm_set_parity: unknown mode");
  std::lock_guard<std::mutex> lk(h->mu);
  h->exact = mode == HSM_PARITY_EXACT;
  h->relaxed = mode == HSM_PARITY_RELAXED;
  h->auto_parity = mode == HSM_PARITY_AUTO;
  return HSM_OK;
}
int hsm_parity(const hsm_ctx* h) {
  if (!h) return HSM_PARITY_FAST;
  return h->exact ? HSM_PARITY_EXACT : (h->relaxed ? HSM_PARITY_RELAXED : (h->auto_parity ? HSM_PARITY_AUTO : HSM_PARITY_FAST));
}

int hsm_last_launch_parity(const hsm_ctx* h) { return h ? h->last_parity : HSM_PARITY_FAST; }

int hsm_set_batch_order(hsm_ctx* h, int order) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  if (order != HSM_ORDER_GIVEN && order != HSM_ORDER_MORTON && order != HSM_ORDER_AUTO) return fail(HSM_ERR_INVALID, "hsm_set_batch_order: unknown order");
  std::lock_guard<std::mutex> lk(h->mu);
  h->batch_order = order;
  for (hsm_ctx::PermBuf& b : h->perm_bufs) b.batch = 0;
  return HSM_OK;
}
int hsm_set_batch_order_refresh(hsm_ctx* h, int launches) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  if (launches < 1) return fail(HSM_ERR_INVALID, "hsm_set_batch_order_refresh: at least 1");
  std::lock_guard<std::mutex> lk(h->mu);
  h->batch_order_refresh = launches;
  for (hsm_ctx::PermBuf& b : h->perm_bufs) b.batch = 0;  // (the next launch computes a fresh one)
  return HSM_OK;
}
int hsm_batch_order(const hsm_ctx* h) { return h ? h->batch_order : HSM_ORDER_AUTO; }
int hsm_last_launch_sorted(const hsm_ctx* h) { return h && h->last_sorted ? 1 : 0; }

int hsm_set_clock_probe(hsm_ctx* h, unsigned long long* d_stamps4) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  std::lock_guard<std::mutex> lk(h->mu);
  h->clock_probe = d_stamps4;
  return HSM_OK;
}

int hsm_device_info(const hsm_ctx* h, int info[4]) {
  if (!h || !info) return fail(HSM_ERR_INVALID, "null argument");
  hipDeviceProp_t p;
  HIP_TRY(hipGetDeviceProperties(&p, h->device));
  info[0] = h->device;
  info[1] = p.multiProcessorCount;
  info[2] = p.clockRate;        // kHz
  info[3] = p.memoryClockRate;  // kHz
  return HSM_OK;
}

int hsm_gn_iterations_per_match(const hsm_ctx* h) {
  return h ? 6 + 4 * ((int)h->levels.size() - 1) : 0;
}
const char* hsm_last_launch_kernel(const hsm_ctx* h) { return h ? h->last_kernel : ""; }
int hsm_last_launch_config(const hsm_ctx* h, int cfg[5]) {
  if (!h || !cfg) return fail(HSM_ERR_INVALID, "null argument");
  for (int i = 0; i < 5; ++i) cfg[i] = h->last_cfg[i];
  if (h->last_cfg[5]) cfg[4] = -cfg[4];  // texel-cache form: endpoints in LDS, not VGPRs
  return HSM_OK;
}

int hsm_match_batch_device(hsm_ctx* h, int batch, const float* d_begin_world, const float* d_pts_xy,
                           const int* d_scan_offsets, int shared_n, float* d_out_pose, float* d_out_cov,
                           void* stream) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  std::lock_guard<std::mutex> lk(h->mu);
  return match_batch_device_nolock(h, batch, d_begin_world, d_pts_xy, d_scan_offsets, shared_n, d_out_pose,
                                   d_out_cov, stream);
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
  if (int rc = match_batch_device_nolock(h, batch, d_begin_world, d_pts_xy, d_scan_offsets, shared_n, d_out_pose, d_out_cov, stream, 0, &f))
    return rc;
  if (h->fused_exchange_done) {
    hsm_host::exchange_fused_commit(x, f);
    return HSM_OK;
  }
  return hsm_exchange_post_wait(x, d_out_pose, first_row, batch, lag, d_out_all, stream);
}

// The weighting step behind a batched match: B (world pose, scan) pairs scored on `level` in one launch of score_batch_kernel
// (gn_match.h).  A reader of the map like the batched match, so ordered like it (order_map_reader); no workspace, no state.
static int score_batch_device_nolock(hsm_ctx* h, int level, int batch, const float* d_poses_world, const float* d_pts_xy,
                                     const int* d_scan_offsets, int shared_n, float* d_out_likelihood,
                                     float* d_out_residual, void* stream) {
  if (int rc = valid_level(h, level)) return rc;
  if (batch < 0 || (!d_out_likelihood && !d_out_residual) || (!d_scan_offsets && shared_n < 0) ||
      (batch > 0 && (!d_poses_world || (!d_pts_xy && !d_scan_offsets && shared_n > 0))))
    return fail(HSM_ERR_INVALID, "hsm_score_batch_device: bad argument");
  if (batch == 0) return HSM_OK;
  if (int rc = select_device(h)) return rc;
  hipStream_t s = (hipStream_t)stream;
  hsm_ctx::ForeignStream* fs = nullptr;
  if (int rc = order_map_reader(h, s, "hsm_score_batch_device", &fs)) return rc;
  const float factor = (float)(1.0 / pow(2.0, (double)level));
  const LevelView v = level_view(h->levels[level], factor, 1);
  const bool exact = wants_exact(h);
  const int grid = (batch + 3) / 4;
  with_sampler_form(h, [&](auto lay, auto ex) {
    hipLaunchKernelGGL((score_batch_kernel<lay(), ex()>), dim3(grid), dim3(256), 0, s, v, d_poses_world, batch,
                       reinterpret_cast<const float2*>(d_pts_xy), d_scan_offsets, d_scan_offsets ? 0 : shared_n,
                       d_out_likelihood, d_out_residual);
  });
  HIP_TRY(hipGetLastError());
  if (fs) fs->pending = true;
  h->last_kernel = "score_batch_kernel";
  h->last_parity = exact ? HSM_PARITY_EXACT : (h->relaxed ? HSM_PARITY_RELAXED : HSM_PARITY_FAST);
  return HSM_OK;
}

int hsm_score_batch_device(hsm_ctx* h, int level, int batch, const float* d_poses_world, const float* d_pts_xy,
                           const int* d_scan_offsets, int shared_n, float* d_out_likelihood, float* d_out_residual,
                           void* stream) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  std::lock_guard<std::mutex> lk(h->mu);
  return score_batch_device_nolock(h, level, batch, d_poses_world, d_pts_xy, d_scan_offsets, shared_n, d_out_likelihood,
                                   d_out_residual, stream);
}

// Groups of at most this many entries (or, with CSR groups whose sizes only the device knows, launches of at least this many
// groups) take one wavefront per group, the others one workgroup per group.  Either shape gives the same result.
constexpr int kSelectWaveGroupMax = 1024;

// reads no map: stream order is all it needs
static int select_best_device_nolock(hsm_ctx* h, int groups, const int* d_group_offsets, int group_size, const float* d_scores,
                                     const float* d_poses_world, int* d_out_index, float* d_out_score,
                                     float* d_out_pose_world, void* stream) {
  if (groups < 0 || (!d_group_offsets && group_size < 0) || !d_out_index || (d_out_pose_world && !d_poses_world) ||
      (!d_scores && groups > 0 && (d_group_offsets || group_size > 0)) ||
      (!d_group_offsets && groups > 0 && (long long)groups * group_size > INT_MAX))
    return fail(HSM_ERR_INVALID, "hsm_select_best_device: bad argument");
  if (groups == 0) return HSM_OK;
  if (int rc = select_device(h)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const bool wave_per_group = d_group_offsets ? groups >= kSelectWaveGroupMax : group_size <= kSelectWaveGroupMax;
  if (wave_per_group)
    hipLaunchKernelGGL((select_best_kernel<true>), dim3((groups + 3) / 4), dim3(256), 0, s, groups, d_group_offsets, group_size,
                       d_scores, d_poses_world, d_out_index, d_out_score, d_out_pose_world);
  else
    hipLaunchKernelGGL((select_best_kernel<false>), dim3(groups), dim3(256), 0, s, groups, d_group_offsets, group_size,
                       d_scores, d_poses_world, d_out_index, d_out_score, d_out_pose_world);
  HIP_TRY(hipGetLastError());
  return HSM_OK;
}

int hsm_select_best_device(hsm_ctx* h, int groups, const int* d_group_offsets, int group_size, const float* d_scores,
                           const float* d_poses_world, int* d_out_index, float* d_out_score, float* d_out_pose_world,
                           void* stream) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  std::lock_guard<std::mutex> lk(h->mu);
  return select_best_device_nolock(h, groups, d_group_offsets, group_size, d_scores, d_poses_world, d_out_index, d_out_score,
                                   d_out_pose_world, stream);
}

// match -> score at the matched poses -> (groups > 0) the winner of every group, queued on `stream` under one lock.  Every
// argument is checked before the first launch, so a bad one queues nothing.
static int match_score_batch_device_nolock(hsm_ctx* h, int batch, const float* d_begin_world, const float* d_pts_xy,
                                           const int* d_scan_offsets, int shared_n, float* d_out_pose, float* d_out_cov,
                                           int score_level, float* d_out_likelihood, float* d_out_residual, int groups,
                                           const int* d_group_offsets, int group_size, int* d_out_index, float* d_out_score,
                                           float* d_out_best_pose, void* stream, int n_bound = 0) {
  if (int rc = valid_level(h, score_level)) return rc;
  if (batch < 0 || !d_begin_world || !d_out_pose || (!d_scan_offsets && shared_n < 0) || (!d_out_likelihood && !d_out_residual) ||
      (batch > 0 && !d_pts_xy && !d_scan_offsets && shared_n > 0) || groups < 0 ||
      (groups > 0 && (!d_out_likelihood || !d_out_index || (!d_group_offsets && (group_size < 0 || (long long)groups * group_size > batch)))))
    return fail(HSM_ERR_INVALID, "hsm_match_score_batch_device: bad argument");
  if (int rc = match_batch_device_nolock(h, batch, d_begin_world, d_pts_xy, d_scan_offsets, shared_n, d_out_pose, d_out_cov, stream, n_bound))
    return rc;
  // the sizing hint of a CSR match means nothing to the score: its kernel reads every scan's length from the offsets
  if (int rc = score_batch_device_nolock(h, score_level, batch, d_out_pose, d_pts_xy, d_scan_offsets, d_scan_offsets ? 0 : shared_n,
                                         d_out_likelihood, d_out_residual, stream))
    return rc;
  if (groups == 0) return HSM_OK;
  return select_best_device_nolock(h, groups, d_group_offsets, group_size, d_out_likelihood, d_out_pose, d_out_index, d_out_score,
                                   d_out_best_pose, stream);
}

}  // extern "C"

int hsm_host::match_score_batch_chain_nolock(hsm_ctx* h, int batch, const float* d_begin_world, const float* d_pts_xy, int shared_n,
                                             float* d_out_pose, float* d_out_cov, int score_level, float* d_out_likelihood,
                                             int groups, int group_size, int* d_out_index, float* d_out_score,
                                             float* d_out_best_pose, void* stream) {
  return match_score_batch_device_nolock(h, batch, d_begin_world, d_pts_xy, nullptr, shared_n, d_out_pose, d_out_cov, score_level,
                                         d_out_likelihood, nullptr, groups, nullptr, group_size, d_out_index, d_out_score,
                                         d_out_best_pose, stream);
}

extern "C" {

int hsm_match_score_batch_device(hsm_ctx* h, int batch, const float* d_begin_world, const float* d_pts_xy,
                                 const int* d_scan_offsets, int shared_n, float* d_out_pose, float* d_out_cov, int score_level,
                                 float* d_out_likelihood, float* d_out_residual, int groups, const int* d_group_offsets,
                                 int group_size, int* d_out_index, float* d_out_score, float* d_out_best_pose, void* stream) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  std::lock_guard<std::mutex> lk(h->mu);
  return match_score_batch_device_nolock(h, batch, d_begin_world, d_pts_xy, d_scan_offsets, shared_n, d_out_pose, d_out_cov,
                                         score_level, d_out_likelihood, d_out_residual, groups, d_group_offsets, group_size,
                                         d_out_index, d_out_score, d_out_best_pose, stream);
}

// what hsm_match_score_batch asks for on top of hsm_match_batch (host pointers)
struct BatchScoreReq {
  int level;
  float* out_lh;
  float* out_res;  // may be null
  int groups;      // 0: no ranking
  const int* group_offsets;
  int group_size;
  int* out_index;
  float* out_score;      // may be null
  float* out_best_pose;  // may be null; in/out (a group without a winner keeps the caller's values)
};

// hsm_match_batch, and with `sr` hsm_match_score_batch: host arrays in, one device call on the context's stream, results out
static int match_batch_host(hsm_ctx* h, int batch, const float* begin_world, const float* pts_xy, const int* scan_offsets,
                            int shared_n, float* out_pose, float* out_cov, const BatchScoreReq* sr, const char* who) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  if (batch < 0 || !begin_world || !out_pose) return fail(HSM_ERR_INVALID, who);
  const int G = sr ? sr->groups : 0;
  if (sr) {
    if (int rc = valid_level(h, sr->level)) return rc;
    if (!sr->out_lh || G < 0 || (G > 0 && (!sr->out_index || (!sr->group_offsets && (sr->group_size < 0 || (long long)G * sr->group_size > batch)))))
      return fail(HSM_ERR_INVALID, who);
    if (G > 0 && sr->group_offsets)
      for (int g = 0; g < G; ++g)
        if (sr->group_offsets[g] < 0 || sr->group_offsets[g] > sr->group_offsets[g + 1] || sr->group_offsets[g + 1] > batch)
          return fail(HSM_ERR_INVALID, who);
  }
  if (batch == 0) return HSM_OK;
  const size_t total = scan_offsets ? (size_t)scan_offsets[batch] : (size_t)(shared_n > 0 ? shared_n : 0);
  if (total > 0 && !pts_xy) return fail(HSM_ERR_INVALID, who);
  BatchBytes b = {};  // (stage_layout.h: the match's own arrays, and behind them the score's and the ranking's)
  b.begin = (size_t)batch * 3 * sizeof(float);
  b.pts = total * 2 * sizeof(float);
  b.offs = scan_offsets ? ((size_t)batch + 1) * sizeof(int) : 0;
  b.cov = (size_t)batch * 9 * sizeof(float);
  b.lh = sr ? (size_t)batch * sizeof(float) : 0, b.res = sr && sr->out_res ? b.lh : 0;
  b.goffs = G > 0 && sr->group_offsets ? ((size_t)G + 1) * sizeof(int) : 0;
  b.idx = (size_t)G * sizeof(int), b.bscore = G > 0 && sr->out_score ? (size_t)G * sizeof(float) : 0;
  b.bpose = G > 0 && sr->out_best_pose ? (size_t)G * 3 * sizeof(float) : 0;
  const BatchLayout L = batch_layout(b, !scan_offsets);
  // the launches behind the copies in: x = the device address of the block
  auto launch = [&](char* x, const float* d_pts, const int* d_offs, int n_or_hint, int n_bound) {
    float* d_pose = (float*)(x + L.pose);
    float* d_cov = out_cov ? (float*)(x + L.cov) : nullptr;
    if (!sr) return match_batch_device_nolock(h, batch, (const float*)x, d_pts, d_offs, n_or_hint, d_pose, d_cov, h->stream, n_bound);
    return match_score_batch_device_nolock(h, batch, (const float*)x, d_pts, d_offs, n_or_hint, d_pose, d_cov, sr->level,
                                           (float*)(x + L.lh), b.res ? (float*)(x + L.res) : nullptr, G,
                                           b.goffs ? (const int*)(x + L.goffs) : nullptr, sr->group_size, (int*)(x + L.idx),
                                           b.bscore ? (float*)(x + L.bscore) : nullptr,
                                           b.bpose ? (float*)(x + L.bpose) : nullptr, h->stream, n_bound);
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
    if (!h->h_hyp_pinned.holds(L.total)) HIP_TRY(hipStreamSynchronize(h->stream));
    if (int rc = h->h_hyp_pinned.reserve(L.total, kHalfMore)) return rc;
    char* hp = h->h_hyp_pinned;
    memcpy(hp, begin_world, b.begin);
    if (out_cov) memcpy(hp + L.cov, out_cov, b.cov);  // in/out: an empty scan leaves the caller's matrices untouched (ScanMatcher.h:68,189)
    if (b.pts) memcpy(hp + L.pts, pts_xy, b.pts);
    if (b.goffs) memcpy(hp + L.goffs, sr->group_offsets, b.goffs);
    if (b.bpose) memcpy(hp + L.bpose, sr->out_best_pose, b.bpose);
    char* dp = nullptr;
    HIP_TRY(hipHostGetDevicePointer((void**)&dp, hp, 0));
    if (int rc = h->d_scan.reserve(total, kScanGrowth)) return rc;
    if (b.pts) HIP_TRY(hipMemcpyAsync(h->d_scan, hp + L.pts, b.pts, hipMemcpyHostToDevice, h->stream));
    if (int rc = launch(dp, (const float*)h->d_scan.p, nullptr, shared_n > 0 ? shared_n : 0, 0)) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    memcpy(out_pose, hp + L.pose, b.begin);
    if (out_cov) memcpy(out_cov, hp + L.cov, b.cov);
    if (sr) {
      memcpy(sr->out_lh, hp + L.lh, b.lh);
      if (b.res) memcpy(sr->out_res, hp + L.res, b.res);
      if (b.idx) memcpy(sr->out_index, hp + L.idx, b.idx);
      if (b.bscore) memcpy(sr->out_score, hp + L.bscore, b.bscore);
      if (b.bpose) memcpy(sr->out_best_pose, hp + L.bpose, b.bpose);
    }
    return HSM_OK;
  }
  if (int rc = h->d_batch.reserve(L.total)) return rc;
  char* base = h->d_batch;
  const float* d_pts = (const float*)(base + L.pts);
  const int* d_offs = (const int*)(base + L.offs);  // (scan_offsets is not null here)
  HIP_TRY(hipMemcpyAsync(base, begin_world, b.begin, hipMemcpyHostToDevice, h->stream));
  if (b.pts) HIP_TRY(hipMemcpyAsync(base + L.pts, pts_xy, b.pts, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(base + L.offs, scan_offsets, b.offs, hipMemcpyHostToDevice, h->stream));
  if (out_cov) HIP_TRY(hipMemcpyAsync(base + L.cov, out_cov, b.cov, hipMemcpyHostToDevice, h->stream));  // in/out
  if (b.goffs) HIP_TRY(hipMemcpyAsync(base + L.goffs, sr->group_offsets, b.goffs, hipMemcpyHostToDevice, h->stream));
  if (b.bpose) HIP_TRY(hipMemcpyAsync(base + L.bpose, sr->out_best_pose, b.bpose, hipMemcpyHostToDevice, h->stream));  // in/out
  int hint = 0;
  for (int i = 0; i < batch; ++i) {
    const int ni = scan_offsets[i + 1] - scan_offsets[i];
    if (ni > hint) hint = ni;
  }
  if (int rc = launch(base, d_pts, d_offs, hint, hint)) return rc;
  HIP_TRY(hipMemcpyAsync(out_pose, base + L.pose, b.begin, hipMemcpyDeviceToHost, h->stream));
  if (out_cov) HIP_TRY(hipMemcpyAsync(out_cov, base + L.cov, b.cov, hipMemcpyDeviceToHost, h->stream));
  if (sr) {
    HIP_TRY(hipMemcpyAsync(sr->out_lh, base + L.lh, b.lh, hipMemcpyDeviceToHost, h->stream));
    if (b.res) HIP_TRY(hipMemcpyAsync(sr->out_res, base + L.res, b.res, hipMemcpyDeviceToHost, h->stream));
    if (b.idx) HIP_TRY(hipMemcpyAsync(sr->out_index, base + L.idx, b.idx, hipMemcpyDeviceToHost, h->stream));
    if (b.bscore) HIP_TRY(hipMemcpyAsync(sr->out_score, base + L.bscore, b.bscore, hipMemcpyDeviceToHost, h->stream));
    if (b.bpose) HIP_TRY(hipMemcpyAsync(sr->out_best_pose, base + L.bpose, b.bpose, hipMemcpyDeviceToHost, h->stream));
  }
  HIP_TRY(hipStreamSynchronize(h->stream));
  return HSM_OK;
}

int hsm_match_batch(hsm_ctx* h, int batch, const float* begin_world, const float* pts_xy,
                    const int* scan_offsets, int shared_n, float* out_pose, float* out_cov) {
  return match_batch_host(h, batch, begin_world, pts_xy, scan_offsets, shared_n, out_pose, out_cov, nullptr,
                          "hsm_match_batch: bad argument");
}

int hsm_match_score_batch(hsm_ctx* h, int batch, const float* begin_world, const float* pts_xy, const int* scan_offsets,
                          int shared_n, float* out_pose, float* out_cov, int score_level, float* out_likelihood,
                          float* out_residual, int groups, const int* group_offsets, int group_size, int* out_index,
                          float* out_score, float* out_best_pose) {
  const BatchScoreReq sr = {score_level, out_likelihood, out_residual, groups, group_offsets, group_size, out_index, out_score,
                            out_best_pose};
  return match_batch_host(h, batch, begin_world, pts_xy, scan_offsets, shared_n, out_pose, out_cov, &sr,
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
  if (h->spin_wait) {
    volatile unsigned* flag = reinterpret_cast<volatile unsigned*>(h->h_small + kDoneFlagOff);
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
  float* hs = h->h_small;
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
  const unsigned seq = ++h->done_seq;
  P.done_flag = h->spin_wait ? reinterpret_cast<unsigned*>(hs_dev + kDoneFlagOff) : nullptr;
  P.done_seq = seq;
  P.err_flag = reinterpret_cast<unsigned*>(hs_dev + kErrFlagOff);
  P.coop_mute_block = h->coop_mute_block;
  P.clock_probe = h->clock_probe;
  // which form: the site the scan was staged for (stage_scan), now with the trace
  MatchSite site = single_scan_site(h, n, trace_steps > 0);
  site.coop_skip = false;
  MatchPlan plan = plan_match(site);
  if (plan.family == Family::kCoop && h->coop_skip > 0) {  // backing off after an exchange timeout: this match goes straight to the one-workgroup form
    --h->coop_skip;
    site.coop_skip = true;
    plan = plan_match(site);
  }
  const bool coop_tried = plan.family == Family::kCoop;
  if (coop_tried) {
    // one dense scan spread over K workgroups of one launch (match_plan.h has the measurements)
    const int K = plan.grid;
    float* partials = h->d_partials;
    unsigned* bar_counter = reinterpret_cast<unsigned*>(h->d_partials + 2 * 64 * 12);
    unsigned bar_base = h->coop_bar_base;
    void* args[] = {(void*)&P, (void*)&partials, (void*)&bar_counter, (void*)&bar_base};
    const void* fn = h->layout == kLayoutPlane ? (const void*)gn_match_coop_kernel<kLayoutPlane, false>
                                                : (const void*)gn_match_coop_kernel<kLayoutQuad, false>;
    // The tagged-record exchange (default) has no grid barrier: a workgroup that is not resident yet only delays the others'
    // polls, which are bounded (a record that never arrives turns into an error return, err_flag) -- so it is an ORDINARY
    // launch: K <= 64 workgroups of 256 lanes are co-resident on an idle 256-CU device, and on a busy one they become so as
    // soon as other kernels retire.  (Round 3 launched it through hipLaunchCooperativeKernel: that goes through the
    // device's cooperative queue -- a slower launch, and a process that has used it segfaults in the runtime's exit
    // handlers when it runs under rocprofv3, profiles/r04/README.md.)  The counter-barrier form (HSM_COOP_TAGGED=0) spins
    // without a bound and keeps the cooperative launch's co-residency guarantee.
    hipError_t le;
    if (h->coop_tagged) {
      if (h->layout == kLayoutPlane)
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
      h->coop_bar_base += (unsigned)K * steps;  // one arrival per workgroup per GN step
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
  h->queued_update = false;  // the match kernel was the last thing on `stream`, and it has completed
  if (*reinterpret_cast<volatile unsigned*>(hs + kErrFlagOff) == seq) {
    // The multi-workgroup matcher's tagged exchange gave up waiting for a record: its K workgroups were not co-resident for
    // ~2^22 polls (a device shared with another process, or a long kernel of another stream holding the CUs -- an ordinary
    // launch carries no co-residency guarantee).  No pose was written.  The scan is matched again by the one-workgroup
    // matcher, which needs no other workgroup to make progress -- same sums in a different tree, so the caller gets a pose
    // within the fast mode's bar instead of an error (round-4 advisor); hsm_last_launch_config() then reports that form.
    const unsigned seq2 = ++h->done_seq;
    P.done_seq = seq2;
    if (int rc = launch_match(h, P, n, h->stream)) return rc;
    if (int rc = wait_single_scan(h, seq2)) return rc;
    ++h->coop_fallbacks;
    h->coop_backoff = h->coop_backoff ? (h->coop_backoff < 1024 ? 2 * h->coop_backoff : 1024) : 1;
    h->coop_skip = h->coop_backoff;
    {
      char b[200];
      snprintf(b, sizeof b, "hsm_match: the multi-workgroup matcher's exchange timed out (device shared or busy); re-ran on one workgroup, "
               "skipping that form for the next %u dense matches", h->coop_skip);
      g_last_error = b;  // (not an error return: the pose is valid; the text tells who asks why a match took long)
    }
    if (*reinterpret_cast<volatile unsigned*>(hs + kErrFlagOff) == seq2)
      return fail(HSM_ERR_HIP, "hsm_match: exchange timeout flagged by the one-workgroup matcher (cannot happen: it has no exchange)");
  }
  else if (coop_tried)
    h->coop_backoff = 0;  // an exchange completed: the device is ours again
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
    if (int rc = h->h_scan_pinned.reserve(n > 0 ? n : 1, kScanGrowth)) return rc;  // (1: also the empty first scan of a fresh context)
    if (n > 0) memcpy(h->h_scan_pinned, pts_xy, (size_t)n * sizeof(float2));
    float2* dev = nullptr;
    HIP_TRY(hipHostGetDevicePointer((void**)&dev, h->h_scan_pinned, 0));
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
  if (!h->copy_stream) {
    HIP_TRY(hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&h->copy_evt, hipEventDisableTiming));
  }
  std::swap(h->d_retained, h->d_retained_alt);
  if (int rc = h->d_retained.reserve((size_t)n, kScanGrowth)) return rc;
  if (!h->h_copy_pinned.holds((size_t)n)) HIP_TRY(hipStreamSynchronize(h->copy_stream));
  if (int rc = h->h_copy_pinned.reserve((size_t)n, kHalfMore)) return rc;
  memcpy(h->h_copy_pinned, pts_xy, (size_t)n * sizeof(float2));
  HIP_TRY(hipMemcpyAsync(h->d_retained, h->h_copy_pinned, (size_t)n * sizeof(float2), hipMemcpyHostToDevice, h->copy_stream));
  HIP_TRY(hipEventRecord(h->copy_evt, h->copy_stream));
  HIP_TRY(hipStreamWaitEvent(h->stream, h->copy_evt, 0));
  *out = h->d_retained;
  return HSM_OK;
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
  // DataContainer::setFrom keeps scaled copies for the coarse levels (MapRepMultiMap.h:127);
  // here: one level-0 copy, scaled by 2^-level on use
  if (h->levels.size() > 1) {
    h->retained_pts.assign(pts_xy, pts_xy + 2 * (size_t)n);
    h->retained_origo[0] = origo ? origo[0] : 0.0f;
    h->retained_origo[1] = origo ? origo[1] : 0.0f;
    h->retained_valid = true;
  }
  const float2* pts = d_prestaged;
  if (!pts) {
    // (the same rule as stage_scan's: scans the matcher reads once stay in pinned host memory)
    const bool to_device = !plan_match(single_scan_site(h, n)).reads_scan_once;
    // ... and only behind an update that was queued and not waited for (the match + update loop): on an idle stream the
    // extra hop through the copy stream's event costs ~10 us of latency and hides nothing (asking the runtime with
    // hipStreamQuery costs half of what the overlap gains: 0.1855 against 0.179 ms per configs[4] step)
    if (to_device && h->overlap_upload && n > 0 && h->queued_update) {
      if (int rc = stage_scan_overlapped(h, pts_xy, n, &pts)) return rc;
    } else if (int rc = stage_scan(h, pts_xy, n, h->d_retained, &pts)) {
      return rc;
    }
  }
  // the device copy of the retained scan is (re)uploaded lazily by the next update when the
  // matcher read the scan from pinned host memory
  h->d_retained_current = h->levels.size() > 1 && pts == h->d_retained;
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

static int update_impl(hsm_ctx* h, const float pose_world[3], const float* pts_xy, int n, const float origo[2],
                       const float2* d_prestaged);

int hsm_update_by_scan(hsm_ctx* h, const float pose_world[3], const float* pts_xy, int n, const float origo[2]) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  if (!pose_world || n < 0 || (n > 0 && !pts_xy)) return fail(HSM_ERR_INVALID, "hsm_update_by_scan: bad argument");
  std::lock_guard<std::mutex> lk(h->mu);
  return update_impl(h, pose_world, pts_xy, n, origo, nullptr);
}

// pts_xy: host copy of the endpoints (always needed: the touched bounding box is computed on the host);
// d_prestaged: the same endpoints already on the device, or nullptr to upload them
static int update_impl(hsm_ctx* h, const float pose_world[3], const float* pts_xy, int n, const float origo[2],
                       const float2* d_prestaged) {
  if (int rc = select_device(h)) return rc;
  if (h->upd_boxes_outstanding)  // this update rewrites Level::bbox: the boxes of device-side updates go in first
    if (int rc = merge_device_boxes(h)) return rc;
  if (h->gate_outstanding)  // ... and numbers its update behind the ones gated calls applied
    if (int rc = fold_gate_counters(h)) return rc;
  if (int rc = order_after_foreign_match(h)) return rc;
  const float zero[2] = {0.0f, 0.0f};
  const float* o = origo ? origo : zero;
  // level 0: the caller's container
  const float2* d_level0 = d_prestaged;
  int slot = -1;
  // The usual flow updates with the scan that was just matched.  When the matcher put that scan into device memory (dense
  // scans, multi-level maps: d_retained) and the caller hands over the same endpoints, they are already where the update
  // kernels read them: no second upload (131 KB from pageable memory for a 16 k-beam scan, which the host waits for).
  const int rn0 = h->retained_valid ? (int)(h->retained_pts.size() / 2) : 0;
  const bool same_as_matched = !d_level0 && h->d_retained_current && rn0 == n && n > 0 &&
                               memcmp(h->retained_pts.data(), pts_xy, (size_t)n * sizeof(float2)) == 0;
  if (same_as_matched) d_level0 = h->d_retained;
  if (!d_level0 && h->async_update) {
    // stage the endpoints in pinned memory (a pageable hipMemcpyAsync would block the host until the copy
    // -- and everything queued before it -- has completed); small scans are then read in place over PCIe
    // (each endpoint is read twice), dense ones copied to the device by a copy the host does not wait for
    slot = h->upd_slot;
    h->upd_slot ^= 1;
    if (h->upd_busy[slot]) {
      HIP_TRY(hipEventSynchronize(h->upd_evt[slot]));
      h->upd_busy[slot] = false;
    }
    if (int rc = h->h_upd_pinned[slot].reserve((size_t)n, kScanGrowth)) return rc;
    if (!h->upd_evt[slot]) HIP_TRY(hipEventCreateWithFlags(&h->upd_evt[slot], hipEventDisableTiming));
    if (n > 0) memcpy(h->h_upd_pinned[slot], pts_xy, (size_t)n * sizeof(float2));
    if (n <= h->update_zero_copy_max) {
      float2* dev = nullptr;
      if (n > 0) HIP_TRY(hipHostGetDevicePointer((void**)&dev, h->h_upd_pinned[slot], 0));
      d_level0 = n > 0 ? dev : h->d_scan;
    } else {
      if (int rc = h->d_scan.reserve((size_t)n, kScanGrowth)) return rc;
      HIP_TRY(hipMemcpyAsync(h->d_scan, h->h_upd_pinned[slot], (size_t)n * sizeof(float2), hipMemcpyHostToDevice,
                             h->stream));
      d_level0 = h->d_scan;
    }
  } else if (!d_level0) {
    if (int rc = h->d_scan.reserve((size_t)n, kScanGrowth)) return rc;
    if (n > 0)
      HIP_TRY(hipMemcpyAsync(h->d_scan, pts_xy, (size_t)n * sizeof(float2), hipMemcpyHostToDevice, h->stream));
    d_level0 = h->d_scan;
  }
  UpdateBatch batch;
  batch.nlev = 0;
  batch.stamped = 0;
  LevelPrep prep[HSM_MAX_LEVELS];
  if (int rc = prepare_level(h, batch, prep[0], 0, pose_world, d_level0, pts_xy, n, 1.0f, o)) return rc;
  // coarse levels: the containers retained by the last matchData (MapRepMultiMap.h:143)
  const int rn = h->retained_valid ? (int)(h->retained_pts.size() / 2) : 0;
  bool coarse_same_container = false;  // the usual flow: update with the container that was just matched
  if (h->levels.size() > 1) {
    const float2* d_coarse = nullptr;
    if (same_as_matched) {
      d_coarse = d_level0;
      coarse_same_container = h->retained_origo[0] == o[0] && h->retained_origo[1] == o[1];
    } else if (rn == n && n > 0 && !h->d_retained_current &&
               memcmp(h->retained_pts.data(), pts_xy, (size_t)n * sizeof(float2)) == 0) {
      d_coarse = d_level0;
      coarse_same_container = h->retained_origo[0] == o[0] && h->retained_origo[1] == o[1];
    } else {
      if (rn > 0 && !h->d_retained_current) {
        if (int rc = h->d_retained.reserve((size_t)rn, kScanGrowth)) return rc;
        HIP_TRY(hipMemcpyAsync(h->d_retained, h->retained_pts.data(), (size_t)rn * sizeof(float2),
                               hipMemcpyHostToDevice, h->stream));
        h->d_retained_current = true;
      }
      d_coarse = h->d_retained;  // read only after a possible (re)allocation above
    }
    for (size_t l = 1; l < h->levels.size(); ++l) {
      const float factor = (float)(1.0 / pow(2.0, (double)l));
      const float ol[2] = {h->retained_origo[0] * factor, h->retained_origo[1] * factor};  // setFrom :48
      if (int rc = prepare_level(h, batch, prep[l], (int)l, pose_world, d_coarse, h->retained_pts.data(), rn, factor, ol))
        return rc;
    }
  }
  // the GPU starts marking (all levels, one launch) while the host works out the boxes of the dense passes
  if (int rc = launch_update_mark(h, batch)) return rc;
  level_bbox(h, batch, prep[0], nullptr, 0);
  for (size_t l = 1; l < h->levels.size(); ++l) {
    const bool derive = coarse_same_container && prep[0].slot >= 0 && prep[0].derivable && h->levels[l].sx == (h->levels[0].sx >> l) &&
                        h->levels[l].sy == (h->levels[0].sy >> l);
    level_bbox(h, batch, prep[l], derive ? &batch.lv[prep[0].slot] : nullptr, (int)l);
  }
  if (int rc = launch_update_apply(h, batch)) return rc;
  for (size_t l = 0; l < h->levels.size(); ++l) update_applied(h, batch, prep[l]);
  h->queued_update = h->async_update;
  if (slot >= 0) {
    HIP_TRY(hipEventRecord(h->upd_evt[slot], h->stream));
    h->upd_busy[slot] = true;
  }
  if (!h->async_update) HIP_TRY(hipStreamSynchronize(h->stream));
  return HSM_OK;
}

int hsm_synchronize(hsm_ctx* h) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->upd_busy[0] = h->upd_busy[1] = false;
  h->queued_update = false;
  return HSM_OK;
}

int hsm_update_by_scan_level(hsm_ctx* h, int level, const float pose_world[3], const float* pts_level_xy, int n,
                             const float origo_level[2]) {
  if (int rc = valid_level(h, level)) return rc;
  if (!pose_world || n < 0 || (n > 0 && !pts_level_xy))
    return fail(HSM_ERR_INVALID, "hsm_update_by_scan_level: bad argument");
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  if (h->upd_boxes_outstanding)
    if (int rc = merge_device_boxes(h)) return rc;
  if (h->gate_outstanding)
    if (int rc = fold_gate_counters(h)) return rc;
  if (int rc = order_after_foreign_match(h)) return rc;
  const float zero[2] = {0.0f, 0.0f};
  if (int rc = h->d_scan.reserve((size_t)n, kScanGrowth)) return rc;
  if (n > 0)
    HIP_TRY(hipMemcpyAsync(h->d_scan, pts_level_xy, (size_t)n * sizeof(float2), hipMemcpyHostToDevice, h->stream));
  UpdateBatch batch;
  batch.nlev = 0;
  batch.stamped = 0;
  LevelPrep prep;
  if (int rc = prepare_level(h, batch, prep, level, pose_world, h->d_scan, pts_level_xy, n, 1.0f,
                             origo_level ? origo_level : zero))
    return rc;
  if (int rc = launch_update_mark(h, batch)) return rc;
  level_bbox(h, batch, prep, nullptr, 0);
  if (int rc = launch_update_apply(h, batch)) return rc;
  update_applied(h, batch, prep);
  HIP_TRY(hipStreamSynchronize(h->stream));
  return HSM_OK;
}

// `count` posed scans that are on the device, integrated in order by stream-ordered launches only: one update_prep_kernel, then
// a mark and an apply launch per scan (map_update.h "posed scans that are already on the device").  The host supplies what it can
// compute without the poses: per level the counters and the key generation before the call, from which scan k's follow.
// `gate`: the gated entries.  update_gate_prep_kernel takes update_prep_kernel's place: it decides on the device which scans are
// integrated and numbers them behind the updates earlier gated calls applied, so the levels' counters are not advanced here
// (fold_gate_counters); a rejected scan's two launches return at once.  (PosedScans, GateCall: hsm_ctx.h.)
static int update_by_scans_device_nolock(hsm_ctx* h, const PosedScans& S, hipStream_t stream) {
  const int count = S.count;
  const GateCall* gate = S.gate;
  const float* origo = S.origo;
  if (count < 0 || S.max_beams < 0 || (count > 0 && !S.d_poses) || (!S.d_offsets && S.shared_n < 0) ||
      (count > 0 && !S.d_offsets && S.shared_n > 0 && !S.d_pts) || ((uintptr_t)S.d_origos & 7u) != 0)  // (origos: float2 loads)
    return fail_at(HSM_ERR_INVALID, S.who, ": bad argument");
  if (!S.d_offsets && S.shared_n > HSM_MAX_UPDATE_BEAMS)
    return fail_at(HSM_ERR_TOO_LARGE, S.who, ": more than HSM_MAX_UPDATE_BEAMS beams");
  if (count == 0) return HSM_OK;
  if (int rc = select_device(h)) return rc;
  // the rule of every map update: refused, before anything is queued, while a stream this call would touch is being captured
  if (stream_capturing(stream))
    return fail_at(HSM_ERR_INVALID, S.who, ": `stream` is being captured into a graph (map updates are not captured)");
  if (int rc = order_after_foreign_match(h)) return rc;  // (refuses the same way for the streams this context has matched on)
  if (!gate && h->gate_outstanding)  // scan k is update k behind EVERY earlier update: the ones gated calls applied go in first
    if (int rc = fold_gate_counters(h)) return rc;
  if (int rc = ensure_update_scans(h, (size_t)count)) return rc;
  if (int rc = wait_for_caller_inputs(h, stream)) return rc;
  const int nlev = (int)h->levels.size();
  UpdatePrepParams A;
  memset(&A, 0, sizeof A);
  A.nlev = nlev;
  A.count = count;
  A.poses_world = S.d_poses;
  A.pts = reinterpret_cast<const float2*>(S.d_pts);
  A.offsets = S.d_offsets;
  A.shared_n = S.shared_n;
  A.origos = reinterpret_cast<const float2*>(S.d_origos);  // per scan, on the device: the host pair below is then not read
  A.out = h->d_upd_batches;
  A.boxes = h->d_upd_boxes;
  size_t max_cells = 0;
  for (int l = 0; l < nlev; ++l) {
    Level& L = h->levels[l];
    if (L.marks_pending)
      if (int rc = scrub_marks(h, L)) return rc;
    UpdatePrepLevel& V = A.lv[l];
    const float factor = (float)(1.0 / pow(2.0, (double)l));
    V.lv = level_rw(L);
    V.mapTworld = L.mapTworld;
    V.pt_scale = factor;
    V.origo_x = l == 0 ? (origo ? origo[0] : 0.0f) : (origo ? origo[0] : 0.0f) * factor;  // setFrom, DataPointContainer.h:48
    V.origo_y = l == 0 ? (origo ? origo[1] : 0.0f) : (origo ? origo[1] : 0.0f) * factor;
    V.log_odds_free = L.log_odds_free;
    V.log_odds_occ = L.log_odds_occ;
    V.serial0 = L.serial;
    V.update_index0 = L.curr_update_index;
    if (L.cells() > max_cells) max_cells = L.cells();
  }
  if (gate) {
    UpdateGateParams G;
    memset(&G, 0, sizeof G);
    G.prep = A;
    G.state = h->d_gate;
    G.min_dist = h->gate_min_dist;
    G.min_angle = h->gate_min_angle;
    G.force = gate->d_force;
    G.out_applied = gate->d_out_applied;
    G.slam = gate->slam ? 1 : 0;
    G.pose_io = gate->pose_io;
    G.cov_io = gate->cov_io;
    G.next_delta = gate->next_delta;
    hipLaunchKernelGGL(update_gate_prep_kernel, dim3(1), dim3(256), 0, h->stream, G);
  } else {
    hipLaunchKernelGGL(update_prep_kernel, dim3((unsigned)count), dim3(64), 0, h->stream, A);
  }
  HIP_TRY(hipGetLastError());
  // launch shapes from the hint alone: the mark grid strides over the scan's real beam count, the apply grid over the scan's
  // box -- sized for the whole level, its blocks return after one scalar load where the box is empty or small
  const int hint = S.max_beams > 0 ? S.max_beams : 1081;
  const unsigned occ_blocks = (unsigned)((hint + 255) / 256), free_blocks = (unsigned)((hint + 3) / 4);
  const unsigned apply_blocks = (unsigned)grid_for(max_cells);
  const bool scatter = h->layout == kLayoutQuad;
  // Restored stamps at or ahead of the first scan's free mark: the whole call takes the stamp-aware apply pass.  (A gated call
  // whose predecessors' counts are still on the device sees a counter that lags: the test errs towards the stamp-aware form.)
  bool stamped = false;
  for (int l = 0; l < nlev; ++l) stamped |= h->levels[l].stamps_ahead();
  auto apply_scan = scatter ? (stamped ? update_apply_scan_kernel<true, true> : update_apply_scan_kernel<true, false>)
                            : (stamped ? update_apply_scan_kernel<false, true> : update_apply_scan_kernel<false, false>);
  for (int l = 0; l < nlev; ++l) h->levels[l].marks_pending = true;  // until every apply pass is queued (scrub_marks)
  for (int k = 0; k < count; ++k) {
    for (int l = 0; l < nlev; ++l) {
      Level& L = h->levels[l];
      // The key generation advances once per scan and level, empty scan or not (the host cannot see n_k; a generation spent on
      // an empty scan is harmless).  Where it wraps, the key planes are cleared between the two scans concerned.
      if (L.serial == kSerialMax) {
        if (int rc = clear_key_planes(h, L)) return rc;
        L.serial = 0;
      }
      ++L.serial;
    }
    int* scan_boxes = h->d_upd_boxes + (size_t)update_box_slot(k, count) * kMaxLevels * 4;
    hipLaunchKernelGGL(update_mark_scan_kernel, dim3(occ_blocks + free_blocks, (unsigned)nlev), dim3(256), 0, h->stream,
                       h->d_upd_batches + k, occ_blocks, scan_boxes, h->d_upd_boxes, h->d_pub_boxes);
    hipLaunchKernelGGL(apply_scan, dim3(apply_blocks, (unsigned)nlev), dim3(256), 0, h->stream, h->d_upd_batches + k, scan_boxes);
    HIP_TRY(hipGetLastError());
  }
  for (int l = 0; l < nlev; ++l) {
    Level& L = h->levels[l];
    L.marks_pending = false;
    if (!gate) {
      // OccGridMapBase.h:123-124, :167 and setUpdated() (GridMapBase.h:343), `count` times: an empty container counts, too
      L.curr_mark_free = L.curr_update_index + 3 * (count - 1) + 1;
      L.curr_mark_occ = L.curr_update_index + 3 * (count - 1) + 2;
      L.curr_update_index += 3 * count;
      L.last_update_index += count;
    }
    L.key_rows[0] = 0;  // which rows carry keys of this generation is known on the device only: the next wrap of a host-side
    L.key_rows[1] = L.sy - 1;  // update clears the whole level
  }
  h->upd_boxes_outstanding = true;
  if (gate) h->gate_outstanding = true;
  h->queued_update = h->async_update;
  if (!h->async_update) HIP_TRY(hipStreamSynchronize(h->stream));
  return HSM_OK;
}

int hsm_set_update_gate(hsm_ctx* h, float min_dist, float min_angle) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  std::lock_guard<std::mutex> lk(h->mu);
  h->gate_min_dist = min_dist;
  h->gate_min_angle = min_angle;
  return HSM_OK;
}

int hsm_reset_update_gate(hsm_ctx* h) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  return reset_update_gate(h);
}

int hsm_update_gate_state(hsm_ctx* h, float last_update_pose[3], long long* applied_total) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  std::lock_guard<std::mutex> lk(h->mu);
  GateState st;
  if (int rc = fold_gate_counters(h, &st)) return rc;
  if (last_update_pose)
    for (int i = 0; i < 3; ++i) last_update_pose[i] = st.last_update_pose[i];
  if (applied_total) *applied_total = h->gate_applied_total;
  return HSM_OK;
}

// what the four device entries share: the context's lock around the update
static int update_by_scans_device_locked(hsm_ctx* h, const PosedScans& S, void* stream) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  std::lock_guard<std::mutex> lk(h->mu);
  return update_by_scans_device_nolock(h, S, static_cast<hipStream_t>(stream));
}

int hsm_update_by_scans_device(hsm_ctx* h, int count, const float* d_poses_world, const float* d_pts_xy,
                               const int* d_scan_offsets, int shared_n, int max_beams, const float origo[2], void* stream) {
  PosedScans S{count, d_poses_world, d_pts_xy, d_scan_offsets, shared_n, max_beams};
  S.origo = origo;
  return update_by_scans_device_locked(h, S, stream);
}

int hsm_update_by_scans_device_origos(hsm_ctx* h, int count, const float* d_poses_world, const float* d_pts_xy,
                                      const int* d_scan_offsets, int shared_n, int max_beams, const float* d_origos,
                                      void* stream) {
  PosedScans S{count, d_poses_world, d_pts_xy, d_scan_offsets, shared_n, max_beams};
  S.d_origos = d_origos;
  S.who = "hsm_update_by_scans_device_origos";
  return update_by_scans_device_locked(h, S, stream);
}

int hsm_update_by_scans_device_gated(hsm_ctx* h, int count, const float* d_poses_world, const float* d_pts_xy,
                                     const int* d_scan_offsets, int shared_n, int max_beams, const float origo[2],
                                     const unsigned char* d_force, int* d_out_applied, void* stream) {
  GateCall gate;
  gate.d_force = d_force;
  gate.d_out_applied = d_out_applied;
  PosedScans S{count, d_poses_world, d_pts_xy, d_scan_offsets, shared_n, max_beams};
  S.origo = origo;
  S.gate = &gate;  // (the texts stay the ungated entry's)
  return update_by_scans_device_locked(h, S, stream);
}

int hsm_update_by_scans_device_gated_origos(hsm_ctx* h, int count, const float* d_poses_world, const float* d_pts_xy,
                                            const int* d_scan_offsets, int shared_n, int max_beams, const float* d_origos,
                                            const unsigned char* d_force, int* d_out_applied, void* stream) {
  GateCall gate;
  gate.d_force = d_force;
  gate.d_out_applied = d_out_applied;
  PosedScans S{count, d_poses_world, d_pts_xy, d_scan_offsets, shared_n, max_beams};
  S.d_origos = d_origos;
  S.gate = &gate;
  S.who = "hsm_update_by_scans_device_gated_origos";
  return update_by_scans_device_locked(h, S, stream);
}

}  // extern "C"

// the loop itself, on the context's stream.  `scans`: the log's CSR end points, beam hint, origo(s) and the name its updates
// report under (count, poses and gate are the loop's to set)
int hsm_host::slam_scans_queue(hsm_ctx* h, const ScanLog& log, const PosedScans& scans) {
  hipLaunchKernelGGL(slam_begin_kernel, dim3(1), dim3(64), 0, h->stream, h->d_gate, log.d_start_pose, log.d_hint_deltas);
  HIP_TRY(hipGetLastError());
  GateCall gate;
  PosedScans one = scans;
  one.count = 1;
  one.shared_n = 0;
  one.gate = &gate;
  for (int k = 0; k < log.count; ++k) {
    if (int rc = match_batch_device_nolock(h, 1, h->d_gate->hint, scans.d_pts, scans.d_offsets + k, scans.max_beams, log.pose(k),
                                           log.cov(k), h->stream))
      return rc;
    gate = log.gate(k);
    one.d_poses = gate.pose_io;
    one.d_offsets = scans.d_offsets + k;
    one.d_origos = scans.d_origos ? scans.d_origos + 2 * (size_t)k : nullptr;
    if (int rc = update_by_scans_device_nolock(h, one, h->stream)) return rc;
  }
  return HSM_OK;
}

extern "C" {

// HectorSlamProcessor::update for a log of scans (HectorSlamProcessor.h:71-95), queued whole.  Everything runs on the context's
// own stream -- the matches too, so a scan costs no event hop: the caller's stream is waited for once, in front, and waits once,
// behind.  Per scan: the exact batch matcher on a batch of one, reading its hint from the gate's device block; then the gated
// update of that one scan, whose gate launch also settles a forced scan's pose and covariance and leaves the next scan's hint.
static int slam_scans_device_impl(hsm_ctx* h, const char* who, const ScanLog& log, PosedScans scans, void* stream) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  if (log.count < 0 || scans.max_beams < 0 || (log.count > 0 && (!scans.d_offsets || !log.d_out_pose)) ||
      ((uintptr_t)scans.d_origos & 7u) != 0)
    return fail_at(HSM_ERR_INVALID, who, ": bad argument");
  if (log.count == 0) return HSM_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = slam_refuse_capture(h, s, who)) return rc;
  if (int rc = wait_for_caller_inputs(h, s)) return rc;
  if (scans.d_origos) scans.who = who;  // (the parent entry's updates keep hsm_update_by_scans_device's texts)
  if (int rc = slam_scans_queue(h, log, scans)) return rc;
  return slam_caller_waits(h, s);
}

int hsm_slam_scans_device(hsm_ctx* h, int count, const float* d_start_pose, const float* d_hint_deltas, const float* d_pts_xy,
                          const int* d_scan_offsets, int max_beams, const float origo[2], const unsigned char* d_force,
                          float* d_out_pose, float* d_out_cov, int* d_out_applied, void* stream) {
  PosedScans scans{count, nullptr, d_pts_xy, d_scan_offsets, 0, max_beams};
  scans.origo = origo;
  const ScanLog log{count, d_start_pose, d_hint_deltas, d_force, d_out_pose, d_out_cov, d_out_applied};
  return slam_scans_device_impl(h, "hsm_slam_scans_device", log, scans, stream);
}

int hsm_slam_scans_device_origos(hsm_ctx* h, int count, const float* d_start_pose, const float* d_hint_deltas,
                                 const float* d_pts_xy, const int* d_scan_offsets, int max_beams, const float* d_origos,
                                 const unsigned char* d_force, float* d_out_pose, float* d_out_cov, int* d_out_applied,
                                 void* stream) {
  PosedScans scans{count, nullptr, d_pts_xy, d_scan_offsets, 0, max_beams};
  scans.d_origos = d_origos;
  const ScanLog log{count, d_start_pose, d_hint_deltas, d_force, d_out_pose, d_out_cov, d_out_applied};
  return slam_scans_device_impl(h, "hsm_slam_scans_device_origos", log, scans, stream);
}

int hsm_update_by_scans(hsm_ctx* h, int count, const float* poses_world, const float* pts_xy, const int* scan_offsets,
                        int shared_n, const float origo[2]) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  if (count < 0 || (count > 0 && !poses_world) || (!scan_offsets && shared_n < 0))
    return fail(HSM_ERR_INVALID, "hsm_update_by_scans: bad argument");
  if (count == 0) return HSM_OK;
  size_t total = scan_offsets ? 0 : (size_t)shared_n;
  int longest = scan_offsets ? 0 : shared_n;
  if (scan_offsets) {
    for (int k = 0; k < count; ++k) {
      if (scan_offsets[k] < 0 || scan_offsets[k + 1] < scan_offsets[k])
        return fail(HSM_ERR_INVALID, "hsm_update_by_scans: scan_offsets must start at >= 0 and not decrease");
      if (scan_offsets[k + 1] - scan_offsets[k] > longest) longest = scan_offsets[k + 1] - scan_offsets[k];
    }
    total = (size_t)scan_offsets[count];
  }
  if (total > 0 && !pts_xy) return fail(HSM_ERR_INVALID, "hsm_update_by_scans: pts_xy is null");
  if (longest > HSM_MAX_UPDATE_BEAMS) return fail(HSM_ERR_TOO_LARGE, "hsm_update_by_scans: more than HSM_MAX_UPDATE_BEAMS beams");
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  for (const hsm_ctx::ForeignStream& f : h->foreign)  // refused before the copies are queued (order_after_foreign_match)
    if (stream_capturing(f.s))
      return fail(HSM_ERR_INVALID, "hsm_update_by_scans: a caller's stream that this context matches on is being captured into a graph");
  // one staging block (the copies are queued on the context's stream, in front of the update)
  const UpdateScansStage st = update_scans_stage(count, total, poses_world, pts_xy, scan_offsets);
  if (int rc = h->d_upd_stage.reserve(st.plan.total(), kHalfMore)) return rc;
  char* base = h->d_upd_stage;
  if (int rc = stage_copy_in(st.plan, base, h->stream)) return rc;
  PosedScans S{count, staged<float>(base, st.poses), staged<float>(base, st.pts),
                             staged<int>(base, st.offs, scan_offsets), shared_n, longest};
  S.origo = origo;
  return update_by_scans_device_nolock(h, S, h->stream);
}

int hsm_match_ingested(hsm_ctx* h, const float begin_world[3], float out_pose_world[3], float cov[9]) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  if (h->ingest_n < 0) return fail(HSM_ERR_INVALID, "hsm_match_ingested: no scan ingested");
  static const float dummy[2] = {0.0f, 0.0f};
  const float* hp = h->ingest_n > 0 ? h->h_ingest.data() : dummy;
  return match_impl(h, begin_world, hp, h->ingest_n, h->ingest_origo, out_pose_world, cov, nullptr, 0, h->d_ingest);
}

int hsm_update_by_ingested(hsm_ctx* h, const float pose_world[3]) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  if (!pose_world || h->ingest_n < 0) return fail(HSM_ERR_INVALID, "hsm_update_by_ingested: no scan ingested");
  std::lock_guard<std::mutex> lk(h->mu);
  static const float dummy[2] = {0.0f, 0.0f};
  const float* hp = h->ingest_n > 0 ? h->h_ingest.data() : dummy;
  return update_impl(h, pose_world, hp, h->ingest_n, h->ingest_origo, h->d_ingest);
}

int hsm_retain_scan(hsm_ctx* h, const float* pts_xy, int n, const float origo[2]) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  if (n < 0 || (n > 0 && !pts_xy)) return fail(HSM_ERR_INVALID, "hsm_retain_scan: bad argument");
  std::lock_guard<std::mutex> lk(h->mu);
  if (h->levels.size() > 1) {
    h->retained_pts.assign(pts_xy, pts_xy + 2 * (size_t)n);
    h->retained_origo[0] = origo ? origo[0] : 0.0f;
    h->retained_origo[1] = origo ? origo[1] : 0.0f;
    h->retained_valid = true;
    h->d_retained_current = false;
  }
  return HSM_OK;
}

}  // extern "C"

