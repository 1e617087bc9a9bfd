// map_update.hip -- everything that launches a kernel of map_update.h or map_update_scans.h, the one unit that includes them and
// the update headers behind them (hsm_ctx.h has the rule): the map-update entries of the C ABI (include/hector_mi355/capi.h: hsm_update_by_scan*, hsm_update_by_scans*, hsm_update_by_ingested,
// the movement gate), the device SLAM scan loop (hsm_slam_scans_device*), and the level maintenance that create, reset, upload,
// copy and shift reach through hsm_ctx.h.  What these need of the core runtime (hector_mi355.hip) is declared there too.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <mutex>

#include "hector_mi355/capi.h"
#include "hsm_ctx.h"
#include "map_update.h"
#include "map_update_scans.h"

using namespace hsm;
using namespace hsm_host;

// the <SCATTER_TEXELS, STAMPED> instantiation of an apply kernel template; a macro of this file only (a function template is no template argument)
#define APPLY_FORM(kernel, scatter, stamped) \
  ((scatter) ? ((stamped) ? kernel<true, true> : kernel<true, false>) : ((stamped) ? kernel<false, true> : kernel<false, false>))

// acc = the hull of acc and b ({x0, y0, x1, y1} inclusive, empty where x1 < x0); b is not empty
static void box_widen(int acc[4], const int b[4]) {
  if (acc[2] < acc[0]) {
    for (int k = 0; k < 4; ++k) acc[k] = b[k];
    return;
  }
  if (b[0] < acc[0]) acc[0] = b[0];
  if (b[1] < acc[1]) acc[1] = b[1];
  if (b[2] > acc[2]) acc[2] = b[2];
  if (b[3] > acc[3]) acc[3] = b[3];
}

// `applied` more updates of a level (an empty container counts, too): OccGridMapBase.h:123-124, :167, setUpdated() (GridMapBase.h:343)
static void advance_update_counters(Level& L, int applied) {
  L.curr_mark_free = L.curr_update_index + 3 * (applied - 1) + 1;
  L.curr_mark_occ = L.curr_update_index + 3 * (applied - 1) + 2;
  L.curr_update_index += 3 * applied;
  L.last_update_index += applied;
}

int hsm_host::fill_level(hsm_ctx* h, Level& L) {  // GridMapBase::clear + LogOddsCell::resetGridCell
  hipLaunchKernelGGL(fill_level_kernel, dim3(grid_for(L.cells())), dim3(256), 0, h->stream, level_rw(L),
                     0.0f, -1);
  HIP_TRY(hipGetLastError());
  return HSM_OK;
}

int hsm_host::rebuild_probability(hsm_ctx* h, Level& L) {
  hipLaunchKernelGGL(rebuild_prob_kernel, dim3(grid_for(L.cells())), dim3(256), 0, h->stream, level_rw(L));
  if (L.d_quad)
    hipLaunchKernelGGL(rebuild_quad_kernel, dim3(grid_for(L.cells())), dim3(256), 0, h->stream, level_rw(L));
  HIP_TRY(hipGetLastError());
  return HSM_OK;
}

int hsm_host::reset_update_gate(hsm_ctx* h) {
  hipLaunchKernelGGL(update_gate_reset_kernel, dim3(1), dim3(64), 0, h->stream, h->upd.d_gate);
  HIP_TRY(hipGetLastError());
  return HSM_OK;
}

// hsm_create's share of the update state: the gate's block, reset, and the publish boxes with their first two rows empty
int hsm_host::create_update_state(hsm_ctx* h) {
  HIP_TRY(hipMalloc((void**)&h->upd.d_gate, sizeof(GateState)));
  HIP_TRY(hipMemsetAsync(h->upd.d_gate, 0, sizeof(GateState), h->stream));
  if (int rc = reset_update_gate(h)) return rc;
  HIP_TRY(hipMalloc((void**)&h->occ.d_pub_boxes, 3 * kMaxLevels * 4 * sizeof(int)));
  hipLaunchKernelGGL(update_boxes_clear_kernel, dim3(1), dim3(64), 0, h->stream, h->occ.d_pub_boxes, 2 * kMaxLevels);
  HIP_TRY(hipGetLastError());
  return HSM_OK;
}

// The marks of an update -- mark bytes (dense scans), end-cell bitmap bits (keyed form) -- are cleared by the apply pass of the
// SAME update and carry no generation tag.  If that pass never ran over them (a HIP error between the two launches, or a box
// the host found empty) they would be applied by a later scan as spurious free / occupied updates.  The level remembers that
// a mark pass is outstanding; the next update on it then clears both mark planes first and widens the rows the key-wrap
// clear covers to the whole level (the failed update's keys carry an older generation and are ignored as such).  (map_shift.hip
// clears the marks a failed update left behind, too.)
int hsm_host::scrub_pending_marks(hsm_ctx* h, Level& L) {
  HIP_TRY(hipMemsetAsync(L.d_free_bytes, 0, mark_plane_bytes(L.sx, L.sy), h->stream));
  HIP_TRY(hipMemsetAsync(L.d_occ_bits, 0, ((L.cells() + 31) / 32 + 1) * sizeof(unsigned int), h->stream));
  L.key_rows[0] = 0;
  L.key_rows[1] = L.sy - 1;
  L.marks_pending = false;
  return HSM_OK;
}

// Device-side updates (hsm_update_by_scans_device) leave their cell boxes on the device: the host never sees their poses.  Whoever
// needs Level::bbox / Level::dirty -- the box getters, and every host-side writer of them -- first waits for the context's stream
// and merges slot 0 (the running dirty boxes) and slot 1 (the last scan's boxes) of d_upd_boxes: one 256-byte copy.  Callers test
// upd_boxes_outstanding themselves, so a context that never took a device-side update pays one branch.
int hsm_host::merge_device_boxes(hsm_ctx* h) {
  if (int rc = select_device(h)) return rc;
  int host[2 * kMaxLevels * 4];
  HIP_TRY(hipMemcpyAsync(host, h->upd.d_upd_boxes, sizeof host, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  hipLaunchKernelGGL(update_boxes_clear_kernel, dim3(1), dim3(64), 0, h->stream, h->upd.d_upd_boxes, kMaxLevels);
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
  h->upd.upd_boxes_outstanding = false;
  return HSM_OK;
}

// Gated updates (hsm_update_by_scans_device_gated, hsm_slam_scans_device) count the scans they integrate on the device: the
// host never sees their decisions.  Whoever needs the levels' update counters on the host -- prepare_level, the ungated
// hsm_update_by_scans_device, hsm_update_index, reset and upload -- first waits for the context's stream, fetches the count and
// folds it in: OccGridMapBase.h:123-124, :167 and setUpdated() (GridMapBase.h:343) that many times.  Callers test
// gate_outstanding themselves, so a context that never made a gated call pays one branch.  *state: the block as fetched.
int hsm_host::fold_gate_counters(hsm_ctx* h, GateState* state) {
  if (int rc = select_device(h)) return rc;
  GateState host;
  HIP_TRY(hipMemcpyAsync(&host, h->upd.d_gate, sizeof host, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (state) *state = host;
  const int applied = host.pending;
  if (applied > 0) {
    HIP_TRY(hipMemsetAsync(&h->upd.d_gate->pending, 0, sizeof(int), h->stream));  // ahead of every later gated call
    for (Level& L : h->levels) advance_update_counters(L, applied);
    h->upd.gate_applied_total += applied;
    if (state) state->pending = 0;
  }
  h->upd.gate_outstanding = false;
  return HSM_OK;
}

namespace {

// rows y0..y1 of a level's key planes back to zero (the free keys by whole rows of 8x4-cell tiles)
int clear_key_rows(hsm_ctx* h, Level& L, size_t y0, size_t y1) {
  HIP_TRY(hipMemsetAsync(L.d_key_occ + y0 * L.sx, 0, (y1 - y0 + 1) * L.sx * sizeof(unsigned int), h->stream));
  const size_t row_words = (size_t)key_free_tiles_x(L.sx) * 32u;  // one row of 8x4-cell tiles
  HIP_TRY(hipMemsetAsync(L.d_key_free + (y0 >> 2) * row_words, 0, ((y1 >> 2) - (y0 >> 2) + 1) * row_words * sizeof(unsigned int), h->stream));
  return HSM_OK;
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
      if (int rc = scrub_pending_marks(h, L)) return rc;
    if (++L.serial > kSerialMax) {
      // key generation wrapped (every 4095 updates of a level): clear the rows that carry keys -- the union of the update
      // boxes since the last clear, not the whole planes (an 8192^2 level would be a 512 MB memset in the middle of a
      // 40 Hz update stream)
      if (L.key_rows[1] >= L.key_rows[0])
        if (int rc = clear_key_rows(h, L, (size_t)L.key_rows[0], (size_t)L.key_rows[1])) return rc;
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
  if (!h->cfg.upd.dense_bits || max_n < h->cfg.upd.merged_mark_max) return false;
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
    if (!h->upd.d_beam_recs.holds((size_t)max_n * HSM_MAX_LEVELS))
      if (int rc = h->upd.d_beam_recs.reserve(grown_capacity((size_t)max_n, kHalfMore) * HSM_MAX_LEVELS)) return rc;
    const size_t per_level = h->upd.d_beam_recs.count() / HSM_MAX_LEVELS;
    for (int i = 0; i < batch.nlev; ++i) batch.lv[i].recs = h->upd.d_beam_recs + (size_t)i * per_level;
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
  const bool quad = h->cfg.layout == kLayoutQuad;
  int max_n = 0;
  for (int i = 0; i < batch.nlev; ++i)
    if (batch.lv[i].n > max_n) max_n = batch.lv[i].n;
  if (use_dense_bits(h, batch, max_n)) {
    // one wavefront per block of 256 cells of the widened box (32 x 8 cells: two 16 x 8 mark tiles; map_update.h)
    const int g = grid_for(max_box / 4 + 4096);
    hipLaunchKernelGGL(APPLY_FORM(update_apply_dense_kernel, quad, batch.stamped), dim3(g, ny), dim3(256), 0, h->stream, batch);
    HIP_TRY(hipGetLastError());
    return HSM_OK;
  }
  // the apply pass writes the texels itself: one dependent launch less for the launch-bound small scans (1081 beams,
  // 3 levels: complete 39 -> 34.5 us) and one dense pass less for the big ones (16 k beams on 8192^2: 0.51 -> 0.45 ms)
  const bool scatter = quad && max_n < h->cfg.upd.scatter_texels_max;
  hipLaunchKernelGGL(APPLY_FORM(update_apply_kernel, scatter, batch.stamped), dim3(grid_for(max_box), ny), dim3(256), 0, h->stream, batch);
  if (quad && !scatter) hipLaunchKernelGGL(update_texels_kernel, dim3(grid_for(max_box), ny), dim3(256), 0, h->stream, batch);
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

// what a host-side update does before it touches a level: it rewrites Level::bbox, so the boxes of device-side updates go in
// first; it numbers its update behind the ones gated calls applied; and it queues behind a caller's batch match
int begin_host_update(hsm_ctx* h) {
  if (int rc = select_device(h)) return rc;
  if (h->upd.upd_boxes_outstanding)
    if (int rc = merge_device_boxes(h)) return rc;
  if (h->upd.gate_outstanding)
    if (int rc = fold_gate_counters(h)) return rc;
  return order_after_foreign_match(h);
}

// ... and what it does with the `nprep` levels it prepared (prep[0] the finest): the GPU starts marking (all levels, one launch)
// while the host works out the boxes of the dense passes.  `same_container`: the coarser levels see prep[0]'s container
int mark_and_apply(hsm_ctx* h, UpdateBatch& batch, LevelPrep* prep, int nprep, bool same_container) {
  if (int rc = launch_update_mark(h, batch)) return rc;
  level_bbox(h, batch, prep[0], nullptr, 0);
  for (int l = 1; l < nprep; ++l) {
    const bool derive = same_container && prep[0].slot >= 0 && prep[0].derivable && h->levels[l].sx == (h->levels[0].sx >> l) &&
                        h->levels[l].sy == (h->levels[0].sy >> l);
    level_bbox(h, batch, prep[l], derive ? &batch.lv[prep[0].slot] : nullptr, l);
  }
  if (int rc = launch_update_apply(h, batch)) return rc;
  for (int l = 0; l < nprep; ++l) update_applied(h, batch, prep[l]);
  return HSM_OK;
}

// pts_xy: host copy of the endpoints (always needed: the touched bounding box is computed on the host);
// d_prestaged: the same endpoints already on the device, or nullptr to upload them
int update_impl(hsm_ctx* h, const float pose_world[3], const float* pts_xy, int n, const float origo[2],
                const float2* d_prestaged) {
  if (int rc = begin_host_update(h)) return rc;
  const float zero[2] = {0.0f, 0.0f};
  const float* o = origo ? origo : zero;
  // level 0: the caller's container
  const float2* d_level0 = d_prestaged;
  int slot = -1;
  // The usual flow updates with the scan that was just matched.  When the matcher put that scan into device memory (dense
  // scans, multi-level maps: d_retained) and the caller hands over the same endpoints, they are already where the update
  // kernels read them: no second upload (131 KB from pageable memory for a 16 k-beam scan, which the host waits for).
  const int rn = h->retained.retained_valid ? (int)(h->retained.retained_pts.size() / 2) : 0;
  auto same_as_retained = [&] { return rn == n && n > 0 && memcmp(h->retained.retained_pts.data(), pts_xy, (size_t)n * sizeof(float2)) == 0; };
  const bool same_as_matched = !d_level0 && h->retained.d_retained_current && same_as_retained();
  if (same_as_matched) d_level0 = h->retained.d_retained;
  if (!d_level0 && h->cfg.upd.async_update) {
    // stage the endpoints in pinned memory (a pageable hipMemcpyAsync would block the host until the copy
    // -- and everything queued before it -- has completed); small scans are then read in place over PCIe
    // (each endpoint is read twice), dense ones copied to the device by a copy the host does not wait for
    slot = h->upd.upd_slot;
    h->upd.upd_slot ^= 1;
    if (h->upd.upd_busy[slot]) {
      HIP_TRY(hipEventSynchronize(h->upd.upd_evt[slot]));
      h->upd.upd_busy[slot] = false;
    }
    if (int rc = h->upd.h_upd_pinned[slot].reserve((size_t)n, kScanGrowth)) return rc;
    if (!h->upd.upd_evt[slot]) HIP_TRY(hipEventCreateWithFlags(&h->upd.upd_evt[slot], hipEventDisableTiming));
    if (n > 0) memcpy(h->upd.h_upd_pinned[slot], pts_xy, (size_t)n * sizeof(float2));
    if (n <= h->cfg.upd.update_zero_copy_max) {
      float2* dev = nullptr;
      if (n > 0) HIP_TRY(hipHostGetDevicePointer((void**)&dev, h->upd.h_upd_pinned[slot], 0));
      d_level0 = n > 0 ? dev : h->d_scan;
    } else {
      if (int rc = h->d_scan.reserve((size_t)n, kScanGrowth)) return rc;
      HIP_TRY(hipMemcpyAsync(h->d_scan, h->upd.h_upd_pinned[slot], (size_t)n * sizeof(float2), hipMemcpyHostToDevice,
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
  batch.nlev = batch.stamped = 0;
  LevelPrep prep[HSM_MAX_LEVELS];
  if (int rc = prepare_level(h, batch, prep[0], 0, pose_world, d_level0, pts_xy, n, 1.0f, o)) return rc;
  // coarse levels: the containers retained by the last matchData (MapRepMultiMap.h:143)
  bool coarse_same_container = false;  // the usual flow: update with the container that was just matched
  if (h->levels.size() > 1) {
    const float2* d_coarse = nullptr;
    if (same_as_matched || (!h->retained.d_retained_current && same_as_retained())) {
      d_coarse = d_level0;
      coarse_same_container = h->retained.retained_origo[0] == o[0] && h->retained.retained_origo[1] == o[1];
    } else {
      if (rn > 0 && !h->retained.d_retained_current) {
        if (int rc = h->retained.d_retained.reserve((size_t)rn, kScanGrowth)) return rc;
        HIP_TRY(hipMemcpyAsync(h->retained.d_retained, h->retained.retained_pts.data(), (size_t)rn * sizeof(float2),
                               hipMemcpyHostToDevice, h->stream));
        h->retained.d_retained_current = true;
      }
      d_coarse = h->retained.d_retained;  // read only after a possible (re)allocation above
    }
    for (size_t l = 1; l < h->levels.size(); ++l) {
      const float factor = level_factor((int)l);
      const float ol[2] = {h->retained.retained_origo[0] * factor, h->retained.retained_origo[1] * factor};  // setFrom :48
      if (int rc = prepare_level(h, batch, prep[l], (int)l, pose_world, d_coarse, h->retained.retained_pts.data(), rn, factor, ol))
        return rc;
    }
  }
  if (int rc = mark_and_apply(h, batch, prep, (int)h->levels.size(), coarse_same_container)) return rc;
  h->upd.queued_update = h->cfg.upd.async_update;
  if (slot >= 0) {
    HIP_TRY(hipEventRecord(h->upd.upd_evt[slot], h->stream));
    h->upd.upd_busy[slot] = true;
  }
  if (!h->cfg.upd.async_update) HIP_TRY(hipStreamSynchronize(h->stream));
  return HSM_OK;
}

// the UpdateBatch blocks and cell boxes of `count` scans (hsm_ctx::d_upd_batches / d_upd_boxes)
int ensure_update_scans(hsm_ctx* h, size_t count) {
  if (h->upd.d_upd_boxes && h->upd.d_upd_batches.holds(count)) return HSM_OK;
  if (h->upd.upd_boxes_outstanding)  // the running boxes live in the block that is about to go
    if (int rc = merge_device_boxes(h)) return rc;
  if (int rc = h->upd.d_upd_boxes.drop()) return rc;  // (both go before either comes back: the box block stands for the pair)
  if (int rc = h->upd.d_upd_batches.drop()) return rc;
  const size_t want = grown_capacity(count, {64, 50});
  if (int rc = h->upd.d_upd_batches.reserve(want)) return rc;
  if (int rc = h->upd.d_upd_boxes.reserve((want + 2) * kMaxLevels * 4)) return rc;
  hipLaunchKernelGGL(update_boxes_clear_kernel, dim3(1), dim3(64), 0, h->stream, h->upd.d_upd_boxes, 2 * kMaxLevels);
  HIP_TRY(hipGetLastError());
  return HSM_OK;
}

// `count` posed scans that are on the device, integrated in order by stream-ordered launches only: one update_prep_kernel, then
// a mark and an apply launch per scan (map_update_scans.h).  The host supplies what it can
// compute without the poses: per level the counters and the key generation before the call, from which scan k's follow.
// `gate`: the gated entries.  update_gate_prep_kernel takes update_prep_kernel's place: it decides on the device which scans are
// integrated and numbers them behind the updates earlier gated calls applied, so the levels' counters are not advanced here
// (fold_gate_counters); a rejected scan's two launches return at once.  (PosedScans, GateCall: hsm_ctx.h.)
int update_by_scans_device_nolock(hsm_ctx* h, const PosedScans& S, hipStream_t stream) {
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
  if (!gate && h->upd.gate_outstanding)  // scan k is update k behind EVERY earlier update: the ones gated calls applied go in first
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
  A.out = h->upd.d_upd_batches;
  A.boxes = h->upd.d_upd_boxes;
  size_t max_cells = 0;
  for (int l = 0; l < nlev; ++l) {
    Level& L = h->levels[l];
    if (L.marks_pending)
      if (int rc = scrub_pending_marks(h, L)) return rc;
    UpdatePrepLevel& V = A.lv[l];
    const float factor = level_factor(l);
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
    G.state = h->upd.d_gate;
    G.min_dist = h->upd.gate_min_dist;
    G.min_angle = h->upd.gate_min_angle;
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
  const bool scatter = h->cfg.layout == kLayoutQuad;
  // Restored stamps at or ahead of the first scan's free mark: the whole call takes the stamp-aware apply pass.  (A gated call
  // whose predecessors' counts are still on the device sees a counter that lags: the test errs towards the stamp-aware form.)
  bool stamped = false;
  for (int l = 0; l < nlev; ++l) stamped |= h->levels[l].stamps_ahead();
  auto apply_scan = APPLY_FORM(update_apply_scan_kernel, scatter, stamped);
  for (int l = 0; l < nlev; ++l) h->levels[l].marks_pending = true;  // until every apply pass is queued (scrub_pending_marks)
  for (int k = 0; k < count; ++k) {
    for (int l = 0; l < nlev; ++l) {
      Level& L = h->levels[l];
      // The key generation advances once per scan and level, empty scan or not (the host cannot see n_k; a generation spent on
      // an empty scan is harmless).  Where it wraps, the key planes are cleared between the two scans concerned: the WHOLE
      // level, not the rows that carry keys -- those rows are known on the device only, and a wrap is one scan in 4095.
      if (L.serial == kSerialMax) {
        if (int rc = clear_key_rows(h, L, 0, (size_t)L.sy - 1)) return rc;
        L.serial = 0;
      }
      ++L.serial;
    }
    int* scan_boxes = h->upd.d_upd_boxes + (size_t)update_box_slot(k, count) * kMaxLevels * 4;
    hipLaunchKernelGGL(update_mark_scan_kernel, dim3(occ_blocks + free_blocks, (unsigned)nlev), dim3(256), 0, h->stream,
                       h->upd.d_upd_batches + k, occ_blocks, scan_boxes, h->upd.d_upd_boxes, h->occ.d_pub_boxes);
    hipLaunchKernelGGL(apply_scan, dim3(apply_blocks, (unsigned)nlev), dim3(256), 0, h->stream, h->upd.d_upd_batches + k, scan_boxes);
    HIP_TRY(hipGetLastError());
  }
  for (int l = 0; l < nlev; ++l) {
    Level& L = h->levels[l];
    L.marks_pending = false;
    if (!gate) advance_update_counters(L, count);  // (a gated call's count stays on the device: fold_gate_counters)
    L.key_rows[0] = 0;  // which rows carry keys of this generation is known on the device only: the next wrap of a host-side
    L.key_rows[1] = L.sy - 1;  // update clears the whole level
  }
  h->upd.upd_boxes_outstanding = true;
  if (gate) h->upd.gate_outstanding = true;
  h->upd.queued_update = h->cfg.upd.async_update;
  if (!h->cfg.upd.async_update) HIP_TRY(hipStreamSynchronize(h->stream));
  return HSM_OK;
}

// what the four device entries share: the context's lock around the update
int update_by_scans_device_locked(hsm_ctx* h, const PosedScans& S, void* stream) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  std::lock_guard<std::mutex> lk(h->mu);
  return update_by_scans_device_nolock(h, S, static_cast<hipStream_t>(stream));
}

// ... and the two gated ones: the call's gate
int update_by_scans_device_gated(hsm_ctx* h, PosedScans S, const unsigned char* d_force, int* d_out_applied, void* stream) {
  GateCall gate;
  gate.d_force = d_force;
  gate.d_out_applied = d_out_applied;
  S.gate = &gate;
  return update_by_scans_device_locked(h, S, stream);
}

}  // namespace

// the loop itself, on the context's stream.  `scans`: the log's CSR end points, beam hint, origo(s) and the name its updates
// report under (count, poses and gate are the loop's to set)
int hsm_host::slam_scans_queue(hsm_ctx* h, const ScanLog& log, const PosedScans& scans) {
  hipLaunchKernelGGL(slam_begin_kernel, dim3(1), dim3(64), 0, h->stream, h->upd.d_gate, log.d_start_pose, log.d_hint_deltas);
  HIP_TRY(hipGetLastError());
  GateCall gate;
  PosedScans one = scans;
  one.count = 1;
  one.shared_n = 0;
  one.gate = &gate;
  for (int k = 0; k < log.count; ++k) {
    // scan k as a batch of one for the matcher: its start from the gate's device block, its slice of the CSR, the log's beam hint
    const ScanBatch scan{1, h->upd.d_gate->hint, scans.d_pts, scans.d_offsets + k, scans.max_beams};
    if (int rc = match_batch_device_nolock(h, scan, {log.pose(k), log.cov(k)}, h->stream)) return rc;
    gate = log.gate(k);
    one.d_poses = gate.pose_io;
    one.d_offsets = scans.d_offsets + k;
    one.d_origos = scans.d_origos ? scans.d_origos + 2 * (size_t)k : nullptr;
    if (int rc = update_by_scans_device_nolock(h, one, h->stream)) return rc;
  }
  return HSM_OK;
}

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

extern "C" {

int hsm_update_by_scan(hsm_ctx* h, const float pose_world[3], const float* pts_xy, int n, const float origo[2]) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  if (!pose_world || n < 0 || (n > 0 && !pts_xy)) return fail(HSM_ERR_INVALID, "hsm_update_by_scan: bad argument");
  std::lock_guard<std::mutex> lk(h->mu);
  return update_impl(h, pose_world, pts_xy, n, origo, nullptr);
}

int hsm_update_by_ingested(hsm_ctx* h, const float pose_world[3]) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  if (!pose_world || h->ingest.ingest_n < 0) return fail(HSM_ERR_INVALID, "hsm_update_by_ingested: no scan ingested");
  std::lock_guard<std::mutex> lk(h->mu);
  static const float dummy[2] = {0.0f, 0.0f};
  const float* hp = h->ingest.ingest_n > 0 ? h->ingest.h_ingest.data() : dummy;
  return update_impl(h, pose_world, hp, h->ingest.ingest_n, h->ingest.ingest_origo, h->ingest.d_ingest);
}

int hsm_update_by_scan_level(hsm_ctx* h, int level, const float pose_world[3], const float* pts_level_xy, int n,
                             const float origo_level[2]) {
  if (int rc = valid_level(h, level)) return rc;
  if (!pose_world || n < 0 || (n > 0 && !pts_level_xy))
    return fail(HSM_ERR_INVALID, "hsm_update_by_scan_level: bad argument");
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = begin_host_update(h)) return rc;
  const float zero[2] = {0.0f, 0.0f};
  if (int rc = h->d_scan.reserve((size_t)n, kScanGrowth)) return rc;
  if (n > 0)
    HIP_TRY(hipMemcpyAsync(h->d_scan, pts_level_xy, (size_t)n * sizeof(float2), hipMemcpyHostToDevice, h->stream));
  UpdateBatch batch;
  batch.nlev = batch.stamped = 0;
  LevelPrep prep;
  if (int rc = prepare_level(h, batch, prep, level, pose_world, h->d_scan, pts_level_xy, n, 1.0f,
                             origo_level ? origo_level : zero))
    return rc;
  if (int rc = mark_and_apply(h, batch, &prep, 1, false)) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  return HSM_OK;
}

int hsm_set_update_gate(hsm_ctx* h, float min_dist, float min_angle) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  std::lock_guard<std::mutex> lk(h->mu);
  h->upd.gate_min_dist = min_dist;
  h->upd.gate_min_angle = min_angle;
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
  if (applied_total) *applied_total = h->upd.gate_applied_total;
  return HSM_OK;
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
  PosedScans S{count, d_poses_world, d_pts_xy, d_scan_offsets, shared_n, max_beams};
  S.origo = origo;  // (the texts stay the ungated entry's)
  return update_by_scans_device_gated(h, S, d_force, d_out_applied, stream);
}

int hsm_update_by_scans_device_gated_origos(hsm_ctx* h, int count, const float* d_poses_world, const float* d_pts_xy,
                                            const int* d_scan_offsets, int shared_n, int max_beams, const float* d_origos,
                                            const unsigned char* d_force, int* d_out_applied, void* stream) {
  PosedScans S{count, d_poses_world, d_pts_xy, d_scan_offsets, shared_n, max_beams};
  S.d_origos = d_origos;
  S.who = "hsm_update_by_scans_device_gated_origos";
  return update_by_scans_device_gated(h, S, d_force, d_out_applied, stream);
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
  for (const hsm_ctx::ForeignStream& f : h->order.foreign)  // refused before the copies are queued (order_after_foreign_match)
    if (stream_capturing(f.s))
      return fail(HSM_ERR_INVALID, "hsm_update_by_scans: a caller's stream that this context matches on is being captured into a graph");
  // one staging block (the copies are queued on the context's stream, in front of the update)
  const UpdateScansStage st = update_scans_stage(count, total, poses_world, pts_xy, scan_offsets);
  if (int rc = h->upd.d_upd_stage.reserve(st.plan.total(), kHalfMore)) return rc;
  char* base = h->upd.d_upd_stage;
  if (int rc = stage_copy_in(st.plan, base, h->stream)) return rc;
  PosedScans S{count, staged<float>(base, st.poses), staged<float>(base, st.pts),
                             staged<int>(base, st.offs, scan_offsets), shared_n, longest};
  S.origo = origo;
  return update_by_scans_device_nolock(h, S, h->stream);
}

}  // extern "C"
