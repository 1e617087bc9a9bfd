// map_shift.hip -- the map window moved under the robot without a host trip (include/hector_mi355/capi.h: hsm_shift_map,
// hsm_map_start): the geometry becomes what hsm_create derives from other start coordinates, and the contents of every level
// keep their WORLD position -- they move by a whole number of cells, what scrolls in is cleared, what scrolls out is gone.  The
// plan is map_shift_plan.h's, the kernels map_shift_kernels.h's; what this entry needs of the core runtime (hector_mi355.hip)
// is declared in hsm_ctx.h.
//
// The planes of a level keep their addresses, so the surviving cells go through the context's staging patch (d_copy_patch, the
// block of hsm_copy_map's staged route: both are queued on the context's stream, so one never reads what the other writes).
// Three launches per pyramid, blockIdx.y = level: stage the survivors, write every cell once, rebuild the texels.
//
// What else carries cell positions between calls, and why none of it is moved:
//   key planes, key_rows   a key is (generation of the scan that wrote it, beam index) and is only ever compared with the keys
//                          of the CURRENT scan; the generation counter (Level::serial) is not touched here, so every key the
//                          planes hold stays older than the next update's, wherever it lies.  key_rows names the rows of the
//                          PLANE the wrap clear has to cover -- the keys did not move, so neither does it.  As after
//                          hsm_upload_level, which replaces a level's cells and leaves both alone.
//   d_occ_bits, d_free_bytes   zero between updates: the apply pass of an update clears the marks its mark pass set.  Only an
//                          update that failed between the two leaves marks behind (Level::marks_pending); those are scrubbed
//                          here, on the stream, instead of waiting for the next update: they would mark other cells' contents.
#include <hip/hip_runtime.h>

#include <cmath>
#include <mutex>

#include "hector_mi355/capi.h"
#include "hsm_ctx.h"
#include "map_shift_kernels.h"

using namespace hsm;
using namespace hsm_host;

static_assert(kShiftMaxLevels == HSM_MAX_LEVELS && kShiftMaxLevels == kMaxLevels, "map_shift_plan.h states the level limit again");

namespace {

const char* refusal_text(int refusal) {
  switch (refusal) {
    case kShiftNonFinite: return ": a start coordinate (or the offset it gives) is not finite";
    case kShiftFraction: return ": the move is further than 1/64 cell from a whole number of level-0 cells";
    case kShiftNotMultiple: return ": level 0's displacement is no multiple of 2^(levels - 1) cells";
    case kShiftTooFar: return ": the displacement is beyond 2^30 cells";
    default: return ": bad map geometry";
  }
}

}  // namespace

extern "C" {

int hsm_shift_map(hsm_ctx* h, float new_start_x, float new_start_y, int shift_cells[2]) {
  const char* who = "hsm_shift_map";
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  std::lock_guard<std::mutex> lk(h->mu);
  const int nlev = (int)h->levels.size();
  const Level& L0 = h->levels[0];
  const float to[2] = {new_start_x, new_start_y};
  const ShiftPlan plan = plan_map_shift(L0.cell_length, L0.sx, L0.sy, nlev, h->start, to);
  if (plan.refusal != kShiftOk) return fail_at(HSM_ERR_INVALID, who, refusal_text(plan.refusal));
  // a move is not captured, like every writer of a map
  for (const hsm_ctx::ForeignStream& f : h->order.foreign)
    if (stream_capturing(f.s))
      return fail_at(HSM_ERR_INVALID, who, ": a caller's stream that the context matches on is being captured into a graph");
  if (shift_cells) shift_cells[0] = plan.d0[0], shift_cells[1] = plan.d0[1];
  if (plan.same_start) return HSM_OK;  // (then the displacement is zero: nothing to queue, nothing to change)

  if (plan.moves) {
    if (int rc = select_device(h)) return rc;
    if (h->upd.upd_boxes_outstanding)  // (their boxes are in old coordinates; the whole level is marked below)
      if (int rc = merge_device_boxes(h)) return rc;
    if (h->upd.gate_outstanding)
      if (int rc = fold_gate_counters(h)) return rc;
    MapShiftParams P = {};
    P.nlev = nlev;
    size_t patch_elems = 0, max_cells = 0;
    unsigned int stage_turns = 0, cell_turns = 0;
    CopyPatch patch[kMaxLevels];
    for (int l = 0; l < nlev; ++l) {
      const Level& L = h->levels[l];
      const CopyBox& b = plan.lv[l].from;
      patch[l] = copy_patch_at(patch_elems, b);
      patch_elems = patch[l].end;
      if (L.cells() > max_cells) max_cells = L.cells();
      const unsigned int ct = (unsigned int)L.sy * (((unsigned int)occupancy_row_slots(L.sx) + 63u) >> 6);
      if (ct > cell_turns) cell_turns = ct;
      if (copy_box_empty(b)) continue;
      const CopyRuns R = copy_box_runs(L.sx, b);
      const unsigned int st = (unsigned int)R.runs * (((unsigned int)copy_run_slots(R) + 63u) >> 6);
      if (st > stage_turns) stage_turns = st;
    }
    if (patch_elems > 0)  // grown here, outside any capture (refused above), before anything is queued
      if (int rc = h->copy.d_copy_patch.reserve(patch_elems, kHalfMore)) return rc;
    // a writer of the map: behind the matches callers' streams may still be running on it, and -- on the context's stream --
    // behind every update queued so far
    if (int rc = order_after_foreign_match(h)) return rc;
    for (int l = 0; l < nlev; ++l) {
      Level& L = h->levels[l];
      if (L.marks_pending)
        if (int rc = scrub_pending_marks(h, L)) return rc;
      MapShiftLevel& M = P.lv[l];
      M.logodds = L.d_logodds;
      M.stamps = L.d_update_index;
      M.prob = L.d_prob;
      M.quad = L.d_quad;
      M.sx = L.sx;
      M.sy = L.sy;
      M.from = plan.lv[l].from;
      M.to = plan.lv[l].to;
      float* base = h->copy.d_copy_patch;
      M.st_logodds = base + patch[l].logodds;
      M.st_stamps = reinterpret_cast<int*>(base + patch[l].stamps);
    }
    if (stage_turns > 0)
      hipLaunchKernelGGL(map_shift_stage_kernel, dim3((unsigned int)grid_for((size_t)stage_turns * 64), (unsigned int)nlev), dim3(256), 0,
                         h->stream, P);
    hipLaunchKernelGGL(map_shift_cells_kernel, dim3((unsigned int)grid_for((size_t)cell_turns * 64), (unsigned int)nlev), dim3(256), 0,
                       h->stream, P);
    if (h->cfg.layout == kLayoutQuad)
      hipLaunchKernelGGL(map_shift_texels_kernel, dim3((unsigned int)grid_for(max_cells), (unsigned int)nlev), dim3(256), 0, h->stream, P);
    HIP_TRY(hipGetLastError());
    // the device's share of the publish boxes: the whole level, from the row hsm_create wrote
    HIP_TRY(hipMemcpyAsync(h->occ.d_pub_boxes, h->occ.d_pub_boxes + 2 * kMaxLevels * 4, (size_t)nlev * 4 * sizeof(int), hipMemcpyDeviceToDevice,
                           h->stream));
  }
  for (int l = 0; l < nlev; ++l) {
    Level& L = h->levels[l];
    set_level_transformation(L, plan.off[0], plan.off[1], L.cell_length);  // hsm_create's arithmetic on the new offsets
    if (!plan.moves) continue;
    L.bbox[0] = L.bbox[1] = 0;
    L.bbox[2] = L.bbox[3] = -1;
    whole_level_changed(L);
  }
  h->start[0] = new_start_x;
  h->start[1] = new_start_y;
  return HSM_OK;
}

int hsm_map_start(const hsm_ctx* h, float start[2]) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  if (!start) return fail(HSM_ERR_INVALID, "hsm_map_start: start is null");
  std::lock_guard<std::mutex> lk(h->mu);
  start[0] = h->start[0];
  start[1] = h->start[1];
  return HSM_OK;
}

}  // extern "C"
