// map_copy.hip -- a pyramid, or one cell box per level of it, from one context into another without a host trip
// (include/hector_mi355/capi.h: hsm_copy_map, hsm_copy_map_boxes): GridMapBase's copy constructor and operator=
// (GridMapBase.h:173-205) between two contexts, and the changed cells of one shipped to another.  The kernels are
// map_copy_kernels.h's, the box arithmetic map_copy_box.h's; what these entries need of the core runtime (hector_mi355.hip) is
// declared in hsm_ctx.h.  (hsm_group_sync_maps, which runs them over a group's replicas, is in group.hip.)
//
// Two routes, one kernel.  Same device: pass 1 reads the source's planes directly.  Different devices (or HSM_COPY_STAGE=1 at
// the destination's hsm_create): the box's rows of both planes are first copied into a staging patch on the destination's
// device, and pass 1 reads the patch.  The copies and both passes run on the DESTINATION's stream.
//
// The whole pyramid is the same two launches with every level's box the whole level, not hipMemcpyAsync of the two planes
// followed by the rebuild kernels: a whole-width box is ONE run of contiguous cells (map_copy_box.h), so pass 1 is a stream of
// 16-byte loads and stores that reads the log-odds once, where the memcpy form reads them a second time for the probabilities,
// four bytes per lane, and takes two copy commands and two launches per level instead of two launches per pyramid.
#include <hip/hip_runtime.h>

#include <mutex>

#include "hector_mi355/capi.h"
#include "hsm_ctx.h"
#include "map_copy_kernels.h"

using namespace hsm;
using namespace hsm_host;

namespace {

void widen(int acc[4], const CopyBox& b) {
  if (acc[2] < acc[0]) {
    acc[0] = b.x0, acc[1] = b.y0, acc[2] = b.x1, acc[3] = b.y1;
    return;
  }
  if (b.x0 < acc[0]) acc[0] = b.x0;
  if (b.y0 < acc[1]) acc[1] = b.y0;
  if (b.x1 > acc[2]) acc[2] = b.x1;
  if (b.y1 > acc[3]) acc[3] = b.y1;
}

bool same_geometry(const hsm_ctx* a, const hsm_ctx* b) {
  if (a->levels.size() != b->levels.size() || a->cfg.layout != b->cfg.layout) return false;
  for (size_t l = 0; l < a->levels.size(); ++l) {
    const Level &A = a->levels[l], &B = b->levels[l];
    if (A.sx != B.sx || A.sy != B.sy || A.cell_length != B.cell_length || A.mapTworld.t0 != B.mapTworld.t0 ||
        A.mapTworld.t1 != B.mapTworld.t1)
      return false;
  }
  return true;
}

// boxes == nullptr: every level whole
int copy_map(hsm_ctx* dst, hsm_ctx* src, const int* boxes, bool whole, const char* who) {
  if (!dst || !src) return fail(HSM_ERR_INVALID, "null context");
  if (dst == src) return fail_at(HSM_ERR_INVALID, who, ": dst and src are the same context");
  if (!whole && !boxes) return fail_at(HSM_ERR_INVALID, who, ": boxes is null");
  // (two copies in opposite directions on two threads must not wait for each other)
  std::unique_lock<std::mutex> lk_a(dst < src ? dst->mu : src->mu);
  std::unique_lock<std::mutex> lk_b(dst < src ? src->mu : dst->mu);
  if (!same_geometry(dst, src))
    return fail_at(HSM_ERR_INVALID, who, ": the contexts differ in level count, size, resolution, offsets or layout");
  const int nlev = (int)dst->levels.size();
  MapCopyParams P = {};
  P.nlev = nlev;
  size_t patch_elems = 0, max_cells = 0, max_texels = 0;
  unsigned int max_turns = 0;
  CopyPatch patch[kMaxLevels];
  for (int l = 0; l < nlev; ++l) {
    const Level& D = dst->levels[l];
    CopyBox b = whole ? CopyBox{0, 0, D.sx - 1, D.sy - 1} : CopyBox{boxes[4 * l], boxes[4 * l + 1], boxes[4 * l + 2], boxes[4 * l + 3]};
    if (copy_box_empty(b)) {
      b = CopyBox{0, 0, -1, -1};
    } else if (!copy_box_inside(b, D.sx, D.sy)) {
      return fail_at(HSM_ERR_INVALID, who, ": a box reaches outside its level");
    }
    P.lv[l].box = b;
    patch[l] = copy_patch_at(patch_elems, b);
    patch_elems = patch[l].end;
    if (copy_box_empty(b)) continue;
    const CopyRuns R = copy_box_runs(D.sx, b);
    const unsigned int turns = (unsigned int)R.runs * (((unsigned int)copy_run_slots(R) + 63u) >> 6);
    if (turns > max_turns) max_turns = turns;
    if (copy_box_cells(b) > max_cells) max_cells = copy_box_cells(b);
    if (copy_box_cells(copy_texel_box(b)) > max_texels) max_texels = copy_box_cells(copy_texel_box(b));
  }
  // copies are not captured, like every writer of a map
  for (const hsm_ctx* h : {dst, src})
    for (const hsm_ctx::ForeignStream& f : h->order.foreign)
      if (stream_capturing(f.s))
        return fail_at(HSM_ERR_INVALID, who, ": a caller's stream that one of the contexts matches on is being captured into a graph");

  // the source's counters: gated updates keep theirs on the device until someone asks (this waits for the source's stream)
  if (src->upd.gate_outstanding)
    if (int rc = fold_gate_counters(src)) return rc;
  if (int rc = select_device(dst)) return rc;
  if (dst->upd.upd_boxes_outstanding)
    if (int rc = merge_device_boxes(dst)) return rc;
  if (dst->upd.gate_outstanding)  // (what they still hold would be added to the counters copied below)
    if (int rc = fold_gate_counters(dst)) return rc;
  const bool staged = dst->device != src->device || dst->cfg.forms.copy_stage;
  if (staged && max_cells > 0)
    if (int rc = dst->copy.d_copy_patch.reserve(patch_elems, kHalfMore)) return rc;

  if (max_cells > 0) {
    // a reader of the source: behind every update queued on its stream
    if (int rc = select_device(src)) return rc;
    if (!src->copy.evt_copy_src) HIP_TRY(hipEventCreateWithFlags(&src->copy.evt_copy_src, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(src->copy.evt_copy_src, src->stream));
    // a writer of the destination: behind the matches callers' streams may still be running on it
    if (int rc = select_device(dst)) return rc;
    if (int rc = order_after_foreign_match(dst)) return rc;
    HIP_TRY(hipStreamWaitEvent(dst->stream, src->copy.evt_copy_src, 0));
    if (!dst->copy.evt_copy_read) HIP_TRY(hipEventCreateWithFlags(&dst->copy.evt_copy_read, hipEventDisableTiming));
    for (int l = 0; l < nlev; ++l) {
      const Level &D = dst->levels[l], &S = src->levels[l];
      MapCopyLevel& M = P.lv[l];
      M.logodds = D.d_logodds;
      M.stamps = D.d_update_index;
      M.prob = D.d_prob;
      M.quad = D.d_quad;
      M.sx = D.sx;
      M.sy = D.sy;
      M.src_logodds = S.d_logodds;
      M.src_stamps = S.d_update_index;
      if (!staged || copy_box_empty(M.box)) continue;
      float* base = dst->copy.d_copy_patch;
      const CopyBox& b = M.box;
      const size_t w = (size_t)(b.x1 - b.x0 + 1), rows = (size_t)(b.y1 - b.y0 + 1), at = (size_t)b.y0 * S.sx + b.x0;
      HIP_TRY(hipMemcpy2DAsync(base + patch[l].logodds, w * 4, S.d_logodds + at, (size_t)S.sx * 4, w * 4, rows, hipMemcpyDefault,
                               dst->stream));
      HIP_TRY(hipMemcpy2DAsync(base + patch[l].stamps, w * 4, S.d_update_index + at, (size_t)S.sx * 4, w * 4, rows,
                               hipMemcpyDefault, dst->stream));
      M.src_logodds = base + patch[l].logodds;
      M.src_stamps = reinterpret_cast<const int*>(base + patch[l].stamps);
    }
    const dim3 grid1((unsigned int)grid_for((size_t)max_turns * 64), (unsigned int)nlev);
    if (staged) {  // the source has been read once the patch is filled
      HIP_TRY(hipEventRecord(dst->copy.evt_copy_read, dst->stream));
      hipLaunchKernelGGL(map_copy_cells_kernel<true>, grid1, dim3(256), 0, dst->stream, P);
    } else {
      hipLaunchKernelGGL(map_copy_cells_kernel<false>, grid1, dim3(256), 0, dst->stream, P);
      HIP_TRY(hipEventRecord(dst->copy.evt_copy_read, dst->stream));
    }
    HIP_TRY(hipGetLastError());
    // the next writer of the source -- all of them queue on its stream -- behind that read
    HIP_TRY(hipStreamWaitEvent(src->stream, dst->copy.evt_copy_read, 0));
    if (dst->cfg.layout == kLayoutQuad) {
      hipLaunchKernelGGL(map_copy_texels_kernel, dim3((unsigned int)grid_for(max_texels), (unsigned int)nlev), dim3(256), 0,
                         dst->stream, P);
      HIP_TRY(hipGetLastError());
    }
  }
  for (int l = 0; l < nlev; ++l) {
    Level& D = dst->levels[l];
    const Level& S = src->levels[l];
    D.curr_update_index = S.curr_update_index;
    D.curr_mark_occ = S.curr_mark_occ;
    D.curr_mark_free = S.curr_mark_free;
    D.last_update_index = S.last_update_index;
    D.uploaded_stamp_max = S.uploaded_stamp_max;
    if (whole) {
      whole_level_changed(D);
    } else if (!copy_box_empty(P.lv[l].box)) {
      widen(D.dirty, P.lv[l].box);
      widen(D.pub, P.lv[l].box);
    }
  }
  return HSM_OK;
}

}  // namespace

extern "C" {

int hsm_copy_map(hsm_ctx* dst, hsm_ctx* src) { return copy_map(dst, src, nullptr, true, "hsm_copy_map"); }

int hsm_copy_map_boxes(hsm_ctx* dst, hsm_ctx* src, const int* boxes) { return copy_map(dst, src, boxes, false, "hsm_copy_map_boxes"); }

}  // extern "C"
