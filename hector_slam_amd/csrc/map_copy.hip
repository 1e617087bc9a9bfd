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
//
// hsm_merge_map, hsm_merge_map_box: another context's pyramid combined INTO this one's under a rigid transform (the reference has
// no such operation).  The same two-context machinery -- locks in address order, the stream hand-over, the staging patch, the
// texel pass -- around map_merge_kernels.h's kernel; the affine of a level and the boxes are map_merge_box.h's, in double.
#include <hip/hip_runtime.h>

#include <mutex>

#include "hector_mi355/capi.h"
#include "hsm_ctx.h"
#include "map_copy_kernels.h"
#include "map_merge_box.h"
#include "map_merge_kernels.h"

using namespace hsm;
using namespace hsm_host;

// (declared in hsm_ctx.h: hsm_align_map of window.hip refuses the pairs a merge refuses)
bool hsm_host::merge_compatible(const hsm_ctx* a, const hsm_ctx* b) {
  if (a->levels.size() != b->levels.size() || a->cfg.layout != b->cfg.layout) return false;
  for (size_t l = 0; l < a->levels.size(); ++l)
    if (a->levels[l].cell_length != b->levels[l].cell_length) return false;
  return true;
}

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

// ---- hsm_merge_map -------------------------------------------------------------------------------------------------------------------

// level `level`'s affine from `dst`'s cells into `src`'s map coordinates (map_merge_box.h), from the offsets hsm_create derives
// a context's transforms from -- (resolution * size) * start in fp32, level 0's for every level -- and the level's scale
MergeAffine merge_affine(const hsm_ctx* dst, const hsm_ctx* src, const float T[3], int level) {
  double od[2], os[2];
  const hsm_ctx* of[2] = {dst, src};
  for (int k = 0; k < 2; ++k) {
    const Level& L0 = of[k]->levels[0];
    double* off = k ? os : od;
    off[0] = merge_map_offset(L0.cell_length, L0.sx, of[k]->start[0]);
    off[1] = merge_map_offset(L0.cell_length, L0.sy, of[k]->start[1]);
  }
  return hsm::merge_affine(od, os, dst->levels[level].scale_to_map, T);
}

// the refusals both entries share that need no lock
int merge_refuse(const hsm_ctx* dst, const hsm_ctx* src, const float* T, const char* who) {
  if (!dst || !src) return fail(HSM_ERR_INVALID, "null context");
  if (!T) return fail_at(HSM_ERR_INVALID, who, ": src_in_dst is null");
  if (dst == src) return fail_at(HSM_ERR_INVALID, who, ": dst and src are the same context");
  if (!isfinite(T[0]) || !isfinite(T[1]) || !isfinite(T[2])) return fail_at(HSM_ERR_INVALID, who, ": src_in_dst is not finite");
  return HSM_OK;
}

int merge_map(hsm_ctx* dst, hsm_ctx* src, const float* T) {
  const char* who = "hsm_merge_map";
  if (int rc = merge_refuse(dst, src, T, who)) return rc;
  std::unique_lock<std::mutex> lk_a(dst < src ? dst->mu : src->mu);
  std::unique_lock<std::mutex> lk_b(dst < src ? src->mu : dst->mu);
  if (!merge_compatible(dst, src)) return fail_at(HSM_ERR_INVALID, who, ": the contexts differ in level count, resolution or layout");
  for (const hsm_ctx* h : {dst, src})  // merges are not captured, like every writer of a map
    for (const hsm_ctx::ForeignStream& f : h->order.foreign)
      if (stream_capturing(f.s))
        return fail_at(HSM_ERR_INVALID, who, ": a caller's stream that one of the contexts matches on is being captured into a graph");
  const int nlev = (int)dst->levels.size();
  MapMergeParams P = {};
  MapCopyParams T2 = {};  // the texel pass reads the destination's planes and the boxes only
  P.nlev = T2.nlev = nlev;
  size_t patch_at[kMaxLevels], patch_elems = 0, max_texels = 0;
  unsigned int max_tiles = 0;
  for (int l = 0; l < nlev; ++l) {
    const Level &D = dst->levels[l], &S = src->levels[l];
    const MergeAffine a = merge_affine(dst, src, T, l);
    MapMergeLevel& M = P.lv[l];
    M.c = (float)a.c, M.s = (float)a.s, M.bx = (float)a.bx, M.by = (float)a.by;
    M.box = merge_dst_box(a, D.sx, D.sy, S.sx, S.sy);
    M.sbox = merge_src_box(a, M.box, S.sx, S.sy);
    T2.lv[l].box = M.box;
    patch_at[l] = patch_elems;
    patch_elems += (copy_box_cells(M.sbox) + 3) & ~(size_t)3;
    if (merge_box_tiles(M.box) > max_tiles) max_tiles = merge_box_tiles(M.box);
    if (copy_box_cells(copy_texel_box(M.box)) > max_texels) max_texels = copy_box_cells(copy_texel_box(M.box));
  }
  if (max_tiles == 0) return HSM_OK;  // `src` lies outside `dst` on every level

  if (int rc = select_device(dst)) return rc;
  if (dst->upd.upd_boxes_outstanding)  // (the boxes below widen what the device-side updates left)
    if (int rc = merge_device_boxes(dst)) return rc;
  if (dst->upd.gate_outstanding)
    if (int rc = fold_gate_counters(dst)) return rc;
  const bool staged = dst->device != src->device || dst->cfg.forms.copy_stage;
  if (staged)
    if (int rc = dst->copy.d_copy_patch.reserve(patch_elems ? patch_elems : 4, kHalfMore)) return rc;

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
    MapMergeLevel& M = P.lv[l];
    M.logodds = D.d_logodds;
    M.prob = D.d_prob;
    M.sx = D.sx, M.sy = D.sy;
    M.ssx = S.sx, M.ssy = S.sy;
    M.src = S.d_logodds;
    T2.lv[l].prob = D.d_prob;
    T2.lv[l].quad = D.d_quad;
    T2.lv[l].sx = D.sx, T2.lv[l].sy = D.sy;
    if (!staged) continue;
    float* base = dst->copy.d_copy_patch;
    M.src = base + patch_at[l];
    if (copy_box_empty(M.sbox)) continue;  // (every sample of this level is outside the source: the patch is not read)
    const CopyBox& b = M.sbox;
    const size_t w = (size_t)(b.x1 - b.x0 + 1), rows = (size_t)(b.y1 - b.y0 + 1), at = (size_t)b.y0 * S.sx + b.x0;
    HIP_TRY(hipMemcpy2DAsync(base + patch_at[l], w * 4, S.d_logodds + at, (size_t)S.sx * 4, w * 4, rows, hipMemcpyDefault, dst->stream));
  }
  const dim3 grid1(max_tiles < 256u * 8u ? max_tiles : 256u * 8u, (unsigned int)nlev);
  if (staged) {  // the source has been read once the patch is filled
    HIP_TRY(hipEventRecord(dst->copy.evt_copy_read, dst->stream));
    hipLaunchKernelGGL(map_merge_cells_kernel<true>, grid1, dim3(256), 0, dst->stream, P);
  } else {
    hipLaunchKernelGGL(map_merge_cells_kernel<false>, grid1, dim3(256), 0, dst->stream, P);
    HIP_TRY(hipEventRecord(dst->copy.evt_copy_read, dst->stream));
  }
  HIP_TRY(hipGetLastError());
  // the next writer of the source behind that read
  HIP_TRY(hipStreamWaitEvent(src->stream, dst->copy.evt_copy_read, 0));
  if (dst->cfg.layout == kLayoutQuad) {
    hipLaunchKernelGGL(map_copy_texels_kernel, dim3((unsigned int)grid_for(max_texels), (unsigned int)nlev), dim3(256), 0, dst->stream,
                       T2);
    HIP_TRY(hipGetLastError());
  }
  // the stamps, the update counters, the marks and the restored-stamp state stay: only the publisher's index moves, on every level
  // as after an update (setUpdated(), GridMapBase.h:343)
  for (int l = 0; l < nlev; ++l) {
    Level& D = dst->levels[l];
    D.last_update_index++;
    if (copy_box_empty(P.lv[l].box)) continue;
    widen(D.dirty, P.lv[l].box);
    widen(D.pub, P.lv[l].box);
  }
  return HSM_OK;
}

}  // namespace

extern "C" {

int hsm_copy_map(hsm_ctx* dst, hsm_ctx* src) { return copy_map(dst, src, nullptr, true, "hsm_copy_map"); }

int hsm_copy_map_boxes(hsm_ctx* dst, hsm_ctx* src, const int* boxes) { return copy_map(dst, src, boxes, false, "hsm_copy_map_boxes"); }

int hsm_merge_map(hsm_ctx* dst, hsm_ctx* src, const float src_in_dst[3]) { return merge_map(dst, src, src_in_dst); }

int hsm_merge_map_box(const hsm_ctx* dst, const hsm_ctx* src, const float src_in_dst[3], int level, int bbox[4]) {
  const char* who = "hsm_merge_map_box";
  if (int rc = merge_refuse(dst, src, src_in_dst, who)) return rc;
  if (!bbox) return fail_at(HSM_ERR_INVALID, who, ": bbox is null");
  std::unique_lock<std::mutex> lk_a(dst < src ? dst->mu : src->mu);  // (hsm_shift_map rewrites the geometry)
  std::unique_lock<std::mutex> lk_b(dst < src ? src->mu : dst->mu);
  if (!merge_compatible(dst, src)) return fail_at(HSM_ERR_INVALID, who, ": the contexts differ in level count, resolution or layout");
  if (int rc = valid_level(dst, level)) return rc;
  const Level &D = dst->levels[level], &S = src->levels[level];
  const CopyBox b = merge_dst_box(merge_affine(dst, src, src_in_dst, level), D.sx, D.sy, S.sx, S.sy);
  bbox[0] = b.x0, bbox[1] = b.y0, bbox[2] = b.x1, bbox[3] = b.y1;
  return HSM_OK;
}

}  // extern "C"
