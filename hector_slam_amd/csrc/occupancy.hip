// occupancy.hip -- the entries of the C ABI (include/hector_mi355/capi.h) that export a level as the node's occupancy grid: the
// whole level (hsm_occupancy_grid*) or the cells that changed since the level was last exported (hsm_occupancy_changes*,
// hsm_occupancy_restart).  The kernels are in occupancy_kernels.h; the publish boxes they read are kept by the map updates
// (map_update.hip); what these entries need of them and of the core runtime (hector_mi355.hip) is declared in hsm_ctx.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <mutex>

#include "hector_mi355/capi.h"
#include "hsm_ctx.h"
#include "occupancy_kernels.h"

using namespace hsm;
using namespace hsm_host;

extern "C" {

int hsm_occupancy_grid(hsm_ctx* h, int level, signed char* out) {
  if (int rc = valid_level(h, level)) return rc;
  if (!out) return fail(HSM_ERR_INVALID, "hsm_occupancy_grid: out is null");
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  Level& L = h->levels[level];
  if (int rc = h->occ.d_occ.reserve(L.cells())) return rc;
  hipLaunchKernelGGL(occupancy_grid_kernel, dim3(grid_for(L.cells() / 4)), dim3(256), 0, h->stream, L.d_logodds,
                     L.cells(), h->occ.d_occ);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, h->occ.d_occ, L.cells(), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return HSM_OK;
}

// ---- the published grid on the device, and its changed cells only (occupancy_kernels.h) ---------------------------
constexpr unsigned kOccupancyBoxBlocks = 512;  // two workgroups per CU of a whole MI355X: the launch shape cannot depend on the box

static int occupancy_export_refusals(hsm_ctx* h, const void* grid, hipStream_t s, const char* who) {
  if (!grid) return fail_at(HSM_ERR_INVALID, who, ": the grid is null");
  return slam_refuse_capture(h, s, who);
}

// occupancy_box_kernel over the box at `d_box` of level L, into a device grid of any alignment
static int launch_occupancy_box(hsm_ctx* h, const Level& L, const int* d_box, signed char* d_grid) {
  hipLaunchKernelGGL(occupancy_box_kernel, dim3(kOccupancyBoxBlocks), dim3(256), 0, h->stream, L.d_logodds, L.sx, d_box, d_grid,
                     ((uintptr_t)d_grid & 3u) == 0 ? 1 : 0);
  HIP_TRY(hipGetLastError());
  return HSM_OK;
}

// The two launches of an export of `level`'s changed cells into d_grid; afterwards the level's publish box is empty on both
// sides.  -> *d_box: where the exported box stands once the prep launch has run (until the level's next export).
static int queue_occupancy_changes(hsm_ctx* h, int level, signed char* d_grid, int* d_out_bbox, const int** d_box) {
  Level& L = h->levels[level];
  OccupancyPrepParams A;
  memset(&A, 0, sizeof A);
  A.nlev = (int)h->levels.size();
  A.pub_boxes = h->occ.d_pub_boxes;
  A.host_box[level] = make_int4(L.pub[0], L.pub[1], L.pub[2], L.pub[3]);
  A.dims[level] = make_int2(L.sx, L.sy);
  A.box_out[level] = h->occ.d_pub_boxes + (kMaxLevels + level) * 4;
  A.bbox_out[level] = d_out_bbox;
  hipLaunchKernelGGL(occupancy_prep_kernel, dim3(1), dim3(64), 0, h->stream, A);
  HIP_TRY(hipGetLastError());
  L.pub[0] = L.pub[1] = 0;
  L.pub[2] = L.pub[3] = -1;
  *d_box = A.box_out[level];
  return launch_occupancy_box(h, L, *d_box, d_grid);
}

int hsm_occupancy_grid_device(hsm_ctx* h, int level, signed char* d_out, void* stream) {
  if (int rc = valid_level(h, level)) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = occupancy_export_refusals(h, d_out, s, "hsm_occupancy_grid_device")) return rc;
  if (int rc = select_device(h)) return rc;
  if (int rc = wait_for_caller_inputs(h, s)) return rc;
  if (int rc = launch_occupancy_box(h, h->levels[level], h->occ.d_pub_boxes + (2 * kMaxLevels + level) * 4, d_out)) return rc;
  return slam_caller_waits(h, s);
}

int hsm_occupancy_changes_device(hsm_ctx* h, int level, signed char* d_grid, int* d_out_bbox, void* stream) {
  if (int rc = valid_level(h, level)) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = occupancy_export_refusals(h, d_grid, s, "hsm_occupancy_changes_device")) return rc;
  if (int rc = select_device(h)) return rc;
  if (int rc = wait_for_caller_inputs(h, s)) return rc;
  const int* d_box = nullptr;
  if (int rc = queue_occupancy_changes(h, level, d_grid, d_out_bbox, &d_box)) return rc;
  return slam_caller_waits(h, s);
}

int hsm_occupancy_changes(hsm_ctx* h, int level, signed char* grid, int bbox[4]) {
  if (int rc = valid_level(h, level)) return rc;
  if (!grid || !bbox) return fail(HSM_ERR_INVALID, "hsm_occupancy_changes: null argument");
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  Level& L = h->levels[level];
  if (int rc = h->occ.d_occ.reserve(L.cells())) return rc;
  const int* d_box = nullptr;
  if (int rc = queue_occupancy_changes(h, level, h->occ.d_occ, nullptr, &d_box)) return rc;
  HIP_TRY(hipMemcpyAsync(bbox, d_box, 4 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (bbox[2] < bbox[0]) return HSM_OK;  // nothing changed: `grid` stays as it is
  const size_t first = (size_t)bbox[1] * L.sx + bbox[0];
  HIP_TRY(hipMemcpy2DAsync(grid + first, (size_t)L.sx, h->occ.d_occ + first, (size_t)L.sx, (size_t)(bbox[2] - bbox[0] + 1),
                           (size_t)(bbox[3] - bbox[1] + 1), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return HSM_OK;
}

int hsm_occupancy_restart(hsm_ctx* h, int level) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  if (level != -1)
    if (int rc = valid_level(h, level)) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  for (int l = 0; l < (int)h->levels.size(); ++l)
    if (level == -1 || l == level) whole_level_changed(h->levels[l], false);
  return HSM_OK;
}

}  // extern "C"
