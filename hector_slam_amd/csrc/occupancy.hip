// occupancy.hip -- the entries of the C ABI (include/hector_mi355/capi.h) that export a level as the node's occupancy grid: the
// whole level (hsm_occupancy_grid*) or the cells that changed since the level was last exported (hsm_occupancy_changes*,
// hsm_occupancy_restart).  The kernels are in occupancy_kernels.h; the publish boxes they read are kept by the map updates
// (map_update.hip); what these entries need of them and of the core runtime (hector_mi355.hip) is declared in hsm_ctx.h.
// Behind them the entries that serve the map's other consumers (the image transport, the GeoTIFF writer): the hull of a level's
// known cells (hsm_map_extents*), a cell box as a y-flipped byte image (hsm_map_image*) and windows of that image around batches
// of poses (hsm_map_tiles*); their kernels are in map_image_kernels.h.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <string.h>

#include <mutex>

#include "hector_mi355/capi.h"
#include "hsm_ctx.h"
#include "map_image_kernels.h"
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

// ---- what the map's consumers draw from: known extents, a cell box as an image, windows of it around poses (map_image_kernels.h) --
namespace {

// the two launches of an extents reduction of L on the context's stream; d_box receives the box
int launch_map_extents(hsm_ctx* h, const Level& L, int* d_box) {
  hipLaunchKernelGGL(map_extents_kernel, dim3(grid_for(L.cells() / 4)), dim3(256), 0, h->stream, L.d_logodds, L.sx, (int)L.cells(),
                     h->occ.d_extents);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(map_extents_finish_kernel, dim3(1), dim3(64), 0, h->stream, h->occ.d_extents, L.sx, d_box);
  HIP_TRY(hipGetLastError());
  return HSM_OK;
}

// How map_tiles_kernel spreads `batch` tiles of tile_w x tile_h over wavefronts: the lanes that share a row (the smallest power
// of two that holds the row's 4-byte groups, a whole wavefront at most), the turns a wider row takes, and the wavefronts that share
// a tile -- a power of two that brings the launch to about kTilesWaves wavefronts where the batch alone does not, and no more than
// a tile has turns.  -> the workgroups to launch.  (The bytes do not depend on any of this.)
constexpr long long kTilesWaves = 8192;  // eight workgroups of four wavefronts per CU of a whole MI355X

unsigned map_tiles_shape(MapTilesParams& P) {
  const int slots = P.tile_w / 4 > 1 ? P.tile_w / 4 : 1;
  P.lanes_log2 = 0;
  while (P.lanes_log2 < 6 && (1 << P.lanes_log2) < slots) ++P.lanes_log2;
  P.chunks = (slots + (1 << P.lanes_log2) - 1) >> P.lanes_log2;
  const int rows_per_turn = 64 >> P.lanes_log2;
  const long long turns = (long long)((P.tile_h + rows_per_turn - 1) / rows_per_turn) * P.chunks;
  P.waves_log2 = 0;
  while ((2ll << P.waves_log2) <= turns && ((long long)P.batch << (P.waves_log2 + 1)) <= kTilesWaves) ++P.waves_log2;
  const long long waves = (long long)P.batch << P.waves_log2;
  const long long blocks = (waves + 3) / 4;
  return (unsigned)(blocks < kTilesWaves / 4 ? blocks : kTilesWaves / 4);
}

int launch_map_tiles(hsm_ctx* h, MapTilesParams P) {
  const unsigned blocks = map_tiles_shape(P);
  hipLaunchKernelGGL(map_tiles_kernel, dim3(blocks), dim3(256), 0, h->stream, P);
  HIP_TRY(hipGetLastError());
  return HSM_OK;
}

MapTilesParams map_tiles_params(const Level& L, unsigned char* d_out) {
  MapTilesParams P;
  memset(&P, 0, sizeof P);
  P.logodds = L.d_logodds;
  P.sx = L.sx;
  P.sy = L.sy;
  P.out = d_out;
  return P;
}

// the image of `box` (inclusive, inside the level) of L into d_out: one tile without a pose
int launch_map_image(hsm_ctx* h, const Level& L, const int box[4], unsigned char* d_out) {
  MapTilesParams P = map_tiles_params(L, d_out);
  P.box = make_int4(box[0], box[1], box[2], box[3]);
  P.tile_w = box[2] - box[0] + 1;
  P.tile_h = box[3] - box[1] + 1;
  P.batch = 1;
  return launch_map_tiles(h, P);
}

// the tiles of `batch` poses on L, located by the level's own OccupancyGrid metadata as it stands now
int launch_map_pose_tiles(hsm_ctx* h, const Level& L, int batch, const float* d_poses, int tile_w, int tile_h, unsigned char* d_out,
                          int* d_out_boxes) {
  MapTilesParams P = map_tiles_params(L, d_out);
  const GridMetadata m = level_grid_metadata(L);
  P.poses = d_poses;
  P.origin_x = m.origin_x;
  P.origin_y = m.origin_y;
  P.inv_resolution = 1.0f / m.resolution;  // CoordinateTransformer::setTransforms, HectorMapTools.h:64
  P.tile_w = tile_w;
  P.tile_h = tile_h;
  P.batch = batch;
  P.out_boxes = d_out_boxes;
  return launch_map_tiles(h, P);
}

// `crop` (null: the whole level) clamped to L -> box; false: nothing of it lies on the level
bool clamp_crop(const Level& L, const int* crop, int box[4]) {
  box[0] = crop ? (crop[0] > 0 ? crop[0] : 0) : 0;
  box[1] = crop ? (crop[1] > 0 ? crop[1] : 0) : 0;
  box[2] = crop && crop[2] < L.sx - 1 ? crop[2] : L.sx - 1;
  box[3] = crop && crop[3] < L.sy - 1 ? crop[3] : L.sy - 1;
  return box[2] >= box[0] && box[3] >= box[1];
}

// what the two tile entries refuse before they look at a pointer; *empty: nothing to do
int map_tiles_refusals(const hsm_ctx* h, int level, int batch, const void* poses, int tile_w, int tile_h, const void* out_tiles,
                       const char* who, bool* empty) {
  if (int rc = valid_level(h, level)) return rc;
  const Level& L = h->levels[level];
  if (batch < 0 || tile_w < 1 || tile_h < 1 || tile_w > L.sx || tile_h > L.sy)
    return fail_at(HSM_ERR_INVALID, who, ": a negative batch, or a tile that is empty or larger than the level");
  if ((long long)batch * tile_w * tile_h > INT_MAX) return fail_at(HSM_ERR_INVALID, who, ": more than INT_MAX bytes of tiles");
  *empty = batch == 0;
  if (!*empty && (!poses || !out_tiles)) return fail_at(HSM_ERR_INVALID, who, ": null poses or tiles");
  return HSM_OK;
}

// The bracket of the three device entries, hsm_occupancy_grid_device's: refused under capture, the context's stream behind the
// caller's, `queue` on the context's stream, the caller's stream behind that
template <class F>
int on_context_stream(hsm_ctx* h, void* stream, const char* who, F&& queue) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = slam_refuse_capture(h, s, who)) return rc;
  if (int rc = select_device(h)) return rc;
  if (int rc = wait_for_caller_inputs(h, s)) return rc;
  if (int rc = queue()) return rc;
  return slam_caller_waits(h, s);
}

}  // namespace

extern "C" {

int hsm_map_extents_device(hsm_ctx* h, int level, int* d_out_box, void* stream) {
  if (int rc = valid_level(h, level)) return rc;
  if (!d_out_box) return fail(HSM_ERR_INVALID, "hsm_map_extents_device: the box is null");
  std::lock_guard<std::mutex> lk(h->mu);
  return on_context_stream(h, stream, "hsm_map_extents_device", [&] { return launch_map_extents(h, h->levels[level], d_out_box); });
}

int hsm_map_extents(hsm_ctx* h, int level, int box[4]) {
  if (int rc = valid_level(h, level)) return rc;
  if (!box) return fail(HSM_ERR_INVALID, "hsm_map_extents: the box is null");
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  int* d_box = h->occ.d_extents + 4;
  if (int rc = launch_map_extents(h, h->levels[level], d_box)) return rc;
  HIP_TRY(hipMemcpyAsync(box, d_box, 4 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return HSM_OK;
}

int hsm_map_image_device(hsm_ctx* h, int level, const int crop[4], unsigned char* d_out, void* stream) {
  if (int rc = valid_level(h, level)) return rc;
  int box[4];
  if (!clamp_crop(h->levels[level], crop, box)) return HSM_OK;  // the crop misses the level: nothing to write
  if (!d_out) return fail(HSM_ERR_INVALID, "hsm_map_image_device: the image is null");
  std::lock_guard<std::mutex> lk(h->mu);
  return on_context_stream(h, stream, "hsm_map_image_device", [&] { return launch_map_image(h, h->levels[level], box, d_out); });
}

int hsm_map_image(hsm_ctx* h, int level, const int crop[4], unsigned char* out) {
  if (int rc = valid_level(h, level)) return rc;
  int box[4];
  if (!clamp_crop(h->levels[level], crop, box)) return HSM_OK;
  if (!out) return fail(HSM_ERR_INVALID, "hsm_map_image: the image is null");
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  const size_t bytes = (size_t)(box[2] - box[0] + 1) * (size_t)(box[3] - box[1] + 1);
  if (int rc = h->occ.d_occ.reserve(bytes)) return rc;
  unsigned char* d_img = reinterpret_cast<unsigned char*>(static_cast<signed char*>(h->occ.d_occ));
  if (int rc = launch_map_image(h, h->levels[level], box, d_img)) return rc;
  HIP_TRY(hipMemcpyAsync(out, d_img, bytes, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return HSM_OK;
}

int hsm_map_tiles_device(hsm_ctx* h, int level, int batch, const float* d_poses_world, int tile_w, int tile_h,
                         unsigned char* d_out_tiles, int* d_out_boxes, void* stream) {
  bool empty = false;
  if (int rc = map_tiles_refusals(h, level, batch, d_poses_world, tile_w, tile_h, d_out_tiles, "hsm_map_tiles_device", &empty)) return rc;
  if (empty) return HSM_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  return on_context_stream(h, stream, "hsm_map_tiles_device", [&] {
    return launch_map_pose_tiles(h, h->levels[level], batch, d_poses_world, tile_w, tile_h, d_out_tiles, d_out_boxes);
  });
}

int hsm_map_tiles(hsm_ctx* h, int level, int batch, const float* poses_world, int tile_w, int tile_h, unsigned char* out_tiles,
                  int* out_boxes) {
  bool empty = false;
  if (int rc = map_tiles_refusals(h, level, batch, poses_world, tile_w, tile_h, out_tiles, "hsm_map_tiles", &empty)) return rc;
  if (empty) return HSM_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  const MapTilesStage st = map_tiles_stage(batch, (size_t)tile_w * tile_h, poses_world, out_tiles, out_boxes);
  if (int rc = h->d_batch.reserve(st.plan.total())) return rc;
  char* base = h->d_batch;
  if (int rc = stage_copy_in(st.plan, base, h->stream)) return rc;
  if (int rc = launch_map_pose_tiles(h, h->levels[level], batch, staged<float>(base, st.poses), tile_w, tile_h,
                                     staged<unsigned char>(base, st.tiles), staged<int>(base, st.boxes, out_boxes)))
    return rc;
  if (int rc = stage_copy_out(st.plan, base, h->stream)) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  return HSM_OK;
}

}  // extern "C"
