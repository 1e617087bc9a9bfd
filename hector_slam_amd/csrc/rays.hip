// rays.hip -- the entries of the C ABI (include/hector_mi355/capi.h) that ask a level "what would a laser see from here?":
// DistanceMeasurementProvider::getDist for arrays of rays (hsm_ray_distances, hsm_ray_distances_device) and for whole scan fans
// cast from batches of sensor poses (hsm_cast_scans_device, hsm_cast_scans).  The kernels are in ray_kernels.h.  The device
// entries read the map like a batched score and are ordered like one (the MapReader bracket of hsm_ctx.h, around
// order_map_reader of the core runtime, hector_mi355.hip, which declares what these entries need of it in hsm_ctx.h).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>

#include <mutex>

#include "hector_mi355/capi.h"
#include "hsm_ctx.h"
#include "ray_kernels.h"

using namespace hsm;
using namespace hsm_host;

namespace {

RayGrid ray_grid(const Level& L, float origin_x, float origin_y, float resolution) {
  RayGrid G;
  G.logodds = L.d_logodds;
  G.sx = L.sx;
  G.sy = L.sy;
  G.origin_x = origin_x;
  G.origin_y = origin_y;
  G.scale = resolution;
  G.inv_scale = 1.0f / resolution;  // CoordinateTransformer::setTransforms, HectorMapTools.h:64
  return G;
}

// ... on the level's own OccupancyGrid metadata (hsm_ctx.h level_grid_metadata)
RayGrid level_ray_grid(const Level& L) {
  const GridMetadata m = level_grid_metadata(L);
  return ray_grid(L, m.origin_x, m.origin_y, m.resolution);
}

// Which walk a cast takes (ray_kernels.h): a lane per beam from 32 beams, a wavefront per beam for the shorter fans, which leave
// most of a lane-per-beam wavefront idle while it still costs its longest ray.  Either gives the same bits.  Measured
// (profiles/r18/, 4096 poses, level 0 of the 2048^2 pyramid, lane against wave): 1081 beams 1.07 against 1.87 ms, 129 beams (a
// third, nearly empty wavefront per pose) 120 against 202 us, 65 beams 76 against 106 us, 48 beams 62 against 82 us, 32 beams 54
// against 57 us, 16 beams 56 against 34 us, one beam 48 against 8 us.
constexpr int kCastLaneMinBeams = 32;

bool cast_lane_per_beam(const hsm_ctx* h, int n) {
  if (h->cfg.forms.cast_form >= 0) return h->cfg.forms.cast_form == 1;
  return n >= kCastLaneMinBeams;
}

int cast_scans_launch(hsm_ctx* h, int level, int batch, const float* d_poses, const float* d_angles, int n, float range_max,
                      float* d_out_ranges, float* d_out_hit, hipStream_t s) {
  CastScansParams P;
  P.grid = level_ray_grid(h->levels[level]);
  P.poses = d_poses;
  P.angles = d_angles;
  P.batch = batch;
  P.n = n;
  P.range_max = range_max;
  P.out_ranges = d_out_ranges;
  P.out_hit = reinterpret_cast<float2*>(d_out_hit);
  if (cast_lane_per_beam(h, n)) {
    const long long waves = (long long)batch * ((n + 63) / 64);
    hipLaunchKernelGGL(cast_scans_lane_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, P);
    h->last.last_kernel = "cast_scans_lane_kernel";
  } else {
    const long long waves = (long long)batch * n;
    hipLaunchKernelGGL(cast_scans_wave_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, P);
    h->last.last_kernel = "cast_scans_wave_kernel";
  }
  HIP_TRY(hipGetLastError());
  return HSM_OK;
}

// the refusals the two cast entries share; *empty: nothing to do
int cast_scans_refusals(const hsm_ctx* h, int level, int batch, const void* poses, const void* angles, int n, float range_max,
                        const void* out_ranges, const char* who, bool* empty) {
  if (int rc = valid_level(h, level)) return rc;
  if (batch < 0 || n < 0 || !(range_max >= 0.0f && range_max <= 3.402823466e38f) || (long long)batch * n > INT_MAX)
    return fail_at(HSM_ERR_INVALID, who, ": bad argument");
  *empty = batch == 0 || n == 0;
  if (!*empty && (!poses || !angles || !out_ranges)) return fail_at(HSM_ERR_INVALID, who, ": null poses, angles or ranges");
  return HSM_OK;
}

}  // namespace

extern "C" {

int hsm_ray_distances(hsm_ctx* h, int level, float origin_x, float origin_y, float resolution, int n,
                      const float* begin_world_xy, const float* end_world_xy, float* out_dist, float* out_hit_xy) {
  if (int rc = valid_level(h, level)) return rc;
  if (n < 0 || (n > 0 && (!begin_world_xy || !end_world_xy || !out_dist)) || !(resolution > 0.0f))
    return fail(HSM_ERR_INVALID, "hsm_ray_distances: bad argument");
  if (n == 0) return HSM_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  const RayDistancesStage st = ray_distances_stage(n, begin_world_xy, end_world_xy, out_dist, out_hit_xy);
  if (int rc = h->d_batch.reserve(st.plan.total())) return rc;
  char* base = h->d_batch;
  RayQueryParams P;
  P.grid = ray_grid(h->levels[level], origin_x, origin_y, resolution);
  P.begin_world = staged<float2>(base, st.begin);
  P.end_world = staged<float2>(base, st.end);
  P.out_hit = staged<float2>(base, st.hit);  // in/out: rays without a hit keep the caller's values
  P.out_dist = staged<float>(base, st.dist);
  P.n = n;
  if (int rc = stage_copy_in(st.plan, base, h->stream)) return rc;
  hipLaunchKernelGGL(ray_distance_kernel<false>, dim3((n + 3) / 4), dim3(256), 0, h->stream, P);
  HIP_TRY(hipGetLastError());
  if (int rc = stage_copy_out(st.plan, base, h->stream)) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  return HSM_OK;
}

int hsm_ray_distances_device(hsm_ctx* h, int level, float origin_x, float origin_y, float resolution, int n,
                             const float* d_begin_world_xy, const float* d_end_world_xy, float* d_out_dist, float* d_out_hit_xy,
                             void* stream) {
  if (int rc = valid_level(h, level)) return rc;
  if (n < 0 || (n > 0 && (!d_begin_world_xy || !d_end_world_xy || !d_out_dist)) || !(resolution > 0.0f))
    return fail(HSM_ERR_INVALID, "hsm_ray_distances_device: bad argument");
  if (n == 0) return HSM_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  MapReader reader;
  if (int rc = reader.begin(h, s, "hsm_ray_distances_device")) return rc;
  RayQueryParams P;
  P.grid = ray_grid(h->levels[level], origin_x, origin_y, resolution);
  P.begin_world = reinterpret_cast<const float2*>(d_begin_world_xy);
  P.end_world = reinterpret_cast<const float2*>(d_end_world_xy);
  P.out_hit = reinterpret_cast<float2*>(d_out_hit_xy);
  P.out_dist = d_out_dist;
  P.n = n;
  hipLaunchKernelGGL(ray_distance_kernel<true>, dim3((n + 3) / 4), dim3(256), 0, s, P);
  HIP_TRY(hipGetLastError());
  reader.queued();
  h->last.last_kernel = "ray_distance_kernel";
  return HSM_OK;
}

int hsm_cast_scans_device(hsm_ctx* h, int level, int batch, const float* d_poses_world, const float* d_beam_angles, int n,
                          float range_max, float* d_out_ranges, float* d_out_hit_xy, void* stream) {
  bool empty = false;
  if (int rc = cast_scans_refusals(h, level, batch, d_poses_world, d_beam_angles, n, range_max, d_out_ranges,
                                   "hsm_cast_scans_device", &empty))
    return rc;
  if (empty) return HSM_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  MapReader reader;
  if (int rc = reader.begin(h, s, "hsm_cast_scans_device")) return rc;
  if (int rc = cast_scans_launch(h, level, batch, d_poses_world, d_beam_angles, n, range_max, d_out_ranges, d_out_hit_xy, s))
    return rc;
  reader.queued();
  return HSM_OK;
}

int hsm_cast_scans(hsm_ctx* h, int level, int batch, const float* poses_world, const float* beam_angles, int n, float range_max,
                   float* out_ranges, float* out_hit_xy) {
  bool empty = false;
  if (int rc = cast_scans_refusals(h, level, batch, poses_world, beam_angles, n, range_max, out_ranges, "hsm_cast_scans", &empty))
    return rc;
  if (empty) return HSM_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  const CastScansStage st = cast_scans_stage(batch, n, poses_world, beam_angles, out_ranges, out_hit_xy);
  if (int rc = h->d_batch.reserve(st.plan.total())) return rc;
  char* base = h->d_batch;
  if (int rc = stage_copy_in(st.plan, base, h->stream)) return rc;
  if (int rc = cast_scans_launch(h, level, batch, staged<float>(base, st.poses), staged<float>(base, st.angles), n, range_max,
                                 staged<float>(base, st.ranges), staged<float>(base, st.hit, out_hit_xy), h->stream))
    return rc;
  if (int rc = stage_copy_out(st.plan, base, h->stream)) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  return HSM_OK;
}

}  // extern "C"
