// ingest.hip -- the entries of the C ABI (include/hector_mi355/capi.h) that take RAW sensor data: one LaserScan or point cloud into
// the context's scan container (hsm_ingest_*), batches of raw scans into the batched matcher (hsm_match_batch_ranges*,
// hsm_ingest_batch_ranges_tf_device, hsm_match_batch_ranges_tf) and a raw scan log through the whole SLAM loop (hsm_slam_ranges_tf*).
// The conversion kernels are in ingest_kernels.h; the match behind them is the matcher's front door's (match.hip), the update
// and the loop in map_update.hip; hsm_ctx.h declares what these entries need of either.  hsm_match_ingested and
// hsm_update_by_ingested, a match and an update that read the container, are there too.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "hector_mi355/capi.h"
#include "hsm_ctx.h"
#include "ingest_kernels.h"

using namespace hsm;
using namespace hsm_host;

extern "C" {

// device buffers of the ingestion entries: raw input (3 floats per element covers ranges and Point32
// clouds; the int behind it is the survivor count), the sensor-geometry table (16 B per beam covers the
// float2 and the double2 variant) and the container
static int ensure_ingest_capacity(hsm_ctx* h, int n) {
  if (h->ingest.d_ingest && h->ingest.d_ingest.holds((size_t)n)) return HSM_OK;
  if (int rc = h->ingest.d_ingest.drop()) return rc;  // (first: it stands for the trio)
  h->ingest.trig_n = -1;
  const size_t want = grown_capacity((size_t)n, {2048, 50});
  if (int rc = h->ingest.d_ranges.reserve(3 * want + 1)) return rc;  // (+ the survivor count, an int)
  if (int rc = h->ingest.d_trig.reserve(want)) return rc;
  return h->ingest.d_ingest.reserve(want);
}

static int* ingest_count_ptr(hsm_ctx* h) { return reinterpret_cast<int*>(h->ingest.d_ranges + 3 * h->ingest.d_ingest.count()); }

// fetch the survivor count + the container the kernel on h->stream just produced
static int finish_ingest(hsm_ctx* h, float* out_pts_xy, int* out_n) {
  int m = 0;
  HIP_TRY(hipMemcpyAsync(&m, ingest_count_ptr(h), sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->ingest.h_ingest.resize(2 * (size_t)m);
  if (m > 0) HIP_TRY(hipMemcpy(h->ingest.h_ingest.data(), h->ingest.d_ingest, (size_t)m * sizeof(float2), hipMemcpyDeviceToHost));
  h->ingest.ingest_n = m;
  if (out_pts_xy && m > 0) memcpy(out_pts_xy, h->ingest.h_ingest.data(), (size_t)m * sizeof(float2));
  if (out_n) *out_n = m;
  return HSM_OK;
}

// the node's running fp32 angle and its float cos/sin (HectorMappingRos.cpp:487,502,505): sensor constants, evaluated on the
// host exactly as the node does, as (cos, sin) pairs -- the table of hsm_ingest_laser_scan and hsm_match_batch_ranges_device
static std::vector<float> node_scan_trig(int n, float angle_min, float angle_increment) {
  std::vector<float> t(2 * (size_t)n);
  float angle = angle_min;
  for (int i = 0; i < n; ++i) {
    t[2 * i] = cosf(angle);
    t[2 * i + 1] = sinf(angle);
    angle += angle_increment;
  }
  return t;
}

// laser_geometry's unit vectors (getUnitVectors_): double cos/sin(angle_min + (double)i * angle_increment), cached per sensor
// geometry there as well -- the table of hsm_ingest_laser_scan_tf and hsm_ingest_batch_ranges_tf_device
static std::vector<double> laser_unit_vectors(int n, float angle_min, float angle_increment) {
  std::vector<double> t(2 * (size_t)n);
  const double a0 = angle_min, inc = angle_increment;
  for (int i = 0; i < n; ++i) {
    t[2 * i] = cos(a0 + (double)i * inc);
    t[2 * i + 1] = sin(a0 + (double)i * inc);
  }
  return t;
}

// the single-scan entries' sensor table in d_trig, cached per geometry: `kind` 0 = node_scan_trig's float pairs, 1 =
// laser_unit_vectors' double pairs; evaluated by `make` and uploaded where the last call's kind or geometry was another
extern "C++" template <class Make>
static int ensure_sensor_table(hsm_ctx* h, int kind, int n, float angle_min, float angle_increment, Make make) {
  if (h->ingest.trig_kind == kind && h->ingest.trig_n == n && h->ingest.trig_a0 == angle_min && h->ingest.trig_inc == angle_increment) return HSM_OK;
  const auto t = make(n, angle_min, angle_increment);
  if (n > 0) HIP_TRY(hipMemcpy(h->ingest.d_trig, t.data(), t.size() * sizeof t[0], hipMemcpyHostToDevice));
  h->ingest.trig_kind = kind;
  h->ingest.trig_n = n;
  h->ingest.trig_a0 = angle_min;
  h->ingest.trig_inc = angle_increment;
  return HSM_OK;
}

int hsm_ingest_laser_scan(hsm_ctx* h, const float* ranges, int n, float angle_min, float angle_increment,
                          float range_min, float range_max, float scale_to_map, float* out_pts_xy, int* out_n) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  if (n < 0 || (n > 0 && !ranges) || n > HSM_MAX_UPDATE_BEAMS)
    return fail(HSM_ERR_INVALID, "hsm_ingest_laser_scan: bad argument");
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  if (int rc = ensure_ingest_capacity(h, n)) return rc;
  if (int rc = ensure_sensor_table(h, 0, n, angle_min, angle_increment, node_scan_trig)) return rc;
  if (n > 0) HIP_TRY(hipMemcpyAsync(h->ingest.d_ranges, ranges, (size_t)n * sizeof(float), hipMemcpyHostToDevice, h->stream));
  const float maxRangeForContainer = range_max - 0.1f;  // :493
  hipLaunchKernelGGL(ingest_laser_scan_kernel, dim3(1), dim3(1024), 0, h->stream, h->ingest.d_ranges,
                     reinterpret_cast<const float2*>(h->ingest.d_trig.p), n, range_min, maxRangeForContainer, scale_to_map,
                     h->ingest.d_ingest, ingest_count_ptr(h));
  HIP_TRY(hipGetLastError());
  h->ingest.ingest_origo[0] = h->ingest.ingest_origo[1] = 0.0f;  // dataContainer.setOrigo(Vector2f::Zero()), :491
  return finish_ingest(h, out_pts_xy, out_n);
}

// shared tail of the two point-cloud entries
static int ingest_cloud(hsm_ctx* h, CloudIngestParams& P, const double tf_rows[12], float sqr_min, float sqr_max,
                        float z_min, float z_max, float scale_to_map, float* out_pts_xy, int* out_n,
                        float out_origo[2]) {
  for (int k = 0; k < 12; ++k) P.T[k] = tf_rows[k];
  P.sqr_min = sqr_min;
  P.sqr_max = sqr_max;
  P.z_min = z_min;
  P.z_max = z_max;
  P.scale = scale_to_map;
  P.out = h->ingest.d_ingest;
  P.out_n = ingest_count_ptr(h);
  hipLaunchKernelGGL(ingest_point_cloud_kernel, dim3(1), dim3(1024), 0, h->stream, P);
  HIP_TRY(hipGetLastError());
  // dataContainer.setOrigo(Eigen::Vector2f(laserPos.x(), laserPos.y()) * scaleToMap)  (:517)
  h->ingest.ingest_origo[0] = (float)tf_rows[3] * scale_to_map;
  h->ingest.ingest_origo[1] = (float)tf_rows[7] * scale_to_map;
  if (out_origo) {
    out_origo[0] = h->ingest.ingest_origo[0];
    out_origo[1] = h->ingest.ingest_origo[1];
  }
  return finish_ingest(h, out_pts_xy, out_n);
}

int hsm_ingest_point_cloud(hsm_ctx* h, const float* pts_xyz, int n, const double tf_rows[12], float sqr_laser_min_dist,
                           float sqr_laser_max_dist, float laser_z_min, float laser_z_max, float scale_to_map,
                           float* out_pts_xy, int* out_n, float out_origo[2]) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  if (n < 0 || (n > 0 && !pts_xyz) || !tf_rows || n > HSM_MAX_UPDATE_BEAMS)
    return fail(HSM_ERR_INVALID, "hsm_ingest_point_cloud: bad argument");
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  if (int rc = ensure_ingest_capacity(h, n)) return rc;
  if (n > 0)
    HIP_TRY(hipMemcpyAsync(h->ingest.d_ranges, pts_xyz, 3 * (size_t)n * sizeof(float), hipMemcpyHostToDevice, h->stream));
  CloudIngestParams P{};
  P.pts_xyz = h->ingest.d_ranges;
  P.n = n;
  return ingest_cloud(h, P, tf_rows, sqr_laser_min_dist, sqr_laser_max_dist, laser_z_min, laser_z_max, scale_to_map,
                      out_pts_xy, out_n, out_origo);
}

int hsm_ingest_laser_scan_tf(hsm_ctx* h, const float* ranges, int n, float angle_min, float angle_increment,
                             float range_min, float range_max, double range_cutoff, const double tf_rows[12],
                             float sqr_laser_min_dist, float sqr_laser_max_dist, float laser_z_min, float laser_z_max,
                             float scale_to_map, float* out_pts_xy, int* out_n, float out_origo[2]) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  if (n < 0 || (n > 0 && !ranges) || !tf_rows || n > HSM_MAX_UPDATE_BEAMS)
    return fail(HSM_ERR_INVALID, "hsm_ingest_laser_scan_tf: bad argument");
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  if (int rc = ensure_ingest_capacity(h, n)) return rc;
  if (int rc = ensure_sensor_table(h, 1, n, angle_min, angle_increment, laser_unit_vectors)) return rc;
  if (n > 0) HIP_TRY(hipMemcpyAsync(h->ingest.d_ranges, ranges, (size_t)n * sizeof(float), hipMemcpyHostToDevice, h->stream));
  CloudIngestParams P{};
  P.ranges = h->ingest.d_ranges;
  P.unit = h->ingest.d_trig;
  P.n = n;
  P.range_min = range_min;
  P.range_cutoff = range_cutoff < 0 ? (double)range_max : range_cutoff;
  return ingest_cloud(h, P, tf_rows, sqr_laser_min_dist, sqr_laser_max_dist, laser_z_min, laser_z_max, scale_to_map,
                      out_pts_xy, out_n, out_origo);
}

// ---- B raw scans of one sensor geometry: ingestion kernels + the batched matcher, one stream-ordered sequence ----

size_t hsm_match_batch_ranges_workspace(int batch, int n) {  // (the layout: stage_layout.h)
  RangesLayout L;
  return ranges_layout(batch, n, &L) ? L.total : 0;
}

// true where `p` is device memory (hipMalloc / a torch allocation), which the compaction may read a second time; false for
// pinned host memory (and anything the runtime does not know), which is read once and copied into the workspace
static bool is_device_memory(const void* p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();  // (the failed query's own error: not left for the next launch check)
    return false;
  }
  return a.type == hipMemoryTypeDevice && !a.isManaged;
}

// the immutable per-geometry table of the batched conversions (hsm_ctx::RangesGeometry / RangesTfGeometry), keyed on
// (n, angle_min bits, angle_increment bits): found, or evaluated by `make`, uploaded on `s` and kept until hsm_destroy
extern "C++" template <class Geometry, class Value, class Make>
static int ranges_geometry_table(std::vector<Geometry>& geoms, int n, float angle_min, float angle_increment, hipStream_t s,
                                 const char* who, Make make, const Value** out) {
  unsigned a0_bits, inc_bits;
  memcpy(&a0_bits, &angle_min, sizeof a0_bits);
  memcpy(&inc_bits, &angle_increment, sizeof inc_bits);
  for (const Geometry& g : geoms)
    if (g.n == n && g.a0_bits == a0_bits && g.inc_bits == inc_bits) {
      *out = g.d;
      return HSM_OK;
    }
  // a new table is an allocation and a copy: not while the caller captures the stream into a graph (nothing is enqueued).
  // The copy goes on the caller's stream, not the null stream, and waits for that stream only
  if (stream_capturing(s))
    return fail_at(HSM_ERR_INVALID, who, ": sensor geometry not seen before while the stream is being captured (no "
                                         "allocation under capture: make one call with this geometry before capturing)");
  const auto t = make(n, angle_min, angle_increment);
  Value* d = nullptr;
  HIP_TRY(hipMalloc((void**)&d, (size_t)n * sizeof(Value)));
  hipError_t e = hipMemcpyAsync(d, t.data(), (size_t)n * sizeof(Value), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);  // (`t` is a host temporary)
  if (e != hipSuccess) {
    (void)hipFree(d);
    return fail_at(HSM_ERR_HIP, who, ": sensor table upload", e);
  }
  geoms.push_back({n, a0_bits, inc_bits, d});
  *out = d;
  return HSM_OK;
}

// ranges_on_device: 1 = d_ranges is known to be device memory, -1 = ask the runtime
static int match_batch_ranges_nolock(hsm_ctx* h, int batch, const float* d_begin_world, const float* d_ranges, int n,
                                     float angle_min, float angle_increment, float range_min, float range_max,
                                     float scale_to_map, float* d_out_pose, float* d_out_cov, int* d_out_counts,
                                     void* d_workspace, size_t workspace_bytes, void* stream, int ranges_on_device = -1) {
  if (batch < 0 || n < 0 || !d_begin_world || !d_out_pose || !d_workspace || (batch > 0 && n > 0 && !d_ranges))
    return fail(HSM_ERR_INVALID, "hsm_match_batch_ranges_device: bad argument");
  RangesLayout L;
  if (!ranges_layout(batch, n, &L))
    return fail(HSM_ERR_TOO_LARGE, "hsm_match_batch_ranges_device: n > HSM_MAX_UPDATE_BEAMS or batch * n > INT_MAX");
  if (workspace_bytes < L.total || ((uintptr_t)d_workspace & 7u) != 0)
    return fail(HSM_ERR_INVALID, "hsm_match_batch_ranges_device: workspace smaller than hsm_match_batch_ranges_workspace(batch, n) "
                                 "or not 8-byte aligned");
  if (batch == 0) return HSM_OK;
  if (int rc = select_device(h)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const float2* trig = nullptr;
  if (n > 0)
    if (int rc = ranges_geometry_table(h->ingest.ranges_geoms, n, angle_min, angle_increment, s, "hsm_match_batch_ranges_device",
                                       node_scan_trig, &trig))
      return rc;
  char* ws = (char*)d_workspace;
  int* counts = reinterpret_cast<int*>(ws + L.counts);
  int* offsets = reinterpret_cast<int*>(ws + L.offsets);
  // pinned host ranges cross the link once (the compaction reads the workspace copy); device ranges are read twice instead
  const bool on_device = n > 0 && (ranges_on_device == 1 || (ranges_on_device < 0 && is_device_memory(d_ranges)));
  float* copy = on_device ? nullptr : reinterpret_cast<float*>(ws + L.copy);
  float2* pts = reinterpret_cast<float2*>(ws + L.pts);
  const float maxRangeForContainer = range_max - 0.1f;  // HectorMappingRos.cpp:493, on the host as in hsm_ingest_laser_scan
  const int blocks = (batch - 1) / kRangesScansPerBlock + 1;
  hipLaunchKernelGGL(ranges_gate_count_kernel, dim3(blocks), dim3(256), 0, s, d_ranges, batch, n, range_min,
                     maxRangeForContainer, copy, counts);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(ranges_offsets_kernel, dim3(1), dim3(1024), 0, s, counts, batch, offsets, d_out_counts);
  HIP_TRY(hipGetLastError());
  if (n > 0) {
    // (however the beams are read, scan b writes below offsets[b] + n <= batch * n: inside the endpoint region)
    hipLaunchKernelGGL(ranges_compact_kernel, dim3(blocks), dim3(256), 0, s, copy ? copy : d_ranges, trig, batch, n, range_min,
                       maxRangeForContainer, scale_to_map, offsets, pts);
    HIP_TRY(hipGetLastError());
  }
  // n is a true bound of every scan's length after the gate
  return match_batch_device_nolock(h, {batch, d_begin_world, reinterpret_cast<const float*>(pts), offsets, n},
                                   {d_out_pose, d_out_cov, n}, stream);
}

int hsm_match_batch_ranges_device(hsm_ctx* h, int batch, const float* d_begin_world, const float* d_ranges, int n,
                                  float angle_min, float angle_increment, float range_min, float range_max,
                                  float scale_to_map, float* d_out_pose, float* d_out_cov, int* d_out_counts,
                                  void* d_workspace, size_t workspace_bytes, void* stream) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  std::lock_guard<std::mutex> lk(h->mu);
  return match_batch_ranges_nolock(h, batch, d_begin_world, d_ranges, n, angle_min, angle_increment, range_min, range_max,
                                   scale_to_map, d_out_pose, d_out_cov, d_out_counts, d_workspace, workspace_bytes, stream);
}

int hsm_match_batch_ranges(hsm_ctx* h, int batch, const float* begin_world, const float* ranges, int n, float angle_min,
                           float angle_increment, float range_min, float range_max, float scale_to_map, float* out_pose,
                           float* out_cov, int* out_counts) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  if (batch < 0 || n < 0 || !begin_world || !out_pose || (batch > 0 && n > 0 && !ranges))
    return fail(HSM_ERR_INVALID, "hsm_match_batch_ranges: bad argument");
  RangesLayout L;
  if (!ranges_layout(batch, n, &L))
    return fail(HSM_ERR_TOO_LARGE, "hsm_match_batch_ranges: n > HSM_MAX_UPDATE_BEAMS or batch * n > INT_MAX");
  if (batch == 0) return HSM_OK;
  const RangesStage st = ranges_stage(batch, n, L.total, begin_world, ranges, out_pose, out_cov, out_counts);
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  if (!h->ingest.d_rbatch.holds(st.plan.total())) HIP_TRY(hipStreamSynchronize(h->stream));
  if (int rc = h->ingest.d_rbatch.reserve(st.plan.total())) return rc;
  char* base = h->ingest.d_rbatch;
  if (int rc = stage_copy_in(st.plan, base, h->stream)) return rc;
  if (int rc = match_batch_ranges_nolock(h, batch, staged<float>(base, st.begin), staged<float>(base, st.ranges), n, angle_min,
                                         angle_increment, range_min, range_max, scale_to_map, staged<float>(base, st.pose),
                                         staged<float>(base, st.cov, out_cov), staged<int>(base, st.counts), base + st.ws, L.total,
                                         h->stream, 1))
    return rc;
  if (int rc = stage_copy_out(st.plan, base, h->stream)) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  return HSM_OK;
}

// ---- B raw scans and a transform per scan through the node's tf path: the CSR container of the batched entries ----

// The tf conversion of `P.batch` raw scans is carried as the kernels' own RangesTfParams: the entry fills everything but `unit`
// (the values in the order of the C ABI; the host-array entries put the staged `ranges` and `tf_rows` in once they have them),
// ranges_tf_unit_table completes it.
static RangesTfParams ranges_tf_params(int batch, const float* ranges, int n, float range_min, float range_max, double range_cutoff,
                                       const double* tf_rows, int shared_tf, const CloudGates& gates) {
  RangesTfParams P{};
  P.ranges = ranges;
  P.tf_rows = tf_rows;
  P.batch = batch;
  P.n = n;
  P.shared_tf = shared_tf != 0;
  P.range_min = range_min;
  P.range_cutoff = range_cutoff < 0 ? (double)range_max : range_cutoff;  // projectLaser's cutoff: range_max where none is given
  P.G = gates;
  return P;
}

// the context's part, under its lock: the device and the unit-vector table of the geometry (nullptr for n == 0)
static int ranges_tf_unit_table(hsm_ctx* h, const char* who, RangesTfParams& P, float angle_min, float angle_increment,
                                hipStream_t s) {
  P.unit = nullptr;
  if (int rc = select_device(h)) return rc;
  if (P.n == 0) return HSM_OK;
  return ranges_geometry_table(h->ingest.ranges_tf_geoms, P.n, angle_min, angle_increment, s, who, laser_unit_vectors, &P.unit);
}

// the three launches on `s`; they read nothing of the context.  d_counts_copy: a second copy of the counts, by the offsets pass
static int launch_ingest_batch_ranges_tf(const RangesTfParams& P, float* d_out_pts_xy, int* d_out_offsets, int* d_out_counts,
                                         float* d_out_origo, hipStream_t s, int* d_counts_copy = nullptr) {
  const int blocks = (P.batch - 1) / kRangesScansPerBlock + 1;
  hipLaunchKernelGGL(ranges_tf_gate_count_kernel, dim3(blocks), dim3(256), 0, s, P, d_out_counts,
                     reinterpret_cast<float2*>(d_out_origo));
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(ranges_offsets_kernel, dim3(1), dim3(1024), 0, s, d_out_counts, P.batch, d_out_offsets, d_counts_copy);
  HIP_TRY(hipGetLastError());
  if (P.n > 0) {
    // (scan b writes below offsets[b] + n <= (b + 1) * n <= batch * n: inside the caller's endpoint array)
    hipLaunchKernelGGL(ranges_tf_compact_kernel, dim3(blocks), dim3(256), 0, s, P, d_out_offsets,
                       reinterpret_cast<float2*>(d_out_pts_xy));
    HIP_TRY(hipGetLastError());
  }
  return HSM_OK;
}

// the argument checks the entries share (pointers: the device entry's, or the host entry's before staging)
static int check_batch_ranges_tf(const char* who, const RangesTfParams& P) {
  if (P.batch < 0 || P.n < 0 || (P.batch > 0 && P.n > 0 && !P.ranges) || (P.batch > 0 && !P.tf_rows))
    return fail_at(HSM_ERR_INVALID, who, ": bad argument");
  if (P.n > HSM_MAX_UPDATE_BEAMS || (size_t)P.batch * (size_t)P.n > (size_t)INT_MAX)
    return fail_at(HSM_ERR_TOO_LARGE, who, ": n > HSM_MAX_UPDATE_BEAMS or batch * n > INT_MAX");
  return HSM_OK;
}

int hsm_ingest_batch_ranges_tf_device(hsm_ctx* h, int batch, const float* d_ranges, int n, float angle_min,
                                      float angle_increment, float range_min, float range_max, double range_cutoff,
                                      const double* d_tf_rows, int shared_tf, float sqr_laser_min_dist,
                                      float sqr_laser_max_dist, float laser_z_min, float laser_z_max, float scale_to_map,
                                      float* d_out_pts_xy, int* d_out_offsets, int* d_out_counts, float* d_out_origo,
                                      void* stream) {
  static const char who[] = "hsm_ingest_batch_ranges_tf_device";
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  if (!d_out_pts_xy || !d_out_offsets || !d_out_counts || ((uintptr_t)d_tf_rows & 7u) != 0)
    return fail(HSM_ERR_INVALID, "hsm_ingest_batch_ranges_tf_device: bad argument");
  RangesTfParams P = ranges_tf_params(batch, d_ranges, n, range_min, range_max, range_cutoff, d_tf_rows, shared_tf,
                                      {sqr_laser_min_dist, sqr_laser_max_dist, laser_z_min, laser_z_max, scale_to_map});
  if (int rc = check_batch_ranges_tf(who, P)) return rc;
  if (batch == 0) return HSM_OK;
  const hipStream_t s = (hipStream_t)stream;
  {
    std::lock_guard<std::mutex> lk(h->mu);  // (for the geometry cache only)
    if (int rc = ranges_tf_unit_table(h, who, P, angle_min, angle_increment, s)) return rc;
  }
  return launch_ingest_batch_ranges_tf(P, d_out_pts_xy, d_out_offsets, d_out_counts, d_out_origo, s);
}

int hsm_match_batch_ranges_tf(hsm_ctx* h, int batch, const float* begin_world, const float* ranges, int n, float angle_min,
                              float angle_increment, float range_min, float range_max, double range_cutoff,
                              const double* tf_rows, int shared_tf, float sqr_laser_min_dist, float sqr_laser_max_dist,
                              float laser_z_min, float laser_z_max, float scale_to_map, float* out_pose, float* out_cov,
                              int* out_counts, float* out_origo) {
  static const char who[] = "hsm_match_batch_ranges_tf";
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  if (!begin_world || !out_pose) return fail(HSM_ERR_INVALID, "hsm_match_batch_ranges_tf: bad argument");
  RangesTfParams P = ranges_tf_params(batch, ranges, n, range_min, range_max, range_cutoff, tf_rows, shared_tf,
                                      {sqr_laser_min_dist, sqr_laser_max_dist, laser_z_min, laser_z_max, scale_to_map});
  if (int rc = check_batch_ranges_tf(who, P)) return rc;
  if (batch == 0) return HSM_OK;
  const RangesTfStage st = ranges_tf_stage(batch, n, shared_tf != 0, tf_rows, begin_world, ranges, out_pose, out_cov, out_counts,
                                           out_origo);
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = ranges_tf_unit_table(h, who, P, angle_min, angle_increment, h->stream)) return rc;
  if (!h->ingest.d_rbatch.holds(st.plan.total())) HIP_TRY(hipStreamSynchronize(h->stream));
  if (int rc = h->ingest.d_rbatch.reserve(st.plan.total())) return rc;
  char* base = h->ingest.d_rbatch;
  P.ranges = staged<float>(base, st.ranges);
  P.tf_rows = staged<double>(base, st.tf);
  float* d_pts = staged<float>(base, st.pts);
  int* d_offs = staged<int>(base, st.offs);
  if (int rc = stage_copy_in(st.plan, base, h->stream)) return rc;
  if (int rc = launch_ingest_batch_ranges_tf(P, d_pts, d_offs, staged<int>(base, st.counts), staged<float>(base, st.origo, out_origo),
                                             h->stream))
    return rc;
  // n is a true bound of every scan's length after the gates
  if (int rc = match_batch_device_nolock(h, {batch, staged<float>(base, st.begin), d_pts, d_offs, n},
                                         {staged<float>(base, st.pose), staged<float>(base, st.cov, out_cov), n}, h->stream))
    return rc;
  if (int rc = stage_copy_out(st.plan, base, h->stream)) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  return HSM_OK;
}

// ---- a raw scan log through the tf conversion and the whole SLAM loop, one call ----

size_t hsm_slam_ranges_tf_workspace(int count, int n) {  // (the layout: stage_layout.h)
  SlamRangesTfLayout L;
  return slam_ranges_tf_layout(count, n, &L) ? L.total : 0;
}

// The conversion's three launches and the loop of hsm_slam_scans_device_origos, all on the context's stream and under its lock;
// `s` is waited for once in front and waits once behind.  Every check comes before the first launch; a geometry not seen before is
// uploaded (on the context's stream, which is waited for) before anything is queued.
static int slam_ranges_tf_nolock(hsm_ctx* h, const char* who, const ScanLog& log, RangesTfParams P, float angle_min,
                                 float angle_increment, void* d_workspace, size_t workspace_bytes, hipStream_t s) {
  SlamRangesTfLayout L;
  if (!slam_ranges_tf_layout(P.batch, P.n, &L)) return fail_at(HSM_ERR_TOO_LARGE, who, ": n > HSM_MAX_UPDATE_BEAMS or count * n > INT_MAX");
  if (!d_workspace || workspace_bytes < L.total || ((uintptr_t)d_workspace & 7u) != 0)
    return fail_at(HSM_ERR_INVALID, who, ": workspace smaller than hsm_slam_ranges_tf_workspace(count, n) or not 8-byte aligned");
  if (int rc = select_device(h)) return rc;
  if (int rc = slam_refuse_capture(h, s, who)) return rc;
  if (int rc = ranges_tf_unit_table(h, who, P, angle_min, angle_increment, h->stream)) return rc;
  if (int rc = wait_for_caller_inputs(h, s)) return rc;
  char* ws = (char*)d_workspace;
  // n is a true bound of every scan's length after the gates
  PosedScans scans{P.batch, nullptr, staged<float>(ws, L.pts), staged<int>(ws, L.offsets), 0, P.n};
  scans.d_origos = staged<float>(ws, L.origos);
  scans.who = who;
  if (int rc = launch_ingest_batch_ranges_tf(P, staged<float>(ws, L.pts), staged<int>(ws, L.offsets), staged<int>(ws, L.counts),
                                             staged<float>(ws, L.origos), h->stream, log.d_out_counts))
    return rc;
  if (int rc = slam_scans_queue(h, log, scans)) return rc;
  return slam_caller_waits(h, s);
}

int hsm_slam_ranges_tf_device(hsm_ctx* h, int count, const float* d_start_pose, const float* d_hint_deltas, const float* d_ranges,
                              int n, float angle_min, float angle_increment, float range_min, float range_max, double range_cutoff,
                              const double* d_tf_rows, int shared_tf, float sqr_laser_min_dist, float sqr_laser_max_dist,
                              float laser_z_min, float laser_z_max, float scale_to_map, const unsigned char* d_force,
                              float* d_out_pose, float* d_out_cov, int* d_out_applied, int* d_out_counts, void* d_workspace,
                              size_t workspace_bytes, void* stream) {
  static const char who[] = "hsm_slam_ranges_tf_device";
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  if ((count > 0 && !d_out_pose) || ((uintptr_t)d_tf_rows & 7u) != 0)
    return fail(HSM_ERR_INVALID, "hsm_slam_ranges_tf_device: bad argument");
  RangesTfParams P = ranges_tf_params(count, d_ranges, n, range_min, range_max, range_cutoff, d_tf_rows, shared_tf,
                                      {sqr_laser_min_dist, sqr_laser_max_dist, laser_z_min, laser_z_max, scale_to_map});
  if (int rc = check_batch_ranges_tf(who, P)) return rc;
  if (count == 0) return HSM_OK;
  const ScanLog log{count, d_start_pose, d_hint_deltas, d_force, d_out_pose, d_out_cov, d_out_applied, d_out_counts};
  std::lock_guard<std::mutex> lk(h->mu);
  return slam_ranges_tf_nolock(h, who, log, P, angle_min, angle_increment, d_workspace, workspace_bytes,
                               static_cast<hipStream_t>(stream));
}

int hsm_slam_ranges_tf(hsm_ctx* h, int count, const float* start_pose, const float* hint_deltas, const float* ranges, int n,
                       float angle_min, float angle_increment, float range_min, float range_max, double range_cutoff,
                       const double* tf_rows, int shared_tf, float sqr_laser_min_dist, float sqr_laser_max_dist, float laser_z_min,
                       float laser_z_max, float scale_to_map, const unsigned char* force, float* out_pose, float* out_cov,
                       int* out_applied, int* out_counts, float* out_origo) {
  static const char who[] = "hsm_slam_ranges_tf";
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  if (count > 0 && !out_pose) return fail(HSM_ERR_INVALID, "hsm_slam_ranges_tf: bad argument");
  RangesTfParams P = ranges_tf_params(count, ranges, n, range_min, range_max, range_cutoff, tf_rows, shared_tf,
                                      {sqr_laser_min_dist, sqr_laser_max_dist, laser_z_min, laser_z_max, scale_to_map});
  if (int rc = check_batch_ranges_tf(who, P)) return rc;
  if (count == 0) return HSM_OK;
  SlamRangesTfLayout L;
  slam_ranges_tf_layout(count, n, &L);  // (the sizes passed check_batch_ranges_tf)
  const SlamRangesTfStage st = slam_ranges_tf_stage(count, n, shared_tf != 0, L, tf_rows, start_pose, hint_deltas, force, ranges,
                                                    out_pose, out_cov, out_applied, out_counts, out_origo);
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  if (int rc = slam_refuse_capture(h, h->stream, who)) return rc;  // (before the copies are queued)
  if (!h->ingest.d_rbatch.holds(st.plan.total())) HIP_TRY(hipStreamSynchronize(h->stream));
  if (int rc = h->ingest.d_rbatch.reserve(st.plan.total())) return rc;
  char* base = h->ingest.d_rbatch;
  P.ranges = staged<float>(base, st.ranges);
  P.tf_rows = staged<double>(base, st.tf);
  const ScanLog log{count,
                    staged<float>(base, st.start, start_pose),
                    staged<float>(base, st.deltas, hint_deltas),
                    staged<unsigned char>(base, st.force, force),
                    staged<float>(base, st.pose),
                    staged<float>(base, st.cov, out_cov),
                    staged<int>(base, st.applied, out_applied),
                    staged<int>(base, st.counts, out_counts)};
  if (int rc = stage_copy_in(st.plan, base, h->stream)) return rc;
  if (int rc = slam_ranges_tf_nolock(h, who, log, P, angle_min, angle_increment, base + st.ws, L.total, h->stream)) return rc;
  if (int rc = stage_copy_out(st.plan, base, h->stream)) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  return HSM_OK;
}

}  // extern "C"
