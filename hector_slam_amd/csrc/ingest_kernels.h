// ingest_kernels.h -- raw sensor data to the matcher's scan containers (ingest.hip): one LaserScan or point cloud through the
// node's conversions, and batches of raw scans of one sensor geometry into the CSR container of the batched entries.  These
// kernels read no map cell.  They are not templates, so exactly one translation unit includes this header.
#pragma once
#include <hip/hip_runtime.h>

namespace hsm {

// rosLaserScanToDataContainer (HectorMappingRos.cpp:483-507).  trig[i] = (cosf(angle_i), sinf(angle_i))
// comes from the host (the running fp32 angle and the libm calls are the node's); this kernel applies
// the range gate, the scale and the products, and compacts the survivors IN ORDER: one workgroup,
// chunks of 1024 beams, wave ballot + LDS for the ordered offsets.
__global__ void __launch_bounds__(1024) ingest_laser_scan_kernel(const float* __restrict__ ranges,
                                                                const float2* __restrict__ trig, int n,
                                                                float range_min, float max_range_for_container,
                                                                float scale_to_map, float2* __restrict__ out,
                                                                int* __restrict__ out_n) {
  __shared__ int wave_count[16];
  __shared__ int base;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) base = 0;
  __syncthreads();
  for (int i0 = 0; i0 < n; i0 += 1024) {
    const int i = i0 + threadIdx.x;
    float dist = i < n ? ranges[i] : 0.0f;
    const bool keep = (i < n) && (dist > range_min) && (dist < max_range_for_container);
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wave_count[wave] = __popcll(m);
    __syncthreads();
    int off = base;
    for (int w = 0; w < wave; ++w) off += wave_count[w];
    if (keep) {
      dist *= scale_to_map;
      const float2 cs = trig[i];
      out[off + __popcll(m & ((1ull << lane) - 1ull))] = make_float2(cs.x * dist, cs.y * dist);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int t = 0;
      for (int w = 0; w < 16; ++w) t += wave_count[w];
      base += t;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) *out_n = base;
}

// The same conversion for B scans of one sensor geometry (hsm_match_batch_ranges_device): ranges[b * n + i] -> the CSR input
// of the batched matcher, in three launches on the caller's stream.
//   gate/count  one wavefront per scan: the range gate above, counts[b] = sum of the ballots' popcounts.  Ranges in host
//               memory (pinned, device-accessible) are copied into the workspace on the way, so they cross the link once and the
//               compaction reads the copy; ranges in device memory are read again by the compaction (copy == nullptr)
//   offsets     one workgroup: exclusive scan of counts into offsets[B + 1], 1024 scans per pass, any B
//   compact     one wavefront per scan: the kept beams in beam order at offsets[b] + rank, with the arithmetic of
//               ingest_laser_scan_kernel operation for operation (scale first, then the two products)
constexpr int kRangesScansPerBlock = 4;  // 256 threads

__global__ void __launch_bounds__(256) ranges_gate_count_kernel(const float* __restrict__ ranges, int batch, int n,
                                                                 float range_min, float max_range_for_container,
                                                                 float* __restrict__ copy, int* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const long long b = (long long)blockIdx.x * kRangesScansPerBlock + (threadIdx.x >> 6);  // (no int overflow for batch near INT_MAX)
  if (b >= batch) return;  // (uniform per wavefront)
  const size_t row = (size_t)b * n;
  int c = 0;
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    const float dist = i < n ? ranges[row + i] : 0.0f;
    if (copy != nullptr && i < n) copy[row + i] = dist;
    c += __popcll(__ballot((i < n) && (dist > range_min) && (dist < max_range_for_container)));
  }
  if (lane == 0) counts[b] = c;
}

__global__ void __launch_bounds__(1024) ranges_offsets_kernel(const int* __restrict__ counts, int batch,
                                                              int* __restrict__ offsets, int* __restrict__ out_counts) {
  __shared__ int wave_sum[16];
  __shared__ int carry;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (long long b0 = 0; b0 < batch; b0 += 1024) {
    const long long b = b0 + threadIdx.x;
    const int c = b < batch ? counts[b] : 0;
    if (out_counts != nullptr && b < batch) out_counts[b] = c;
    int x = c;  // inclusive scan inside the wavefront
    for (int d = 1; d < 64; d <<= 1) {
      const int y = __shfl_up(x, d);
      if (lane >= d) x += y;
    }
    if (lane == 63) wave_sum[wave] = x;
    __syncthreads();
    int base = carry;
    for (int w = 0; w < wave; ++w) base += wave_sum[w];
    if (b < batch) offsets[b] = base + x - c;
    __syncthreads();                              // every thread has read `carry`
    if (threadIdx.x == 1023) carry = base + x;    // the last thread's inclusive sum: everything up to this pass's end
    __syncthreads();
  }
  if (threadIdx.x == 0) offsets[batch] = carry;
}

__global__ void __launch_bounds__(256) ranges_compact_kernel(const float* __restrict__ ranges, const float2* __restrict__ trig,
                                                              int batch, int n, float range_min, float max_range_for_container,
                                                              float scale_to_map, const int* __restrict__ offsets,
                                                              float2* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long b = (long long)blockIdx.x * kRangesScansPerBlock + (threadIdx.x >> 6);
  if (b >= batch) return;
  const float* __restrict__ r = ranges + (size_t)b * n;
  const unsigned long long below = (1ull << lane) - 1ull;
  int pos = offsets[b];
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    float dist = i < n ? r[i] : 0.0f;
    const bool keep = (i < n) && (dist > range_min) && (dist < max_range_for_container);
    const unsigned long long m = __ballot(keep);
    if (keep) {
      dist *= scale_to_map;
      const float2 cs = trig[i];
      out[pos + __popcll(m & below)] = make_float2(cs.x * dist, cs.y * dist);
    }
    pos += __popcll(m);
  }
}

// rosPointCloudToDataContainer (HectorMappingRos.cpp:509-542), optionally preceded by
// laser_geometry's projectLaser (the node's default path, :273-282; third party, algorithm stated in
// include/hector_mi355/capi.h): one pass, ordered compaction like the kernel above.  tf arithmetic is fp64
// (tfScalar), the gates and the products fp32, exactly the node's types.
struct CloudIngestParams {
  const float* pts_xyz;  // [n,3] geometry_msgs::Point32, or nullptr when projecting from ranges
  const float* ranges;   // projectLaser input, or nullptr
  const double2* unit;   // (cos, sin)(angle_min + (double)i * angle_increment): sensor constants from the host
  int n;
  float range_min;       // projectLaser gate: range < range_cutoff (double compare) && range >= range_min
  double range_cutoff;
  double T[12];          // laser -> base transform, rows [R | t]
  float sqr_min, sqr_max, z_min, z_max, scale;
  float2* out;
  int* out_n;
};

// One beam of the tf path, the only statement of its arithmetic: the single-scan kernel and both passes of the batched
// conversion call these two, so a count and a compaction cannot disagree and the entries cannot drift apart.  The fp64
// products and sums stay separate operations (the build sets -ffp-contract=off: no FMA), in the node's order.
// projectLaser: point = float((double)range * unit), kept when range < range_cutoff (double compare) && range >= range_min
__device__ __forceinline__ bool project_laser_beam(float range, double2 unit, float range_min, double range_cutoff,
                                                   float* px, float* py) {
  const double r = (double)range;
  *px = (float)(r * unit.x);
  *py = (float)(r * unit.y);
  return ((double)range < range_cutoff) && (range >= range_min);
}

struct CloudGates {
  float sqr_min, sqr_max, z_min, z_max, scale;
};

// rosPointCloudToDataContainer's loop body (:519-540): true = the point is kept, *e = its endpoint.  T: rows [R | t]
__device__ __forceinline__ bool cloud_point_endpoint(float px, float py, float pz, const double* __restrict__ T,
                                                     const CloudGates& G, float2* e) {
  const float dist_sqr = px * px + py * py;
  if (!((dist_sqr > G.sqr_min) && (dist_sqr < G.sqr_max)) || ((px < 0.0f) && (dist_sqr < 0.50f))) return false;
  const double vx = px, vy = py, vz = pz;
  const double bx = (T[0] * vx + T[1] * vy + T[2] * vz) + T[3];
  const double by = (T[4] * vx + T[5] * vy + T[6] * vz) + T[7];
  const double bz = (T[8] * vx + T[9] * vy + T[10] * vz) + T[11];
  const float zl = (float)(bz - T[11]);
  if (!(zl > G.z_min && zl < G.z_max)) return false;
  *e = make_float2((float)bx * G.scale, (float)by * G.scale);
  return true;
}

__global__ void __launch_bounds__(1024) ingest_point_cloud_kernel(CloudIngestParams P) {
  __shared__ int wave_count[16];
  __shared__ int base;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const CloudGates G{P.sqr_min, P.sqr_max, P.z_min, P.z_max, P.scale};
  if (threadIdx.x == 0) base = 0;
  __syncthreads();
  for (int i0 = 0; i0 < P.n; i0 += 1024) {
    const int i = i0 + threadIdx.x;
    bool keep = false;
    float2 e = make_float2(0.0f, 0.0f);
    if (i < P.n) {
      float px, py, pz;
      bool valid = true;
      if (P.ranges) {
        valid = project_laser_beam(P.ranges[i], P.unit[i], P.range_min, P.range_cutoff, &px, &py);
        pz = 0.0f;
      } else {
        px = P.pts_xyz[3 * (size_t)i];
        py = P.pts_xyz[3 * (size_t)i + 1];
        pz = P.pts_xyz[3 * (size_t)i + 2];
      }
      keep = valid && cloud_point_endpoint(px, py, pz, P.T, G, &e);
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wave_count[wave] = __popcll(m);
    __syncthreads();
    int off = base;
    for (int w = 0; w < wave; ++w) off += wave_count[w];
    if (keep) P.out[off + __popcll(m & ((1ull << lane) - 1ull))] = e;
    __syncthreads();
    if (threadIdx.x == 0) {
      int t = 0;
      for (int w = 0; w < 16; ++w) t += wave_count[w];
      base += t;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) *P.out_n = base;
}

// The tf path for B scans of one sensor geometry (hsm_ingest_batch_ranges_tf_device): ranges[b * n + i] and a transform per
// scan -> the CSR container of the batched entries, in the three-launch shape of the ranges_* kernels above.
//   gate/count  one wavefront per scan: counts[b] = kept beams; lane 0 also writes the scan's origo (:517)
//   offsets     ranges_offsets_kernel
//   compact     one wavefront per scan: the kept beams in beam order at offsets[b] + rank
// Both passes evaluate ranges_tf_beam, i.e. the two functions above; the second pass recomputes ~20 fp64 operations per beam
// instead of reading back a staged 8 B per beam.  The twelve transform values of a scan are wave-uniform: the scan index is
// made scalar, so they are fetched once per wavefront through the scalar cache and stay in SGPRs.
struct RangesTfParams {
  const float* ranges;    // [batch * n]
  const double2* unit;    // [n] (cos, sin)(angle_min + (double)i * angle_increment)
  const double* tf_rows;  // [batch][12], or [12] with shared_tf
  int batch, n, shared_tf;
  float range_min;
  double range_cutoff;
  CloudGates G;
};

__device__ __forceinline__ long long ranges_tf_scan_index() {  // wave-uniform, no int overflow for batch near INT_MAX
  return (long long)blockIdx.x * kRangesScansPerBlock + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
}

__device__ __forceinline__ void ranges_tf_load_rows(const RangesTfParams& P, long long b, double (&T)[12]) {
  const double* __restrict__ t = P.tf_rows + (P.shared_tf ? (size_t)0 : (size_t)b * 12);
#pragma unroll
  for (int k = 0; k < 12; ++k) T[k] = t[k];
}

__device__ __forceinline__ bool ranges_tf_beam(const RangesTfParams& P, const float* __restrict__ r, int i,
                                               const double (&T)[12], float2* e) {
  if (i >= P.n) return false;
  float px, py;
  const bool valid = project_laser_beam(r[i], P.unit[i], P.range_min, P.range_cutoff, &px, &py);
  return valid && cloud_point_endpoint(px, py, 0.0f, T, P.G, e);
}

__global__ void __launch_bounds__(256) ranges_tf_gate_count_kernel(const RangesTfParams P, int* __restrict__ counts,
                                                                    float2* __restrict__ out_origo) {
  const int lane = threadIdx.x & 63;
  const long long b = ranges_tf_scan_index();
  if (b >= P.batch) return;  // (uniform per wavefront)
  double T[12];
  ranges_tf_load_rows(P, b, T);
  const float* __restrict__ r = P.ranges + (size_t)b * P.n;
  int c = 0;
  for (int i0 = 0; i0 < P.n; i0 += 64) {
    float2 e;
    c += __popcll(__ballot(ranges_tf_beam(P, r, i0 + lane, T, &e)));
  }
  if (lane == 0) {
    counts[b] = c;
    // dataContainer.setOrigo(Eigen::Vector2f(laserPos.x(), laserPos.y()) * scaleToMap)  (:517)
    if (out_origo != nullptr) out_origo[b] = make_float2((float)T[3] * P.G.scale, (float)T[7] * P.G.scale);
  }
}

__global__ void __launch_bounds__(256) ranges_tf_compact_kernel(const RangesTfParams P, const int* __restrict__ offsets,
                                                                 float2* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long b = ranges_tf_scan_index();
  if (b >= P.batch) return;
  double T[12];
  ranges_tf_load_rows(P, b, T);
  const float* __restrict__ r = P.ranges + (size_t)b * P.n;
  const unsigned long long below = (1ull << lane) - 1ull;
  int pos = offsets[b];  // (<= b * n: every count is at most n, so scan b stays below (b + 1) * n <= batch * n)
  for (int i0 = 0; i0 < P.n; i0 += 64) {
    float2 e;
    const bool keep = ranges_tf_beam(P, r, i0 + lane, T, &e);
    const unsigned long long m = __ballot(keep);
    if (keep) out[pos + __popcll(m & below)] = e;
    pos += __popcll(m);
  }
}

}  // namespace hsm
