// ray_kernels.h -- the kernels of rays.hip: DistanceMeasurementProvider::getDist (hector_map_tools/.../HectorMapTools.h:133-234)
// for arrays of rays, and for the rays of whole scan fans cast from a batch of sensor poses, straight on the log-odds plane (a
// cell of the published grid is 100 <=> logOdds > 0).  The kernels are not templates of anything another unit instantiates:
// exactly one translation unit may include this header.
//
// One ray, however it is walked (ray_line): both end points to cells (truncation), the in-map test of both, the Bresenham line
// between them (map_cells.h BeamLine), at most 5000 steps of it (bresenham2D's max_length), the FIRST step whose cell is
// occupied, and (int)sqrtf of the cell distance to it.  Two walks find that step:
//   * one WAVEFRONT per ray (ray_walk_wave): lane k tests steps k, k+64, ... through the closed form of the error accumulator
//     (line_cell), a ballot finds the first occupied step and the search stops at that chunk -- the sequential early-exit walk of
//     the reference without walking sequentially.  Few load instructions per ray; a load touches up to 64 lines on a steep ray.
//   * one LANE per ray (ray_walk_lane): the lane runs the reference's own error accumulator, kRayLaneSteps cells per round; the
//     addresses do not depend on the loaded values, so a round's loads are all in flight together: their values are folded into
//     one bit mask before anything branches on them (in the gfx950 code seven loads are issued, the wait that follows is for the
//     oldest alone, and the eighth load goes out behind it; no branch lies between the eight).  The
//     64 lanes of a wavefront hold 64 ADJACENT beams of one fan, whose cells stay within a few lines of each other for most of
//     the walk; the wavefront leaves the loop when its longest ray is done.
// The result is a function of the ray alone, so both walks give the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include "beam_sample.h"
#include "map_cells.h"

namespace hsm {

// the published grid of a level: its cells and the CoordinateTransformer of its metadata (HectorMapTools.h:58-98)
struct RayGrid {
  const float* logodds;
  int sx, sy;
  float origin_x, origin_y, scale, inv_scale;
};

struct RayQueryParams {
  RayGrid grid;
  const float2* begin_world;
  const float2* end_world;
  int n;
  float* out_dist;
  float2* out_hit;  // may be null
};

constexpr unsigned int kRayMaxSteps = 5000u;  // bresenham2D(..., max_length = 5000)

// The line of one ray and the steps to test, [0, *end).  false: an end point outside the level (checkOccupancyBresenhami :157,
// :167) -- or, CHECK_FINITE, a cell coordinate that is no finite number, which the float -> int conversion would otherwise
// turn into whatever cell the hardware makes of it (x86-64 gives INT_MIN, outside every map; this device gives 0 for a NaN).
template <bool CHECK_FINITE>
__device__ __forceinline__ bool ray_line(const RayGrid& G, float2 bw, float2 ew, BeamLine& b, int& x0, int& y0,
                                         unsigned int& end) {
  // getC2Coords(...).cast<int>(): ((world - origo) * inv_scale), truncated
  const float fx0 = (bw.x - G.origin_x) * G.inv_scale, fy0 = (bw.y - G.origin_y) * G.inv_scale;
  const float fx1 = (ew.x - G.origin_x) * G.inv_scale, fy1 = (ew.y - G.origin_y) * G.inv_scale;
  if (CHECK_FINITE && !(fabsf(fx0) <= 3.402823466e38f && fabsf(fy0) <= 3.402823466e38f && fabsf(fx1) <= 3.402823466e38f &&
                        fabsf(fy1) <= 3.402823466e38f))
    return false;
  x0 = (int)fx0;
  y0 = (int)fy0;
  const int x1 = (int)fx1, y1 = (int)fy1;
  if ((x0 < 0) || (x0 >= G.sx) || (y0 < 0) || (y0 >= G.sy) || (x1 < 0) || (x1 >= G.sx) || (y1 < 0) || (y1 >= G.sy)) return false;
  const int dx = x1 - x0, dy = y1 - y0;
  const unsigned int abs_dx = (unsigned int)(dx < 0 ? -dx : dx), abs_dy = (unsigned int)(dy < 0 ? -dy : dy);
  const int offset_dx = dx > 0 ? 1 : -1;
  const int offset_dy = (dy > 0 ? 1 : -1) * G.sx;
  b.start = (unsigned int)(y0 * G.sx + x0);
  if (abs_dx >= abs_dy) {
    b.abs_da = abs_dx; b.abs_db = abs_dy; b.offset_a = offset_dx; b.offset_b = offset_dy;
  } else {
    b.abs_da = abs_dy; b.abs_db = abs_dx; b.offset_a = offset_dy; b.offset_b = offset_dx;
  }
  b.e0 = b.abs_da / 2;
  end = b.abs_da < kRayMaxSteps ? b.abs_da : kRayMaxSteps;
  return true;
}

// what a ray with its first occupied cell `c` returns: the distance in cells, and the cell's world coordinates
__device__ __forceinline__ float ray_hit(const RayGrid& G, int x0, int y0, unsigned int c, float2& hit_world) {
  const int ex = (int)(c % (unsigned int)G.sx), ey = (int)(c / (unsigned int)G.sx);
  const float fx = (float)(x0 - ex), fy = (float)(y0 - ey);
  hit_world = make_float2(G.origin_x + ((float)ex * G.scale), G.origin_y + ((float)ey * G.scale));  // getC1Coords
  return (float)(int)sqrtf(fx * fx + fy * fy);  // int distMap = (begin - end).cast<float>().norm()
}

// One wavefront, one ray (the same in every lane): the distance in cells or -1, and *hit_world where there is a hit.
template <bool CHECK_FINITE>
__device__ __forceinline__ float ray_walk_wave(const RayGrid& G, float2 bw, float2 ew, int lane, float2& hit_world) {
  BeamLine b;
  int x0, y0;
  unsigned int end;
  if (!ray_line<CHECK_FINITE>(G, bw, ew, b, x0, y0, end)) return -1.0f;
  for (unsigned int i0 = 0; i0 < end; i0 += 64) {
    const unsigned int i = i0 + lane;
    const bool occ = i < end && G.logodds[line_cell(b, i)] > 0.0f;  // data[offset] == 100
    const unsigned long long m = __ballot(occ);
    if (m) return ray_hit(G, x0, y0, line_cell(b, i0 + (unsigned int)__ffsll((long long)m) - 1u), hit_world);
  }
  return -1.0f;
}

// One lane, one ray (`active`: this lane has one).  Every cell a round loads is a cell of the line -- both end cells are inside
// the level and so is everything between them; the steps of a round that lie behind `end` load the start cell again.
constexpr int kRayLaneSteps = 8;

__device__ __forceinline__ float ray_walk_lane(const RayGrid& G, float2 bw, float2 ew, bool active, float2& hit_world) {
  BeamLine b;
  int x0 = 0, y0 = 0;
  unsigned int end = 0;
  if (!active || !ray_line<true>(G, bw, ew, b, x0, y0, end)) return -1.0f;
  unsigned int offset = b.start, error_b = b.e0;  // bresenham2D's own state (:212-232)
  for (unsigned int i0 = 0; i0 < end; i0 += kRayLaneSteps) {
    unsigned int cell[kRayLaneSteps];
    float v[kRayLaneSteps];
#pragma unroll
    for (int u = 0; u < kRayLaneSteps; ++u) {
      cell[u] = i0 + u < end ? offset : b.start;
      offset += (unsigned int)b.offset_a;
      error_b += b.abs_db;
      if (error_b >= b.abs_da) {
        offset += (unsigned int)b.offset_b;
        error_b -= b.abs_da;
      }
    }
#pragma unroll
    for (int u = 0; u < kRayLaneSteps; ++u) v[u] = G.logodds[cell[u]];
    // every value of the round goes into one mask before anything branches on it: a chain of early exits would let the
    // compiler sink each load behind the test of the one before it, a memory round trip per step
    unsigned int occ = 0u;
#pragma unroll
    for (int u = 0; u < kRayLaneSteps; ++u) occ |= (i0 + u < end && v[u] > 0.0f ? 1u : 0u) << u;
    if (occ) {  // the first one in step order
      const int first = __ffs((int)occ) - 1;
      unsigned int c = cell[0];
#pragma unroll
      for (int u = 1; u < kRayLaneSteps; ++u) c = first == u ? cell[u] : c;
      return ray_hit(G, x0, y0, c, hit_world);
    }
  }
  return -1.0f;
}

// hsm_ray_distances (CHECK_FINITE = false: as it always was) and hsm_ray_distances_device: the caller's rays, a wavefront each
template <bool CHECK_FINITE>
__global__ void __launch_bounds__(256) ray_distance_kernel(const RayQueryParams P) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (r >= P.n) return;
  float2 hit;
  const float dist = ray_walk_wave<CHECK_FINITE>(P.grid, P.begin_world[r], P.end_world[r], lane, hit);
  if (lane != 0) return;
  if (dist >= 0.0f && P.out_hit) P.out_hit[r] = hit;
  P.out_dist[r] = P.grid.scale * dist;  // getC1Scale
}

// hsm_cast_scans*: beam i of pose b is the ray from the pose to range_max along theta + angles[i], every operation fp32 and
// un-fused; it never exists in memory.
struct CastScansParams {
  RayGrid grid;
  const float* poses;   // [batch * 3] world: x, y, theta
  const float* angles;  // [n] sensor frame
  int batch, n;
  float range_max;
  float* out_ranges;  // [batch * n]
  float2* out_hit;    // [batch * n] or null
};

__device__ __forceinline__ void cast_ray(float px, float py, float theta, float beam_angle, float range_max, float2& bw,
                                         float2& ew) {
  float s, c;
  sincos_f32(theta + beam_angle, s, c);
  bw = make_float2(px, py);
  ew = make_float2(px + range_max * c, py + range_max * s);
}

// a wavefront per ray: ray r = b * n + i
__global__ void __launch_bounds__(256) cast_scans_wave_kernel(const CastScansParams P) {
  const int lane = threadIdx.x & 63;
  const unsigned int r = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  if (r >= (unsigned int)P.batch * (unsigned int)P.n) return;
  const unsigned int b = r / (unsigned int)P.n, i = r - b * (unsigned int)P.n;
  float2 bw, ew, hit;
  cast_ray(P.poses[3 * b], P.poses[3 * b + 1], P.poses[3 * b + 2], P.angles[i], P.range_max, bw, ew);
  const float dist = ray_walk_wave<true>(P.grid, bw, ew, lane, hit);
  if (lane != 0) return;
  if (dist >= 0.0f && P.out_hit) P.out_hit[r] = hit;
  P.out_ranges[r] = P.grid.scale * dist;
}

// a lane per ray: a wavefront holds beams [64 k, 64 k + 64) of one pose
__global__ void __launch_bounds__(256) cast_scans_lane_kernel(const CastScansParams P) {
  const int lane = threadIdx.x & 63;
  const unsigned int per_pose = ((unsigned int)P.n + 63u) >> 6;
  const unsigned int w = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  if (w >= (unsigned int)P.batch * per_pose) return;
  const unsigned int b = w / per_pose, i = (w - b * per_pose) * 64u + (unsigned int)lane;
  const bool active = i < (unsigned int)P.n;
  float2 bw, ew, hit;
  cast_ray(P.poses[3 * b], P.poses[3 * b + 1], P.poses[3 * b + 2], P.angles[active ? i : 0u], P.range_max, bw, ew);
  const float dist = ray_walk_lane(P.grid, bw, ew, active, hit);
  if (!active) return;
  const size_t r = (size_t)b * (unsigned int)P.n + i;
  if (dist >= 0.0f && P.out_hit) P.out_hit[r] = hit;
  P.out_ranges[r] = P.grid.scale * dist;
}

}  // namespace hsm
