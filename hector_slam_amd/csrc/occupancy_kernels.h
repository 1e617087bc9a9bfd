// occupancy_kernels.h -- a level's log-odds as the occupancy grid the node publishes (occupancy.hip): the whole level, or the
// cells of its publish box only.  They are not templates, so exactly one translation unit includes this header.
#pragma once
#include <hip/hip_runtime.h>

#include "map_cells.h"
#include "match_types.h"
#include "occupancy_rows.h"

namespace hsm {

// ---- rows next to the path ----------------------------------------------------
// publishMap's cell loop (hector_mapping/src/HectorMappingRos.cpp:449-468): four cells per thread,
// one coalesced 16-byte load and one 4-byte store
__global__ void occupancy_grid_kernel(const float* __restrict__ logodds, size_t n, signed char* __restrict__ out) {
  const size_t n4 = n / 4;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const float4 l = reinterpret_cast<const float4*>(logodds)[i];
    char4 o;
    o.x = l.x < 0.0f ? 0 : (l.x > 0.0f ? 100 : -1);  // isFree / isOccupied, GridMapLogOdds.h:76-84
    o.y = l.y < 0.0f ? 0 : (l.y > 0.0f ? 100 : -1);
    o.z = l.z < 0.0f ? 0 : (l.z > 0.0f ? 100 : -1);
    o.w = l.w < 0.0f ? 0 : (l.w > 0.0f ? 100 : -1);
    reinterpret_cast<char4*>(out)[i] = o;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const float l = logodds[n4 * 4 + threadIdx.x];
    out[n4 * 4 + threadIdx.x] = l < 0.0f ? 0 : (l > 0.0f ? 100 : -1);
  }
}

// ---- the published grid, changed cells only (hsm_occupancy_changes*) ------------------------------------------------------------
// Per level a PUBLISH box: the hull of every cell whose log-odds may have changed since the level was last exported.  Host-side
// writers widen a host copy (Level::pub); device-side updates widen one more block of boxes next to the mirror's
// (update_mark_scan_kernel, mark_box_block) that the host never fetches.  An export is two launches on the context's stream:
//   occupancy_prep_kernel  one wavefront, lane = level: the union of the host copy (by value) and the device box, clamped to the
//                          level, goes to `box_out` (what the convert launch reads) and, as x0,y0,x1,y1 or 0,0,-1,-1, to the
//                          caller's `bbox_out`; the device box goes back to empty.  Levels without a `box_out` are left alone.
//   occupancy_box_kernel   the cells of that box only, into a row-major sx * sy byte grid.  The host does not know the box, so
//                          the grid is fixed and strides over it: one wavefront takes 64 slots of one row at a time
//                          (occupancy_rows.h: a slot is a 4-cell group aligned on the GRID -- one coalesced 16-byte load, one
//                          4-byte store -- or the row's ragged head and tail, byte stores).  The box is read through a
//                          wave-uniform address (scalar loads); a wavefront of an empty box returns after that load.
struct OccupancyPrepParams {
  int4 host_box[kMaxLevels];  // the host's copy, empty where x1 < x0
  int2 dims[kMaxLevels];      // sx, sy
  int* box_out[kMaxLevels];   // 4 ints, or nullptr: this level is not exported
  int* bbox_out[kMaxLevels];  // the caller's 4 ints, or nullptr
  int* pub_boxes;             // [kMaxLevels * 4] the device publish boxes
  int nlev;
};

__global__ void __launch_bounds__(64) occupancy_prep_kernel(const OccupancyPrepParams A) {
  const int l = threadIdx.x;
  if (l >= A.nlev || A.box_out[l] == nullptr) return;
  int* pub = A.pub_boxes + 4 * l;
  int x0 = pub[0], y0 = pub[1], x1 = pub[2], y1 = pub[3];
  pub[0] = pub[1] = kBoxEmptyLo;
  pub[2] = pub[3] = kBoxEmptyHi;
  const int4 hb = A.host_box[l];
  if (hb.z >= hb.x) {
    x0 = min(x0, hb.x);
    y0 = min(y0, hb.y);
    x1 = max(x1, hb.z);
    y1 = max(y1, hb.w);
  }
  x0 = max(x0, 0);
  y0 = max(y0, 0);
  x1 = min(x1, A.dims[l].x - 1);
  y1 = min(y1, A.dims[l].y - 1);
  if (x1 < x0 || y1 < y0) {
    x0 = y0 = 0;
    x1 = y1 = -1;
  }
  int* box = A.box_out[l];
  box[0] = x0;
  box[1] = y0;
  box[2] = x1;
  box[3] = y1;
  if (int* bb = A.bbox_out[l]) {
    bb[0] = x0;
    bb[1] = y0;
    bb[2] = x1;
    bb[3] = y1;
  }
}

// out_aligned == 0: `out` is no multiple of 4, a group is stored as four bytes
__global__ void __launch_bounds__(256) occupancy_box_kernel(const float* __restrict__ logodds, int sx, const int* __restrict__ box_in,
                                                            signed char* __restrict__ out, int out_aligned) {
  const int4 box = *reinterpret_cast<const int4*>(box_in);
  if (box.z < box.x) return;  // nothing changed
  const unsigned int slots = (unsigned int)occupancy_row_slots(box.z - box.x + 1), chunks = (slots + 63u) >> 6;
  const unsigned int turns = (unsigned int)(box.w - box.y + 1) * chunks;
  const unsigned int lane = threadIdx.x & 63u, waves = (gridDim.x * blockDim.x) >> 6;
  const unsigned int wave = (unsigned int)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
  for (unsigned int t = wave; t < turns; t += waves) {
    const unsigned int row = t / chunks, chunk = t - row * chunks;
    const OccRowSplit r = occupancy_row_split((box.y + (int)row) * sx, box.x, box.z);
    const int g = (int)(chunk * 64u + lane);
    if (g < r.body_groups) {
      const int c = r.body0 + 4 * g;
      const float4 l = *reinterpret_cast<const float4*>(logodds + c);
      const signed char o0 = occupancy_value(l.x), o1 = occupancy_value(l.y), o2 = occupancy_value(l.z), o3 = occupancy_value(l.w);
      if (out_aligned) {  // one 4-byte store (cell c in the low byte)
        *reinterpret_cast<unsigned int*>(out + c) = (unsigned int)(unsigned char)o0 | ((unsigned int)(unsigned char)o1 << 8) |
                                                    ((unsigned int)(unsigned char)o2 << 16) | ((unsigned int)(unsigned char)o3 << 24);
      } else {
        out[c] = o0;
        out[c + 1] = o1;
        out[c + 2] = o2;
        out[c + 3] = o3;
      }
    } else if (g == r.body_groups) {
      for (int i = 0; i < r.head_n; ++i) out[r.head0 + i] = occupancy_value(logodds[r.head0 + i]);
      for (int i = 0; i < r.tail_n; ++i) out[r.tail0 + i] = occupancy_value(logodds[r.tail0 + i]);
    }
  }
}

}  // namespace hsm
