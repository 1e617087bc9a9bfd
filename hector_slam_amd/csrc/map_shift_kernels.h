// map_shift_kernels.h -- the contents of every level of a pyramid moved by a whole number of cells inside their own planes
// (map_shift.hip: hsm_shift_map; the plan: map_shift_plan.h).  They are not templates of a layout, so exactly one translation
// unit includes this header.  The planes keep their addresses (other units and queued launches hold them), so the cells that
// survive the move take a trip through a staging block:
//   map_shift_stage_kernel   pass 1, over the surviving box in OLD coordinates: its log-odds and stamps into the staging block at
//                            pitch box-width (map_copy_box.h copy_patch_index).  The box is cut into runs and slots as a map
//                            copy's is, aligned on the PLANE: per lane two 16-byte loads, and two stores of four cells through a
//                            type that says the block is 4-byte aligned only.
//   map_shift_cells_kernel   pass 2, over EVERY cell of every level, each written once: a survivor from the staging block, a cell
//                            that scrolled in as the cleared cell (log-odds 0, stamp -1: LogOddsCell::resetGridCell), and
//                            getGridProbability of either into the probability plane -- grid_probability of map_cells.h, the
//                            function rebuild_prob_kernel calls, so the plane holds the rebuild's bits.  A row is cut like a row
//                            of the occupancy export (occupancy_rows.h): a body of 4-cell groups aligned on the destination
//                            GRID, three 16-byte stores per lane, and a ragged head and tail cell by cell (on levels whose
//                            width is no multiple of 4 the phase changes from row to row).  A group that lies wholly inside
//                            the surviving box reads the block through Cells4F / Cells4I, one that straddles its edge cell by cell.
//   map_shift_texels_kernel  pass 3, quad layout: the texels of the whole level from the finished probability plane --
//                            rebuild_quad_kernel's and map_copy_texels_kernel's gather of four stored floats.
// One wavefront takes 64 slots of one run (pass 1) or row (pass 2) at a time; blockIdx.y is the level.  No LDS, no scratch.
#pragma once
#include <hip/hip_runtime.h>

#include "beam_sample.h"
#include "map_cells.h"
#include "map_copy_box.h"
#include "map_shift_plan.h"
#include "match_types.h"

namespace hsm {

struct MapShiftLevel {
  float* logodds;  // the level's planes
  int* stamps;
  float* prob;
  float4* quad;    // null in the plane layout
  float* st_logodds;  // the staging block's share of this level
  int* st_stamps;
  int sx, sy;
  CopyBox from, to;  // the surviving cells in old and in new coordinates (ShiftLevel), inside the level or empty
};

struct MapShiftParams {
  MapShiftLevel lv[kMaxLevels];
  int nlev;
};

// four 4-byte cells at an address that is a multiple of 4 only (as map_copy_kernels.h's)
struct __attribute__((packed, aligned(4))) ShiftCells4F {
  float x, y, z, w;
};
struct __attribute__((packed, aligned(4))) ShiftCells4I {
  int x, y, z, w;
};

__global__ void __launch_bounds__(256) map_shift_stage_kernel(const MapShiftParams A) {
  const MapShiftLevel& L = A.lv[blockIdx.y];
  if (copy_box_empty(L.from)) return;
  const CopyRuns R = copy_box_runs(L.sx, L.from);
  const unsigned int slots = (unsigned int)copy_run_slots(R), chunks = (slots + 63u) >> 6;
  const unsigned int turns = (unsigned int)R.runs * chunks;
  const unsigned int lane = threadIdx.x & 63u, waves = (gridDim.x * blockDim.x) >> 6;
  const unsigned int wave = (unsigned int)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
  for (unsigned int t = wave; t < turns; t += waves) {
    const unsigned int run = t / chunks, chunk = t - run * chunks;
    const OccRowSplit r = copy_run_split(R, (int)run);
    const int g = (int)(chunk * 64u + lane);
    if (g < r.body_groups) {
      const int c = r.body0 + 4 * g;
      const float4 l = *reinterpret_cast<const float4*>(L.logodds + c);
      const int4 s = *reinterpret_cast<const int4*>(L.stamps + c);
      const int p = copy_patch_index(R, (int)run, c);
      ShiftCells4F lu;
      ShiftCells4I su;
      lu.x = l.x, lu.y = l.y, lu.z = l.z, lu.w = l.w;
      su.x = s.x, su.y = s.y, su.z = s.z, su.w = s.w;
      *reinterpret_cast<ShiftCells4F*>(L.st_logodds + p) = lu;
      *reinterpret_cast<ShiftCells4I*>(L.st_stamps + p) = su;
    } else if (g == r.body_groups) {
      auto cell = [&](int c) {
        const int p = copy_patch_index(R, (int)run, c);
        L.st_logodds[p] = L.logodds[c];
        L.st_stamps[p] = L.stamps[c];
      };
      for (int i = 0; i < r.head_n; ++i) cell(r.head0 + i);
      for (int i = 0; i < r.tail_n; ++i) cell(r.tail0 + i);
    }
  }
}

__global__ void __launch_bounds__(256) map_shift_cells_kernel(const MapShiftParams A) {
  const MapShiftLevel& L = A.lv[blockIdx.y];
  const CopyBox B = L.to;
  const int bw = B.x1 - B.x0 + 1;  // the staging block's pitch
  const unsigned int slots = (unsigned int)occupancy_row_slots(L.sx), chunks = (slots + 63u) >> 6;
  const unsigned int turns = (unsigned int)L.sy * chunks;
  const unsigned int lane = threadIdx.x & 63u, waves = (gridDim.x * blockDim.x) >> 6;
  const unsigned int wave = (unsigned int)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
  for (unsigned int t = wave; t < turns; t += waves) {
    const int y = (int)(t / chunks);
    const unsigned int chunk = t - (unsigned int)y * chunks;
    const int row = y * L.sx;
    const OccRowSplit r = occupancy_row_split(row, 0, L.sx - 1);
    const bool row_in = !copy_box_empty(B) && y >= B.y0 && y <= B.y1;
    const int st_row = (y - B.y0) * bw - B.x0;  // staging index of the row's cell x: st_row + x
    const int g = (int)(chunk * 64u + lane);
    if (g < r.body_groups) {
      const int c = r.body0 + 4 * g;
      const int x = c - row;
      float4 l = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      int4 s = make_int4(-1, -1, -1, -1);
      if (row_in && x >= B.x0 && x + 3 <= B.x1) {
        const ShiftCells4F lu = *reinterpret_cast<const ShiftCells4F*>(L.st_logodds + st_row + x);
        const ShiftCells4I su = *reinterpret_cast<const ShiftCells4I*>(L.st_stamps + st_row + x);
        l = make_float4(lu.x, lu.y, lu.z, lu.w);
        s = make_int4(su.x, su.y, su.z, su.w);
      } else if (row_in && x + 3 >= B.x0 && x <= B.x1) {  // the group straddles the box's edge
        if (x >= B.x0 && x <= B.x1) l.x = L.st_logodds[st_row + x], s.x = L.st_stamps[st_row + x];
        if (x + 1 >= B.x0 && x + 1 <= B.x1) l.y = L.st_logodds[st_row + x + 1], s.y = L.st_stamps[st_row + x + 1];
        if (x + 2 >= B.x0 && x + 2 <= B.x1) l.z = L.st_logodds[st_row + x + 2], s.z = L.st_stamps[st_row + x + 2];
        if (x + 3 >= B.x0 && x + 3 <= B.x1) l.w = L.st_logodds[st_row + x + 3], s.w = L.st_stamps[st_row + x + 3];
      }
      *reinterpret_cast<float4*>(L.logodds + c) = l;
      *reinterpret_cast<int4*>(L.stamps + c) = s;
      *reinterpret_cast<float4*>(L.prob + c) =
          make_float4(grid_probability(l.x), grid_probability(l.y), grid_probability(l.z), grid_probability(l.w));
    } else if (g == r.body_groups) {
      auto cell = [&](int c) {
        const int x = c - row;
        float l = 0.0f;
        int s = -1;
        if (row_in && x >= B.x0 && x <= B.x1) {
          l = L.st_logodds[st_row + x];
          s = L.st_stamps[st_row + x];
        }
        L.logodds[c] = l;
        L.stamps[c] = s;
        L.prob[c] = grid_probability(l);
      };
      for (int i = 0; i < r.head_n; ++i) cell(r.head0 + i);
      for (int i = 0; i < r.tail_n; ++i) cell(r.tail0 + i);
    }
  }
}

__global__ void __launch_bounds__(256) map_shift_texels_kernel(const MapShiftParams A) {
  const MapShiftLevel& L = A.lv[blockIdx.y];
  if (L.quad == nullptr) return;
  const size_t n = (size_t)L.sx * L.sy;
  const float* p = L.prob;
  for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < n; t += (size_t)gridDim.x * blockDim.x) {
    const int x = (int)(t % (size_t)L.sx), y = (int)(t / (size_t)L.sx);
    const int xn = x + 1 < L.sx ? x + 1 : x;
    const int yn = y + 1 < L.sy ? y + 1 : y;
    L.quad[quad_index(x, y, (L.sx + 3) / 4, L.sx)] =
        make_float4(p[(size_t)y * L.sx + x], p[(size_t)y * L.sx + xn], p[(size_t)yn * L.sx + x], p[(size_t)yn * L.sx + xn]);
  }
}

}  // namespace hsm
