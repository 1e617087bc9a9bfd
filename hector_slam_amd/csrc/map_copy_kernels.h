// map_copy_kernels.h -- one cell box per level of a pyramid copied from another context's planes (map_copy.hip: hsm_copy_map,
// hsm_copy_map_boxes).  They are not templates of a layout, so exactly one translation unit includes this header.
//   map_copy_cells_kernel    pass 1, over the boxes: log-odds and stamps from the source into the destination's planes, and
//                            getGridProbability of every copied cell into its probability plane -- grid_probability of
//                            map_cells.h, the function rebuild_prob_kernel calls, so the plane holds the rebuild's bits.
//                            STAGED = false: the source is the other context's planes (same device, same pitch, same flat
//                            index).  STAGED = true: it is the staging patch the box's rows were copied into, at pitch
//                            box-width (map_copy_box.h copy_patch_index), on this device.
//   map_copy_texels_kernel   pass 2, quad layout: the texels of every box grown by one cell towards -x / -y, from the finished
//                            probability plane -- update_texels_kernel's and rebuild_quad_kernel's gather of four stored floats.
// A box is cut into runs and a run into slots by map_copy_box.h: a slot of the body is four cells whose flat index in the
// DESTINATION is a multiple of 4 -- per lane one 16-byte load and three 16-byte stores of planes that are read and written
// once, 1 KiB per wavefront and instruction (on levels whose width is no multiple of 4 the phase changes from row to row;
// the split is per run).  A patch cell is 4-byte aligned only, so the staged form reads its four cells through a type that says so.
// One wavefront takes 64 slots of one run at a time, as occupancy_box_kernel does; blockIdx.y is the level.  No LDS, no scratch.
#pragma once
#include <hip/hip_runtime.h>

#include "beam_sample.h"
#include "map_cells.h"
#include "map_copy_box.h"
#include "match_types.h"

namespace hsm {

struct MapCopyLevel {
  const float* src_logodds;  // the source context's plane, or the patch
  const int* src_stamps;
  float* logodds;            // the destination's planes
  int* stamps;
  float* prob;
  float4* quad;              // null in the plane layout
  int sx, sy;
  CopyBox box;               // inside the level, or empty: nothing is copied on this level
};

struct MapCopyParams {
  MapCopyLevel lv[kMaxLevels];
  int nlev;
};

// four 4-byte cells at an address that is a multiple of 4 only
struct __attribute__((packed, aligned(4))) Cells4F {
  float x, y, z, w;
};
struct __attribute__((packed, aligned(4))) Cells4I {
  int x, y, z, w;
};

template <bool STAGED>
__global__ void __launch_bounds__(256) map_copy_cells_kernel(const MapCopyParams A) {
  const MapCopyLevel& L = A.lv[blockIdx.y];
  if (copy_box_empty(L.box)) return;
  const CopyRuns R = copy_box_runs(L.sx, L.box);
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
      float4 l;
      int4 s;
      if (STAGED) {
        const int p = copy_patch_index(R, (int)run, c);
        const Cells4F lu = *reinterpret_cast<const Cells4F*>(L.src_logodds + p);
        const Cells4I su = *reinterpret_cast<const Cells4I*>(L.src_stamps + p);
        l = make_float4(lu.x, lu.y, lu.z, lu.w);
        s = make_int4(su.x, su.y, su.z, su.w);
      } else {
        l = *reinterpret_cast<const float4*>(L.src_logodds + c);
        s = *reinterpret_cast<const int4*>(L.src_stamps + c);
      }
      *reinterpret_cast<float4*>(L.logodds + c) = l;
      *reinterpret_cast<int4*>(L.stamps + c) = s;
      *reinterpret_cast<float4*>(L.prob + c) =
          make_float4(grid_probability(l.x), grid_probability(l.y), grid_probability(l.z), grid_probability(l.w));
    } else if (g == r.body_groups) {
      auto cell = [&](int c) {
        const int p = STAGED ? copy_patch_index(R, (int)run, c) : c;
        const float l = L.src_logodds[p];
        L.logodds[c] = l;
        L.stamps[c] = L.src_stamps[p];
        L.prob[c] = grid_probability(l);
      };
      for (int i = 0; i < r.head_n; ++i) cell(r.head0 + i);
      for (int i = 0; i < r.tail_n; ++i) cell(r.tail0 + i);
    }
  }
}

__global__ void __launch_bounds__(256) map_copy_texels_kernel(const MapCopyParams A) {
  const MapCopyLevel& L = A.lv[blockIdx.y];
  if (copy_box_empty(L.box) || L.quad == nullptr) return;
  const CopyBox T = copy_texel_box(L.box);
  const int w = T.x1 - T.x0 + 1, h = T.y1 - T.y0 + 1;
  const size_t n = (size_t)w * h;
  const float* p = L.prob;
  for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < n; t += (size_t)gridDim.x * blockDim.x) {
    const int x = T.x0 + (int)(t % (size_t)w), y = T.y0 + (int)(t / (size_t)w);
    const int xn = x + 1 < L.sx ? x + 1 : x;
    const int yn = y + 1 < L.sy ? y + 1 : y;
    L.quad[quad_index(x, y, (L.sx + 3) / 4, L.sx)] =
        make_float4(p[(size_t)y * L.sx + x], p[(size_t)y * L.sx + xn], p[(size_t)yn * L.sx + x], p[(size_t)yn * L.sx + xn]);
  }
}

}  // namespace hsm
