// map_merge_kernels.h -- another context's pyramid merged into this one's under a rigid transform (map_copy.hip: hsm_merge_map).
// Included by map_copy.hip only.
//   map_merge_cells_kernel   over one cell box per level of the DESTINATION: every cell (x, y) of the box is taken through the
//                            affine of its level into the source's map coordinates, the source's log-odds at the nearest cell is
//                            combined into the destination's (merge_cell_value below: the rule of capi.h, stated once), and
//                            grid_probability of every cell it writes goes into the probability plane -- the function
//                            rebuild_prob_kernel calls, so the plane holds the rebuild's bits (a cell that is not written keeps
//                            the probability every writer of the map left for its log-odds).  Stamps are neither read nor written.
//                            STAGED = false: the source is the other context's plane.  STAGED = true: it is the staging patch
//                            the rows of the source box `sbox` were copied into, read through copy_patch_index (map_copy_box.h).
// The texels of the boxes are map_copy_texels_kernel's second pass, unchanged (map_copy_kernels.h).
//
// The destination side is streamed like the copy's: a box row is cut into a head, 4-cell slots aligned on the destination grid
// and a tail (map_copy_box.h copy_run_split); a body slot is one 16-byte load of the log-odds and one 16-byte store each of the
// log-odds and the probabilities.  A slot whose four source values are all 0 neither loads nor stores.
//
// The source side is a gather whose shape turns with the angle, so the walk is a 2-D tile: a wavefront takes 4 slots x 16 rows
// (16 x 16 cells, lane = row * 4 + slot), a workgroup four such tiles side by side (64 x 16 cells), and the workgroups walk the
// box's tiles row-major.  Why not the copy's walk (64 slots of ONE row per wavefront): at theta = 0 that reads one or two source
// rows, but at theta = pi/2 its 256 cells read 256 source rows, 256 cache lines for 1 KiB of payload.  The tile's footprint is a
// turned 16 x 16 square at every angle: at most 23 source rows, 16 at 0 and at pi/2, each a piece of 64 bytes or less.  The price
// is on the destination side, 64-byte pieces of 16 rows per instruction instead of 1 KiB of one row; a workgroup still covers
// whole 256-byte stretches of each of its rows.  Chosen from the code, not from a measurement; tools/bench_merge_map.py times
// theta = 0, 0.3 and pi/2 against each other.  No LDS (no cell is read twice by a workgroup), no scratch.
#pragma once
#include <hip/hip_runtime.h>

#include "map_cells.h"
#include "map_copy_box.h"
#include "match_types.h"

namespace hsm {

struct MapMergeLevel {
  const float* src;    // the source level's log-odds plane, or the patch
  float* logodds;      // the destination's planes
  float* prob;
  int sx, sy;          // the destination level
  int ssx, ssy;        // the source level
  CopyBox box;         // of the destination, inside the level, or empty: nothing is merged on this level
  CopyBox sbox;        // STAGED: the box of the source level whose rows the patch holds
  float c, s, bx, by;  // source map coordinates of (x, y): ((c x + s y) + bx, ((-s) x + c y) + by)
};

struct MapMergeParams {
  MapMergeLevel lv[kMaxLevels];
  int nlev;
};

constexpr int kMergeTileSlots = 4, kMergeTileRows = 16;  // per wavefront
constexpr int kMergeBlockSlots = 4 * kMergeTileSlots;      // per workgroup of four wavefronts

// tiles of a box: (slots of a row / 16, rounded up) x (rows / 16, rounded up)
HSM_OCC_HD inline unsigned int merge_box_tiles(const CopyBox& b) {
  if (copy_box_empty(b)) return 0u;
  const int slots = occupancy_row_slots(b.x1 - b.x0 + 1), rows = b.y1 - b.y0 + 1;
  return (unsigned int)((slots + kMergeBlockSlots - 1) / kMergeBlockSlots) * (unsigned int)((rows + kMergeTileRows - 1) / kMergeTileRows);
}

// the source's log-odds for destination cell (x, y): every operation rounded to fp32, none fused
template <bool STAGED>
__device__ __forceinline__ float merge_sample(const MapMergeLevel& L, const CopyRuns& SR, int x, int y) {
#pragma clang fp contract(off)
  const float fx = (float)x, fy = (float)y;
  const float cx = L.c * fx, sv = L.s * fy;
  const float nsx = (-L.s) * fx, cy = L.c * fy;
  const float mx = (cx + sv) + L.bx;
  const float my = (nsx + cy) + L.by;
  const float rx = floorf(mx + 0.5f), ry = floorf(my + 0.5f);
  // (compared as floats: a coordinate beyond the range of int is outside like any other)
  if (!(rx >= 0.0f && rx < (float)L.ssx && ry >= 0.0f && ry < (float)L.ssy)) return 0.0f;
  const int ix = (int)rx, iy = (int)ry;
  float v;
  if (STAGED) {
    if (ix < L.sbox.x0 || ix > L.sbox.x1 || iy < L.sbox.y0 || iy > L.sbox.y1) return 0.0f;
    v = L.src[copy_patch_index(SR, SR.step ? iy - L.sbox.y0 : 0, iy * L.ssx + ix)];
  } else {
    v = L.src[(size_t)iy * L.ssx + ix];
  }
  return (v - v == 0.0f) ? v : 0.0f;  // NaN and the infinities count as 0
}

// what the source's value v makes of the destination's d (written only where v != 0)
__device__ __forceinline__ float merge_cell_value(float d, float v) {
  if (v < 0.0f) return d + v;
  if (v > 0.0f) return d < 50.0f ? fminf(d + v, 50.0f) : d;
  return d;
}

template <bool STAGED>
__global__ void __launch_bounds__(256) map_merge_cells_kernel(const MapMergeParams A) {
  const MapMergeLevel& L = A.lv[blockIdx.y];
  if (copy_box_empty(L.box)) return;
  const int w = L.box.x1 - L.box.x0 + 1, h = L.box.y1 - L.box.y0 + 1;
  const CopyRuns R = {L.box.y0 * L.sx + L.box.x0, w, h, L.sx};  // one run per row, also where the box spans the level's width
  const CopyRuns SR = STAGED ? copy_box_runs(L.ssx, L.sbox) : CopyRuns{0, 0, 0, 0};
  const int slots = copy_run_slots(R);
  const unsigned int tiles_x = (unsigned int)((slots + kMergeBlockSlots - 1) / kMergeBlockSlots);
  const unsigned int tiles = tiles_x * (unsigned int)((h + kMergeTileRows - 1) / kMergeTileRows);
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  for (unsigned int t = blockIdx.x; t < tiles; t += gridDim.x) {
    const unsigned int ty = t / tiles_x, tx = t - ty * tiles_x;
    const int run = (int)ty * kMergeTileRows + (lane >> 2);
    const int g = (int)tx * kMergeBlockSlots + wave * kMergeTileSlots + (lane & 3);
    if (run >= h) continue;
    const OccRowSplit r = copy_run_split(R, run);
    const int y = L.box.y0 + run, row_base = y * L.sx;
    if (g < r.body_groups) {
      const int c = r.body0 + 4 * g, x = c - row_base;
      const float v0 = merge_sample<STAGED>(L, SR, x, y), v1 = merge_sample<STAGED>(L, SR, x + 1, y);
      const float v2 = merge_sample<STAGED>(L, SR, x + 2, y), v3 = merge_sample<STAGED>(L, SR, x + 3, y);
      if (v0 != 0.0f || v1 != 0.0f || v2 != 0.0f || v3 != 0.0f) {
        float4 d = *reinterpret_cast<const float4*>(L.logodds + c);
        d = make_float4(merge_cell_value(d.x, v0), merge_cell_value(d.y, v1), merge_cell_value(d.z, v2), merge_cell_value(d.w, v3));
        *reinterpret_cast<float4*>(L.logodds + c) = d;
        *reinterpret_cast<float4*>(L.prob + c) =
            make_float4(grid_probability(d.x), grid_probability(d.y), grid_probability(d.z), grid_probability(d.w));
      }
    } else if (g == r.body_groups) {
      auto cell = [&](int c) {
        const float v = merge_sample<STAGED>(L, SR, c - row_base, y);
        if (v != 0.0f) {
          const float d = merge_cell_value(L.logodds[c], v);
          L.logodds[c] = d;
          L.prob[c] = grid_probability(d);
        }
      };
      for (int i = 0; i < r.head_n; ++i) cell(r.head0 + i);
      for (int i = 0; i < r.tail_n; ++i) cell(r.tail0 + i);
    }
  }
}

}  // namespace hsm
