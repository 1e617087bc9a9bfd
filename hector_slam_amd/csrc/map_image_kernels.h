// map_image_kernels.h -- a level's log-odds as the images and the box the map consumers draw from (occupancy.hip): the hull of
// its known cells (hsm_map_extents*), a cell box as a y-flipped byte image (hsm_map_image*) and windows of that image clamped
// around batches of poses (hsm_map_tiles*).  They are not templates, so exactly one translation unit includes this header.
// One cell rule for all of them, publishMap's (occupancy_rows.h occupancy_value): free where the log-odds is < 0, occupied where it
// is > 0, unknown otherwise (+0, -0, NaN); a KNOWN cell is free or occupied.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "occupancy_rows.h"

namespace hsm {

// map_to_image_node's bytes (hector_compressed_map_transport/src/map_to_image_node.cpp:123-136): free 255, occupied 0, unknown 127
__device__ __forceinline__ unsigned int map_image_byte(float logodds) {
  const signed char v = occupancy_value(logodds);
  return v == 0 ? 255u : (v > 0 ? 0u : 127u);
}

// ---- the hull of the known cells (hsm_map_extents*) -----------------------------------------------------------------------------
// Two launches on the context's stream:
//   map_extents_kernel         one pass over the plane, four cells a thread at a time (one coalesced 16-byte load: the plane starts
//                              on an allocation and a group on a flat index that is a multiple of 4, whatever the level's width).
//                              A thread keeps the smallest and largest column and FLAT index of its known cells -- the rows follow
//                              from the flat indices by one division at the very end --, a wavefront folds them across its lanes, a
//                              workgroup through LDS, and one thread of a workgroup that saw a known cell sends them to the four
//                              accumulators with integer atomic minima (the maxima negated).  Minima commute: the result does not
//                              depend on the launch shape or on the order of arrival.
//   map_extents_finish_kernel  one thread: the accumulators as x0,y0,x1,y1 (or 0,0,-1,-1) into the caller's box -- its only write
//                              -- and back to kExtentsNone for the next call.
// acc[4]: min column | min flat index | min -(column) | min -(flat index); kExtentsNone where no known cell was seen (every byte
// 0x7f: what hsm_create fills the block with).
constexpr int kExtentsNone = 0x7f7f7f7f;

__device__ __forceinline__ bool cell_known(float logodds) { return logodds < 0.0f || logodds > 0.0f; }

__global__ void __launch_bounds__(256) map_extents_kernel(const float* __restrict__ logodds, int sx, int n, int* __restrict__ acc) {
  __shared__ int part[4][4];
  const int step = (int)(gridDim.x * blockDim.x) * 4;  // (at most 2^21: grid_for launches 2048 workgroups at most)
  int i = (int)(blockIdx.x * blockDim.x + threadIdx.x) * 4;
  int x = i % sx;            // the column of cell i; it advances by step % sx a turn
  const int dx = step % sx;
  int x_lo = kExtentsNone, f_lo = kExtentsNone, x_hi = -1, f_hi = -1;
  for (; i + 3 < n; i += step) {
    const float4 l = *reinterpret_cast<const float4*>(logodds + i);
    const float v[4] = {l.x, l.y, l.z, l.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (cell_known(v[k])) {
        int xk = x + k;
        while (xk >= sx) xk -= sx;  // (a group can cross a row's end; twice on a level two cells wide)
        x_lo = min(x_lo, xk);
        x_hi = max(x_hi, xk);
        f_lo = min(f_lo, i + k);
        f_hi = max(f_hi, i + k);
      }
    }
    x += dx;
    if (x >= sx) x -= sx;
  }
  if (blockIdx.x == 0 && (int)threadIdx.x < (n & 3)) {  // the plane's last one to three cells
    const int c = (n & ~3) + (int)threadIdx.x;
    if (cell_known(logodds[c])) {
      const int xc = c % sx;
      x_lo = min(x_lo, xc);
      x_hi = max(x_hi, xc);
      f_lo = min(f_lo, c);
      f_hi = max(f_hi, c);
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    x_lo = min(x_lo, __shfl_xor(x_lo, o, 64));
    f_lo = min(f_lo, __shfl_xor(f_lo, o, 64));
    x_hi = max(x_hi, __shfl_xor(x_hi, o, 64));
    f_hi = max(f_hi, __shfl_xor(f_hi, o, 64));
  }
  const unsigned int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0) {
    part[w][0] = x_lo;
    part[w][1] = f_lo;
    part[w][2] = x_hi;
    part[w][3] = f_hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 4; ++k) {
      x_lo = min(x_lo, part[k][0]);
      f_lo = min(f_lo, part[k][1]);
      x_hi = max(x_hi, part[k][2]);
      f_hi = max(f_hi, part[k][3]);
    }
    if (f_hi >= 0) {  // an accumulator only ever falls, so one that is low enough already needs no atomic
      if (x_lo < __hip_atomic_load(acc + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(acc + 0, x_lo);
      if (f_lo < __hip_atomic_load(acc + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(acc + 1, f_lo);
      if (-x_hi < __hip_atomic_load(acc + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(acc + 2, -x_hi);
      if (-f_hi < __hip_atomic_load(acc + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(acc + 3, -f_hi);
    }
  }
}

__global__ void __launch_bounds__(64) map_extents_finish_kernel(int* __restrict__ acc, int sx, int* __restrict__ out_box) {
  if (threadIdx.x != 0) return;
  const int x_lo = acc[0], f_lo = acc[1], nx_hi = acc[2], nf_hi = acc[3];
  acc[0] = acc[1] = acc[2] = acc[3] = kExtentsNone;
  const bool none = f_lo == kExtentsNone;
  out_box[0] = none ? 0 : x_lo;
  out_box[1] = none ? 0 : f_lo / sx;
  out_box[2] = none ? -1 : -nx_hi;
  out_box[3] = none ? -1 : -nf_hi / sx;
}

// ---- a cell box as an image, and windows of it around poses (hsm_map_image*, hsm_map_tiles*) ---------------------------------------
// One kernel.  A TILE is tile_w x tile_h bytes of `out`, row major, its row 0 the TOP map row of the tile's cell box; tiles are
// contiguous, so `out` is one matrix of batch * tile_h rows of tile_w bytes.  The box of tile b comes from pose b (tile_box below),
// or, without poses, is `box`: the image entries launch one tile that is the clamped crop.
// A row of a tile is a contiguous run of floats in and of bytes out.  It is cut on the OUTPUT: 4-byte groups that start on a
// 4-byte boundary of the caller's memory (one packed store each, fed by one 16-byte load of four adjacent cells, which needs no more
// than the plane's 4-byte alignment), a ragged head of up to three bytes in front and a ragged tail behind (byte stores, by the
// lanes of the first and the last group).  2^lanes_log2 lanes of a wavefront share a row, a group each, so that a wavefront takes
// 64 >> lanes_log2 rows of a narrow tile at a time and `chunks` turns for a row of a wide one; 2^waves_log2 wavefronts share a
// tile's turns.  The host picks the three numbers from the tile's width and the batch (occupancy.hip map_tiles_shape); every byte
// is written once, by one lane, from one cell: the bytes do not depend on them.
struct MapTilesParams {
  const float* logodds;
  int sx, sy;
  const float* poses;  // [batch * 3] world x, y, theta (theta is not read), or nullptr: the one tile is `box`
  int4 box;            // x0, y0, x1, y1 inclusive and inside the level
  float origin_x, origin_y, inv_resolution;  // the level's OccupancyGrid metadata (hsm_ctx.h level_grid_metadata)
  int tile_w, tile_h, batch;
  unsigned char* out;
  int* out_boxes;      // [batch * 4] or nullptr
  int lanes_log2, chunks, waves_log2;
};

// map_to_image_node.cpp:147-193 for one axis -> the window's first cell; its last is lo + tile - 1 (tile <= size: the second lower
// clamp never bites).  The map coordinate is clamped to +-2^30 in float in front of the conversion, where the reference's cast is
// undefined; the clamps then give the window on the level's edge.
__device__ __forceinline__ int tile_axis_lo(float p, float origin, float inv_resolution, int tile, int size) {
  float m = (p - origin) * inv_resolution;  // getC2Coords, HectorMapTools.h:89-92 (un-fused: the library is built without contraction)
  m = fminf(fmaxf(m, -1073741824.0f), 1073741824.0f);
  int lo = (int)m - tile / 2;
  if (lo < 0) lo = 0;
  const int hi = lo + tile;
  if (hi > size) lo -= hi - size;
  if (lo < 0) lo = 0;
  return lo;
}

struct __attribute__((packed, aligned(4))) Cells4 {
  float x, y, z, w;
};

__global__ void __launch_bounds__(256) map_tiles_kernel(const MapTilesParams P) {
  const unsigned int lane = threadIdx.x & 63u, waves = (gridDim.x * blockDim.x) >> 6;
  const unsigned int wave = (unsigned int)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
  const unsigned int rows_per_turn = 64u >> P.lanes_log2, sub = lane >> P.lanes_log2, in_row = lane & ((1u << P.lanes_log2) - 1u);
  const unsigned int w = (unsigned int)P.tile_w, hgt = (unsigned int)P.tile_h, chunks = (unsigned int)P.chunks;
  const unsigned int turns = (hgt + rows_per_turn - 1u) / rows_per_turn * chunks, sharers = 1u << P.waves_log2;
  const unsigned int mis = (unsigned int)((uintptr_t)P.out & 3u);
  unsigned char* const out0 = P.out - mis;  // on a 4-byte boundary; nothing in front of P.out is touched
  const unsigned long long tasks = (unsigned long long)P.batch << P.waves_log2;
  for (unsigned long long task = wave; task < tasks; task += waves) {
    const unsigned int b = (unsigned int)(task >> P.waves_log2), share = (unsigned int)task & (sharers - 1u);
    int4 box = P.box;
    bool blank = false;  // a non-finite position: 127 throughout, the empty box
    if (P.poses) {
      const float px = P.poses[3 * (size_t)b], py = P.poses[3 * (size_t)b + 1];
      blank = !(__builtin_isfinite(px) && __builtin_isfinite(py));
      if (blank) {
        box = make_int4(0, 0, -1, -1);
      } else {
        box.x = tile_axis_lo(px, P.origin_x, P.inv_resolution, P.tile_w, P.sx);
        box.y = tile_axis_lo(py, P.origin_y, P.inv_resolution, P.tile_h, P.sy);
        box.z = box.x + P.tile_w - 1;
        box.w = box.y + P.tile_h - 1;
      }
    }
    if (P.out_boxes && share == 0 && lane == 0) {
      int* ob = P.out_boxes + 4 * (size_t)b;
      ob[0] = box.x;
      ob[1] = box.y;
      ob[2] = box.z;
      ob[3] = box.w;
    }
    for (unsigned int t = share; t < turns; t += sharers) {
      const unsigned int row_group = t / chunks, r = row_group * rows_per_turn + sub;
      if (r >= hgt) continue;
      const unsigned int slot = (t - row_group * chunks) * (1u << P.lanes_log2) + in_row;
      const unsigned int flat = mis + (b * hgt + r) * w;  // of the row's first byte, from out0 (batch * tile_w * tile_h <= INT_MAX)
      const unsigned int head_n = min((4u - (flat & 3u)) & 3u, w), groups = (w - head_n) >> 2, tail_n = (w - head_n) & 3u;
      const float* in = blank ? P.logodds : P.logodds + (size_t)(box.w - (int)r) * (size_t)P.sx + (size_t)box.x;
      if (slot < groups) {
        const unsigned int c = head_n + 4u * slot;
        unsigned int packed = 0x7f7f7f7fu;
        if (!blank) {
          const Cells4 l = *reinterpret_cast<const Cells4*>(in + c);
          packed = map_image_byte(l.x) | (map_image_byte(l.y) << 8) | (map_image_byte(l.z) << 16) | (map_image_byte(l.w) << 24);
        }
        *reinterpret_cast<unsigned int*>(out0 + flat + c) = packed;
      }
      if (slot == 0)
        for (unsigned int i = 0; i < head_n; ++i) out0[flat + i] = (unsigned char)(blank ? 127u : map_image_byte(in[i]));
      if (slot == (groups ? groups - 1u : 0u))
        for (unsigned int i = w - tail_n; i < w; ++i) out0[flat + i] = (unsigned char)(blank ? 127u : map_image_byte(in[i]));
    }
  }
}

}  // namespace hsm
