// map_points_kernels.h -- the occupied cells of a cell box of one level as a point set in level-0 units (window.hip:
// hsm_occupied_points*, and the first step of hsm_align_map).  Included by window.hip only.  The rule is capi.h's; in short: a
// cell is occupied when its log-odds is > 0.0f (occupancy_value(...) == 100 of occupancy_rows.h), occupied cells are ranked in
// row-major order of the box, the cell of rank r is kept when r % every == 0, and kept cell number j < max_points is written to
// out[j].  The output index is a function of the map alone: no atomics, no dependence on the launch shape.
//
// Three launches over the box's cells in box order c = (y - y0) * w + (x - x0), cut into tiles of kPointsTile cells:
//   map_points_count_kernel    a workgroup per tile (grid-strided): the occupied cells of the tile into tile_counts[t]
//   map_points_scan_kernel     ONE workgroup: tile_counts becomes its exclusive prefix sum in place, the total gives the counts
//   map_points_scatter_kernel  a workgroup per tile again: rank = prefix of the tile + the occupied cells in front inside the
//                              tile; kept cells below the cap are written.  A tile whose first possible output index is at or
//                              beyond max_points is skipped without being read.
// A wavefront owns kPointsTile / 4 consecutive cells of a tile, 64 at a time: the lanes of one load are neighbours in memory,
// all kPointsWaveIters loads are issued before the first is used, the occupied lanes of each are one ballot, and a lane's place
// is the population count of the ballot below it.  The four wavefront totals meet in 16 bytes of LDS, once per tile.
// WHOLE = the box spans the level's width: box order is memory order and the passes divide nothing per cell.
//
// The point of cell (x, y): affine_apply (beam_sample.h) of the level's worldTmap on ((float)x, (float)y), which is operation
// for operation affine_apply_host (hsm_ctx.h) behind hsm_world_coords_pose -- t0 + (l00 * x + l01 * y), every operation rounded
// to fp32, nothing fused -- and each coordinate times hsm_scale_to_map in fp32.  The two functions agree in operation order, so
// there is nothing to choose between them.
//
// Traffic: the box's log-odds twice (4 B a cell each pass; the second pass stops where the cap is reached), 16 B a tile of
// counts (written by the count, read and written by the scan, read by the scatter, 4 B each), 8 B a point written.  No scratch,
// 16 B of LDS (64 B in the scan).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "beam_sample.h"
#include "match_types.h"

namespace hsm {

constexpr int kPointsTile = 4096;                              // cells a workgroup of four wavefronts takes at a time
constexpr int kPointsWaveCells = kPointsTile / 4;              // ... and one wavefront of it
constexpr int kPointsWaveIters = kPointsWaveCells / 64;        // loads per lane and tile
constexpr int kPointsScanThreads = 1024;

// the inclusive box {x0, y0, x1, y1} (null: the whole level) clamped to a level of sx x sy cells -> origin, width and height;
// w == 0 and h == 0 where the box is empty or misses the level
struct PointsBox {
  int x0, y0, w, h;
};
inline PointsBox points_clamp_box(const int* bbox, int sx, int sy) {
  PointsBox b = {0, 0, sx, sy};
  if (!bbox) return b;
  const int x0 = bbox[0] < 0 ? 0 : bbox[0], y0 = bbox[1] < 0 ? 0 : bbox[1];
  const int x1 = bbox[2] > sx - 1 ? sx - 1 : bbox[2], y1 = bbox[3] > sy - 1 ? sy - 1 : bbox[3];
  if (x1 < x0 || y1 < y0) return PointsBox{0, 0, 0, 0};
  return PointsBox{x0, y0, x1 - x0 + 1, y1 - y0 + 1};
}
inline int points_tiles(long long cells) { return (int)((cells + kPointsTile - 1) / kPointsTile); }
// the tile counts, one int a tile (one at least); a multiple of 8; 0 for a negative cell count
inline size_t points_workspace_bytes(long long cells) {
  if (cells < 0) return 0;
  const size_t tiles = cells ? (size_t)points_tiles(cells) : 1;
  return (tiles * sizeof(int) + 7) & ~(size_t)7;
}

// the kept ranks 0, every, 2 every, ... below `ranks` >= 0: ceil(ranks / every) without the sum that overflows for a large `every`
__host__ __device__ inline int points_kept_below(int ranks, int every) { return ranks > 0 ? (ranks - 1) / every + 1 : 0; }

struct MapPointsParams {
  const float* logodds;  // the level's plane
  int sx;                // its width
  int x0, y0, w;         // the clamped box
  int cells, tiles;      // w * h and the tiles they make; 0 and 0 for an empty box
  int every, max_points;
  Affine2 worldTmap;
  float scale;           // hsm_scale_to_map
  float2* out;           // [max_points]
  int* out_count;        // [2]: written, kept
  int* tile_counts;      // [tiles]
};

// where box cell c lies in the plane
template <bool WHOLE>
__device__ __forceinline__ size_t points_cell_index(const MapPointsParams& P, int c) {
  if (WHOLE) return (size_t)P.y0 * P.sx + c;
  const int row = c / P.w;
  return (size_t)(P.y0 + row) * P.sx + (P.x0 + (c - row * P.w));
}

// The occupied lanes of this wavefront's kPointsWaveIters loads of tile t, one ballot per load; -> their number.
template <bool WHOLE>
__device__ __forceinline__ int points_tile_ballots(const MapPointsParams& P, int t, int wave, int lane,
                                                   unsigned long long (&mask)[kPointsWaveIters]) {
  const int first = t * kPointsTile + wave * kPointsWaveCells + lane;
  float v[kPointsWaveIters];
#pragma unroll
  for (int i = 0; i < kPointsWaveIters; ++i) {
    const int c = first + i * 64;
    v[i] = c < P.cells ? P.logodds[points_cell_index<WHOLE>(P, c)] : 0.0f;
  }
  int total = 0;
#pragma unroll
  for (int i = 0; i < kPointsWaveIters; ++i) {
    mask[i] = __ballot(v[i] > 0.0f);  // NaN and +-0 compare false
    total += __popcll(mask[i]);
  }
  return total;
}

template <bool WHOLE>
__global__ void __launch_bounds__(256) map_points_count_kernel(const MapPointsParams P) {
  __shared__ int wave_total[4];
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  for (int t = (int)blockIdx.x; t < P.tiles; t += (int)gridDim.x) {
    unsigned long long mask[kPointsWaveIters];
    const int total = points_tile_ballots<WHOLE>(P, t, wave, lane, mask);
    if (lane == 0) wave_total[wave] = total;
    __syncthreads();
    if (threadIdx.x == 0) P.tile_counts[t] = (wave_total[0] + wave_total[1]) + (wave_total[2] + wave_total[3]);
    __syncthreads();
  }
}

// exclusive prefix sum of tile_counts in place, kPointsScanThreads entries a round with the running total carried; then the counts
__global__ void __launch_bounds__(kPointsScanThreads) map_points_scan_kernel(const MapPointsParams P) {
  constexpr int kWaves = kPointsScanThreads / 64;
  __shared__ int wave_sum[kWaves];
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  int carry = 0;
  for (int base = 0; base < P.tiles; base += kPointsScanThreads) {
    const int t = base + (int)threadIdx.x;
    const int mine = t < P.tiles ? P.tile_counts[t] : 0;
    int incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const int s = wave_sum[w];
      if (w < wave) before += s;
      all += s;
    }
    if (t < P.tiles) P.tile_counts[t] = carry + before + (incl - mine);
    carry += all;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int kept = points_kept_below(carry, P.every);
    P.out_count[0] = kept < P.max_points ? kept : P.max_points;
    P.out_count[1] = kept;
  }
}

template <bool WHOLE>
__global__ void __launch_bounds__(256) map_points_scatter_kernel(const MapPointsParams P) {
#pragma clang fp contract(off)
  __shared__ int wave_total[4];
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int t = (int)blockIdx.x; t < P.tiles; t += (int)gridDim.x) {
    const int tile_rank = P.tile_counts[t];  // (the same for every lane: the tile is skipped or taken by the whole workgroup)
    // the first rank at or behind tile_rank that is kept has output index ceil(tile_rank / every): nothing of this tile is written
    if (points_kept_below(tile_rank, P.every) >= P.max_points) continue;
    unsigned long long mask[kPointsWaveIters];
    const int total = points_tile_ballots<WHOLE>(P, t, wave, lane, mask);
    if (lane == 0) wave_total[wave] = total;
    __syncthreads();
    int rank = tile_rank;
    for (int w = 0; w < wave; ++w) rank += wave_total[w];
    __syncthreads();
    const int first = t * kPointsTile + wave * kPointsWaveCells + lane;
#pragma unroll
    for (int i = 0; i < kPointsWaveIters; ++i) {
      if ((mask[i] >> lane) & 1ull) {
        const int r = rank + __popcll(mask[i] & below);
        const int j = r / P.every;
        if (j * P.every == r && j < P.max_points) {
          const int c = first + i * 64;
          const int row = c / P.w;
          const float x = (float)(P.x0 + (c - row * P.w)), y = (float)(P.y0 + row);
          float wx, wy;
          affine_apply(P.worldTmap, x, y, wx, wy);  // getWorldCoordsPose
          P.out[j] = make_float2(wx * P.scale, wy * P.scale);
        }
      }
      rank += __popcll(mask[i]);
    }
  }
}

}  // namespace hsm
