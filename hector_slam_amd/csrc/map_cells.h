// map_cells.h -- what every kernel that walks a level's cells shares: the read-write view of a level, the tilings of its key and
// mark planes, the cell probability, the empty cell box, and the closed form of a Bresenham line.  No kernel is defined here:
// update_types.h (map_update.hip), probe_kernels.h (probes.hip), ray_kernels.h (rays.hip) and occupancy_kernels.h (occupancy.hip)
// all include it.
#pragma once
#include <hip/hip_runtime.h>

#include "libm_exact.h"

namespace hsm {

// read-write view of one level for the update path
struct LevelRW {
  float* logodds;         // LogOddsCell::logOddsVal plane
  int* update_index;      // LogOddsCell::updateIndex plane
  float* prob;            // p = e^l / (e^l + 1)
  float4* quad;           // {P(x,y), P(x+1,y), P(x,y+1), P(x+1,y+1)}
  unsigned int* key_free; // first free-touching beam of the current scan
  unsigned int* key_occ;  // first end-cell beam of the current scan
  unsigned int* occ_bits; // 1 bit per cell: "some beam of the current scan ends here" (set in pass 1a, cleared in pass 2)
  unsigned char* free_bytes; // dense scans: 1 byte per cell "some beam of the current scan crosses this cell", in tiles of 16 x 8
                             // cells (index = mark_index: a tile is one 128-byte line); set by update_mark_free_dense_kernel,
                             // cleared by the dense apply pass
  int sx, sy;
  int tiles_x, quad_texels;  // tiled texel plane geometry (beam_sample.h quad_index)
  int kf_tiles_x;            // free-key tiles per row = key_free_tiles_x(sx): ceil(sx / 64) * 8   (key_free_index)
};

// The free-key plane is stored in 8x4-cell tiles (= one 128-byte line).  The line walk (mark_free_block)
// writes one 4-byte key per visited cell: row major, a y-major beam touches a new cache line every step and an
// x-major one every 32 steps; tiled, both touch a new line every 4..8 steps, and the lanes of a wave (64
// consecutive steps of one beam) share lines either way.
// tiles per tile row, padded to whole 64-cell BLOCKS (8 tiles): the dense apply pass owns the marks of a 64 x 4-cell block as
// 256 CONTIGUOUS bytes, so the last block of a row must not run into the next tile row -- with the padding the dense form
// works for every map width (round 4; until then rows had to be a multiple of 64 cells)
__host__ __device__ __forceinline__ int key_free_tiles_x(int sx) { return ((sx + 63) / 64) * 8; }
__host__ __device__ __forceinline__ size_t key_free_cells(int sx, int sy) {
  return (size_t)key_free_tiles_x(sx) * (size_t)((sy + 3) / 4) * 32u;
}
__device__ __forceinline__ unsigned int key_free_index(const LevelRW& L, unsigned int x, unsigned int y) {
  return ((((y >> 2) * (unsigned int)L.kf_tiles_x) + (x >> 3)) << 5) | ((y & 3u) << 3) | (x & 7u);
}

// The mark BYTES of the dense form (free_bytes): tiles of 16 x 8 cells = one 128-byte line each.  The 64 steps of a line-walk
// iteration cross about (dx / 16 + dy / 8 + 1) lines -- ~10 averaged over the beam directions of a 360-degree scan -- and the
// line walk is bound by exactly these scattered byte accesses (profiles/r04/README.md 5).  The apply pass owns 32 x 8-cell
// blocks (two tiles = 256 contiguous mark bytes, its plane accesses two 128-byte row segments per wavefront).  (Measured
// against the free-key plane's 8 x 4 tiling, where a line of bytes is 32 x 4 cells and an iteration crosses ~14.5 lines:
// profiles/r04/README.md 20.)
__host__ __device__ __forceinline__ int mark_tiles_x(int sx) { return ((sx + 31) / 32) * 2; }  // 16-cell tiles per row, whole 32-cell blocks
__host__ __device__ __forceinline__ size_t mark_bytes(int sx, int sy) {
  return (size_t)mark_tiles_x(sx) * (size_t)((sy + 7) / 8) * 128u;
}
// One byte per 16 x 8 mark TILE behind the mark bytes: "a beam of the current scan ends in this tile" (set by the end-cell pass,
// cleared by the apply pass).  Without it the line walk has to read every mark byte before storing to it -- to learn whether a
// beam ends in the cell (then the keyed atomicMax decides the revert artefact), and to skip marks already set; that load, ~10
// lines of a 67 MB plane per iteration, was a third of the walk.  So it reads the TILE's byte -- a 128 x smaller, cache-resident
// map, 1-4 lines per iteration -- and only in the ~1/6 of the tiles where it is set the cell's own byte; everywhere else it
// stores its mark unread (an already set mark is stored again: same value).
// configs[4]: line walk 57.5 -> 50.0 us, update 0.135 -> 0.127 ms (profiles/r04/README.md 21).
__host__ __device__ __forceinline__ size_t mark_tile_end_offset(int sx, int sy) { return mark_bytes(sx, sy) + 256; }
__host__ __device__ __forceinline__ size_t mark_plane_bytes(int sx, int sy) {
  return mark_bytes(sx, sy) + 256 + ((mark_bytes(sx, sy) / 128 + 3) & ~(size_t)3) + 256;
}
__device__ __forceinline__ unsigned int mark_index(const LevelRW& L, unsigned int x, unsigned int y) {
  return ((((y >> 3) * (unsigned int)mark_tiles_x(L.sx)) + (x >> 4)) << 7) | ((y & 7u) << 4) | (x & 15u);
}

// Key = (generation of the scan << kBeamBits) | (kBeamMask - beam index): atomicMax keeps the newest scan and, within
// it, the LOWEST beam index.  20 bits of beam index (scans of up to 1 048 575 beams; the reference has no limit, and
// neither has any sensor), 12 bits of generation: the key planes are cleared once every 4095 updates of a level.
constexpr unsigned int kBeamBits = 20;
constexpr unsigned int kBeamMask = (1u << kBeamBits) - 1u;
constexpr unsigned int kSerialMax = (1u << (32 - kBeamBits)) - 1u;

// GridMapLogOddsFunctions::getGridProbability (GridMapLogOdds.h:163-166): exp(float) is glibc's expf
// there; libm_exact.h reproduces it bit for bit
__device__ __forceinline__ float grid_probability(float log_odds) {
  const float odds = libm::expf_glibc(log_odds);
  return odds / (odds + 1.0f);
}

// A cell box on the device: {x0, y0, x1, y1}, inclusive; empty = {INT_MAX, INT_MAX, -1, -1}, the identity of the atomics.
constexpr int kBoxEmptyLo = 0x7fffffff, kBoxEmptyHi = -1;

struct BeamLine {
  bool valid;
  int x1, y1;
  unsigned int abs_da, abs_db;
  int offset_a, offset_b;
  unsigned int e0;
  unsigned int start;
  bool x_major;  // the major (per-step) axis is x
};

// cell visited at Bresenham step i (0 = start cell), closed form of bresenham2D (:243-260):
// after i major steps the error accumulator has crossed abs_da floor((e0 + i*db)/da) times.
__device__ __forceinline__ unsigned int line_cell(const BeamLine& b, unsigned int i) {
  const unsigned int minor = (b.e0 + i * b.abs_db) / b.abs_da;
  return b.start + (unsigned int)((int)i * b.offset_a) + (unsigned int)((int)minor * b.offset_b);
}

}  // namespace hsm
