// map_shift_plan.h -- the host-side plan of a window move (map_shift.hip: hsm_shift_map), stated once: from the start coordinates
// the geometry derives from now and the ones it shall derive from, the whole number of cells every level's contents move by, the
// box of cells that survive the move in old and in new cell coordinates, and whether the move is refused.
// Plain C++ (no HIP header): map_shift.hip and map_shift_kernels.h compile this text, and tests/cpp/shift_plan_check.cpp holds it
// to a numpy model with the host compiler alone (tests/test_shift_plan_model.py).
//
// The offsets are hsm_create's: off = (resolution * size) * start per axis, in fp32 (MapRepMultiMap.h:53-57).  They are always
// derived from the start coordinates, never accumulated, so a sequence of moves does not drift.  A world point's map
// coordinate on level l is scale_l * (world + off): a larger offset moves the CONTENTS towards higher cell indices,
// new(x, y) = old(x - d_l, y - d_l').
#pragma once
#include <math.h>

#include "map_copy_box.h"

namespace hsm {

constexpr int kShiftMaxLevels = 8;  // HSM_MAX_LEVELS (capi.h); map_shift.hip asserts it

enum ShiftRefusal {
  kShiftOk = 0,
  kShiftNonFinite = 1,    // a start coordinate, or the offset it gives, is no finite number
  kShiftFraction = 2,     // the move is further than 1/64 cell of level 0 from a whole number of cells
  kShiftNotMultiple = 3,  // level 0's displacement is no multiple of 2^(levels - 1): the coarsest level would move by a fraction
  kShiftTooFar = 4,       // the displacement does not fit an int (beyond 2^30 cells)
  kShiftBadGeometry = 5,  // not a geometry hsm_create accepts
};

struct ShiftLevel {
  int dx, dy;       // the level's displacement in its own cells: d_0 >> level, exactly
  CopyBox from;     // the surviving cells in OLD cell coordinates, empty where |d| reaches the level's extent
  CopyBox to;       // the same cells in NEW coordinates: from + (dx, dy)
};

struct ShiftPlan {
  int refusal;      // ShiftRefusal; the rest is only meaningful with kShiftOk
  int nlev;
  int d0[2];        // level 0's displacement
  float off[2];     // the new offsets, as hsm_create derives them
  bool moves;       // a displacement is not zero: cells move
  bool same_start;  // the new start coordinates are the old ones, bit for bit (then d0 = 0 and nothing at all changes)
  ShiftLevel lv[kShiftMaxLevels];
};

// hsm_create's offset of one axis (fp32, un-fused)
inline float shift_offset(float resolution, int size, float start) {
  const float total = resolution * (float)size;
  return total * start;
}

// the cells of an axis of `size` cells that survive a displacement d: new indices [lo, hi] (hi < lo: none)
inline void shift_axis_survivors(int size, int d, int& lo, int& hi) {
  lo = d > 0 ? d : 0;
  hi = d < 0 ? size - 1 + d : size - 1;
  if (d >= size || -d >= size) {
    lo = 0;
    hi = -1;
  }
}

inline ShiftPlan plan_map_shift(float resolution, int size_x, int size_y, int levels, const float old_start[2],
                                const float new_start[2]) {
  ShiftPlan P = {};
  P.nlev = levels;
  if (levels < 1 || levels > kShiftMaxLevels || size_x < 2 || size_y < 2 || !(resolution > 0.0f) || (size_x >> (levels - 1)) < 2 ||
      (size_y >> (levels - 1)) < 2) {
    P.refusal = kShiftBadGeometry;
    return P;
  }
  const int size[2] = {size_x, size_y};
  bool same = true;
  for (int a = 0; a < 2; ++a) {
    const float off_old = shift_offset(resolution, size[a], old_start[a]);
    const float off_new = shift_offset(resolution, size[a], new_start[a]);
    P.off[a] = off_new;
    if (!isfinite(new_start[a]) || !isfinite(off_new) || !isfinite(off_old)) {
      P.refusal = kShiftNonFinite;
      return P;
    }
    same = same && new_start[a] == old_start[a];
    const double q = ((double)off_new - (double)off_old) / (double)resolution;
    if (!(fabs(q) <= 1073741824.0)) {
      P.refusal = kShiftTooFar;
      return P;
    }
    const double d = floor(q + 0.5);
    if (fabs(q - d) > 1.0 / 64.0) {
      P.refusal = kShiftFraction;
      return P;
    }
    P.d0[a] = (int)d;
  }
  for (int a = 0; a < 2; ++a)
    if (P.d0[a] % (1 << (levels - 1)) != 0) {
      P.refusal = kShiftNotMultiple;
      return P;
    }
  P.same_start = same;
  P.moves = P.d0[0] != 0 || P.d0[1] != 0;
  for (int l = 0; l < levels; ++l) {
    ShiftLevel& L = P.lv[l];
    const int sx = size_x >> l, sy = size_y >> l;
    L.dx = P.d0[0] >> l;  // (a multiple of 2^l: the arithmetic shift is exact for negative values too)
    L.dy = P.d0[1] >> l;
    int x0, x1, y0, y1;
    shift_axis_survivors(sx, L.dx, x0, x1);
    shift_axis_survivors(sy, L.dy, y0, y1);
    if (x1 < x0 || y1 < y0) {
      L.to = CopyBox{0, 0, -1, -1};
      L.from = CopyBox{0, 0, -1, -1};
    } else {
      L.to = CopyBox{x0, y0, x1, y1};
      L.from = CopyBox{x0 - L.dx, y0 - L.dy, x1 - L.dx, y1 - L.dy};
    }
  }
  return P;
}

}  // namespace hsm
