// map_copy_box.h -- the box arithmetic of a map copy between two contexts (map_copy.hip, map_copy_kernels.h), stated once: the
// box whose texels a copied cell box changes, how the box is cut into runs of contiguous cells and a run into slots, and where a
// cell lies in the staging patch of the cross-device route.
// Plain C++ (no HIP header): the kernels and the host compile the same text, and tests/cpp/copy_box_check.cpp holds it to a
// cell-by-cell restatement with the host compiler alone (tests/test_copy_box_model.py).
#pragma once
#include <stddef.h>

#include "occupancy_rows.h"

namespace hsm {

// cells [x0..x1] x [y0..y1] of a level, inclusive; empty where x1 < x0 or y1 < y0
struct CopyBox {
  int x0, y0, x1, y1;
};

HSM_OCC_HD inline bool copy_box_empty(const CopyBox& b) { return b.x1 < b.x0 || b.y1 < b.y0; }
// a box that is not empty lies inside a level of sx * sy cells
HSM_OCC_HD inline bool copy_box_inside(const CopyBox& b, int sx, int sy) {
  return b.x0 >= 0 && b.y0 >= 0 && b.x1 < sx && b.y1 < sy;
}
HSM_OCC_HD inline size_t copy_box_cells(const CopyBox& b) {
  return copy_box_empty(b) ? 0 : (size_t)(b.x1 - b.x0 + 1) * (size_t)(b.y1 - b.y0 + 1);
}

// Texel (x, y) holds P(x, y), P(x+1, y), P(x, y+1) and P(x+1, y+1) (the last column and row replicate the edge), so the cells of a
// box change the texels of the box grown by one cell towards lower x and y, clamped to the level.
HSM_OCC_HD inline CopyBox copy_texel_box(const CopyBox& b) {
  CopyBox t = b;
  if (t.x0 > 0) --t.x0;
  if (t.y0 > 0) --t.y0;
  return t;
}

// The cells of a box as `runs` runs of `len` cells that are contiguous in the level's planes: run r is the flat cell indices
// [first + r * step, first + r * step + len).  One run per box row -- or, where the box spans the level's whole width, ONE run of
// all its rows, which lie back to back in the plane.
struct CopyRuns {
  int first, len, runs, step;
};

HSM_OCC_HD inline CopyRuns copy_box_runs(int sx, const CopyBox& b) {
  const int w = b.x1 - b.x0 + 1, h = b.y1 - b.y0 + 1;
  CopyRuns r;
  if (b.x0 == 0 && w == sx) {
    r.first = b.y0 * sx;
    r.len = w * h;
    r.runs = 1;
    r.step = 0;
  } else {
    r.first = b.y0 * sx + b.x0;
    r.len = w;
    r.runs = h;
    r.step = sx;
  }
  return r;
}

// A run is cut like a row of the occupancy export (occupancy_rows.h): a body of 4-cell groups aligned on the destination GRID --
// 16-byte loads and stores of the 4-byte planes -- and a ragged head and tail of at most 3 cells each, copied cell by cell.
// Work slots of a run, the same for every run of a box: slot g < body_groups is group g, slot body_groups copies the head and
// the tail, the others idle.
HSM_OCC_HD inline OccRowSplit copy_run_split(const CopyRuns& r, int run) {
  return occupancy_row_split(r.first + run * r.step, 0, r.len - 1);
}
HSM_OCC_HD inline int copy_run_slots(const CopyRuns& r) { return occupancy_row_slots(r.len); }

// The staging patch holds the box's cells at pitch box-width: cell (x, y) at (y - y0) * w + (x - x0).  In runs: the cell at flat
// index c of run `run` sits at run * len + (c - first - run * step), for either kind of run.
HSM_OCC_HD inline int copy_patch_index(const CopyRuns& r, int run, int c) { return run * r.len + (c - r.first - run * r.step); }

// One patch per level and plane, in one block: the log-odds cells of the box, then its stamps, each padded to a multiple of
// four 4-byte elements so that every patch starts on a 16-byte boundary.  Offsets in elements from the block's start.
struct CopyPatch {
  size_t logodds, stamps, end;
};

HSM_OCC_HD inline CopyPatch copy_patch_at(size_t start, const CopyBox& b) {
  const size_t padded = (copy_box_cells(b) + 3) & ~(size_t)3;
  CopyPatch p;
  p.logodds = start;
  p.stamps = start + padded;
  p.end = start + 2 * padded;
  return p;
}

}  // namespace hsm
