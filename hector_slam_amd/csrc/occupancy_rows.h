// occupancy_rows.h -- how occupancy_box_kernel (occupancy_kernels.h) cuts one row of a cell box into a ragged head, a body of 4-cell
// groups and a ragged tail, and publishMap's rule for one cell.  The groups are aligned on the GRID: a group starts at a flat
// cell index (y * sx + x) that is a multiple of 4, where a 16-byte load of the log-odds plane and a 4-byte store into the byte
// grid are aligned -- whatever column the box starts at, and on levels whose width is no multiple of 4 (the phase then changes
// from row to row).
// Plain C++ (no HIP header): the kernel and the host compile the same text, and tests/cpp/occupancy_rows_check.cpp holds it to a
// byte-by-byte restatement with the host compiler alone (tests/test_occupancy_rows.py).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HSM_OCC_HD __host__ __device__
#else
#define HSM_OCC_HD
#endif

namespace hsm {

// LogOddsCell::isFree / isOccupied as publishMap reads them (GridMapLogOdds.h:76-84, HectorMappingRos.cpp:449-468):
// 0 free (logOdds < 0), 100 occupied (logOdds > 0), -1 unknown -- a log-odds of +-0 and a NaN compare false both times
HSM_OCC_HD inline signed char occupancy_value(float logodds) {
  return logodds < 0.0f ? (signed char)0 : (logodds > 0.0f ? (signed char)100 : (signed char)-1);
}

// One row of a box, in flat cell indices: cells [head0, head0 + head_n) and [tail0, tail0 + tail_n) are written byte by byte,
// group g of the body is cells [body0 + 4 g, body0 + 4 g + 4) with body0 % 4 == 0.  The three pieces are disjoint and cover
// the row's cells of the box exactly; head_n and tail_n are at most 3.
struct OccRowSplit {
  int head0, head_n;
  int body0, body_groups;
  int tail0, tail_n;
};

// the split of columns [x0, x1] (inclusive, x0 <= x1) of the row that starts at flat index row_base = y * sx
HSM_OCC_HD inline OccRowSplit occupancy_row_split(int row_base, int x0, int x1) {
  const int s = row_base + x0, e = row_base + x1 + 1;  // [s, e)
  const int a0 = (s + 3) & ~3, a1 = e & ~3;            // the aligned indices at or behind s, at or in front of e
  OccRowSplit r;
  r.head0 = s;
  if (a0 > a1) {  // s and e inside one group: at most 2 cells, all of them the head
    r.head_n = e - s;
    r.body0 = a0;
    r.body_groups = 0;
    r.tail0 = e;
    r.tail_n = 0;
  } else {
    r.head_n = a0 - s;
    r.body0 = a0;
    r.body_groups = (a1 - a0) >> 2;
    r.tail0 = a1;
    r.tail_n = e - a1;
  }
  return r;
}

// Work slots of one row of a box `w` cells wide, the same for every row whatever its phase: slot g < body_groups is group g,
// slot body_groups writes the head and the tail, the others idle.  (A body holds at most w / 4 whole groups.)
HSM_OCC_HD inline int occupancy_row_slots(int w) { return w / 4 + 1; }

}  // namespace hsm
