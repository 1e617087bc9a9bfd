// map_merge_box.h -- the host arithmetic of a merge of two pyramids under a rigid transform (map_copy.hip: hsm_merge_map,
// hsm_merge_map_box), stated once and in double: the affine that takes a cell of the destination's level into the source's map
// coordinates, the box of destination cells the merge visits, and the box of source cells those map back to (what the staged route
// copies).  include/hector_mi355/capi.h states the rule.
// Plain C++ (no HIP header): tests/cpp/merge_box_check.cpp compiles it with the host compiler alone, and tests/test_merge_map_abi.py
// holds it to the numpy model of tests/merge_cases.py.  Built without contraction (-ffp-contract=off): every product and sum
// below is one rounded double operation, as the model's are.
#pragma once
#include <math.h>

#include "map_copy_box.h"

namespace hsm {

// the source's map coordinates of the destination's cell (x, y), on one level: (c x + s y + bx, -s x + c y + by)
struct MergeAffine {
  double c, s, bx, by;
};

// hsm_create's offset of one axis in fp32, (resolution * size) * start, widened
inline double merge_map_offset(float resolution, int size, float start) { return (double)((resolution * (float)size) * start); }

// T = (tx, ty, theta): the pose of the source's world frame in the destination's, p_dst = R(theta) p_src + t.  A world point p of a
// context sits at scale * (p + off) in its map coordinates, so b = scale * (R(-theta) (-off_dst - t) + off_src)
inline MergeAffine merge_affine(const double off_dst[2], const double off_src[2], float scale_to_map, const float T[3]) {
  MergeAffine a;
  a.c = cos((double)T[2]);
  a.s = sin((double)T[2]);
  const double scale = (double)scale_to_map;
  const double ux = -off_dst[0] - (double)T[0], uy = -off_dst[1] - (double)T[1];
  a.bx = scale * ((a.c * ux + a.s * uy) + off_src[0]);
  a.by = scale * ((-a.s * ux + a.c * uy) + off_src[1]);
  return a;
}

// the bounding box of four points, from floor of the least to ceil of the greatest coordinate, grown by one cell on every side and
// clamped to a level of sx * sy cells; {0, 0, -1, -1} where it misses the level.  (Clamped as doubles: a far translation does not
// fit an int.)
inline CopyBox merge_grown_bounds(const double px[4], const double py[4], int sx, int sy) {
  double lo[2] = {px[0], py[0]}, hi[2] = {px[0], py[0]};
  for (int k = 1; k < 4; ++k) {
    lo[0] = fmin(lo[0], px[k]), hi[0] = fmax(hi[0], px[k]);
    lo[1] = fmin(lo[1], py[k]), hi[1] = fmax(hi[1], py[k]);
  }
  const double x0 = fmax(floor(lo[0]) - 1.0, 0.0), x1 = fmin(ceil(hi[0]) + 1.0, (double)(sx - 1));
  const double y0 = fmax(floor(lo[1]) - 1.0, 0.0), y1 = fmin(ceil(hi[1]) + 1.0, (double)(sy - 1));
  if (!(x0 <= x1 && y0 <= y1)) return CopyBox{0, 0, -1, -1};
  return CopyBox{(int)x0, (int)y0, (int)x1, (int)y1};
}

// the cells of the destination's level (dsx * dsy) the merge visits: the corners of the source's level rectangle
// [-0.5, ssx - 0.5] x [-0.5, ssy - 0.5] through the inverse affine
inline CopyBox merge_dst_box(const MergeAffine& a, int dsx, int dsy, int ssx, int ssy) {
  double px[4], py[4];
  for (int k = 0; k < 4; ++k) {
    const double qx = ((k & 1) ? (double)ssx - 0.5 : -0.5) - a.bx, qy = ((k & 2) ? (double)ssy - 0.5 : -0.5) - a.by;
    px[k] = a.c * qx - a.s * qy;
    py[k] = a.s * qx + a.c * qy;
  }
  return merge_grown_bounds(px, py, dsx, dsy);
}

// the cells of the source's level that the cells of `box` map back to: the same construction the other way round.  The kernel's
// fp32 coordinates differ from these by far less than the cell the box is grown by.
inline CopyBox merge_src_box(const MergeAffine& a, const CopyBox& box, int ssx, int ssy) {
  if (copy_box_empty(box)) return CopyBox{0, 0, -1, -1};
  double px[4], py[4];
  for (int k = 0; k < 4; ++k) {
    const double x = (k & 1) ? (double)box.x1 + 0.5 : (double)box.x0 - 0.5, y = (k & 2) ? (double)box.y1 + 0.5 : (double)box.y0 - 0.5;
    px[k] = (a.c * x + a.s * y) + a.bx;
    py[k] = (-a.s * x + a.c * y) + a.by;
  }
  return merge_grown_bounds(px, py, ssx, ssy);
}

}  // namespace hsm
