// merge_box_check.cpp -- map_merge_box.h with the host compiler alone (tests/test_merge_map_abi.py): for the geometries and the
// transform on the command line, per level the fp32 constants the kernel receives (as bit patterns) and the two boxes, computed
// as map_copy.hip computes them from what hsm_create derives.  The test holds the lines to tests/merge_cases.py's model.
//   merge_box_check res dsx dsy dstart_x dstart_y ssx ssy sstart_x sstart_y levels tx ty theta
// (every real number an fp32 value printed exactly)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "map_merge_box.h"

using namespace hsm;

static unsigned int bits(float f) {
  unsigned int u;
  memcpy(&u, &f, sizeof u);
  return u;
}

int main(int argc, char** argv) {
  if (argc != 14) return 2;
  float res = (float)atof(argv[1]);
  int dsx = atoi(argv[2]), dsy = atoi(argv[3]);
  const float dstart[2] = {(float)atof(argv[4]), (float)atof(argv[5])};
  int ssx = atoi(argv[6]), ssy = atoi(argv[7]);
  const float sstart[2] = {(float)atof(argv[8]), (float)atof(argv[9])};
  const int levels = atoi(argv[10]);
  const float T[3] = {(float)atof(argv[11]), (float)atof(argv[12]), (float)atof(argv[13])};
  const double od[2] = {merge_map_offset(res, dsx, dstart[0]), merge_map_offset(res, dsy, dstart[1])};
  const double os[2] = {merge_map_offset(res, ssx, sstart[0]), merge_map_offset(res, ssy, sstart[1])};
  for (int l = 0; l < levels; ++l) {  // hsm_create: sizes halve, the cell length doubles, the scale is its fp32 inverse
    const MergeAffine a = merge_affine(od, os, 1.0f / res, T);
    const CopyBox b = merge_dst_box(a, dsx, dsy, ssx, ssy), s = merge_src_box(a, b, ssx, ssy);
    printf("%d %08x %08x %08x %08x %d %d %d %d %d %d %d %d\n", l, bits((float)a.c), bits((float)a.s), bits((float)a.bx), bits((float)a.by),
           b.x0, b.y0, b.x1, b.y1, s.x0, s.y0, s.x1, s.y1);
    dsx /= 2, dsy /= 2, ssx /= 2, ssy /= 2;
    res *= 2.0f;
  }
  return 0;
}
