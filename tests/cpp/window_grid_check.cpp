// Prints what hector_slam_amd/csrc/window_grid.h computes, compiled with the host compiler alone (tests/test_window_model.py):
//   window_grid_check poses hx hy ht sx sy st cx cy ct   -> per window index "w i j k index(i,j,k) bits(x) bits(y) bits(t)"
//   window_grid_check count hx hy ht                     -> window_count
//   window_grid_check topk count k                       -> topk_workspace_bytes, topk_slices
//   window_grid_check reloc W k                          -> the RelocalizeLayout offsets and total
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "window_grid.h"

static unsigned bits(float f) {
  unsigned u;
  memcpy(&u, &f, 4);
  return u;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (!strcmp(argv[1], "poses") && argc == 11) {
    hsm::WindowGrid g = {atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), strtof(argv[5], 0), strtof(argv[6], 0), strtof(argv[7], 0)};
    const float cx = strtof(argv[8], 0), cy = strtof(argv[9], 0), ct = strtof(argv[10], 0);
    const long long W = hsm::window_count(g.hx, g.hy, g.ht);
    for (int w = 0; w < (int)W; ++w) {
      int i, j, k;
      hsm::window_ijk(g, w, i, j, k);
      float x, y, t;
      hsm::window_pose(g, cx, cy, ct, w, x, y, t);
      printf("%d %d %d %d %d %u %u %u\n", w, i, j, k, hsm::window_index(g, i, j, k), bits(x), bits(y), bits(t));
    }
    return 0;
  }
  if (!strcmp(argv[1], "count") && argc == 5) {
    printf("%lld\n", hsm::window_count(atoi(argv[2]), atoi(argv[3]), atoi(argv[4])));
    return 0;
  }
  if (!strcmp(argv[1], "topk") && argc == 4) {
    printf("%zu %d\n", hsm::topk_workspace_bytes(atoi(argv[2]), atoi(argv[3])), hsm::topk_slices(atoi(argv[2])));
    return 0;
  }
  if (!strcmp(argv[1], "reloc") && argc == 4) {
    const hsm::RelocalizeLayout L = hsm::relocalize_layout(atoll(argv[2]), atoi(argv[3]));
    printf("%zu %zu %zu %zu %zu %zu\n", L.scores, L.topk, L.index, L.kscore, L.pose, L.total);
    return 0;
  }
  return 2;
}
