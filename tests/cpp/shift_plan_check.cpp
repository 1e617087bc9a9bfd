// shift_plan_check.cpp -- hector_slam_amd/csrc/map_shift_plan.h with the host compiler alone (tests/test_shift_plan_model.py).
// Reads one plan request per line from standard input,
//   <resolution bits> <size_x> <size_y> <levels> <old start x bits> <old start y bits> <new start x bits> <new start y bits>
// (the floats as the decimal value of their 32 bits, so that nothing is rounded on the way), and prints per request one line:
//   <refusal> [<d0 x> <d0 y> <moves> <same_start> <new offset x bits> <new offset y bits> then per level <dx> <dy> <from box> <to box>]
// The test holds every line to its numpy model.
#include <stdio.h>
#include <string.h>

#include "map_shift_plan.h"

static float from_bits(unsigned int u) {
  float f;
  memcpy(&f, &u, sizeof f);
  return f;
}

static unsigned int to_bits(float f) {
  unsigned int u;
  memcpy(&u, &f, sizeof u);
  return u;
}

int main() {
  unsigned int res, osx, osy, nsx, nsy;
  int sx, sy, levels;
  long lines = 0;
  while (scanf("%u %d %d %d %u %u %u %u", &res, &sx, &sy, &levels, &osx, &osy, &nsx, &nsy) == 8) {
    const float old_start[2] = {from_bits(osx), from_bits(osy)}, new_start[2] = {from_bits(nsx), from_bits(nsy)};
    const hsm::ShiftPlan P = hsm::plan_map_shift(from_bits(res), sx, sy, levels, old_start, new_start);
    printf("%d", P.refusal);
    if (P.refusal == hsm::kShiftOk) {
      printf(" %d %d %d %d %u %u", P.d0[0], P.d0[1], P.moves ? 1 : 0, P.same_start ? 1 : 0, to_bits(P.off[0]), to_bits(P.off[1]));
      for (int l = 0; l < P.nlev; ++l) {
        const hsm::ShiftLevel& L = P.lv[l];
        printf(" %d %d %d %d %d %d %d %d %d %d", L.dx, L.dy, L.from.x0, L.from.y0, L.from.x1, L.from.y1, L.to.x0, L.to.y0, L.to.x1,
               L.to.y1);
      }
    }
    printf("\n");
    ++lines;
  }
  fprintf(stderr, "%ld plans\n", lines);
  return 0;
}
