// sigma_stats_check.cpp -- a HOST build of the sigma-point functions the two covariance kernels share
// (hector_slam_amd/csrc/gn_step.h: sigma_points, sigma_point_statistics), for tests/test_covariance_batch_abi.py: compiled as HIP for
// the host only, with the library's -ffp-contract=off.  Each input line holds 11 fp32 bit patterns in hex -- a map-frame pose
// (x, y, angle), the cell length and the seven sigma-point likelihoods -- and is answered by one line of 46 patterns: the sigma
// points [7][3], the map-frame covariance [9], the world-frame covariance [9] and the likelihoods as written out [7].
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "gn_step.h"

static float f32(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}
static uint32_t u32(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

int main() {
  uint32_t in[11];
  for (;;) {
    for (int i = 0; i < 11; ++i)
      if (scanf("%x", &in[i]) != 1) return 0;
    float sp[7][3], lh[7], out_lh7[7], cov_map[9], cov_world[9];
    for (int i = 0; i < 7; ++i) lh[i] = f32(in[4 + i]);
    hsm::sigma_points(f32(in[0]), f32(in[1]), f32(in[2]), sp);
    hsm::sigma_point_statistics(sp, lh, f32(in[3]), out_lh7, cov_map, cov_world);
    for (int i = 0; i < 7; ++i)
      for (int r = 0; r < 3; ++r) printf("%08x ", u32(sp[i][r]));
    for (int i = 0; i < 9; ++i) printf("%08x ", u32(cov_map[i]));
    for (int i = 0; i < 9; ++i) printf("%08x ", u32(cov_world[i]));
    for (int i = 0; i < 7; ++i) printf("%08x ", u32(out_lh7[i]));
    printf("\n");
  }
}
