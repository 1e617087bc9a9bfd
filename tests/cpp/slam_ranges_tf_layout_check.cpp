// Host build of hector_slam_amd/csrc/stage_layout.h for tests/test_origos_abi.py: the workspace layout of
// hsm_slam_ranges_tf_device for the (count, n) pairs on the command line, one line each:
//   ok counts offsets origos pts total
#include <cstdio>
#include <cstdlib>

#include "stage_layout.h"

int main(int argc, char** argv) {
  for (int i = 1; i + 1 < argc; i += 2) {
    hsm_host::SlamRangesTfLayout L = {0, 0, 0, 0, 0};
    const bool ok = hsm_host::slam_ranges_tf_layout(atoi(argv[i]), atoi(argv[i + 1]), &L);
    printf("%d %zu %zu %zu %zu %zu\n", ok ? 1 : 0, L.counts, L.offsets, L.origos, L.pts, L.total);
  }
  return 0;
}
