// Prints what hector_slam_amd/csrc/window_grid.h and stage_layout.h compute for the batched relocalisation, compiled with the
// host compiler alone (tests/test_relocalize_batch_abi.py):
//   relocalize_batch_check topk groups group_size k    -> TopKGroupsLayout "cand_score cand_index total", topk_slices(group_size)
//   relocalize_batch_check reloc B W k total_points    -> the RelocalizeBatchLayout offsets and total
//   relocalize_batch_check stage B k points ws cov idx score csr -> the RelocalizeBatchStage offsets, total and region count
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "stage_layout.h"
#include "window_grid.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (!strcmp(argv[1], "topk") && argc == 5) {
    const hsm::TopKGroupsLayout L = hsm::topk_groups_layout(atoll(argv[2]), atoll(argv[3]), atoi(argv[4]));
    printf("%zu %zu %zu %d\n", L.cand_score, L.cand_index, L.total, hsm::topk_slices(atoi(argv[3])));
    return 0;
  }
  if (!strcmp(argv[1], "reloc") && argc == 6) {
    const hsm::RelocalizeBatchLayout L = hsm::relocalize_batch_layout(atoll(argv[2]), atoll(argv[3]), atoi(argv[4]), atoll(argv[5]));
    printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", L.scores, L.topk, L.index, L.kscore, L.pose, L.offsets, L.pts, L.total);
    return 0;
  }
  if (!strcmp(argv[1], "stage") && argc == 10) {
    static float f[1];
    static int i[1];
    const bool cov = atoi(argv[6]), idx = atoi(argv[7]), score = atoi(argv[8]), csr = atoi(argv[9]);
    const hsm_host::RelocalizeBatchStage s = hsm_host::relocalize_batch_stage(
        atoi(argv[2]), atoi(argv[3]), (size_t)atoll(argv[4]), (size_t)atoll(argv[5]), f, f, csr ? i : nullptr, f, cov ? f : nullptr, f,
        idx ? i : nullptr, f, score ? f : nullptr, i);
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d\n", s.centers, s.pts, s.offs, s.ws, s.pose, s.cov, s.lh, s.cidx, s.bpose,
           s.bscore, s.bidx, s.plan.total(), s.plan.n);
    return 0;
  }
  return 2;
}
