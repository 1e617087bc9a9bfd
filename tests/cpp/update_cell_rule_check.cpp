// Host build of hector_slam_amd/csrc/update_cell_rule.h for tests/test_update_cell_rule_model.py: the rule on a file of cells,
// as raw little-endian records.
//   update_cell_rule_check <in> <out>
//     in:  N x {float32 log-odds, int32 stamp, int32 first crossing beam, int32 first ending beam, int32 n, int32 mark_free,
//               float32 f, float32 o, int32 stamped}      (a beam index of n: no beam crosses / ends here; mark_occ = mark_free + 1)
//     out: N x {int32 written, float32 log-odds, int32 stamp}      (an unwritten cell keeps what it came with)
#include <cstdio>
#include <cstring>
#include <vector>

#include "update_cell_rule.h"

struct Record {
  float logodds;
  int stamp, first_free, first_occ, n, mark_free;
  float f, o;
  int stamped;
};
static_assert(sizeof(Record) == 36, "Record: nine 4-byte fields");

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  Record r;
  while (fread(&r, sizeof r, 1, in) == 1) {
    const bool occ = r.first_occ < r.n, fre = r.first_free < r.n;
    const unsigned int bo = (unsigned int)r.first_occ, bf = (unsigned int)r.first_free;
    const int F = r.mark_free, O = r.mark_free + 1;
    const hsm::CellUpdate u = r.stamped ? hsm::update_cell_rule<true>(r.logodds, r.stamp, occ, fre, bo, bf, r.f, r.o, F, O)
                                        : hsm::update_cell_rule<false>(r.logodds, r.stamp, occ, fre, bo, bf, r.f, r.o, F, O);
    const int written = u.written ? 1 : 0, stamp = u.written ? u.stamp : r.stamp;
    const float logodds = u.written ? u.logodds : r.logodds;
    fwrite(&written, sizeof written, 1, out);
    fwrite(&logodds, sizeof logodds, 1, out);
    fwrite(&stamp, sizeof stamp, 1, out);
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 1;
}
