// Host build of hector_slam_amd/csrc/occupancy_rows.h for tests/test_occupancy_rows.py: the row split of occupancy_box_kernel
// against a byte-by-byte restatement.  For a grid `width` cells wide (argv[1]) and 8 rows (every phase of row_base % 4 that the
// width produces), every box row 0 <= x0 <= x1 < min(40, width):
//   * the split is run the way the kernel runs it -- occupancy_row_slots() slots per row, slot g < body_groups converts one
//     4-cell group, slot body_groups the head and the tail bytes -- on a plane of log-odds into a poisoned byte grid;
//   * the restatement walks the cells of [x0, x1] one by one.
// The two grids must be equal (so nothing outside the box is written and every cell inside is), every cell inside written exactly
// ONCE, every group aligned on the grid (flat index % 4 == 0) and inside the box, head and tail at most 3 cells.
// Prints "ok <rows checked>" and returns 0, or the first failure and 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "occupancy_rows.h"

static signed char restated(float l) {  // GridMapLogOdds.h:76-84 as publishMap reads it
  if (l < 0.0f) return 0;
  if (l > 0.0f) return 100;
  return -1;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const int width = atoi(argv[1]), rows = 8, xmax = width < 40 ? width : 40;
  if (width < 1) return 2;
  const int cells = width * rows;
  std::vector<float> lo(cells);
  const float values[7] = {-1.5f, 0.0f, 2.0f, -0.0f, 0.25f, -0.25f, 1e-30f};
  for (int i = 0; i < cells; ++i) lo[i] = values[(i * 5 + i / 7) % 7];
  long checked = 0;
  for (int y = 0; y < rows; ++y) {
    for (int x0 = 0; x0 < xmax; ++x0) {
      for (int x1 = x0; x1 < xmax; ++x1) {
        std::vector<signed char> got(cells, 55), want(cells, 55);
        std::vector<int> writes(cells, 0);
        for (int x = x0; x <= x1; ++x) want[y * width + x] = restated(lo[y * width + x]);
        const hsm::OccRowSplit r = hsm::occupancy_row_split(y * width, x0, x1);
        const int slots = hsm::occupancy_row_slots(x1 - x0 + 1);
        bool ok = r.head_n >= 0 && r.head_n <= 3 && r.tail_n >= 0 && r.tail_n <= 3 && r.body_groups >= 0 && r.body_groups < slots &&
                  (r.body0 & 3) == 0;
        for (int g = 0; ok && g < slots; ++g) {
          if (g < r.body_groups) {
            const int c = r.body0 + 4 * g;
            ok = (c & 3) == 0 && c >= y * width + x0 && c + 3 <= y * width + x1;
            for (int i = 0; ok && i < 4; ++i) {
              got[c + i] = hsm::occupancy_value(lo[c + i]);
              ++writes[c + i];
            }
          } else if (g == r.body_groups) {
            for (int i = 0; i < r.head_n; ++i) {
              const int c = r.head0 + i;
              if (c < 0 || c >= cells) { ok = false; break; }
              got[c] = hsm::occupancy_value(lo[c]);
              ++writes[c];
            }
            for (int i = 0; ok && i < r.tail_n; ++i) {
              const int c = r.tail0 + i;
              if (c < 0 || c >= cells) { ok = false; break; }
              got[c] = hsm::occupancy_value(lo[c]);
              ++writes[c];
            }
          }
        }
        for (int i = 0; ok && i < cells; ++i) {
          const bool inside = i >= y * width + x0 && i <= y * width + x1;
          ok = got[i] == want[i] && writes[i] == (inside ? 1 : 0);
        }
        if (!ok) {
          printf("FAIL width %d row %d x0 %d x1 %d: head %d+%d body %d x %d tail %d+%d\n", width, y, x0, x1, r.head0, r.head_n, r.body0,
                 r.body_groups, r.tail0, r.tail_n);
          return 1;
        }
        ++checked;
      }
    }
  }
  printf("ok %ld\n", checked);
  return 0;
}
