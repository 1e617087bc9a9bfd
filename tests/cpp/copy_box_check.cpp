// Host build of hector_slam_amd/csrc/map_copy_box.h for tests/test_copy_box_model.py: the box arithmetic of a map copy against a
// cell-by-cell restatement.  For a level `width` cells wide (argv[1]) and 9 rows, every box 0 <= x0 <= x1 < width,
// 0 <= y0 <= y1 < 9 with y0 in {0, 1, 4} (a box on the level's first row, on its second, in its middle):
//   * the slots are run the way map_copy_cells_kernel runs them -- copy_box_runs() runs, copy_run_slots() slots per run, slot
//     g < body_groups copies one 4-cell group, slot body_groups the head and the tail -- from a patch filled at pitch box-width
//     through copy_patch_index() into a poisoned plane; the restatement walks the box's cells one by one.  The planes must be
//     equal (nothing outside the box is written), every box cell written exactly ONCE, every group aligned on the grid (flat
//     index % 4 == 0) and inside its run, every patch index inside the patch;
//   * copy_texel_box() must be exactly the set of texels whose four cells (x..x+1, y..y+1, clamped to the level) touch the box.
// Then the patch offsets of a one-cell box, a one-row box, a one-column box and the whole level.
// Prints "ok <boxes checked>" and returns 0, or the first failure and 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "map_copy_box.h"

using namespace hsm;

static int fail(const char* what, int width, const CopyBox& b) {
  printf("FAIL %s: width %d box %d %d %d %d\n", what, width, b.x0, b.y0, b.x1, b.y1);
  return 1;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const int width = atoi(argv[1]), rows = 9;
  if (width < 2) return 2;
  const int cells = width * rows;
  std::vector<int> src(cells);
  for (int i = 0; i < cells; ++i) src[i] = 1000 + i;
  long checked = 0;
  const int y0s[3] = {0, 1, 4};
  for (int yi = 0; yi < 3; ++yi) {
    const int y0 = y0s[yi];
    for (int y1 = y0; y1 < rows; ++y1) {
      for (int x0 = 0; x0 < width; ++x0) {
        for (int x1 = x0; x1 < width; ++x1) {
          const CopyBox b{x0, y0, x1, y1};
          if (copy_box_empty(b) || !copy_box_inside(b, width, rows)) return fail("box test", width, b);
          const int w = x1 - x0 + 1, h = y1 - y0 + 1;
          if (copy_box_cells(b) != (size_t)w * h) return fail("cell count", width, b);
          // the patch, as the row copies fill it
          std::vector<int> patch((size_t)w * h);
          for (int y = y0; y <= y1; ++y)
            for (int x = x0; x <= x1; ++x) patch[(size_t)(y - y0) * w + (x - x0)] = src[y * width + x];
          std::vector<int> got(cells, -7), want(cells, -7), writes(cells, 0);
          for (int y = y0; y <= y1; ++y)
            for (int x = x0; x <= x1; ++x) want[y * width + x] = src[y * width + x];
          const CopyRuns R = copy_box_runs(width, b);
          if ((long)R.runs * R.len != (long)w * h) return fail("runs", width, b);
          const int slots = copy_run_slots(R);
          for (int run = 0; run < R.runs; ++run) {
            const OccRowSplit r = copy_run_split(R, run);
            const int lo = R.first + run * R.step, hi = lo + R.len;  // [lo, hi)
            if (r.head_n < 0 || r.head_n > 3 || r.tail_n < 0 || r.tail_n > 3 || r.body_groups < 0 || r.body_groups >= slots)
              return fail("split", width, b);
            auto put = [&](int c) -> bool {
              if (c < lo || c >= hi) return false;
              const int p = copy_patch_index(R, run, c);
              if (p < 0 || p >= w * h) return false;
              got[c] = patch[p];
              ++writes[c];
              return true;
            };
            for (int g = 0; g < slots; ++g) {
              if (g < r.body_groups) {
                const int c = r.body0 + 4 * g;
                if ((c & 3) != 0) return fail("group alignment", width, b);
                for (int i = 0; i < 4; ++i)
                  if (!put(c + i)) return fail("group outside its run", width, b);
                if (copy_patch_index(R, run, c + 3) != copy_patch_index(R, run, c) + 3) return fail("group not contiguous in the patch", width, b);
              } else if (g == r.body_groups) {
                for (int i = 0; i < r.head_n; ++i)
                  if (!put(r.head0 + i)) return fail("head", width, b);
                for (int i = 0; i < r.tail_n; ++i)
                  if (!put(r.tail0 + i)) return fail("tail", width, b);
              }
            }
          }
          for (int i = 0; i < cells; ++i) {
            const int x = i % width, y = i / width;
            const bool inside = x >= x0 && x <= x1 && y >= y0 && y <= y1;
            if (got[i] != want[i] || writes[i] != (inside ? 1 : 0)) return fail("cells", width, b);
          }
          // the texels a box changes
          const CopyBox T = copy_texel_box(b);
          for (int y = 0; y < rows; ++y)
            for (int x = 0; x < width; ++x) {
              const int xn = x + 1 < width ? x + 1 : x, yn = y + 1 < rows ? y + 1 : y;
              auto in = [&](int cx, int cy) { return cx >= x0 && cx <= x1 && cy >= y0 && cy <= y1; };
              const bool touched = in(x, y) || in(xn, y) || in(x, yn) || in(xn, yn);
              const bool grown = x >= T.x0 && x <= T.x1 && y >= T.y0 && y <= T.y1;
              if (touched != grown) return fail("texel box", width, b);
            }
          if (T.x0 < 0 || T.y0 < 0 || T.x0 != (x0 > 0 ? x0 - 1 : 0) || T.y0 != (y0 > 0 ? y0 - 1 : 0) || T.x1 != x1 || T.y1 != y1)
            return fail("texel box clamp", width, b);
          ++checked;
        }
      }
    }
  }
  // patch offsets: log-odds first, stamps behind them, both on 16-byte boundaries, levels back to back
  struct Case {
    CopyBox b;
    size_t cells;
  };
  const Case cases[4] = {{{3, 2, 3, 2}, 1}, {{1, 5, width - 2, 5}, (size_t)width - 2}, {{width - 1, 0, width - 1, rows - 1}, (size_t)rows},
                         {{0, 0, width - 1, rows - 1}, (size_t)cells}};
  size_t at = 0;
  for (const Case& c : cases) {
    const CopyPatch p = copy_patch_at(at, c.b);
    const size_t padded = (c.cells + 3) / 4 * 4;
    if (p.logodds != at || p.stamps != at + padded || p.end != at + 2 * padded || (p.logodds & 3) || (p.stamps & 3) || (p.end & 3))
      return fail("patch offsets", width, c.b);
    const CopyRuns R = copy_box_runs(width, c.b);
    const int w = c.b.x1 - c.b.x0 + 1;
    for (int run = 0; run < R.runs; ++run)
      for (int i = 0; i < R.len; ++i) {
        const int cflat = R.first + run * R.step + i, x = cflat % width, y = cflat / width;
        if (copy_patch_index(R, run, cflat) != (y - c.b.y0) * w + (x - c.b.x0)) return fail("patch index", width, c.b);
      }
    at = p.end;
  }
  const CopyPatch e = copy_patch_at(8, CopyBox{0, 0, -1, -1});
  if (e.logodds != 8 || e.stamps != 8 || e.end != 8 || copy_box_cells(CopyBox{5, 5, 4, 9}) != 0) return fail("empty box", width, CopyBox{0, 0, -1, -1});
  printf("ok %ld\n", checked);
  return 0;
}
