"""The box arithmetic of a map copy between contexts (hector_slam_amd/csrc/map_copy_box.h: the runs of a box, the slots of a run,
the texel box, the staging patch) on the CPU: tests/cpp/copy_box_check.cpp compiles the header with the host compiler alone and
holds it to a cell-by-cell restatement for every box of three row ranges on levels 25, 38 and 40 cells wide -- an odd width, an
even one that is no multiple of 4, and a multiple of 4, so every phase of a run's first cell against the 4-cell alignment
occurs, boxes that touch x = 0 and y = 0 included, and whole-width boxes, which are one run.  Equality of planes: no tolerance."""
import subprocess

import pytest

from support import build_check


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return build_check(tmp_path_factory.mktemp("copy_box"), "copy_box_check.cpp")


@pytest.mark.parametrize("width", [25, 38, 40])
def test_box_arithmetic_equals_the_cell_by_cell_restatement(model, width):
    r = subprocess.run([str(model), str(width)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    row_ranges = 9 + 8 + 5  # y0 = 0, 1, 4 on 9 rows
    assert r.stdout.split() == ["ok", str(row_ranges * width * (width + 1) // 2)], r.stdout  # every box was checked
