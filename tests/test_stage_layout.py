"""The arithmetic of the host runtime's staging blocks (hector_slam_amd/csrc/stage_layout.h: the 256-byte round-up, the carver of
aligned regions, the growth rule of the grow-on-demand buffers, the workspace layout behind hsm_match_batch_ranges_workspace and the
blocks of hsm_match_batch / hsm_match_score_batch) against the sums written out term by term, on the CPU:
tests/cpp/stage_layout_check.cpp restates them literally and compares every offset and every capacity over a grid of sizes --
batch or n of 0 and 1, sizes one byte either side of a 256-byte multiple, n = HSM_MAX_UPDATE_BEAMS, refused batch * n > INT_MAX.
Exact comparison, no tolerance."""
import json
import subprocess

from support import INCLUDE, build_check


def test_header_gives_the_written_out_sums(tmp_path):
    exe = build_check(tmp_path, "stage_layout_check.cpp", "-I", INCLUDE)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert r.returncode == 0 and rec["mismatches"] == 0, (rec, r.stderr[-2000:])
    assert rec["cases"] > 1000000, rec  # the grid did run
