"""The staging plan of hsm_cast_scans (stage_layout.h: cast_scans_stage) on the CPU, held to its layout written out term by term
by tests/cpp/cast_stage_check.cpp -- with and without the optional hit array, whose region then has no bytes and no copies."""
import json
import subprocess

from support import INCLUDE, build_check


def test_cast_scans_stage_gives_the_written_out_sums(tmp_path):
    exe = build_check(tmp_path, "cast_stage_check.cpp", "-I", INCLUDE)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout)
    assert out["mismatches"] == 0 and out["cases"] > 2000
