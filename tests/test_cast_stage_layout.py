"""The staging plan of hsm_cast_scans (stage_layout.h: cast_scans_stage) on the CPU, held to its layout written out term by term
by tests/cpp/cast_stage_check.cpp -- with and without the optional hit array, whose region then has no bytes and no copies."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cast_scans_stage_gives_the_written_out_sums(tmp_path):
    exe = tmp_path / "cast_stage_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "hector_slam_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "cast_stage_check.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout)
    assert out["mismatches"] == 0 and out["cases"] > 2000
