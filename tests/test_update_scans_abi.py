"""hsm_update_by_scans_device / hsm_update_by_scans without a GPU: the ABI is declared, bound and exported, and the one libm
call the device-side preparation makes differently from the host path -- one sincosf instead of sinf and cosf -- gives the same
floats (csrc/libm_exact.h compiled with g++, against the host libm).
"""
import json
import os
import re
import subprocess

from support import header_code

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ("hsm_update_by_scans_device", "hsm_update_by_scans")


def test_update_by_scans_entries_are_declared_bound_and_exported():
    from hector_slam_amd import build, capi
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\b(hsm_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", header_code(), re.S)}
    for name in NEW:
        assert name in decl, f"{name} is not declared in capi.h"
        assert name in capi.SIGNATURES, f"{name} is not bound in capi.py"
        n_args = len([a for a in decl[name].split(",") if a.strip()])
        assert len(capi.SIGNATURES[name][1]) == n_args, (name, n_args, capi.SIGNATURES[name][1])
    assert len(capi.SIGNATURES["hsm_update_by_scans_device"][1]) == 9  # h, count, poses, pts, offsets, shared_n, max_beams, origo, stream
    assert len(capi.SIGNATURES["hsm_update_by_scans"][1]) == 7
    build.build_native()
    lib = capi.load_library()
    for name in NEW:
        assert hasattr(lib, name), name
    for name in ("update_by_scans_device", "update_by_scans"):
        assert callable(getattr(capi.MapRepMultiMap, name, None)), name
    # the update kernels are not templates: one unit includes their headers (and the gate's and the cell rule's behind them), and
    # no other
    own = {"map_update.h", "map_update_scans.h", "update_types.h", "update_cell_rule.h", "update_gate.h"}
    assert own <= {os.path.basename(d) for d in build.UNITS["map_update.hip"]}
    for unit, deps in build.UNITS.items():
        assert unit == "map_update.hip" or not own & {os.path.basename(d) for d in deps}, unit


def _cpu_has_fma():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("flags"):
                f = line.split()
                return "fma" in f and "avx2" in f
    except OSError:
        pass
    return False


def test_sincosf_pair_equals_separate_host_sinf_and_cosf(tmp_path):
    """prepare_level() calls sinf(theta) and cosf(theta); update_prep_kernel calls libm::sincosf_glibc(theta) once"""
    assert _cpu_has_fma(), "host CPU without FMA/AVX2: glibc uses its unfused sinf / cosf variants; parity would be unpinned"
    exe = tmp_path / "sincos_pair_check"
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-pthread", os.path.join(HERE, "cpp", "sincos_pair_check.cpp"),
                    "-o", str(exe), "-lm"], check=True)
    stride = os.environ.get("HSM_LIBM_SWEEP_STRIDE", "61")  # the sampling of tests/test_libm_model.py
    r = subprocess.run([str(exe), stride], capture_output=True, text=True)
    out = json.loads(r.stdout)
    assert out["mismatches"] == 0, out
    assert out["checked"] >= (1 << 32) // int(stride)
    assert out["boundary_checked"] >= 2 * 8193 * 10
    assert r.returncode == 0
