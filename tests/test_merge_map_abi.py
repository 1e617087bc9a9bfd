"""A merge of two pyramids under a rigid transform (hsm_merge_map, hsm_merge_map_box): what can be checked without a GPU.

* both symbols are declared in capi.h, bound in capi.SIGNATURES with as many arguments, and exported by the built library; the
  header stays C99 and says which route has not been run; the kernel header is part of map_copy.hip's build and of no other unit's;
* the host arithmetic behind hsm_merge_map_box (hector_slam_amd/csrc/map_merge_box.h, compiled by tests/cpp/merge_box_check.cpp with
  the host compiler alone, a context needs a device) gives the model's box on every level of every case of tests/merge_cases.py,
  and the model's fp32 constants bit for bit;
* the refusals that are decided before a context is read: a NULL context, a NULL transform, dst == src, a component that is not
  finite (the contexts there are addresses that are never followed).  The refusals that need two real contexts -- geometries that
  differ, a capturing stream -- and hsm_merge_map_box itself on real contexts are in tests/test_gpu_merge_map.py.

At the parent commit the symbol test fails: the entries do not exist.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import merge_cases as mc
import newer_entry_cases as nc
from support import check_symbols, compile_c99, header_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("hsm_merge_map", "hsm_merge_map_box")
HSM_ERR_INVALID = -1
F = np.float32


def test_new_symbols_declared_bound_and_exported():
    from hector_slam_amd import build, capi
    check_symbols(NEW_SYMBOLS)
    head = header_text()
    assert "fminf(d + v, 50.0f)" in head and "HSM_COPY_STAGE=1" in head
    assert "the cross-device merge itself has not been run" in head
    assert callable(capi.merge_map) and callable(capi.merge_map_box)
    for unit, deps in build.UNITS.items():
        names = {os.path.basename(d) for d in deps}
        assert ("map_merge_kernels.h" in names) == (unit == "map_copy.hip"), unit
        assert ("map_merge_box.h" in names) == (unit == "map_copy.hip"), unit


def test_header_with_the_new_entries_is_plain_c99(tmp_path):
    compile_c99(tmp_path,
                "int main(void) { hsm_ctx* a = 0; hsm_ctx* b = 0; const float t[3] = {0.0f, 0.0f, 0.0f}; int box[4];\n"
                "  int rc = hsm_merge_map(a, b, t);\n"
                "  rc += hsm_merge_map_box(a, b, t, 0, box);\n"
                "  return rc; }\n")


def test_box_header_is_plain_cpp():
    from hector_slam_amd import build
    closure = build._closure(os.path.join(ROOT, "hector_slam_amd", "csrc", "map_merge_box.h"), [])
    assert {os.path.basename(p) for p in closure} == {"map_merge_box.h", "map_copy_box.h", "occupancy_rows.h"}
    for path in closure:
        assert "hip_runtime" not in open(path).read(), path


# ---- the box and the constants ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def box_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("merge_box") / "merge_box_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(ROOT, "hector_slam_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "merge_box_check.cpp"), "-o", str(exe)], check=True)
    return exe


def _exact(v):
    return repr(float(F(v)))


# merge_cases' pairs and those of tests/newer_entry_cases.py: a start outside [0, 1], the far frame, 6 and 8 levels, the strip
HOST_CASES = [mc.PAIRS[pair] + (t,) for pair, _, t in mc.CASES] + [nc.PAIRS[pair] + (nc.transform(pair, name),) for pair, name in nc.MERGE_CASES]
HOST_IDS = mc.CASE_IDS + nc.MERGE_IDS


@pytest.mark.parametrize("gd,gs,t", HOST_CASES, ids=HOST_IDS)
def test_host_arithmetic_gives_the_models_box_and_constants(box_check, gd, gs, t):
    assert gd[0] == gs[0] and gd[3] == gs[3]
    args = [_exact(gd[0]), str(gd[1]), str(gd[2]), _exact(gd[4][0]), _exact(gd[4][1]), str(gs[1]), str(gs[2]), _exact(gs[4][0]),
            _exact(gs[4][1]), str(gd[3])] + [_exact(v) for v in t]
    r = subprocess.run([str(box_check)] + args, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == gd[3]
    for lvl, line in enumerate(lines):
        w = line.split()
        assert int(w[0]) == lvl
        consts = [int(x, 16) for x in w[1:5]]
        want = [int(F(v).view(np.uint32)) for v in mc.affine(gd, gs, lvl, t)]
        assert consts == want, (lvl, "c, s, bx, by", consts, want)
        assert tuple(int(x) for x in w[5:9]) == mc.merge_box(gd, gs, lvl, t), (lvl, "box")
        assert tuple(int(x) for x in w[9:13]) == mc.merge_src_box(gd, gs, lvl, t), (lvl, "src box")


# ---- refusals that read no context ---------------------------------------------------------------------------------------------------
def test_refusals_decided_before_a_context_is_read():
    from hector_slam_amd import capi
    lib = capi.load_library()
    a, b = (C.c_char * 64)(), (C.c_char * 64)()   # two addresses that stand for contexts; a refusal here follows neither
    pa, pb = C.addressof(a), C.addressof(b)
    ok = F([0.1, 0.2, 0.3])
    box = np.full(4, 7, np.int32)

    def refused(rc, text):
        assert rc == HSM_ERR_INVALID and text in lib.hsm_last_error(), (rc, lib.hsm_last_error())

    for dst, src in ((None, pb), (pa, None), (None, None)):
        refused(lib.hsm_merge_map(dst, src, ok.ctypes.data), b"null context")
        refused(lib.hsm_merge_map_box(dst, src, ok.ctypes.data, 0, box.ctypes.data), b"null context")
    refused(lib.hsm_merge_map(pa, pb, None), b"src_in_dst is null")
    refused(lib.hsm_merge_map_box(pa, pb, None, 0, box.ctypes.data), b"src_in_dst is null")
    refused(lib.hsm_merge_map(pa, pa, ok.ctypes.data), b"same context")
    refused(lib.hsm_merge_map_box(pa, pa, ok.ctypes.data, 0, box.ctypes.data), b"same context")
    for k in range(3):
        for bad in (np.nan, np.inf, -np.inf):
            t = ok.copy()
            t[k] = bad
            refused(lib.hsm_merge_map(pa, pb, t.ctypes.data), b"not finite")
            refused(lib.hsm_merge_map_box(pa, pb, t.ctypes.data, 0, box.ctypes.data), b"not finite")
    assert box.tolist() == [7, 7, 7, 7] and bytes(a) == bytes(64) and bytes(b) == bytes(64)
