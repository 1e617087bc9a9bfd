"""Sigma-point covariances of batched matches on the device (hsm_covariance_batch_device, hsm_match_cov_batch_device,
hsm_covariance_batch): what can be checked without a GPU.

* the three symbols are declared in capi.h, bound in capi.SIGNATURES with as many arguments and exported by the built library; the
  header stays C99;
* a NULL context is HSM_ERR_INVALID from each entry (no device needed);
* covariance_batch_kernel is in the code object for both layouts and both summation orders, without scratch, with 7 x 64 x 4 B of
  LDS per wavefront in the reference order and none in the tree order;
* the facade method compiles against the include tree it drops into;
* the staging plan of the host form gives the written-out sums (tests/cpp/covariance_stage_check.cpp);
* the statistics function that the probe's kernel and the new one share (gn_step.h sigma_point_statistics), built for the host, gives
  the bits of the scalar fp32 restatement sigma_statistics_f32 of tests/test_node_rows.py.
"""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from support import build_check,check_symbols, compile_c99, header_text
from test_node_rows import sigma_statistics_f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hector_slam_amd", "csrc")
NEW_SYMBOLS = ("hsm_covariance_batch_device", "hsm_match_cov_batch_device", "hsm_covariance_batch")
HSM_ERR_INVALID = -1


def test_new_symbols_declared_bound_and_exported():
    from hector_slam_amd import capi
    head = header_text()
    check_symbols(NEW_SYMBOLS)
    for name in NEW_SYMBOLS:
        # each declaration carries its citation: the comment right in front of it has a "replaces:" line
        comment = re.findall(r"/\*(.*?)\*/\s*int\s+" + name + r"\s*\(", head, re.S)[-1].rsplit("/*", 1)[-1]
        assert "replaces:" in comment, name
    assert "OccGridMapUtil.h:106-160" in head and "ScanMatcher.h:134-147" in head
    for meth in ("covariance_batch_device", "match_cov_batch_device", "covariance_batch"):
        assert callable(getattr(capi.MapRepMultiMap, meth)), meth


def test_header_with_the_new_entries_is_plain_c99(tmp_path):
    compile_c99(tmp_path,
                "int main(void) { hsm_ctx* h = 0; int idx[1] = {0}; float f[9] = {0.0f};\n"
                "  int rc = hsm_covariance_batch_device(h, 0, 1, f, f, 0, 1, f, f, f, f, 0);\n"
                "  rc += hsm_match_cov_batch_device(h, 1, f, f, 0, 1, f, 0, 0, f, f, f, f, 1, 0, 1, idx, f, f, 0);\n"
                "  rc += hsm_covariance_batch(h, 0, 1, f, f, 0, 1, f, f, f, f);\n"
                "  return rc; }\n")


def test_null_context_is_invalid_for_every_new_entry():
    from hector_slam_amd import capi
    lib = capi.load_library()
    f = (C.c_float * 16)()
    i = (C.c_int * 4)()
    fp, ip = C.addressof(f), C.addressof(i)
    assert lib.hsm_covariance_batch_device(None, 0, 1, fp, fp, None, 1, fp, fp, fp, fp, None) == HSM_ERR_INVALID
    assert b"null context" in lib.hsm_last_error() and b"hsm_covariance_batch_device" in lib.hsm_last_error()
    assert lib.hsm_match_cov_batch_device(None, 1, fp, fp, None, 1, fp, None, 0, fp, fp, fp, fp, 1, None, 1, ip, fp, fp,
                                          None) == HSM_ERR_INVALID
    assert b"null context" in lib.hsm_last_error() and b"hsm_match_cov_batch_device" in lib.hsm_last_error()
    assert lib.hsm_covariance_batch(None, 0, 1, fp, fp, None, 1, fp, fp, fp, fp) == HSM_ERR_INVALID
    assert b"null context" in lib.hsm_last_error() and b"hsm_covariance_batch" in lib.hsm_last_error()


def test_kernel_is_in_the_code_object_without_scratch():
    from hector_slam_amd import build
    from test_kernel_resources import kernels
    if build.hipcc_path() is None:
        pytest.skip("hipcc not found")
    ks = {k: v for k, v in kernels(build.device_asm()).items() if "covariance_batch_kernel" in k}
    assert len(ks) == 4, sorted(ks)  # 2 layouts x 2 orders
    forms = set()
    for k, v in ks.items():
        lay, exact = re.search(r"covariance_batch_kernelILi(\d)ELb([01])E", k).groups()
        forms.add((lay, exact))
        assert v["scratch"] == 0, (k, v)
        assert v["vgpr"] <= 128, (k, v)  # four wavefronts per SIMD, as launched
        assert v["lds"] == (4 * 7 * 64 * 4 if exact == "1" else 0), (k, v)  # four wavefronts of seven rows; the tree order has none
    assert forms == {("1", "0"), ("1", "1"), ("2", "0"), ("2", "1")}


def test_kernel_and_statistics_live_where_the_include_graph_wants_them():
    score = open(os.path.join(CSRC, "score_kernels.h")).read()
    assert re.search(r"__global__[^;{]*\bcovariance_batch_kernel\s*\(", score)
    step = open(os.path.join(CSRC, "gn_step.h")).read()
    assert re.search(r"\bsigma_point_statistics\s*\([^;{]*\)\s*\{", step)
    # one copy of the statistics: both kernels call it, neither restates it
    for name in ("score_kernels.h", "probe_kernels.h"):
        text = open(os.path.join(CSRC, name)).read()
        assert "sigma_point_statistics(" in text and "invLhNormalizer" not in text, name


def test_facade_covariance_batch_compiles():
    """include/hector_slam_lib/slam_main/MapRepMultiMap.h::getCovarianceForPosesBatch against the include tree it drops into
    (present where the reference-compiled checkers were built)"""
    overlay = os.path.join(ROOT, "oracle", "_ref", "overlay", "hector_slam_lib")
    if not os.path.exists(os.path.join(overlay, "slam_main", "HectorSlamProcessor.h")):
        pytest.skip("oracle/_ref/overlay not built (needs the reference include tree)")
    subprocess.run(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-Wno-sign-compare",
                    "-Wno-unused-variable", "-Wno-delete-non-virtual-dtor", "-Wno-unused-function", "-fsyntax-only",
                    "-I", os.path.join(ROOT, "oracle", "stubs"), "-I", overlay, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "facade_cov_check.cpp")], check=True)


def test_staging_plan_gives_the_written_out_sums(tmp_path):
    exe = build_check(tmp_path, "covariance_stage_check.cpp", "-I", os.path.join(ROOT, "include"))
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert r.returncode == 0 and rec["mismatches"] == 0, (rec, r.stderr[-2000:])
    assert rec["cases"] > 50000, rec  # the grid did run


# ---- the shared statistics function, built for the host -------------------------------------------------------------------------
def statistics_cases():
    """(map-frame pose, cell length, seven likelihoods)"""
    rng = np.random.default_rng(2601)
    F = np.float32
    cases = [((F(256.3), F(255.1), F(0.4)), F(0.05), np.full(7, 0.37, F)),                      # all entries equal
             ((F(100.5), F(7.25), F(-3.1)), F(0.1), F([0.31, 0.0, 0.29, 0.33, 0.30, 0.28, 0.35])),  # one of them zero
             ((F(1.0), F(510.0), F(3.0)), F(0.025), F([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.2])),      # only the pose sees the map
             ((F(64.0), F(64.0), F(0.0)), F(0.2), F([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]))]
    for _ in range(12):
        pose = (rng.uniform(0, 512, 2).tolist() + [rng.uniform(-3.2, 3.2)])
        cases.append((tuple(F(v) for v in pose), F(rng.choice([0.025, 0.05, 0.1, 0.2])), rng.uniform(0.01, 0.9, 7).astype(F)))
    return cases


def world_from_map(cov, cell):
    """getCovMatrixWorldCoords (:162-188) in scalar fp32: the translation block by cell^2, the mixed terms by cell"""
    c, sq = np.float32(cell), np.float32(cell) * np.float32(cell)
    w = np.empty(9, np.float32)
    w[0], w[4], w[1] = cov[0] * sq, cov[4] * sq, cov[1] * sq
    w[3] = w[1]
    w[2] = cov[2] * c
    w[6] = w[2]
    w[5] = cov[5] * c
    w[7] = w[5]
    w[8] = cov[8]
    return w


def test_shared_statistics_function_gives_the_restatements_bits(tmp_path):
    from hector_slam_amd import build
    hipcc = build.hipcc_path()
    if hipcc is None:
        pytest.skip("hipcc not found")
    exe = tmp_path / "sigma_stats_check"
    subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, "-I",
                    os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "sigma_stats_check.cpp"), "-o", str(exe)],
                   check=True)
    cases = statistics_cases()
    text = "\n".join(" ".join("%08x" % v for v in np.concatenate([np.float32(p), [c], lh]).astype(np.float32).view(np.uint32))
                     for p, c, lh in cases)
    r = subprocess.run([str(exe)], input=text + "\n", capture_output=True, text=True, check=True)
    rows = [np.array([int(w, 16) for w in line.split()], np.uint32) for line in r.stdout.strip().splitlines()]
    assert len(rows) == len(cases)
    F = np.float32
    for (pose, cell, lh), row in zip(cases, rows):
        assert row.size == 46
        x, y, a = pose
        sp = F([[x + F(1.5), y, a], [x - F(1.5), y, a], [x, y + F(1.5), a], [x, y - F(1.5), a], [x, y, a + F(0.05)],
                [x, y, a - F(0.05)], [x, y, a]])
        assert np.array_equal(row[:21], sp.reshape(-1).view(np.uint32)), pose
        with np.errstate(all="ignore"):
            want = sigma_statistics_f32(pose, lh)
            world = world_from_map(want, cell)
        assert np.array_equal(row[21:30], want.view(np.uint32)), (pose, lh)
        assert np.array_equal(row[30:39], world.view(np.uint32)), (pose, lh)
        assert np.array_equal(row[39:46], lh.view(np.uint32)), (pose, lh)
        cov = row[21:30].view(np.float32).reshape(3, 3)
        assert np.isfinite(cov).all() and np.array_equal(cov, cov.T)
