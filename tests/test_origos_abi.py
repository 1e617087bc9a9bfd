"""The per-scan origo entries (hsm_update_by_scans_device_origos, hsm_update_by_scans_device_gated_origos,
hsm_slam_scans_device_origos) and the one-call raw-log entries (hsm_slam_ranges_tf_device, hsm_slam_ranges_tf_workspace,
hsm_slam_ranges_tf) without a GPU: declared, bound and exported with matching argument counts; the parents keep their
signatures; what can be refused without a device is refused with its outputs untouched; the workspace size is the sum of its
256-byte aligned parts (csrc/stage_layout.h compiled with the host compiler) and 0 for the sizes the entry refuses.  The
argument checks that need a context run in tests/test_gpu_slam_ranges_tf.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from support import build_check, header_code, header_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HSM_OK, HSM_ERR_INVALID = 0, -1
HSM_MAX_UPDATE_BEAMS = 1048575
NEW = {"hsm_update_by_scans_device_origos": 9, "hsm_update_by_scans_device_gated_origos": 11, "hsm_slam_scans_device_origos": 13,
       "hsm_slam_ranges_tf_device": 26, "hsm_slam_ranges_tf_workspace": 2, "hsm_slam_ranges_tf": 24}
PARENTS = {"hsm_update_by_scans_device": 9, "hsm_update_by_scans_device_gated": 11, "hsm_slam_scans_device": 13,
           "hsm_ingest_batch_ranges_tf_device": 21}
METHODS = ("update_by_scans_device_origos", "update_by_scans_device_gated_origos", "slam_scans_device_origos",
           "slam_ranges_tf_device", "slam_ranges_tf_workspace", "slam_ranges_tf")


def declarations():
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(hsm_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", header_code(), re.S)}


def test_entries_are_declared_bound_and_exported():
    from hector_slam_amd import build, capi
    decl = declarations()
    build.build_native()
    lib = capi.load_library()
    for name, n_args in {**NEW, **PARENTS}.items():
        assert name in decl, f"{name} is not declared in capi.h"
        assert name in capi.SIGNATURES, f"{name} is not bound in capi.py"
        assert len([a for a in decl[name].split(",") if a.strip()]) == n_args == len(capi.SIGNATURES[name][1]), name
        assert hasattr(lib, name), name
    # the origo is a device pointer in the new entries and stays the host pair in the parents
    for name in ("hsm_update_by_scans_device", "hsm_update_by_scans_device_gated", "hsm_slam_scans_device"):
        assert re.search(r"const float origo\[2\]", decl[name]) and re.search(r"const float\* d_origos", decl[name + "_origos"])
    for name in METHODS:
        assert callable(getattr(capi.MapRepMultiMap, name, None)), name


def test_header_says_what_is_left():
    src = header_text()
    assert "Not built: per-scan origos" not in src and "splits the log" not in src
    for word in ("capture into graphs", "hsm_group_*", "byte-map (dense) form", "non-tf conversion", "facade"):
        assert word in src[src.index("hsm_slam_scans_device_origos on what it wrote"):src.index("int hsm_slam_ranges_tf_device(")], word


def test_refusals_without_a_device_leave_the_outputs_untouched():
    from hector_slam_amd import capi
    lib = capi.load_library()
    pose, cov = np.full((4, 3), -9.0, np.float32), np.full((4, 9), -9.0, np.float32)
    applied, counts, origo = np.full(4, -9, np.int32), np.full(4, -9, np.int32), np.full((4, 2), -9.0, np.float32)
    ranges, tf = np.ones((4, 8), np.float32), np.tile(np.eye(3, 4).reshape(12), (4, 1))
    p = lambda a: a.ctypes.data  # noqa: E731
    geom = (8, -1.0, 0.25, 0.1, 30.0, 30.0)
    gates = (0, 0.16, 900.0, -1.0, 1.0, 20.0)
    rc = lib.hsm_slam_ranges_tf(None, 4, None, None, p(ranges), *geom, p(tf), *gates, None, p(pose), p(cov), p(applied), p(counts), p(origo))
    assert rc == HSM_ERR_INVALID and b"null context" in lib.hsm_last_error()
    ws = np.full(1 << 16, 0x5A, np.uint8)
    rc = lib.hsm_slam_ranges_tf_device(None, 4, None, None, p(ranges), *geom, p(tf), *gates, None, p(pose), p(cov), p(applied), p(counts),
                                       p(ws), ws.size, None)
    assert rc == HSM_ERR_INVALID
    for name, args in (("hsm_update_by_scans_device_origos", (None, 4, p(pose), p(ranges), None, 8, 8, p(origo), None)),
                       ("hsm_update_by_scans_device_gated_origos", (None, 4, p(pose), p(ranges), None, 8, 8, p(origo), None, p(applied), None)),
                       ("hsm_slam_scans_device_origos", (None, 4, None, None, p(ranges), p(counts), 8, p(origo), None, p(pose), p(cov),
                                                         p(applied), None))):
        assert getattr(lib, name)(*args) == HSM_ERR_INVALID, name
    assert (pose == -9.0).all() and (cov == -9.0).all() and (applied == -9).all() and (counts == -9).all() and (origo == -9.0).all()
    assert (ws == 0x5A).all()


def test_workspace_is_the_sum_of_its_parts(tmp_path):
    from hector_slam_amd import capi
    lib = capi.load_library()
    exe = build_check(tmp_path, "slam_ranges_tf_layout_check.cpp", "-I", os.path.join(ROOT, "include"))
    sizes = [(1, 1), (24, 1081), (256, 1081), (63, 64), (64, 63), (65, 65), (7, 0), (0, 181), (0, 0), (1, HSM_MAX_UPDATE_BEAMS),
             (2048, HSM_MAX_UPDATE_BEAMS), (-1, 181), (4, -1), (1, HSM_MAX_UPDATE_BEAMS + 1), (4096, HSM_MAX_UPDATE_BEAMS)]
    out = subprocess.run([str(exe)] + [str(v) for s in sizes for v in s], capture_output=True, text=True, check=True).stdout.split("\n")
    align = lambda b: (b + 255) // 256 * 256  # noqa: E731
    refused = 0
    for (count, n), line in zip(sizes, out):
        ok, o_counts, o_offs, o_origos, o_pts, total = (int(v) for v in line.split())
        got = int(lib.hsm_slam_ranges_tf_workspace(count, n))
        assert got == capi.MapRepMultiMap.slam_ranges_tf_workspace(count, n)
        if count < 0 or n < 0 or n > HSM_MAX_UPDATE_BEAMS or count * n > 2 ** 31 - 1:
            assert not ok and got == 0, (count, n, got)
            refused += 1
            continue
        # counts[count] | offsets[count + 1] | origos[count * 2] | endpoints[max(count * n, 1) * 2], each 256-byte aligned
        parts = [4 * count, 4 * (count + 1), 8 * count, 8 * max(count * n, 1)]
        assert ok and (o_counts, o_offs) == (0, align(parts[0])), (count, n)
        assert o_origos == o_offs + align(parts[1]) and o_pts == o_origos + align(parts[2]), (count, n)
        assert got == total == sum(align(b) for b in parts) and got > 0, (count, n, got, total)
    assert refused == 4
