"""Occupied cells as a point set and the alignment of two maps (hsm_occupied_points*, hsm_align_map*): what can be checked
without a GPU.

* the five symbols are declared in capi.h, bound in capi.SIGNATURES with as many arguments, and exported by the built library; the
  header stays C99, states the rule and what is not built;
* the kernel header map_points_kernels.h is part of window.hip's build and of no other unit's, and no unit was added;
* HSM_MAX_ALIGN_POINTS is stated once, in capi.h, and the Python constants are the headers';
* the refusals that are decided before a context is read.

At the parent commit the symbol test fails: the entries do not exist.
"""
import ctypes as C
import os
import re

import numpy as np

from support import CSRC, check_symbols, compile_c99, header_code, header_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_SYMBOLS = ("hsm_occupied_points_device", "hsm_occupied_points", "hsm_align_map")
SIZE_SYMBOLS = ("hsm_occupied_points_workspace", "hsm_align_map_workspace")
HSM_ERR_INVALID = -1


def test_new_symbols_declared_bound_and_exported():
    from hector_slam_amd import capi
    check_symbols(INT_SYMBOLS)
    check_symbols(SIZE_SYMBOLS, restype=r"size_t")
    head = header_text()
    for phrase in ("r % every == 0", "THE ONE HOST WAIT", "contexts on different devices", "A device-resident count".lower(),
                   "free cells as points", "points weighted by log-odds", "the C++ facade"):
        assert phrase in head, phrase
    for name in ("occupied_points", "occupied_points_device", "occupied_points_workspace", "align_map_from", "align_map_workspace"):
        assert callable(getattr(capi.MapRepMultiMap, name)), name


def test_header_with_the_new_entries_is_plain_c99(tmp_path):
    compile_c99(tmp_path,
                "int main(void) { hsm_ctx* a = 0; hsm_ctx* b = 0; const float g[3] = {0.0f, 0.0f, 0.0f}; const int half[3] = {1, 1, 1};\n"
                "  const int box[4] = {0, 0, 9, 9}; float out[3], cov[9], lh, pts[2 * HSM_MAX_ALIGN_POINTS]; int counts[2], w;\n"
                "  size_t bytes = hsm_occupied_points_workspace(100) + hsm_align_map_workspace(100, 27, 4, HSM_MAX_ALIGN_POINTS);\n"
                "  int rc = hsm_occupied_points(a, 0, box, 1, HSM_MAX_ALIGN_POINTS, pts, counts);\n"
                "  rc += hsm_occupied_points_device(a, 0, 0, 1, 4, pts, counts, cov, bytes, 0);\n"
                "  rc += hsm_align_map(a, b, 0, box, 1, 4, 0, g, g, half, 4, out, cov, &lh, counts, &w);\n"
                "  return rc; }\n")


def test_kernel_header_is_window_hips_alone_and_no_unit_was_added():
    from hector_slam_amd import build
    assert len(build.UNITS) == 14
    for unit, deps in build.UNITS.items():
        names = {os.path.basename(d) for d in deps}
        assert ("map_points_kernels.h" in names) == (unit == "window.hip"), unit
    text = open(os.path.join(CSRC, "map_points_kernels.h")).read()
    for kernel in ("map_points_count_kernel", "map_points_scan_kernel", "map_points_scatter_kernel"):
        assert re.search(r"__global__[^;{]*\b%s\s*\(" % kernel, text), kernel
        assert kernel in open(os.path.join(CSRC, "window.hip")).read(), kernel
    assert "atomic" not in re.sub(r"//[^\n]*", "", text)   # the output index is a function of the map alone


def test_constants_are_stated_once():
    from hector_slam_amd import capi
    assert len(re.findall(r"#\s*define\s+HSM_MAX_ALIGN_POINTS\b", header_text())) == 1
    assert int(re.search(r"#\s*define\s+HSM_MAX_ALIGN_POINTS\s+(\d+)", header_code()).group(1)) == capi.MAX_ALIGN_POINTS == 16384
    for f in ("window.hip", "map_points_kernels.h", "stage_layout.h"):   # the sources name the macro, never the number
        assert "16384" not in open(os.path.join(CSRC, f)).read(), f
    tile = re.findall(r"constexpr int kPointsTile = (\d+);", open(os.path.join(CSRC, "map_points_kernels.h")).read())
    assert len(tile) == 1 and int(tile[0]) == capi.POINTS_TILE and capi.POINTS_TILE % 256 == 0


def test_refusals_decided_before_a_context_is_read():
    from hector_slam_amd import capi
    lib = capi.load_library()
    a = (C.c_char * 64)()   # an address that stands for a context; a refusal here does not follow it
    pa = C.addressof(a)
    g = np.zeros(3, np.float32)
    out = np.full(3, 7.0, np.float32)
    st, hf = (C.c_float * 3)(0.1, 0.1, 0.1), (C.c_int * 3)(1, 1, 1)
    cnt = np.full(2, 7, np.int32)

    def refused(rc, text):
        assert rc == HSM_ERR_INVALID and text in lib.hsm_last_error(), (rc, lib.hsm_last_error())

    refused(lib.hsm_occupied_points(None, 0, None, 1, 4, out.ctypes.data, cnt.ctypes.data), b"null context")
    refused(lib.hsm_occupied_points_device(None, 0, None, 1, 4, out.ctypes.data, cnt.ctypes.data, out.ctypes.data, 64, None),
            b"null context")
    args = (0, None, 1, 4, 0, g.ctypes.data, st, hf, 4, out.ctypes.data, None, None, cnt.ctypes.data, None)
    refused(lib.hsm_align_map(None, pa, *args), b"null context")
    refused(lib.hsm_align_map(pa, None, *args), b"null context")
    refused(lib.hsm_align_map(pa, pa, *args), b"same context")
    assert out.tolist() == [7.0] * 3 and cnt.tolist() == [7, 7] and bytes(a) == bytes(64)
