"""The window move (hsm_shift_map, hsm_map_start): what can be checked without a GPU.

* both symbols are declared in capi.h, bound in capi.SIGNATURES with as many arguments, and exported by the built library; the
  header stays C99 and says what a graph captured before a move carries and what the move does not cover;
* a NULL context is HSM_ERR_INVALID from both, with the documented text (no device needed);
* the new unit is part of the build, with its kernels and its plan.
"""
import ctypes as C

from support import check_symbols, compile_c99, header_text

NEW_SYMBOLS = ("hsm_shift_map", "hsm_map_start")
HSM_ERR_INVALID = -1


def test_new_symbols_declared_bound_and_exported():
    from hector_slam_amd import build, capi
    check_symbols(NEW_SYMBOLS)
    head = header_text()
    assert "carries the old transforms in its kernel arguments" in head and "capture it again after the move" in head
    assert "1/64 cell" in head and "2^(levels - 1)" in head and "never accumulated" in head
    assert "group-wide move" in head and "C++ facade" in head and "hsm_slam_scans_device" in head
    for method in ("shift_map", "map_start", "start_for_shift"):
        assert callable(getattr(capi.MapRepMultiMap, method)), method
    unit = build.UNITS["map_shift.hip"]
    assert any(d.endswith("map_shift_kernels.h") for d in unit) and any(d.endswith("map_shift_plan.h") for d in unit)
    assert len(build.UNITS) == 14


def test_header_with_the_new_entries_is_plain_c99(tmp_path):
    compile_c99(tmp_path,
                "int main(void) { hsm_ctx* a = 0; int d[2] = {0, 0}; float s[2] = {0.0f, 0.0f};\n"
                "  int rc = hsm_shift_map(a, 0.5f, 0.5f, d);\n"
                "  rc += hsm_shift_map(a, 0.5f, 0.5f, 0);\n"
                "  rc += hsm_map_start(a, s);\n"
                "  return rc; }\n")


def test_null_context_is_invalid_for_both_entries():
    from hector_slam_amd import capi
    lib = capi.load_library()
    d = (C.c_int * 2)(7, 7)
    assert lib.hsm_shift_map(None, 0.5, 0.5, C.addressof(d)) == HSM_ERR_INVALID
    assert b"null context" in lib.hsm_last_error()
    assert (d[0], d[1]) == (7, 7)   # a refusal writes nothing
    assert lib.hsm_shift_map(None, float("nan"), 0.5, None) == HSM_ERR_INVALID
    import numpy as np
    s = np.full(2, 9.0, np.float32)
    assert lib.hsm_map_start(None, s) == HSM_ERR_INVALID
    assert b"null context" in lib.hsm_last_error()
    assert (s == 9.0).all()
