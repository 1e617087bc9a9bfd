"""Expected scans cast on the device-resident map (hsm_ray_distances_device, hsm_cast_scans_device, hsm_cast_scans): what can
be checked without a GPU.

* every new symbol is declared in capi.h, bound in capi.SIGNATURES with as many arguments, and exported by the built library;
  the header stays C99 and says what a ray without a hit is;
* a NULL context is HSM_ERR_INVALID from each new entry (no device needed);
* the new unit is part of the build, and the fp32 restatement of a beam's ray (tests/cast_cases.py) is the arithmetic the header
  states.
"""
import ctypes as C

import numpy as np

import cast_cases
from support import check_symbols, compile_c99, header_text

NEW_SYMBOLS = ("hsm_ray_distances_device", "hsm_cast_scans_device", "hsm_cast_scans")
HSM_ERR_INVALID = -1


def test_new_symbols_declared_bound_and_exported():
    from hector_slam_amd import build, capi
    check_symbols(NEW_SYMBOLS)
    head = header_text()
    assert "5000 steps" in head and "either end point outside the level" in head and "non-finite" in head
    for meth in ("cast_scans", "cast_scans_device", "ray_distances_device"):
        assert callable(getattr(capi.MapRepMultiMap, meth)), meth
    assert "rays.hip" in build.UNITS and any(d.endswith("ray_kernels.h") for d in build.UNITS["rays.hip"])


def test_header_with_the_new_entries_is_plain_c99(tmp_path):
    compile_c99(tmp_path,
                "int main(void) { hsm_ctx* h = 0; float f[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};\n"
                "  int rc = hsm_ray_distances_device(h, 0, 0.0f, 0.0f, 0.05f, 1, f, f, f, 0, 0);\n"
                "  rc += hsm_cast_scans_device(h, 0, 1, f, f, 1, 30.0f, f, 0, 0);\n"
                "  rc += hsm_cast_scans(h, 0, 1, f, f, 1, 30.0f, f, f);\n"
                "  return rc; }\n")


def test_null_context_is_invalid_for_every_new_entry():
    from hector_slam_amd import capi
    lib = capi.load_library()
    f = (C.c_float * 16)()
    fp = C.addressof(f)
    assert lib.hsm_cast_scans_device(None, 0, 1, fp, fp, 1, 30.0, fp, fp, None) == HSM_ERR_INVALID
    assert b"null context" in lib.hsm_last_error()
    assert lib.hsm_ray_distances_device(None, 0, 0.0, 0.0, 0.05, 1, fp, fp, fp, fp, None) == HSM_ERR_INVALID
    assert lib.hsm_cast_scans(None, 0, 1, fp, fp, 1, 30.0, fp, fp) == HSM_ERR_INVALID
    assert b"null context" in lib.hsm_last_error()


def test_ray_restatement_is_the_stated_arithmetic(oracle_mod):
    """hand-checked against float64: each operation of the recipe rounds once to fp32, in the stated order"""
    p = np.array([[1.25, -2.5, 0.3], [0.1, 0.2, -3.0]], np.float32)
    ang = cast_cases.beam_table(65)
    begin, end = cast_cases.cast_rays(p, ang, 8.0)
    assert begin.shape == end.shape == (2 * 65, 2) and begin.dtype == end.dtype == np.float32
    for b in range(2):
        for i in (0, 1, 7, 30, 64):
            a = np.float32(p[b, 2] + ang[i])
            s, c = (v[0] for v in oracle_mod.libm_sincosf(np.array([a], np.float32)))
            want = (np.float32(p[b, 0] + np.float32(np.float32(8.0) * c)), np.float32(p[b, 1] + np.float32(np.float32(8.0) * s)))
            k = b * 65 + i
            assert (begin[k, 0], begin[k, 1]) == (p[b, 0], p[b, 1])
            assert end[k, 0].view(np.uint32) == want[0].view(np.uint32) and end[k, 1].view(np.uint32) == want[1].view(np.uint32)
    # the table: exact multiples of pi/4, duplicates, and a stretch that is not sorted
    q = np.float32(np.pi / 4)
    assert ang[0] == 0 and ang[1] == q and ang[7] == np.float32(4) * q
    assert np.unique(ang).size < ang.size and (np.diff(ang[20:40]) < 0).all() and (np.diff(ang[41:64]) > 0).all()
