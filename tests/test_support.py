"""The shared helpers of tests/support.py still bite: `same` is a comparison of bits, `pack` has one answer for an empty log,
`check_symbols` fails for a name that is missing or has another return type, and the two compile helpers run the strict
command lines.  No device."""
import os
import subprocess

import numpy as np
import pytest

from support import build_check, check_symbols, compile_c99, pack, same


def test_same_compares_bits_not_values():
    assert not same(np.float32(0.0), np.float32(-0.0))
    nans = np.array([0x7FC00000, 0x7FC00001], np.uint32).view(np.float32)
    assert np.isnan(nans).all() and not same(nans[:1], nans[1:])
    assert same(nans, nans.copy())
    assert not same(np.ones((2, 3), np.float32), np.ones(6, np.float32))


def test_same_rounds_float64_to_float32_first():
    a = np.array([0.1, 1.0 / 3.0, 1e-40], np.float64)
    assert same(a, a.astype(np.float32))


def test_pack_of_an_empty_log_is_a_0_by_2_array():
    for scans, offsets in (([], [0]), ([np.zeros((0, 2), np.float32)] * 3, [0, 0, 0, 0]), ([[], []], [0, 0, 0])):
        pts, offs = pack(scans)
        assert pts.shape == (0, 2) and pts.dtype == np.float32
        assert offs.dtype == np.int32 and offs.tolist() == offsets


def test_pack_offsets_count_points_per_scan():
    pts, offs = pack([np.arange(6, dtype=np.float64).reshape(3, 2), np.zeros((0, 2), np.float32)])
    assert offs.dtype == np.int32 and offs.tolist() == [0, 3, 3]
    assert pts.dtype == np.float32 and pts.flags.c_contiguous and pts.tolist() == [[0.0, 1.0], [2.0, 3.0], [4.0, 5.0]]


def test_check_symbols_passes_for_an_entry_and_fails_for_a_missing_one():
    check_symbols(["hsm_create"])
    with pytest.raises(AssertionError):
        check_symbols(["hsm_no_such_entry"])


def test_check_symbols_holds_the_return_type():
    with pytest.raises(AssertionError):
        check_symbols(["hsm_select_topk_workspace"])
    check_symbols(["hsm_select_topk_workspace"], restype=r"(int|size_t)")


def test_compile_c99_turns_a_warning_into_an_error(tmp_path):
    with pytest.raises(subprocess.CalledProcessError):
        compile_c99(tmp_path, "int main(void) { int unused; return 0; }\n")


def test_build_check_returns_the_executable(tmp_path):
    exe = build_check(tmp_path, "window_grid_check.cpp")
    assert os.path.isfile(exe) and os.access(exe, os.X_OK)
