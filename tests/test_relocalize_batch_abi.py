"""The host side of the batched relocalisation: hsm_select_topk_groups_workspace / hsm_relocalize_batch_workspace and the
layouts behind them (hector_slam_amd/csrc/window_grid.h, stage_layout.h through tests/cpp/relocalize_batch_check.cpp), the
symbols, and the header as C99.  No device.

A layout is held to what its users need, not to written-out numbers: every region starts 8-byte aligned (256 for a staging
plan), regions lie in their stated order, each is at least as large as the array it holds, and the total is what the library's
entry returns.  Sizes the entries refuse give 0.
"""
import subprocess

import pytest

import window_cases
from support import INCLUDE, build_check, check_symbols, compile_c99

INT_MAX = 2**31 - 1
NEW = ("hsm_score_windows_batch_device", "hsm_select_topk_groups_device", "hsm_relocalize_batch_device", "hsm_relocalize_batch")
SIZES = ("hsm_select_topk_groups_workspace", "hsm_relocalize_batch_workspace")


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    return str(build_check(tmp_path_factory.mktemp("relocalize_batch"), "relocalize_batch_check.cpp", "-Wextra", "-I", INCLUDE))


def run(exe, *args):
    out = subprocess.run([exe, *map(str, args)], check=True, capture_output=True, text=True).stdout
    return [int(v) for v in out.split()]


@pytest.fixture(scope="module")
def lib():
    from hector_slam_amd import build, capi
    build.build_native()
    return capi.load_library()


def slices(count):
    return min(max((count + 63) // 64, 1), 256)


def test_symbols_are_declared_bound_and_exported():
    check_symbols(NEW)
    check_symbols(SIZES, restype=r"size_t")


def test_header_is_c99_with_the_batched_entries(tmp_path):
    compile_c99(tmp_path, """
int use(hsm_ctx* h, const float* c, const float* p, const int* o, float* f, int* i, void* ws) {
  const float step[3] = {0.1f, 0.1f, 0.1f};
  const int half[3] = {1, 1, 1};
  size_t need = hsm_relocalize_batch_workspace(2, 27, 4, 100) + hsm_select_topk_groups_workspace(2, 27, 4);
  int rc = hsm_score_windows_batch_device(h, 0, 2, c, step, half, p, o, 0, f, 0, 0);
  rc += hsm_select_topk_groups_device(h, 2, 27, f, 4, i, f, ws, need, 0);
  rc += hsm_relocalize_batch_device(h, 0, 2, c, step, half, 4, p, o, 0, 100, ws, need, f, 0, f, i, f, 0, i, 0);
  return rc + hsm_relocalize_batch(h, 0, 2, c, step, half, 4, p, o, 0, f, 0, f, i, f, 0, i);
}
""")


@pytest.mark.parametrize("k", [1, 8, 64])
@pytest.mark.parametrize("group_size", [0, 1, 63, 65, 16385, 5625])
def test_grouped_topk_workspace(check_exe, lib, group_size, k):
    for groups in (1, 2, 3, 512):
        cand_score, cand_index, total, sl = run(check_exe, "topk", groups, group_size, k)
        assert sl == slices(group_size)
        cands = groups * sl * k
        # all the candidates' scores, then all their indices: neither overlaps the other, both fit, both 4-byte aligned
        assert cand_score == 0 and cand_index == 4 * cands and total >= cand_index + 4 * cands and total % 8 == 0
        assert total == lib.hsm_select_topk_groups_workspace(groups, group_size, k)
        if groups == 1:
            assert total == lib.hsm_select_topk_workspace(group_size, k)


def test_grouped_topk_workspace_refuses(check_exe, lib):
    for groups, group_size, k in ((-1, 10, 4), (2, -1, 4), (2, 10, 0), (2, 10, 65), (2, 2**30, 4), (2**30, 2, 4), (2**26, 1, 64),
                                  (0, 10, 4)):
        assert run(check_exe, "topk", groups, group_size, k)[:3] == [0, 0, 0], (groups, group_size, k)
        assert lib.hsm_select_topk_groups_workspace(groups, group_size, k) == 0, (groups, group_size, k)
    assert lib.hsm_select_topk_groups_workspace(2**25, 1, 63) > 0  # groups * k just inside INT_MAX


RELOC_W = window_cases.window_count(window_cases.RELOC_HALF)


@pytest.mark.parametrize("B,W,k,total", [(1, 1, 1, 0), (3, RELOC_W, window_cases.RELOC_K, 2981), (4, 105, 8, 1278), (4, 11, 64, 0),
                                         (512, 4225, 16, 512 * 1081), (0, 27, 4, 0), (1, 16385, 64, 1081)])
def test_relocalize_batch_layout(check_exe, lib, B, W, k, total):
    scores, topk, index, kscore, pose, offsets, pts, end = run(check_exe, "reloc", B, W, k, total)
    regions = [(scores, 4 * B * W), (topk, lib.hsm_select_topk_groups_workspace(B, W, k)), (index, 4 * B * k), (kscore, 4 * B * k),
               (pose, 12 * B * k), (offsets, 4 * (B * k + 1)), (pts, 8 * max(k * total, 1))]
    at = 0
    for off, need in regions:  # in order, aligned, none reaching into the next
        assert off % 8 == 0 and off >= at, regions
        at = off + need
    assert end >= at and end % 8 == 0
    assert end == lib.hsm_relocalize_batch_workspace(B, W, k, total)
    if B == 1:
        assert end >= lib.hsm_relocalize_workspace(W, k)


def test_relocalize_batch_workspace_of_one_scan_covers_the_single_entry(lib):
    for W in (1, 105, RELOC_W, 16385):
        for k in (1, 8, 64):
            for n in (0, 1081):
                assert lib.hsm_relocalize_batch_workspace(1, W, k, n) >= lib.hsm_relocalize_workspace(W, k) > 0


def test_relocalize_batch_workspace_refuses(check_exe, lib):
    for B, W, k, total in ((-1, 27, 4, 0), (2, 0, 4, 0), (2, -5, 4, 0), (2, 27, 0, 0), (2, 27, 65, 0), (2, 27, 4, -1),
                           (2, 2**30, 4, 0),                   # B * W > INT_MAX
                           (INT_MAX // 9 // 4 + 1, 1, 4, 0),   # B * k > INT_MAX / 9
                           (2, 27, 4, 2**29)):                 # k * total_points > INT_MAX
        assert run(check_exe, "reloc", B, W, k, total)[-1] == 0, (B, W, k, total)
        assert lib.hsm_relocalize_batch_workspace(B, W, k, total) == 0, (B, W, k, total)
    assert lib.hsm_relocalize_batch_workspace(INT_MAX // 9 // 4, 1, 4, 0) > 0
    assert lib.hsm_relocalize_batch_workspace(2, 27, 4, INT_MAX // 4) > 0


@pytest.mark.parametrize("cov,idx,score,csr", [(1, 1, 1, 1), (0, 0, 0, 0), (1, 0, 1, 0), (0, 1, 0, 1)])
def test_relocalize_batch_stage(check_exe, cov, idx, score, csr):
    B, k, points, ws = 3, 8, 2981, 123456
    *offs, total, n = run(check_exe, "stage", B, k, points, ws, cov, idx, score, csr)
    need = [12 * B, 8 * points, 4 * (B + 1) * csr, ws, 12 * B * k, 36 * B * k * cov, 4 * B * k, 4 * B * k * idx, 12 * B, 4 * B * score,
            4 * B]
    assert n == len(need) == len(offs) <= 12  # StagePlan::kMaxRegions
    at = 0
    for off, bytes_ in zip(offs, need):
        assert off % 256 == 0 and off >= at, (offs, need)
        at = off + bytes_
    assert total >= at and total % 256 == 0
