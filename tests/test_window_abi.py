"""The window entries (hsm_score_window*, hsm_window_poses_device, hsm_select_topk_*, hsm_relocalize*): what can be checked
without a GPU.

* every new symbol is declared in capi.h, bound in capi.SIGNATURES with as many arguments, and exported by the built library;
  the header stays C99 with a call of each new entry;
* a NULL context is HSM_ERR_INVALID from each entry (no device needed);
* the workspace functions are host arithmetic: 0 for refused sizes, non-decreasing in the count and in k, multiples of 8.
"""
import ctypes as C
import os

from support import check_symbols, compile_c99, header_text

NEW_SYMBOLS = ("hsm_score_window_device", "hsm_score_window", "hsm_window_poses_device", "hsm_select_topk_device",
               "hsm_select_topk_workspace", "hsm_relocalize_device", "hsm_relocalize_workspace", "hsm_relocalize")
HSM_ERR_INVALID = -1


def test_new_symbols_declared_bound_and_exported():
    from hector_slam_amd import build, capi
    check_symbols(NEW_SYMBOLS, restype=r"(int|size_t)")
    head = header_text()
    assert "#define HSM_MAX_TOPK 64" in head and "HSM_WINDOW_FORM" in head and "non-maximum suppression" in head
    for meth in ("score_window_device", "score_window", "window_poses_device", "select_topk_device", "select_topk_workspace",
                 "relocalize_device", "relocalize_workspace", "relocalize"):
        assert callable(getattr(capi.MapRepMultiMap, meth)), meth
    assert "window.hip" in build.UNITS
    assert {os.path.basename(d) for d in build.UNITS["window.hip"]} >= {"window_kernels.h", "window_grid.h"}


def test_header_with_the_new_entries_is_plain_c99(tmp_path):
    compile_c99(tmp_path,
                "int main(void) { hsm_ctx* h = 0; float f[9] = {0.0f}; float st[3] = {0.1f, 0.1f, 0.1f}; int hf[3] = {1, 1, 1};\n"
                "  int idx[HSM_MAX_TOPK]; char ws[64];\n"
                "  int rc = hsm_score_window_device(h, 0, f, st, hf, f, 1, f, 0, 0);\n"
                "  rc += hsm_score_window(h, 0, f, st, hf, f, 1, f, f);\n"
                "  rc += hsm_window_poses_device(h, f, st, hf, idx, 1, f, 0);\n"
                "  rc += hsm_select_topk_device(h, 1, f, 1, idx, f, ws, hsm_select_topk_workspace(1, 1), 0);\n"
                "  rc += hsm_relocalize_device(h, 0, f, st, hf, 1, f, 1, ws, hsm_relocalize_workspace(27, 1), f, f, f, f, f, idx, 0);\n"
                "  rc += hsm_relocalize(h, 0, f, st, hf, 1, f, 1, f, f, f, f, f, idx);\n"
                "  return rc; }\n")


def test_null_context_is_invalid_for_every_new_entry():
    from hector_slam_amd import capi
    lib = capi.load_library()
    f = (C.c_float * 32)()
    fp = C.addressof(f)
    st, hf = (C.c_float * 3)(0.1, 0.1, 0.1), (C.c_int * 3)(1, 1, 1)
    calls = (lambda: lib.hsm_score_window_device(None, 0, fp, st, hf, fp, 1, fp, fp, None),
             lambda: lib.hsm_score_window(None, 0, fp, st, hf, fp, 1, fp, fp),
             lambda: lib.hsm_window_poses_device(None, fp, st, hf, None, 1, fp, None),
             lambda: lib.hsm_select_topk_device(None, 1, fp, 1, fp, fp, fp, 64, None),
             lambda: lib.hsm_relocalize_device(None, 0, fp, st, hf, 1, fp, 1, fp, 1 << 20, fp, fp, fp, fp, fp, fp, None),
             lambda: lib.hsm_relocalize(None, 0, fp, st, hf, 1, fp, 1, fp, fp, fp, fp, fp, fp))
    for call in calls:
        assert lib.hsm_shard_bounds(1, 0, 0, None, None) != 0  # (another refusal: the text below is this call's own)
        assert call() == HSM_ERR_INVALID
        assert b"null context" in lib.hsm_last_error()


def test_workspace_sizes_are_host_arithmetic():
    from hector_slam_amd import capi
    topk, reloc = capi.MapRepMultiMap.select_topk_workspace, capi.MapRepMultiMap.relocalize_workspace
    for k in (0, -1, 65):
        assert topk(100, k) == 0 and reloc(100, k) == 0
    assert topk(-1, 8) == 0 and reloc(0, 8) == 0 and reloc(-5, 8) == 0
    assert topk(0, 1) > 0  # an empty array still leaves k places of one slice
    counts = (0, 1, 63, 64, 65, 257, 4096, 16384, 16385, 100_000, 269_001, 2**31 - 1)
    for f, cs in ((topk, counts), (reloc, counts[1:])):
        for k in (1, 8, 16, 64):
            sizes = [f(c, k) for c in cs]
            assert all(s > 0 and s % 8 == 0 for s in sizes), (f, k, sizes)
            assert sizes == sorted(sizes), (f, k)
        for c in cs:
            sizes = [f(c, k) for k in range(1, 65)]
            assert sizes == sorted(sizes), (f, c)
    # the relocalisation's block holds the scores, the selection's candidates, and k indices, scores and poses
    for W, k in ((5625, 8), (1, 64), (269_001, 16)):
        assert reloc(W, k) >= 4 * W + topk(W, k) + k * (4 + 4 + 12)
