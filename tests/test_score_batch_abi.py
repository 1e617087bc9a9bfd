"""Scoring and ranking batched pose hypotheses on the device (hsm_score_batch_device, hsm_select_best_device and the chained
forms): what can be checked without a GPU.

* every new symbol is declared in capi.h, bound in capi.SIGNATURES and exported by the built library; the header stays C99;
* a NULL context is HSM_ERR_INVALID from each new entry (no device needed);
* the numpy restatement of the ranking rule (tests/select_rule.py, the expected value of the GPU tests) on hand-made arrays;
* why the step matters, on the oracle alone: Gauss-Newton from 32 wide starts per scan often ends in a wrong basin, and the
  hypothesis with the highest likelihood at its matched pose is the one closest to the truth;
* the new kernels are in the code object and use no scratch.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import select_rule
from conftest import make_oracle, oracle_kinds
from support import check_symbols, compile_c99, header_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("hsm_score_batch_device", "hsm_select_best_device", "hsm_match_score_batch_device", "hsm_match_score_batch")
HSM_ERR_INVALID = -1


def test_new_symbols_declared_bound_and_exported():
    from hector_slam_amd import capi
    check_symbols(NEW_SYMBOLS)
    head = header_text()
    assert "OccGridMapUtil.h:184-221" in head and "getMapCoordsPose" in head  # the "replaces:" line of the new block
    for meth in ("score_batch_device", "select_best_device", "match_score_batch_device", "score_batch", "match_score_batch"):
        assert callable(getattr(capi.MapRepMultiMap, meth)), meth


def test_header_with_the_new_entries_is_plain_c99(tmp_path):
    compile_c99(tmp_path,
                "int main(void) { hsm_ctx* h = 0; int idx[1] = {0}; float f[3] = {0.0f, 0.0f, 0.0f};\n"
                "  int rc = hsm_score_batch_device(h, 0, 1, f, f, 0, 1, f, 0, 0);\n"
                "  rc += hsm_select_best_device(h, 1, 0, 1, f, f, idx, f, f, 0);\n"
                "  rc += hsm_match_score_batch_device(h, 1, f, f, 0, 1, f, 0, 0, f, 0, 1, 0, 1, idx, f, f, 0);\n"
                "  rc += hsm_match_score_batch(h, 1, f, f, 0, 1, f, 0, 0, f, 0, 1, 0, 1, idx, f, f);\n"
                "  return rc; }\n")


def test_null_context_is_invalid_for_every_new_entry():
    from hector_slam_amd import capi
    lib = capi.load_library()
    f = (C.c_float * 16)()
    i = (C.c_int * 4)()
    fp, ip = C.addressof(f), C.addressof(i)
    assert lib.hsm_score_batch_device(None, 0, 1, fp, fp, None, 1, fp, fp, None) == HSM_ERR_INVALID
    assert b"null context" in lib.hsm_last_error()
    assert lib.hsm_select_best_device(None, 1, None, 1, fp, fp, ip, fp, fp, None) == HSM_ERR_INVALID
    assert lib.hsm_match_score_batch_device(None, 1, fp, fp, None, 1, fp, None, 0, fp, fp, 1, None, 1, ip, fp, fp,
                                            None) == HSM_ERR_INVALID
    assert lib.hsm_match_score_batch(None, 1, fp, fp, None, 1, fp, None, 0, fp, fp, 1, None, 1, ip, fp, fp) == HSM_ERR_INVALID
    assert b"null context" in lib.hsm_last_error()


# ---- the ranking rule, restated (tests/select_rule.py) ---------------------------------------------------------------------
NAN = np.float32(np.nan)


def selection_cases():
    """(name, scores, kwargs of select_rule.select_best, expected index): shared with the GPU test of the kernel"""
    return [
        ("ties_lowest_index", [0.5, 0.9, 0.9, 0.1, 0.9], dict(groups=1, group_size=5), [1]),
        ("nan_never_wins", [NAN, 0.2, NAN, 0.7, NAN], dict(groups=1, group_size=5), [3]),
        ("nan_first_then_tie", [NAN, 0.7, 0.7], dict(groups=1, group_size=3), [1]),
        ("all_nan_and_empty", [NAN, NAN, 0.3], dict(group_offsets=[0, 2, 2, 3]), [-1, -1, 2]),
        ("signed_zero_tie", [-1.0, -0.0, 0.0, -0.0], dict(groups=1, group_size=4), [1]),
        ("signed_zero_tie_reversed", [0.0, -0.0, -5.0], dict(groups=1, group_size=3), [0]),
        ("negative_and_inf", [-np.inf, -3.0, -2.0, -np.inf, np.inf, np.inf], dict(groups=2, group_size=3), [2, 4]),
        ("fixed_groups", [1, 2, 3, 3, 2, 1, 5, 5, 5], dict(groups=3, group_size=3), [2, 3, 6]),
        ("fixed_groups_leave_a_tail", [1, 2, 9, 3, 7], dict(groups=2, group_size=2), [1, 2]),
        ("ragged_groups", [4, 4, 1, 9, NAN, 2, 2, 8, 8], dict(group_offsets=[0, 2, 3, 5, 5, 9]), [0, 2, 3, -1, 7]),
        ("offsets_not_from_zero", [9, 9, 1, 2, 3], dict(group_offsets=[2, 5]), [4]),
        ("zero_size_groups", [1, 2], dict(groups=3, group_size=0), [-1, -1, -1]),
    ]


@pytest.mark.parametrize("case", selection_cases(), ids=lambda c: c[0])
def test_selection_rule_restatement(case):
    _, scores, kw, want = case
    s = np.asarray(scores, np.float32)
    idx, sc = select_rule.select_best(s, **kw)
    assert idx.dtype == np.int32 and idx.tolist() == want
    for g, i in enumerate(idx):
        if i < 0:
            assert np.isnan(sc[g])
        else:
            assert sc[g].view(np.uint32) == s[i].view(np.uint32)  # the winner's own bits (a -0 stays a -0)


def test_selection_rule_winner_poses():
    poses = np.arange(15, dtype=np.float32).reshape(5, 3)
    before = np.full((3, 3), -7.0, np.float32)
    idx, _ = select_rule.select_best([NAN, NAN, 1.0, 2.0, 2.0], group_offsets=[0, 2, 2, 5])
    out = select_rule.winner_poses(idx, poses, before)
    assert idx.tolist() == [-1, -1, 3]
    assert np.array_equal(out[:2], before[:2]) and np.array_equal(out[2], poses[3])


def test_selection_rule_is_independent_of_how_a_group_is_split():
    """the pair order (score, index) is total, so reducing parts first and the partial winners afterwards -- what any launch
    shape does -- finds the same entry"""
    rng = np.random.default_rng(11)
    s = rng.integers(0, 6, 1000).astype(np.float32)  # many ties
    s[rng.integers(0, 1000, 100)] = NAN
    whole, _ = select_rule.select_best(s, groups=1, group_size=1000)
    for parts in (2, 7, 64, 256):
        cand = []
        for lane in range(parts):  # strided like the lanes of the kernel
            sub = np.arange(lane, 1000, parts)
            i, _ = select_rule.select_best(s[sub], groups=1, group_size=sub.size)
            if i[0] >= 0:
                cand.append(int(sub[i[0]]))
        cand.sort()
        j, _ = select_rule.select_best(s[cand], groups=1, group_size=len(cand))
        assert cand[j[0]] == whole[0], parts


# ---- why the step matters: the oracle alone ---------------------------------------------------------------------------------
def wide_start_hypotheses(scene, q_count=4, k=32, seed=5):
    """the recipe of the finding: 32 start poses per scan, uniform over +-0.6 m / +-0.3 rad around the truth"""
    rng = np.random.default_rng(seed)
    out = []
    for q in range(q_count):
        init = (scene.query_truth[q] + rng.uniform(-1, 1, (k, 3)) * [0.6, 0.6, 0.3]).astype(np.float32)
        out.append(init)
    return out


@pytest.mark.parametrize("kind", oracle_kinds())
def test_highest_likelihood_picks_the_hypothesis_closest_to_the_truth(oracle_mod, pyramid_scene, kind):
    """Full 3-level match from every start, getLikelihoodForState on level 0 at the matched pose: for each of the first four
    query scans the winner by likelihood is the hypothesis with the smallest position error among the 32, or within 1 mm of it
    (reference figures: the smallest-error one for scans 0, 1, 3; 0.0015 mm behind it for scan 2), while the median hypothesis
    is centimetres off and the worst one most of a metre."""
    sc = pyramid_scene
    o = make_oracle(oracle_mod, kind, sc)
    for q, init in enumerate(wide_start_hypotheses(sc)):
        pts, truth = sc.query_scans[q], sc.query_truth[q]
        poses = np.stack([o.match(init[k], pts)[0] for k in range(init.shape[0])])
        pm = np.stack([o.map_coords_pose(0, p) for p in poses]).astype(np.float32)
        lh = o.likelihood_states(0, pm, pts)
        idx, _ = select_rule.select_best(lh, groups=1, group_size=lh.size)
        err = np.hypot(*(poses[:, :2] - truth[:2]).T)
        print(f"scan {q} {kind}: winner {idx[0]} err {err[idx[0]] * 1e3:.4f} mm, min {err.min() * 1e3:.4f} mm, "
              f"median {np.median(err) * 1e3:.1f} mm, worst {err.max():.2f} m, distinct likelihoods {np.unique(lh).size}")
        assert idx[0] >= 0
        assert err[idx[0]] - err.min() <= 1e-3, (q, err[idx[0]], err.min())
        assert np.unique(lh).size < lh.size  # ties are the normal case: several starts reach the bit-identical pose


def test_reference_likelihood_of_an_empty_scan_is_nan(oracle_mod, pyramid_scene):
    o = make_oracle(oracle_mod, "ho", pyramid_scene, build=False)
    lh = o.likelihood_states(0, np.zeros((2, 3), np.float32), np.zeros((0, 2), np.float32))
    assert np.isnan(lh).all()


# ---- the code object ------------------------------------------------------------------------------------------------------
def test_new_kernels_are_in_the_code_object_without_scratch():
    from hector_slam_amd import build
    from test_kernel_resources import kernels
    if build.hipcc_path() is None:
        pytest.skip("hipcc not found")
    ks = kernels(build.device_asm())
    score = {k: v for k, v in ks.items() if "score_batch_kernel" in k}
    select = {k: v for k, v in ks.items() if "select_best_kernel" in k}
    assert len(score) == 4 and len(select) == 2, (sorted(score), sorted(select))  # 2 layouts x 2 orders; 2 launch shapes
    for k, v in {**score, **select}.items():
        assert v["scratch"] == 0, (k, v)
        assert v["vgpr"] <= 128, (k, v)  # four wavefronts per SIMD, as launched


def test_facade_scored_batch_compiles():
    """include/hector_slam_lib/slam_main/MapRepMultiMap.h::matchDataBatchScored against the include tree it drops into (present
    where the reference-compiled checkers were built)"""
    overlay = os.path.join(ROOT, "oracle", "_ref", "overlay", "hector_slam_lib")
    if not os.path.exists(os.path.join(overlay, "slam_main", "HectorSlamProcessor.h")):
        pytest.skip("oracle/_ref/overlay not built (needs the reference include tree)")
    subprocess.run(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-Wno-sign-compare",
                    "-Wno-unused-variable", "-Wno-delete-non-virtual-dtor", "-Wno-unused-function", "-fsyntax-only",
                    "-I", os.path.join(ROOT, "oracle", "stubs"), "-I", overlay, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "facade_scored_check.cpp")], check=True)
