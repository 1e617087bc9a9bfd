"""The arithmetic behind the window entries, on the CPU.

* tests/window_cases.window_poses (numpy fp32) is hand-checked against float64 with one rounding per operation, and held to
  hector_slam_amd/csrc/window_grid.h -- the text the kernels compile -- through tests/cpp/window_grid_check.cpp for every index
  of the windows the GPU tests use, the index <-> (i, j, k) round trip included;
* tests/topk_rule.topk follows the stated order on every case of topk_cases(), and with k == 1 names select_rule's winner;
* the workspace arithmetic of the header is what the library's entry points return;
* the feature does what it is for, on the reference alone: the committed case of window_cases.py lies beyond the matcher's
  basin, and the reference composition over the window finds the true pose.
"""
import os
import subprocess

import numpy as np
import pytest

import select_rule
import topk_rule
import window_cases
from conftest import ang_diff, bits, make_oracle, oracle_kinds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CENTRE = (1.2345678, -2.7182817, 0.31415927)


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("window_grid") / "window_grid_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I",
                    os.path.join(ROOT, "hector_slam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "window_grid_check.cpp"),
                    "-o", str(exe)], check=True)
    return str(exe)


def run(exe, *args):
    out = subprocess.run([exe] + [repr(float(a)) if isinstance(a, (float, np.floating)) else str(a) for a in args], check=True,
                         capture_output=True, text=True).stdout
    return [[int(v) for v in line.split()] for line in out.splitlines()]


def test_restatement_is_the_stated_arithmetic():
    """float64 products and sums of fp32 operands are exact, so rounding each once to fp32 is the stated recipe"""
    half, step = (3, 2, 1), window_cases.STEP
    poses = window_cases.window_poses(CENTRE, step, half)
    assert poses.shape == (105, 3) and poses.dtype == np.float32
    c, s = np.asarray(CENTRE, np.float32), np.asarray(step, np.float32)
    for w in (0, 1, 6, 7, 34, 35, 52, 104):
        i, j, k = w % 7, (w // 7) % 5, w // 35
        for a, d in enumerate((i - 3, j - 2, k - 1)):
            prod = np.float32(np.float64(np.float32(d)) * np.float64(s[a]))
            want = np.float32(np.float64(c[a]) + np.float64(prod))
            assert bits(poses[w, a]) == bits(want), (w, a)
    assert np.array_equal(bits(poses[52]), bits(c))  # the middle of the window is the centre itself
    got = window_cases.window_poses(CENTRE, step, half, [-1, 105, 7, 7, 104])
    assert np.isnan(got[:2]).all() and np.array_equal(bits(got[2:]), bits(poses[[7, 7, 104]]))


@pytest.mark.parametrize("half", window_cases.WINDOWS)
def test_restatement_equals_the_header_for_every_index(check_exe, half):
    step = np.asarray(window_cases.STEP, np.float32)
    c = np.asarray(CENTRE, np.float32)
    rows = np.array(run(check_exe, "poses", *half, *step, *c), np.int64)
    W = window_cases.window_count(half)
    assert rows.shape == (W, 8) and run(check_exe, "count", *half) == [[W]]
    assert np.array_equal(rows[:, 0], np.arange(W)) and np.array_equal(rows[:, 4], np.arange(W))  # the round trip
    i, j, k = window_cases.window_ijk(half, np.arange(W))
    assert np.array_equal(rows[:, 1], i) and np.array_equal(rows[:, 2], j) and np.array_equal(rows[:, 3], k)
    assert np.array_equal(rows[:, 5:].astype(np.uint32), bits(window_cases.window_poses(c, step, half)))


def test_window_count_and_workspaces_of_the_header(check_exe):
    from hector_slam_amd import capi
    assert run(check_exe, "count", -1, 0, 0) == [[0]]
    assert run(check_exe, "count", 40, 40, 20) == [[81 * 81 * 41]]
    assert run(check_exe, "count", 1000000, 1000, 1000)[0][0] > 2**31 - 1  # refused by its size, without overflow
    assert run(check_exe, "count", 2**31 - 1, 2**31 - 1, 2**31 - 1)[0][0] > 2**31 - 1
    for count, k in ((0, 1), (1, 1), (64, 8), (65, 8), (100_000, 16), (269_001, 64), (5, 65), (-1, 4)):
        total, slices = run(check_exe, "topk", count, k)[0]
        assert total == capi.MapRepMultiMap.select_topk_workspace(count, k)
        if total:
            assert slices == min(max((count + 63) // 64, 1), 256) and total == slices * k * 8
    for W, k in ((1, 1), (5625, 8), (269_001, 16), (0, 4), (10, 0)):
        L = run(check_exe, "reloc", W, k)[0]
        assert L[-1] == capi.MapRepMultiMap.relocalize_workspace(W, k)
        if L[-1]:
            assert L[0] == 0 and L == sorted(L) and all(v % 8 == 0 for v in L)
            assert L[1] >= 4 * W and L[2] - L[1] == capi.MapRepMultiMap.select_topk_workspace(W, k)
            assert L[3] - L[2] >= 4 * k and L[4] - L[3] >= 4 * k and L[5] - L[4] >= 12 * k


def brute_topk(s, k):
    """the order, literally: repeatedly the entry no other entry beats"""
    left = [i for i in range(len(s)) if s[i] == s[i]]
    out = []
    while left and len(out) < k:
        b = left[0]
        for i in left[1:]:
            if s[i] > s[b]:  # ascending i: an equal score later on never replaces the earlier one
                b = i
        out.append(b)
        left.remove(b)
    return out


def test_topk_rule_on_every_case():
    names = []
    for name, s in topk_rule.topk_cases():
        names.append(name)
        for k in (1, 8, 64):
            idx, sc = topk_rule.topk(s, k)
            assert idx.dtype == np.int32 and sc.dtype == np.float32 and idx.shape == sc.shape == (k,)
            filled = idx >= 0
            m = int(filled.sum())
            assert m == min(k, int((~np.isnan(s)).sum())) and filled[:m].all() and np.isnan(sc[~filled]).all()
            assert np.array_equal(bits(sc[filled]), bits(s[idx[filled]])) and len(set(idx[filled].tolist())) == m
            if s.size <= 300:
                assert idx[filled].tolist() == brute_topk(s, k), (name, k)
            else:  # rank order, ties by index, and nothing better left out
                a, b = sc[:m][:-1], sc[:m][1:]
                assert ((a > b) | ((a == b) & (idx[:m][:-1] < idx[:m][1:]))).all()
                rest = np.ones(s.size, bool)
                rest[idx[filled]] = False
                rest &= ~np.isnan(s)
                if rest.any() and m:
                    assert s[rest].max() <= sc[m - 1]
                    tied = np.flatnonzero(rest & (s == sc[m - 1]))
                    assert tied.size == 0 or tied.min() > idx[:m][sc[:m] == sc[m - 1]].max()
        best, best_score = select_rule.select_best(s, groups=1, group_size=s.size)
        idx, sc = topk_rule.topk(s, 1)
        assert idx[0] == best[0] and (np.isnan(sc[0]) if best[0] < 0 else bits(sc[0]) == bits(best_score[0])), name
    assert {"ties", "signed zeros", "nans", "all nan", "count below k", "empty", "100000 in 16 values"} <= set(names)
    assert {f"count {n}" for n in (1, 63, 64, 65, 257)} <= set(names)
    assert topk_rule.topk(np.array([-0.0, 0.0, -0.0], np.float32), 3)[0].tolist() == [0, 1, 2]
    assert topk_rule.topk(np.array([0.5, np.nan, 0.7, 0.7], np.float32), 8)[0].tolist() == [2, 3, 0, -1, -1, -1, -1, -1]


def reference_relocalize(o, scene, centre, scan, step, half, k, search_level=None):
    """the reference composition: likelihoods over the window on the search level, the k best, a match from each, the likelihood
    of every matched pose on level 0, the winner.  Unfilled places are NaN rows that never win."""
    lvl = scene.levels - 1 if search_level is None else search_level
    poses = window_cases.window_poses(centre, step, half)
    pm = np.stack([o.map_coords_pose(lvl, p) for p in poses])
    scores = o.likelihood_states(lvl, pm, np.asarray(scan, np.float32) * np.float32(1.0 / 2 ** lvl))
    idx, top = topk_rule.topk(scores, k)
    cand = np.full((k, 3), np.nan, np.float32)
    cov = np.zeros((k, 9), np.float32)
    lh0 = np.full(k, np.nan, np.float32)
    for c, w in enumerate(idx):
        if w < 0:
            continue
        cand[c], cov[c] = o.match(poses[w], scan)
        lh0[c] = o.likelihood_states(0, o.map_coords_pose(0, cand[c])[None], scan)[0]
    best, best_score = select_rule.select_best(lh0, groups=1, group_size=k)
    return dict(scores=scores, index=idx, top=top, start=window_cases.window_poses(centre, step, half, idx), cand=cand, cov=cov,
                lh0=lh0, best=int(best[0]), best_score=best_score[0], best_index=int(idx[best[0]]) if best[0] >= 0 else -1,
                best_pose=cand[best[0]] if best[0] >= 0 else None)


@pytest.mark.parametrize("kind", oracle_kinds())
def test_committed_case_lies_beyond_the_basin_and_the_window_finds_it(oracle_mod, pyramid_scene, kind):
    sc = pyramid_scene
    o = make_oracle(oracle_mod, kind, sc)
    truth, centre, scan = window_cases.reloc_case(sc)
    plain, _ = o.match(centre, scan)
    d, a = np.hypot(*(plain[:2] - truth[:2])), ang_diff(plain[2], truth[2])
    assert d > 0.2 or a > 0.1, (d, a)  # the matcher alone does not come back
    r = reference_relocalize(o, sc, centre, scan, window_cases.RELOC_STEP, window_cases.RELOC_HALF, window_cases.RELOC_K)
    d, a = np.hypot(*(r["best_pose"][:2] - truth[:2])), ang_diff(r["best_pose"][2], truth[2])
    print(f"{kind}: plain match ends {np.hypot(*(plain[:2] - truth[:2])):.3f} m / {ang_diff(plain[2], truth[2]):.3f} rad off, "
          f"the window's winner {d:.4f} m / {a:.5f} rad (candidate {r['best']} of {r['index'].tolist()})")
    assert d <= sc.resolution and a <= 0.02, (d, a)
    assert (r["index"] >= 0).all() and r["best"] > 0  # the coarse level's best cell is not the winner on level 0
