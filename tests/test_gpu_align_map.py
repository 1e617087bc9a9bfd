"""Another context's map aligned to this one (hsm_align_map) on the MI355X.

* bit for bit the two public calls, hsm_occupied_points then hsm_relocalize with the guess as the centre and as the seed of the
  best pose: transform, covariance, likelihood, counts and window index; both layouts, the pairs of tests/merge_cases.py and a
  dense pair whose 1 268 points take the batch matcher off its one-wavefront-row form, and a point set of HSM_MAX_ALIGN_POINTS
  where the cap bites;
* bit for bit the reference chain of tests/test_window_model.py on the points the device extracted: the CPU checker's likelihoods
  over the written-out window on the search level, the strict top k, its match from each start, its likelihood on level 0;
* end to end: `src`'s world frame lies at (0.25 m, -0.15 m, 0.12 rad) in `dst`'s, the search starts at zero, and hsm_merge_map at
  the returned transform equals the numpy merge model at that transform.  The returned transform is held to the truth within
  twice the error the REFERENCE chain leaves on this scene, measured on the CPU by tools/align_reference_error.py:
      reference error  0.00341 m, 0.00092 m, 0.00153 rad      bound  0.00683 m, 0.00184 m, 0.00305 rad
  (below one level-0 cell of 0.1 m and 0.02 rad).  The chain is the reference's bit for bit, so the factor only guards a scene edit;
* no winner, the refusals, and that neither context's planes, stamps, update indices, dirty or publish boxes change.

The maps are the CPU checker's, built from hector_slam_amd.synth scans and uploaded, so that the checker and the device hold the
same cells.  At the parent commit every test of this file fails: the entries do not exist."""
import ctypes as C
import types

import numpy as np
import pytest

import align_cases as ac
import merge_cases as mc
from conftest import bits, oracle_kinds
from support import capi, new_context
from test_window_model import reference_relocalize

pytestmark = pytest.mark.gpu

HSM_ERR_INVALID = -1
F = np.float32
LAYOUTS = pytest.mark.parametrize("layout", ("quad", "plane"))
KIND = oracle_kinds()[-1]


def new_ctx(capi, geom, layout):
    return new_context(capi, geom[0], geom[1], geom[2], geom[3], geom[4], layout)


@pytest.fixture(scope="module")
def checker(oracle_mod):
    """checker(geom, tag, scans) -> the CPU checker holding the map of those scans, built once"""
    made = {}

    def get(geom, tag, scans):
        if (geom, tag) not in made:
            o = oracle_mod.Oracle(KIND, geom[0], geom[1], geom[2], geom[3], geom[4])
            o.set_update_factor_free(0.4)
            o.set_update_factor_occupied(0.9)
            o.build_map([p for p, _ in scans], [s for _, s in scans])
            made[geom, tag] = o
        return made[geom, tag]
    return get


def uploaded(capi, o, geom, layout):
    g = new_ctx(capi, geom, layout)
    for lvl in range(geom[3]):
        g.upload_level(lvl, *o.download_level(lvl))
    return g


def same_bits(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def public_chain(capi, dst, src, src_level, bbox, every, max_points, search_level, guess, step, half, k):
    """hsm_occupied_points on src, then hsm_relocalize on dst with the guess as the centre and the seed of the best pose
    -> (the points, what hsm_align_map is to return)"""
    pts, counts = src.occupied_points(src_level, bbox, every, max_points)
    g = np.ascontiguousarray(guess, F)
    st, hf = dst._window(step, half)
    cand, cov, lh = np.empty((k, 3), F), np.zeros((k, 9), F), np.empty(k, F)
    best, score, index = g.copy(), np.empty(1, F), np.empty(1, np.int32)
    p = np.ascontiguousarray(pts, F)
    capi._check(dst._lib.hsm_relocalize(dst._h, search_level, g.ctypes.data, st, hf, k, p.ctypes.data if len(p) else None, len(p),
                                        cand.ctypes.data, cov.ctypes.data, lh.ctypes.data, best.ctypes.data, score.ctypes.data,
                                        index.ctypes.data), "hsm_relocalize")
    win_cov = None
    if index[0] >= 0:   # the place the winner took among the k: its refined pose and its level-0 likelihood
        place = [j for j in range(k) if same_bits(cand[j], best) and bits(lh[j]) == bits(score[0])]
        assert place, "the winner is one of the candidates"
        win_cov = cov[place[0]]
    return pts, dict(pose=best, cov=win_cov, likelihood=score[0], counts=counts, index=int(index[0]))


def assert_align_equals(what, got, want):
    pose, cov, lh, counts, index = got
    print(what, "pose", pose.tolist(), "likelihood", float(lh), "counts", counts.tolist(), "window index", index)
    assert same_bits(pose, want["pose"]), (what, "pose", pose, want["pose"])
    assert index == want["index"] and np.array_equal(counts, want["counts"]), (what, index, counts)
    assert same_bits(lh, want["likelihood"]), (what, "likelihood")
    if want["cov"] is not None:
        assert same_bits(cov, want["cov"]), (what, "covariance")


# ---- 1. the public chain and the reference chain ----------------------------------------------------------------------------------
@LAYOUTS
@pytest.mark.parametrize("pair", sorted(mc.PAIRS))
def test_align_equals_the_public_calls_and_the_reference_chain(capi, checker, pair, layout):
    gd, gs = mc.PAIRS[pair]
    scans = mc.build_scans(31)
    o_dst, o_src = checker(gd, "room31", scans), checker(gs, "room31", scans)
    dst, src = uploaded(capi, o_dst, gd, layout), uploaded(capi, o_src, gs, layout)
    guess = F(ac.GUESSES[pair])
    for every in (1, 2):
        args = (0, None, every, ac.MAX_POINTS, ac.SEARCH_LEVEL, guess, ac.STEP, ac.HALF, ac.K)
        pts, want = public_chain(capi, dst, src, *args)
        assert 40 < len(pts) <= 1100 and want["index"] >= 0, (len(pts), want["index"])
        got = dst.align_map_from(src, *args)
        assert_align_equals(f"{pair} {layout} every {every}", got, want)
        ref = reference_relocalize(o_dst, types.SimpleNamespace(levels=gd[3]), guess, pts, ac.STEP, ac.HALF, ac.K,
                                   search_level=ac.SEARCH_LEVEL)
        assert got[4] == ref["best_index"] and same_bits(got[0], ref["best_pose"]), (got[0], ref["best_pose"], ref["best_index"])
        assert bits(got[2]) == bits(ref["best_score"]) and same_bits(got[1], ref["cov"][ref["best"]])
        print("distance from the identity, under which both maps were built:", ac.error(got[0], (0.0, 0.0, 0.0)).tolist())
    # a box of src: the points of that box alone
    box = (5, 4, 40, 30)
    pts, want = public_chain(capi, dst, src, 0, box, 1, ac.MAX_POINTS, ac.SEARCH_LEVEL, guess, ac.STEP, ac.HALF, ac.K)
    assert_align_equals(f"{pair} {layout} box", dst.align_map_from(src, 0, box, 1, ac.MAX_POINTS, ac.SEARCH_LEVEL, guess, ac.STEP,
                                                                  ac.HALF, ac.K), want)
    dst.close()
    src.close()


@LAYOUTS
def test_dense_pair_equals_the_public_calls(capi, checker, layout):
    o = checker(ac.DENSE_GEOM, "dense", ac.dense_scans())
    dst, src = uploaded(capi, o, ac.DENSE_GEOM, layout), uploaded(capi, o, ac.DENSE_GEOM, layout)
    args = (0, None, 1, ac.DENSE_MAX_POINTS, ac.SEARCH_LEVEL, F(ac.DENSE_GUESS), ac.DENSE_STEP, ac.HALF, ac.K)
    pts, want = public_chain(capi, dst, src, *args)
    assert 1100 < len(pts) <= 2500 and want["counts"].tolist() == [len(pts)] * 2 and want["index"] >= 0
    assert_align_equals(f"dense {layout}", dst.align_map_from(src, *args), want)
    dst.close()
    src.close()


def test_a_point_set_at_the_cap_equals_the_public_calls(capi, checker):
    """HSM_MAX_ALIGN_POINTS points: src's level 0 is a random plane of 400 x 320 cells with more occupied cells than the cap, so the
    cap bites and the matcher takes the longest scan the entry admits"""
    import points_cases as pc
    o = checker(ac.DENSE_GEOM, "dense", ac.dense_scans())
    dst, src = uploaded(capi, o, ac.DENSE_GEOM, "quad"), uploaded(capi, o, ac.DENSE_GEOM, "quad")
    lo = pc.random_plane(400, 320, 21)
    src.upload_level(0, lo, np.full(lo.shape, -1, np.int32))
    args = (0, None, 1, capi.MAX_ALIGN_POINTS, ac.SEARCH_LEVEL, F(ac.DENSE_GUESS), ac.DENSE_STEP, ac.HALF, ac.K)
    pts, want = public_chain(capi, dst, src, *args)
    assert want["counts"][0] == len(pts) == capi.MAX_ALIGN_POINTS < want["counts"][1] == len(pc.kept_cells(lo, None, 1))
    assert want["index"] >= 0
    assert_align_equals("at the cap", dst.align_map_from(src, *args), want)
    dst.close()
    src.close()


# ---- 2. end to end -----------------------------------------------------------------------------------------------------------------
@LAYOUTS
def test_align_then_merge(capi, checker, layout):
    geom = ac.E2E_GEOM
    dst_scans, src_scans = ac.e2e_scans()
    o_dst, o_src = checker(geom, "e2e dst", dst_scans), checker(geom, "e2e src", src_scans)
    dst, src = uploaded(capi, o_dst, geom, layout), uploaded(capi, o_src, geom, layout)
    n_occ = int((o_src.download_level(0)[0] > 0).sum())
    every = max(1, -(-n_occ // ac.MAX_POINTS))
    t, cov, lh, counts, index = dst.align_map_from(src, 0, None, every, ac.MAX_POINTS, ac.SEARCH_LEVEL, np.zeros(3, F), ac.STEP,
                                                   ac.HALF, ac.K)
    err = ac.error(t)
    print(layout, "src_in_dst", t.tolist(), "truth", ac.TRUTH, "error", err.tolist(), "bound", ac.E2E_BOUND, "points", counts.tolist(),
          "likelihood", float(lh), "window index", index)
    assert index >= 0 and counts[0] == counts[1] > 100
    before = [dst.download_level(lvl)[0] for lvl in range(geom[3])]
    src_lo = [src.download_level(lvl)[0] for lvl in range(geom[3])]
    capi.merge_map(dst, src, t)
    changed = 0
    for lvl, (want, box) in enumerate(mc.merge_pyramid(before, src_lo, geom, geom, t)):
        lo = dst.download_level(lvl)[0]
        assert np.array_equal(bits(lo), bits(want)), (lvl, int((bits(lo) != bits(want)).sum()))
        changed += int((bits(want) != bits(before[lvl])).sum())
    assert changed > 0
    assert ac.E2E_REFERENCE_ERROR[0] < geom[0] and ac.E2E_REFERENCE_ERROR[1] < geom[0] and ac.E2E_REFERENCE_ERROR[2] < 0.02
    assert (err <= np.array(ac.E2E_BOUND)).all(), (err, ac.E2E_BOUND)
    dst.close()
    src.close()


# ---- 3. no winner -------------------------------------------------------------------------------------------------------------------
def test_an_empty_src_returns_the_guess(capi, checker):
    gd, gs = mc.PAIRS["local"]
    dst = uploaded(capi, checker(gd, "room31", mc.build_scans(31)), gd, "quad")
    src = new_ctx(capi, gs, "quad")
    guess = F([0.3, -0.2, 0.1])
    t, cov, lh, counts, index = dst.align_map_from(src, 0, None, 1, ac.MAX_POINTS, ac.SEARCH_LEVEL, guess, ac.STEP, ac.HALF, ac.K)
    assert same_bits(t, guess) and np.isnan(lh) and index == -1 and counts.tolist() == [0, 0] and not cov.any()
    # ... and with max_points == 0 on a map that has cells
    full = uploaded(capi, checker(gs, "room31", mc.build_scans(31)), gs, "quad")
    t, cov, lh, counts, index = dst.align_map_from(full, 0, None, 1, 0, ac.SEARCH_LEVEL, guess, ac.STEP, ac.HALF, ac.K)
    assert same_bits(t, guess) and np.isnan(lh) and index == -1 and counts[0] == 0 and counts[1] > 40
    for g in (dst, src, full):
        g.close()


# ---- 4. refusals and what an align leaves alone -----------------------------------------------------------------------------------------
def state(g, grids):
    """planes, stamps, update indices, and the dirty and publish boxes (taking them empties them)"""
    levels = g.getMapLevels()
    return ([g.download_level(lvl) for lvl in range(levels)], [g.getUpdateIndex(lvl) for lvl in range(levels)],
            [g.take_dirty_bbox(lvl).tolist() for lvl in range(levels)],
            [g.occupancy_changes(lvl, grids[lvl]).tolist() for lvl in range(levels)])


def test_refusals_and_both_contexts_stay_as_they_are(capi, checker):
    gd, gs = mc.PAIRS["local"]
    scans = mc.build_scans(31)
    dst, src = uploaded(capi, checker(gd, "room31", scans), gd, "quad"), uploaded(capi, checker(gs, "room31", scans), gs, "quad")
    others = {"level count": new_ctx(capi, (mc.RES, 48, 44, 2, (0.5, 0.5)), "quad"), "layout": new_ctx(capi, gs, "plane"),
              "resolution": new_ctx(capi, (0.05, 48, 44, 3, (0.5, 0.5)), "quad")}
    grids = {id(g): [np.full(mc.level_size(geom, lvl)[::-1], 55, np.int8) for lvl in range(3)] for g, geom in ((dst, gd), (src, gs))}
    was = {id(g): state(g, grids[id(g)]) for g in (dst, src)}
    lib = dst._lib
    guess, out = F([0.1, 0.0, 0.05]), np.full(3, 7.0, F)
    st, hf = dst._window(ac.STEP, ac.HALF)
    I3, F3 = C.c_int * 3, C.c_float * 3
    ok = dict(dst=dst._h, src=src._h, lvl=0, box=None, every=1, cap=ac.MAX_POINTS, search=ac.SEARCH_LEVEL, guess=guess.ctypes.data, st=st,
              hf=hf, k=ac.K, out=out.ctypes.data)
    changes = [dict(src=dst._h), dict(dst=None), dict(src=None), dict(cap=capi.MAX_ALIGN_POINTS + 1), dict(cap=-1), dict(every=0),
               dict(lvl=3), dict(lvl=-1), dict(search=3), dict(guess=None), dict(st=None), dict(hf=None), dict(hf=I3(1, -1, 1)),
               dict(hf=I3(40000, 40000, 0)), dict(st=F3(0.1, float("inf"), 0.1)), dict(k=0), dict(k=65), dict(out=None)]
    changes += [dict(src=g._h) for g in others.values()] + [dict(dst=g._h, src=dst._h) for g in others.values()]
    rcs = []
    for change in changes:
        a = dict(ok, **change)
        rcs.append(lib.hsm_align_map(a["dst"], a["src"], a["lvl"], a["box"], a["every"], a["cap"], a["search"], a["guess"], a["st"], a["hf"],
                                     a["k"], a["out"], None, None, None, None))
    assert all(rc == HSM_ERR_INVALID for rc in rcs), rcs
    assert out.tolist() == [7.0] * 3
    got = dst.align_map_from(src, 0, None, 1, ac.MAX_POINTS, ac.SEARCH_LEVEL, guess, ac.STEP, ac.HALF, ac.K)   # ... and one that runs
    assert got[4] >= 0 and got[3][0] > 40
    for g in (dst, src):
        planes, index, dirty, pub = state(g, grids[id(g)])
        for lvl in range(3):
            assert np.array_equal(bits(planes[lvl][0]), bits(was[id(g)][0][lvl][0])) and np.array_equal(planes[lvl][1], was[id(g)][0][lvl][1])
            assert dirty[lvl][2] < dirty[lvl][0] and pub[lvl][2] < pub[lvl][0], (lvl, dirty[lvl], pub[lvl])
        assert index == was[id(g)][1]
    for g in [dst, src] + list(others.values()):
        g.close()
