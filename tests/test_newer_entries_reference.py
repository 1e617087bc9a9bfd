"""CPU pin of tests/newer_entry_cases.py, no device: the inputs of tests/test_gpu_newer_entries.py meet the conditions that
keep its comparisons from being vacuous, so an input that drifts fails here instead of passing blind on the GPU.

Covariance cases: both checkers give the same bits, the reference defines every case, the poses see the map on every level of at
least entry_geometry_cases.MIN_SIDE cells both ways, and each border pose there stands inside [0, lim] with a sigma point
outside.  Below MIN_SIDE only definedness and finiteness are asked -- and on the levels with a side of 2 cells (10 x 2, 2 x 10,
2 x 2: lim = 0) finiteness of the likelihoods alone: every beam at every sigma point is off such a level, all seven likelihoods
are 0 and the reference's weighted mean is 0 / 0, so its covariances are NaN for every scan.  That is the reference's answer and
the device has to give it; the pin holds that it happens on those levels and, elsewhere, to the scan of one beam alone and
never on level 0.

Merge cases: the numpy model restates the formula of map_merge_box.h, so a convention shared by both passes every bit-for-bit
test.  Here the model's affine is tied to what the two contexts' own world-to-map transforms say: the src cell the model reads
for a dst cell lies, carried through the src checker, p_dst = R(theta) p_src + t and the dst checker, within half a cell of that
dst cell -- per axis of SRC's grid, where the nearest cell was taken -- plus 8 fp32 ulps of the case's largest coordinate.  That
margin is the only tolerance of this file and of the GPU file; it is computed per case and printed.  Two wrong models (theta
negated; the two offsets swapped) fail the same check.
"""
import math

import numpy as np
import pytest

import entry_geometry_cases as egc
import merge_cases as mc
import newer_entry_cases as nc
from conftest import oracle_kinds
from support import same

F = np.float32
COV = pytest.mark.parametrize("m", nc.COV_MAPS, ids=[m.id for m in nc.COV_MAPS])
ULPS = 8


def test_the_lists_are_the_issues():
    assert [m.id for m in nc.COV_MAPS[:8]] == [egc.map_of(f, g).id for g in ((90, 24, 2), (96, 40, 3)) for f in nc.COV_FRAMES]
    assert [m.geom for m in nc.COV_MAPS[8:]] == [(333, 90, 6), (90, 333, 6), (256, 256, 8)]
    assert sum(layout == "plane" for _, layout in nc.COV_MAP_LAYOUTS) == 3
    assert nc.CSR_LENS == (0, 1, 63, 64, 65, 128, 129, 0, 181) and nc.SHARED_BATCHES == (1, 3, 4, 5)
    assert list(nc.PAIRS) == ["frames", "far", "deep", "tiny", "strip"]
    assert nc.PAIRS["strip"][0][2] == 16 * 2049 + 5 and nc.PAIRS["tiny"][0][3] == 8
    assert len(nc.MERGE_CASES) == 4 * 5 + 2 and len(nc.MERGE_RUNS) == 2 * 4 * 5 + 3
    assert len(nc.MOVED_CASES) == 2 * 2 * 3
    n_cases = sum(m.levels * (2 + len(nc.SHARED_BATCHES)) for m in nc.COV_MAPS)
    for m in nc.COV_MAPS:   # fewer than one case in ten per map was searched
        picked = sum(1 for k in nc.PICKS if k[1] == m.id)
        assert 10 * picked < m.levels * (2 + len(nc.SHARED_BATCHES)), (m.id, picked)
    assert n_cases > 0


# ---- covariance ------------------------------------------------------------------------------------------------------------------------
@COV
def test_covariance_cases_are_defined_and_see_the_map(oracle_mod, m):
    guard = m.checker(oracle_mod, "ho")
    u0 = guard.undefined_reads()
    for lvl in range(m.levels):
        want = nc.expected_cov(oracle_mod, m, lvl, "ho")
        assert guard.undefined_reads() == u0, (m.id, lvl, "the reference does not define a case: replace it in the case module")
        for kind in oracle_kinds()[1:]:
            other = nc.expected_cov(oracle_mod, m, lvl, kind)
            for name in want:
                for k in ("cm", "cw", "l7"):
                    nan = np.isnan(want[name][k])
                    assert np.array_equal(nan, np.isnan(other[name][k])) and same(want[name][k][~nan], other[name][k][~nan]), (lvl, name, k)
        for name, poses, scans in nc.cov_batches(oracle_mod, m, lvl):
            empty = np.array([len(s) == 0 for s in scans])
            for k in ("cm", "cw", "l7"):
                assert np.isnan(want[name][k][empty]).all(), (m.id, lvl, name, k)
            assert np.isfinite(want[name]["l7"][~empty]).all(), (m.id, lvl, name)
            if min(m.dims(lvl)) > 2:   # (the scan of ONE beam ends off the coarse levels of the long maps: finite on level 0)
                full = np.array([len(s) > (60 if lvl else 0) for s in scans])
                assert np.isfinite(want[name]["cm"][full]).all() and np.isfinite(want[name]["cw"][full]).all(), (m.id, lvl, name)
                dead = ~empty & ~np.isfinite(want[name]["cm"]).all(1)
                assert (want[name]["l7"][dead] == 0).all(), (m.id, lvl, name, "a NaN covariance comes from seven likelihoods of 0 alone")
            else:   # lim = 0: every beam at every sigma point is off the level, seven likelihoods of 0, and their mean is 0 / 0
                assert (want[name]["l7"][~empty] == 0).all(), (m.id, lvl, name)
                assert np.isnan(want[name]["cm"][~empty]).all() and np.isnan(want[name]["cw"][~empty]).all(), (m.id, lvl, name)
        if min(m.dims(lvl)) < egc.MIN_SIDE:
            continue
        lh = want["csr"]["lh"]
        assert (lh[np.asarray(nc.CSR_LENS) > 60] > 0.05).all(), (m.id, lvl, "the CSR poses do not see the map", lh)
        for B in nc.SHARED_BATCHES:
            assert (want["shared x%d" % B]["lh"] > 0.05).all(), (m.id, lvl, B)
        poses, _, maps = nc.cov_level_case(oracle_mod, m, lvl)["border"]
        limx, limy = m.dims(lvl)[0] - 2, m.dims(lvl)[1] - 2
        assert len(maps) == 9
        for w, mp in zip(poses, maps):
            pm = guard.map_coords_pose(lvl, w)
            assert 0 <= pm[0] <= limx and 0 <= pm[1] <= limy, (m.id, lvl, mp, pm)
        for mp in maps[:8]:   # the sigma points stand 1.5 cells off the pose along each axis
            assert mp[0] - 1.5 < 0 or mp[0] + 1.5 > limx or mp[1] - 1.5 < 0 or mp[1] + 1.5 > limy, (m.id, lvl, mp)


def test_the_small_levels_put_every_sigma_point_off_the_map():
    for dims in ((10, 2), (2, 10), (2, 2)):
        maps = nc.border_map_poses(dims)
        assert len(maps) == 5
        lim = (dims[0] - 2, dims[1] - 2)
        for mp in maps:   # along the short axis both sigma points are outside [0, lim]
            a = int(np.argmin(dims))
            assert mp[a] - 1.5 < 0 and mp[a] + 1.5 > lim[a], (dims, mp)
    assert len(nc.border_map_poses((4, 4))) == 9


# ---- merge: the model's affine against the contexts' own transforms ------------------------------------------------------------------------
def nearest(aff, box, ssx, ssy):
    """steps 1-2 of the rule for the cells of `box` with the affine `aff` = (c, s, bx, by) in double -> (ix, iy, inside):
    merge_cases.sampled's arithmetic, the affine an argument"""
    c, s, bx, by = (F(v) for v in aff)
    x0, y0, x1, y1 = box
    with np.errstate(over="ignore", invalid="ignore"):
        x = np.arange(x0, x1 + 1, dtype=F)[None, :]
        y = np.arange(y0, y1 + 1, dtype=F)[:, None]
        mx = ((c * x).astype(F) + (s * y).astype(F)).astype(F) + bx
        my = ((F(-s) * x).astype(F) + (c * y).astype(F)).astype(F) + by
        rx, ry = np.floor(mx + F(0.5)), np.floor(my + F(0.5))
    inside = (rx >= 0) & (rx < ssx) & (ry >= 0) & (ry < ssy)
    return np.where(inside, rx, 0).astype(np.int64), np.where(inside, ry, 0).astype(np.int64), inside


def margin_cells(gd, gs, t, level):
    """ULPS fp32 ulps of the largest number of the case on `level`, in cells: a cell coordinate, an offset or a translation"""
    scale = float(mc.level_scale(gd, level))
    big = max([gd[1] >> level, gd[2] >> level, gs[1] >> level, gs[2] >> level] +
              [abs(float(v)) * scale for v in mc.offsets(gd) + mc.offsets(gs)] + [abs(float(t[0])) * scale, abs(float(t[1])) * scale] +
              [abs(v) for v in mc.affine(gd, gs, level, t)[2:]])
    return ULPS * float(np.spacing(F(big)))


def affine_excess(aff, box, o_dst, o_src, gs, t, level, stride=1):
    """the largest distance, in cells of src's grid and per axis, between a dst cell's centre and the src cell the affine `aff`
    reads for it, both taken to the world by their checkers and src's through p_dst = R(theta) p_src + t; None without a sample"""
    ssx, ssy = mc.level_size(gs, level)
    ix, iy, inside = nearest(aff, box, ssx, ssy)
    ys, xs = np.nonzero(inside)
    if len(xs) == 0:
        return None
    pick = slice(None, None, stride)
    ys, xs = ys[pick], xs[pick]
    th = float(F(t[2]))
    c, s = math.cos(th), math.sin(th)
    cell = 1.0 / float(mc.level_scale(gs, level))
    worst = 0.0
    for yy, xx in zip(ys, xs):
        ps = o_src.world_coords_pose(level, F([ix[yy, xx], iy[yy, xx], 0])).astype(np.float64)
        pd = o_dst.world_coords_pose(level, F([box[0] + xx, box[1] + yy, 0])).astype(np.float64)
        dx = (c * ps[0] - s * ps[1] + float(F(t[0]))) - pd[0]
        dy = (s * ps[0] + c * ps[1] + float(F(t[1]))) - pd[1]
        worst = max(worst, abs(c * dx + s * dy) / cell, abs(-s * dx + c * dy) / cell)   # back on src's axes
    return worst


def plain_checker(oracle_mod, geom):
    return oracle_mod.Oracle("ho", geom[0], geom[1], geom[2], geom[3], geom[4])


def check_affine(case, o_dst, o_src, what, stride=1):
    gd, gs, t = case["gd"], case["gs"], case["t"]
    turned = float(t[2]) != 0.0
    apart = mc.offsets(gd) != mc.offsets(gs)
    failed = {"theta negated": not turned, "offsets swapped": not apart}   # (a wrong model that IS the model cannot fail)
    for lvl, (_, box) in enumerate(case["model"]):
        margin = margin_cells(gd, gs, t, lvl)
        _, ix, iy, inside = mc.sampled(case["src"][lvl], gd, gs, lvl, t, box)
        mine = nearest(mc.affine(gd, gs, lvl, t), box, *mc.level_size(gs, lvl))
        assert np.array_equal(inside, mine[2]) and np.array_equal(ix, mine[0]) and np.array_equal(iy, mine[1]), (what, lvl)
        if not inside.any():   # (a box is grown by a cell: on a level of 10 x 2 it can be all there is)
            assert lvl > 0 and same(case["model"][lvl][0], case["dst"][lvl]), (what, lvl, "no sample inside src")
            continue
        worst = affine_excess(mc.affine(gd, gs, lvl, t), box, o_dst, o_src, gs, t, lvl, stride)
        print(what, "level", lvl, "margin %.3g cells," % margin, "largest distance %.6f cells" % worst)
        assert worst <= 0.5 + margin, (what, lvl, worst, margin)
        wrong = {"theta negated": mc.affine(gd, gs, lvl, F([t[0], t[1], -t[2]])), "offsets swapped": mc.affine(gs, gd, lvl, t)}
        for name, aff in wrong.items():
            w = affine_excess(aff, box, o_dst, o_src, gs, t, lvl, stride)
            failed[name] = failed[name] or w is None or w > 0.5 + margin
        # the staged route reads the same cells: every inside sample lies in the src box it copies
        sb = mc.merge_src_box(gd, gs, lvl, t)
        assert (ix[inside] >= sb[0]).all() and (ix[inside] <= sb[2]).all() and (iy[inside] >= sb[1]).all() and \
            (iy[inside] <= sb[3]).all(), (what, lvl, sb)
        # the box holds every cell the rule changes: visit the whole level
        sx, sy = mc.level_size(gd, lvl)
        whole, _ = mc.merge_model(case["dst"][lvl], case["src"][lvl], gd, gs, lvl, t, visit=(0, 0, sx - 1, sy - 1))
        assert same(whole, case["model"][lvl][0]), (what, lvl, box)
    assert all(failed.values()), (what, "a wrong model passes the check", failed)


@pytest.mark.parametrize("pair,name", nc.MERGE_CASES, ids=nc.MERGE_IDS)
def test_merge_models_affine_is_the_contexts_own(oracle_mod, pair, name):
    case = nc.merge_case(pair, name)
    changed = nc.conditions(case, (pair, name))
    tiles = [nc.box_tiles(box) for _, box in case["model"]]
    print(pair, name, "cells changed on level 0:", changed, "tiles per level:", tiles)
    if (pair, name) == ("strip", "identity"):
        assert tiles[0] == 2050 > nc.MAX_GRID, "the tile loop's second trip"
    assert len(case["model"]) == case["gd"][3]
    o_dst, o_src = plain_checker(oracle_mod, case["gd"]), plain_checker(oracle_mod, case["gs"])
    check_affine(case, o_dst, o_src, (pair, name), stride=nc.STRIP_STRIDE if pair == "strip" else 1)
    o_dst.close()
    o_src.close()


def test_the_pairs_reach_what_they_are_there_for():
    gd, gs = nc.PAIRS["frames"]
    assert float(mc.level_scale(gd, 0)) * 0.03 != 1.0 and gs[4][0] < 0 and gs[4][1] > 1
    for name in nc.PAIR_TRANSFORMS:   # the far frame: offsets of thousands of cells
        a = mc.affine(*nc.PAIRS["far"], 0, nc.transform("far", name))
        assert max(abs(float(v)) * float(mc.level_scale(nc.PAIRS["far"][0], 0)) for v in mc.offsets(nc.PAIRS["far"][0])) > 1000
        assert abs(a[2]) < 200 and abs(a[3]) < 200   # ... which the translation takes back
    assert [mc.level_size(nc.PAIRS["deep"][0], l) for l in (3, 5)] == [(41, 11), (10, 2)]
    assert mc.level_size(nc.PAIRS["deep"][1], 5) == (2, 10) and mc.level_size(nc.PAIRS["tiny"][0], 7) == (2, 2)
    for lvl in range(8):   # levels narrower than a slot and lower than a tile are reached with a body of 0 groups
        box = nc.merge_case("tiny", "theta_0.3")["model"][lvl][1]
        assert box == (0, 0, (256 >> lvl) - 1, (256 >> lvl) - 1)


@pytest.mark.parametrize("m,move,side", nc.MOVED_CASES, ids=nc.MOVED_IDS)
def test_moved_merge_models_affine_is_the_moved_checkers(oracle_mod, m, move, side):
    case = nc.moved_case(oracle_mod, m, move, side)
    changed = nc.conditions(case, (m.id, move, side))
    print(m.id, move, side, "d0", case["d0"], "cells changed on level 0:", changed)
    moved_dst, moved_src = side in ("dst", "both"), side in ("src", "both")
    assert (case["gd"][4] != nc.geometry_of(m)[4]) == moved_dst and (case["gs"][4] != nc.geometry_of(m)[4]) == moved_src
    o_dst, o_src = (nc.moved_side_checker(oracle_mod, m, move, x) for x in (moved_dst, moved_src))
    check_affine(case, o_dst, o_src, (m.id, move, side))
    # the creation-time start gives another model: a merge that ignores the move shows
    stale = mc.merge_pyramid(case["dst"], case["src"], nc.geometry_of(m), nc.geometry_of(m), case["t"])
    if side != "both":
        assert not same(stale[0][0], case["model"][0][0]), "the move must matter to the merge"
