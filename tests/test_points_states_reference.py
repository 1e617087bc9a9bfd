"""CPU pin of tests/points_state_cases.py, no device: the inputs of tests/test_gpu_points_states.py meet the conditions that keep
its comparisons from being vacuous, so an input that drifts fails here instead of passing blind on the GPU.

* The statements of the expected points agree bit for bit on every map, level and box: the numpy model with
  points_cases.world_from_map of the geometry tuple, and the checkers' own cells (occupancy_grid == 100, row-major) through
  their world_coords_pose times fp32 1 / resolution; world_from_map equals frame_cases.frame_numpy's worldTmap.  The same on the
  moved maps against moved_entry_cases.reader_checker.  (The third statement, the device's getWorldCoordsPose, is the GPU file's.)
* Every level of every map holds an occupied cell, level 0 a hundred and more.
* The frames see the faults the GPU file is there for.  Per frame, on level 0 of both geometries: the points differ from those
  of the affine written as a single fused multiply-add, fma(l00, x, t0) (emulated in float64, then rounded), in at least one
  cell; from those of level 1's transform in every cell; and level 1's points from those under level 1's scale.  Fused and
  unfused AGREE on every cell in these frames:
      res1_start0.7_0.2      (the cell length is 1: the product is exact)
      res0.025_start-50_37   (the far frame: a translation of 120 m, under whose ulp the product's rounding error vanishes)
      res0.125_start0.5_0.5  (the control: a cell length of 2^-3)
  and differ on the five others, in 265 to 834 of the 1060 cells.  At least five of the seven frames besides the control must
  differ; the test prints the list.  A contraction of the expression AS WRITTEN, fma(l00, x, l01 * y) + t0, cannot show on any map:
  l01 is 0 on every map hsm_create makes, the addend an exact zero.  The test asserts that too, so the fault to plant is the
  fused translation.
* points_cases.brute_force agrees with kept_cells on the levels of fewer than 64 cells and on the boxes one cell wide.
* Every alignment case is defined, has a winner that sees the map (but for the deep maps' coarsest search level, where every
  likelihood is 0: points_state_cases.ALL_ZERO) and between 41 and 1100 points; PICKS holds and stays within its cap.
* Every moved map has a level with fewer occupied cells than before the move, and a cell that survives on level 0 -- but for
  the two frame maps under one_left (points_state_cases.NOTHING_SURVIVES), whose surviving corner lies outside the room: there
  no cell survives on any level, which is asserted as well.

Durations on the build machine: this file 3.3 s; its siblings test_entry_geometries_reference.py 4.4 s and
test_newer_entries_reference.py 49 s.
"""
import numpy as np
import pytest

import frame_cases as fc
import moved_entry_cases as mec
from merge_cases import level_scale
import points_cases as pc
import points_state_cases as psc
from conftest import bits, oracle_kinds

F = np.float32
MAPS = pytest.mark.parametrize("m", psc.MAPS, ids=[m.id for m in psc.MAPS])


def test_the_lists_are_the_issues():
    assert len(psc.MAPS) == 2 * 8 + 3 and len(psc.MAP_LAYOUTS) == 19 + 3
    assert [m.geom for m in psc.MAPS[16:]] == [(333, 90, 6), (90, 333, 6), (256, 256, 8)]
    assert {m.geom for m in psc.MAPS[:16]} == {(90, 24, 2), (96, 40, 3)} and {m.frame for m in psc.MAPS[:16]} == set(fc.FRAMES)
    assert len(psc.MOVED_CASES) == len(mec.MAP_LAYOUTS) * len(mec.READER_MOVES) + 2
    assert len(psc.ALIGN_CASES) == 4 * 2 + 2 * 2 * 2 + 2 and len(set(psc.ALIGN_IDS)) == len(psc.ALIGN_IDS)
    assert [m.dims(m.levels - 1) for m in psc.MAPS[16:]] == [(10, 2), (2, 10), (2, 2)]
    for sx, sy in ((96, 40), (10, 2), (2, 10), (2, 2), (83, 22)):
        boxes = dict(psc.level_boxes(sx, sy))
        assert ("odd start, odd width" in boxes) == (sx >= 4) and boxes["last column"] == (sx - 1, 0, sx - 1, sy - 1)
        assert boxes["last row"] == (0, sy - 1, sx - 1, sy - 1) and boxes["whole"] is None
        if sx >= 4:
            x0, _, x1, _ = boxes["odd start, odd width"]
            assert x0 % 2 == 1 and (x1 - x0 + 1) % 2 == 1 and x1 < sx


def assert_statements_agree(what, o, lo, geom, lvl, resolution):
    sy, sx = lo.shape
    for name, box in psc.level_boxes(sx, sy):
        cells, pts = psc.checker_points(o, lvl, resolution, box)
        assert np.array_equal(cells, pc.kept_cells(lo, box, 1)), (what, lvl, name, "the occupied cells")
        want, count = psc.model(lo, geom, lvl, box, 1, sx * sy)
        assert count == (len(cells), len(cells)) and np.array_equal(bits(want), bits(pts)), (what, lvl, name, "the points")
        for every in psc.EVERY:   # (thinning and the cap select among those cells and points)
            kept = len(pc.kept_cells(lo, box, every))
            for cap in psc.caps(kept):
                got, cnt = psc.model(lo, geom, lvl, box, every, cap)
                assert cnt == (min(kept, cap), kept) and np.array_equal(bits(got), bits(pts[::every][:cap])), (what, lvl, name, every, cap)


@MAPS
def test_the_statements_of_the_points_agree(oracle_mod, m):
    geom = psc.geometry(m)
    for kind in oracle_kinds():
        o = m.checker(oracle_mod, kind)
        assert bits(F(o.scale_to_map())) == bits(pc.scale_to_map(geom))
        for lvl, (lo, _) in enumerate(psc.planes(oracle_mod, m)):
            assert_statements_agree((m.id, kind), o, lo, geom, lvl, m.resolution)
    if m.kind == "frame":
        for lvl, lv in enumerate(fc.frame_numpy(m.frame, m.geom)):
            l00, l10, l01, l11, t0, t1 = pc.world_from_map(geom, lvl)
            assert np.array_equal(bits(F([l00, l01, l10, l11, t0, t1])), bits(F(lv["w"]))), (m.id, lvl)


@pytest.mark.parametrize("m,name", psc.MOVED_MAPS, ids=["%s-%s" % (m.id, name) for m, name in psc.MOVED_MAPS])
def test_the_statements_agree_on_the_moved_maps_and_the_move_shows(oracle_mod, m, name):
    mv = psc.moved_case(oracle_mod, m, name)
    old = psc.planes(oracle_mod, m)
    for kind in oracle_kinds():
        o = mec.reader_checker(oracle_mod, kind, m, name)
        for lvl, (lo, _) in enumerate(mv["planes"]):
            assert_statements_agree((m.id, name, kind), o, lo, mv["geom"], lvl, m.resolution)
    before = [int((lo > 0).sum()) for lo, _ in old]
    after = [int((lo > 0).sum()) for lo, _ in mv["planes"]]
    print(m.id, name, "occupied cells before", before, "after", after)
    assert any(a < b for a, b in zip(after, before)) and all(a <= b for a, b in zip(after, before))
    if (m.id, name) in psc.NOTHING_SURVIVES:
        assert after == [0] * m.levels, (m.id, name, after)
        return
    assert after[0] >= 1, "no cell survives on level 0"
    # the old frame gives other points for the cells that survived: an extraction that missed the new transform shows
    stale, _ = psc.model(mv["planes"][0][0], psc.geometry(m), 0, None, 1, 10 ** 6)
    fresh, _ = psc.model(mv["planes"][0][0], mv["geom"], 0, None, 1, 10 ** 6)
    assert (bits(stale) != bits(fresh)).any(axis=1).all()


@MAPS
def test_every_level_holds_cells(oracle_mod, m):
    occ = [int((lo > 0).sum()) for lo, _ in psc.planes(oracle_mod, m)]
    assert all(n >= 1 for n in occ) and occ[0] >= 100, (m.id, occ)
    for lvl, (lo, _) in enumerate(psc.planes(oracle_mod, m)):
        assert lo.shape == m.dims(lvl)[::-1]


def test_the_frames_see_a_fused_affine_and_another_levels_transform(oracle_mod):
    differ, agree = [], []
    for frame in fc.FRAMES:
        n_fused, n_level, n_scale = 0, 0, 0
        for geom3 in psc.GEOMETRIES:
            m = next(x for x in psc.MAPS if x.frame == frame and x.geom == geom3)
            geom = psc.geometry(m)
            pl = psc.planes(oracle_mod, m)
            cells = pc.kept_cells(pl[0][0], None, 1)
            affine, scale = psc.frame_of(geom, 0)
            want = pc.cell_points(cells, affine, scale)
            contracted, fused = psc.fused_points(cells, affine, scale)
            assert affine[1] == 0 and affine[2] == 0 and np.array_equal(bits(contracted), bits(want)), (m.id, "l01 == 0: an exact addend")
            n_fused += int((bits(fused) != bits(want)).any(axis=1).sum())
            n_level += int((bits(pc.cell_points(cells, pc.world_from_map(geom, 1), scale)) != bits(want)).any(axis=1).sum())
            # level 1's own cells with level 1's scale in place of level 0's
            c1 = pc.kept_cells(pl[1][0], None, 1)
            a1 = pc.world_from_map(geom, 1)
            n_scale += int((bits(pc.cell_points(c1, a1, level_scale(geom, 1))) != bits(pc.cell_points(c1, a1, scale))).any(axis=1).sum())
        print(fc.fid(frame), "cells of level 0 whose point differs: fused", n_fused, "level 1's transform", n_level,
              "| of level 1 under its own scale", n_scale)
        assert n_level >= 1 and n_scale >= 1, fc.fid(frame)
        if frame != fc.CONTROL:
            (differ if n_fused >= 1 else agree).append(fc.fid(frame))
    print("fused and unfused differ on", differ, "and agree on", agree)
    assert len(differ) >= 5 and len(differ) + len(agree) == 7, (differ, agree)
    assert fc.fid(fc.FRAMES[1]) in differ, "the frame the GPU file's stream and alignment cases lean on"


def test_brute_force_agrees_on_the_small_levels_and_the_one_cell_wide_boxes(oracle_mod):
    small = wide1 = 0
    for m in psc.MAPS[15:]:   # the control frame of 96 x 40 x 3 and the deep pyramids: every plane the cases have is among them
        for lvl, (lo, _) in enumerate(psc.planes(oracle_mod, m)):
            sy, sx = lo.shape
            for name, box in psc.level_boxes(sx, sy):
                if sx * sy >= psc.SMALL_LEVEL and name != "last column":
                    continue
                small += sx * sy < psc.SMALL_LEVEL
                wide1 += name == "last column"
                for every in psc.EVERY:
                    kept = len(pc.kept_cells(lo, box, every))
                    for cap in psc.caps(kept):
                        cells, count = pc.brute_force(lo, box, every, cap)
                        assert count == (min(kept, cap), kept), (m.id, lvl, name, every, cap)
                        assert np.array_equal(np.array(cells, np.int64).reshape(-1, 2), pc.kept_cells(lo, box, every)[:cap]), (m.id, lvl, name)
    assert small == 4 + 3 + 4 + 3 and wide1 == 3 + 6 + 6 + 8   # 10 x 2, 2 x 10, 4 x 4, 2 x 2 (a level 2 cells wide has no odd box)


@pytest.mark.parametrize("c", psc.ALIGN_CASES, ids=psc.ALIGN_IDS)
def test_every_align_case_is_defined_and_has_a_winner(oracle_mod, c):
    pts, (written, kept) = psc.align_points(oracle_mod, c)
    assert psc.MIN_POINTS < written == kept <= psc.MAX_POINTS, (c.id, written, kept)
    want = psc.expected_align(oracle_mod, "ho", c)   # asserts that the reference defines the case
    for kind in oracle_kinds()[1:]:
        other = psc.expected_align(oracle_mod, kind, c)
        assert other["best_index"] == want["best_index"] and np.array_equal(bits(other["best_pose"]), bits(want["best_pose"])), c.id
        assert bits(other["best_score"]) == bits(want["best_score"]), c.id
    print(c.id, "points", written, "guess", psc.align_guess(oracle_mod, c).tolist(), "winner", want["best_index"], want["best_pose"].tolist(),
          "likelihood", float(want["best_score"]))
    assert want["best_index"] >= 0 and np.isfinite(want["best_pose"]).all()
    if c.id in psc.ALL_ZERO:
        assert want["best_score"] == 0 and (want["scores"] == 0).all(), c.id
    elif c.id in psc.WANDERS:
        assert 0 < want["best_score"] < psc.SEES_THE_MAP and len(psc.WANDERS) == 1, (c.id, want["best_score"])
    else:
        assert want["best_score"] > psc.SEES_THE_MAP, (c.id, want["best_score"])
        # the world did not move: the winner lies within a cell of the search level and 0.05 rad of the identity
        cell = psc.align_step(oracle_mod, c)[0]
        assert abs(want["best_pose"][0]) <= cell and abs(want["best_pose"][1]) <= cell and abs(want["best_pose"][2]) <= 0.05, c.id


def test_the_picks_hold_and_stay_within_their_cap(oracle_mod):
    assert len(psc.PICKS) <= psc.MAX_PICKS and set(psc.PICKS) <= set(psc.ALIGN_IDS)
    assert psc.search_picks(oracle_mod) == psc.PICKS
    assert len(psc.ALL_ZERO) == 4
