"""CPU pin of tests/late_entry_cases.py, no device: the inputs of tests/test_gpu_late_entries.py meet the conditions that keep its
comparisons from being vacuous, and the faults it is there to see change an expected value of the committed cases.

* The lists are the issue's; every level gets the level-sized tile, a 1 x 1 tile and a full-width tile, and six crops.
* The statements of a level's metadata agree bit for bit: image_cases.metadata of the geometry tuple and the checkers'
  cast_cases.metadata, on every map and on every moved map.  (The third, the device's map_metadata, is the GPU file's.)
* The tile model equals image_cases.tile_loop, the reference loop's transcription, on the 2 x 2, 10 x 2 and 41 x 11 levels and on
  a level of the far frame, over every pose and tile size of the case.
* Faults of the tile box.  On every level of every frame map with an inexact reciprocal, and of the far frame, each fault that
  hands the box another number -- a swapped origin (where origin_x != origin_y), another level's reciprocal, level 0's cell
  length on a coarser level, a single fused multiply-add -- moves the 1 x 1 tile of at least one SENSITIVE pose of that level.
* An extents accumulator that starts at 0 gives another box on some level of every moved, reset, copied and merged case.
* A window slot of b * (W rounded up to 64) and a scan taken from row b - 1 give other scores on every map's batch.
* Every relocalisation row is defined by the reference; PICKS holds and stays within its cap; the moved cases dropped as
  undefined are named and at most two; outside the tied levels row 0's winner sees the map.

Durations on the build machine: this file 6.9 s (129 ids); the suite's other CPU files 260 s.
"""
import numpy as np
import pytest

import entry_geometry_cases as egc
import frame_cases as fc
import image_cases as ic
import late_entry_cases as lec
import moved_entry_cases as mec
import points_state_cases as psc
import reset_cases
from conftest import bits, oracle_kinds
from support import same

F = np.float32
MAPS = pytest.mark.parametrize("m", lec.MAPS, ids=egc.MAP_IDS)


def test_the_lists_are_the_issues():
    assert len(lec.MAPS) == 3 * 8 + 3 and len(lec.MAP_LAYOUTS) == 27 + 4
    assert [m.dims(m.levels - 1) for m in lec.MAPS[24:]] == [(10, 2), (2, 10), (2, 2)]
    assert lec.MOVED_CASES == psc.MOVED_CASES and len(lec.MOVED_CASES) == len(mec.MAP_LAYOUTS) * len(mec.READER_MOVES) + 2
    assert lec.RESET_LAYOUTS == reset_cases.MAP_LAYOUTS and lec.COPY_MAP is egc.map_of(*egc.COPY_FRAME)
    assert lec.BATCH_LENS == (200, 65, 0, 1, 64) and lec.BATCH_HALVES[:2] == egc.WINDOWS and lec.PADS == (67, 66, 64)
    assert len(lec.RELOC_CASES) == 24 + 3 * 2 and len(lec.TIED) == 3 and len(lec.RELOC_MOVED) == 2 * (1 + 2)
    for sx, sy in ((96, 40), (83, 22), (41, 11), (10, 2), (2, 10), (2, 2), (256, 256)):
        sizes = lec.tile_sizes(sx, sy)
        assert (sx, sy) in sizes and (1, 1) in sizes and (sx, min(sy, 3)) in sizes and len(set(sizes)) == len(sizes)
        assert all(1 <= tw <= sx and 1 <= th <= sy for tw, th in sizes)
        names = [name for name, _ in lec.crops(sx, sy)]
        assert names == ["whole"] + ["odd start, odd width"] * (sx >= 4) + ["last column", "last row", "overhangs two sides"]
        x0, y0, x1, y1 = dict(lec.crops(sx, sy))["overhangs two sides"]
        assert 0 <= x0 < sx <= x1 and 0 <= y0 < sy <= y1


@MAPS
def test_the_statements_of_the_metadata_agree(oracle_mod, m):
    geom = lec.geometry(m)
    for kind in oracle_kinds():
        o = m.checker(oracle_mod, kind)
        for lvl in range(m.levels):
            assert same(F(ic.metadata(geom, lvl)), F(lec.checker_metadata(o, lvl))), (m.id, kind, lvl)


@pytest.mark.parametrize("m,name", lec.MOVED_MAPS, ids=["%s-%s" % (m.id, name) for m, name in lec.MOVED_MAPS])
def test_the_statements_agree_on_the_moved_maps(oracle_mod, m, name):
    mv = psc.moved_case(oracle_mod, m, name)
    for kind in oracle_kinds():
        o = mec.reader_checker(oracle_mod, kind, m, name)
        for lvl in range(m.levels):
            assert same(F(ic.metadata(mv["geom"], lvl)), F(lec.checker_metadata(o, lvl))), (m.id, name, kind, lvl)
    assert not same(F(ic.metadata(mv["geom"], 0)), F(ic.metadata(lec.geometry(m), 0))), "the move changes the origin"


LOOP_LEVELS = [(egc.map_of(None, (256, 256, 8)), 7, (2, 2)), (egc.map_of(None, (333, 90, 6)), 5, (10, 2)),
               (egc.map_of(None, (333, 90, 6)), 3, (41, 11)), (egc.map_of(fc.FAR, (96, 40, 3)), 1, (48, 20))]


@pytest.mark.parametrize("m,lvl,dims", LOOP_LEVELS, ids=["%s-level%d" % (m.id, lvl) for m, lvl, _ in LOOP_LEVELS])
def test_the_tile_model_is_the_reference_loops_transcription(oracle_mod, m, lvl, dims):
    assert m.dims(lvl) == dims
    lo = lec.planes(oracle_mod, m)[lvl][0]
    sx, sy = dims
    c = lec.image_level(lec.geometry(m), lvl, sx, sy)
    grid = ic.published(lo)
    for tw, th in c["sizes"]:
        tiles, boxes = ic.tiles_model(lo, c["meta"], c["poses"], tw, th)
        for b, pose in enumerate(c["poses"]):
            tile, box = ic.tile_loop(grid, c["meta"], pose, tw, th)
            assert tuple(boxes[b]) == tuple(box) and np.array_equal(tiles[b], tile), (m.id, lvl, (tw, th), b)


@MAPS
def test_the_sensitive_poses_see_the_faults_of_the_tile_box(oracle_mod, m):
    geom = lec.geometry(m)
    for lvl in range(m.levels):
        sx, sy = m.dims(lvl)
        poses = lec.sensitive_poses(geom, lvl, sx, sy)
        assert 2 <= len(poses) <= 4 + 2 * len(lec.FAULTS) and np.isfinite(poses).all()
        meta = ic.metadata(geom, lvl)
        inv = F(F(1.0) / meta[2])
        near = [min(abs(float(c) - round(float(c))) for c in (F(F(p[0] - meta[0]) * inv), F(F(p[1] - meta[1]) * inv))) for p in poses]
        assert max(near) <= 1e-2, (m.id, lvl, "a sensitive pose lies next to an integer map coordinate", near)
        seen = lec.faults_seen(geom, lvl, poses, sx, sy)
        print(m.id, "level", lvl, "poses", len(poses), "boxes a fault moves", seen)
        if lec.held_to_faults(m):
            for fault in lec.FAULTS:
                if lec.fault_changes_a_number(fault, geom, lvl):
                    assert seen[fault] >= 1, (m.id, lvl, fault)
    # the un-sensitive poses alone: image_cases.poses puts no position next to an integer of an inexact frame
    assert len([x for x in lec.MAPS if lec.held_to_faults(x)]) >= 12


def test_an_accumulator_that_starts_at_zero_shows_on_every_state_case(oracle_mod):
    cases = lec.state_cases(oracle_mod)
    assert len(cases) == len(lec.MOVED_MAPS) + len(reset_cases.MAPS) + 2
    for name, levels in cases:
        other = [lvl for lvl, lo in enumerate(levels) if lec.zeroed_extents(lo) != ic.extents_model(lo)]
        print(name, "levels with another box", other)
        assert other, name
    committed = lec.merge_cases_of_this_file()["committed"]
    assert all(ic.extents_model(lo)[:2] == (0, 0) for lo, _ in committed["model"]), "the committed merge: a hull from (0, 0)"
    for m, name in lec.MOVED_MAPS:
        if (m.id, name) in psc.NOTHING_SURVIVES:
            # no OCCUPIED cell survives there; the corner that does is free space of frame_cases.map_planes, which is known: the
            # hull is that corner (d0 cells in from the window's edge), not empty, and the image holds 255 there and 127 elsewhere
            mv = psc.moved_case(oracle_mod, m, name)
            for lvl, (lo, _) in enumerate(mv["planes"]):
                sx, sy = m.dims(lvl)
                dx, dy = mv["d0"][0] >> lvl, mv["d0"][1] >> lvl
                assert dx > 0 > dy and ic.extents_model(lo) == (dx, 0, sx - 1, sy - 1 + dy), (m.id, lvl, ic.extents_model(lo))
                assert set(np.unique(ic.image_model(lo)).tolist()) == {127, 255}, (m.id, lvl)


@MAPS
def test_the_batch_sees_a_wrong_slot_and_a_wrong_scan_row(oracle_mod, m):
    centres, scans, step = lec.batch_case(oracle_mod, m)
    assert [len(s) for s in scans] == list(lec.BATCH_LENS) and np.isinf(centres[lec.INF_ROW, 2])
    assert np.isfinite(np.delete(centres, lec.INF_ROW, 0)).all() and len({tuple(c) for c in centres}) == 5
    finite = [b for b in range(5) if b != lec.INF_ROW]
    for half in lec.BATCH_HALVES:
        want = lec.expected_batch(oracle_mod, m, 0, half, "ho")
        W = len(want[0][0])
        assert np.isnan(want[lec.EMPTY_ROW][0]).all() and (bits(want[lec.EMPTY_ROW][1]) == 0).all()
        model = np.stack([np.full(W, 0.25, F) if w is None else np.nan_to_num(w[1], nan=-1.0) + F(b) for b, w in enumerate(want)])
        assert not np.array_equal(lec.slot_fault(model), model), (m.id, half, "a slot of b * W rounded up to 64")
        for kind in oracle_kinds()[1:]:
            other = lec.expected_batch(oracle_mod, m, 0, half, kind)
            for b in finite:
                if b != lec.EMPTY_ROW:
                    assert same(other[b][0], want[b][0]) and same(other[b][1], want[b][1]), (m.id, half, kind, b)
    half = lec.BATCH_HALVES[0]
    want = lec.expected_batch(oracle_mod, m, 0, half, "ho")
    wrong = lec.expected_batch(oracle_mod, m, 0, half, "ho", tag="row_fault", scan_of=lec.row_fault)
    differ = [b for b in finite if not same(np.nan_to_num(wrong[b][1]), np.nan_to_num(want[b][1]))]
    assert len(differ) == len(finite), (m.id, "a scan taken from row b - 1", differ)


@pytest.mark.parametrize("m,lvl", lec.RELOC_CASES, ids=lec.RELOC_IDS)
def test_every_relocalisation_row_is_defined_and_row_0_sees_the_map(oracle_mod, m, lvl):
    rows = lec.expected_reloc_batch(oracle_mod, m, lvl, "ho")   # asserts that the reference defines every row
    for kind in oracle_kinds()[1:]:
        for a, b in zip(rows, lec.expected_reloc_batch(oracle_mod, m, lvl, kind)):
            assert a["best_index"] == b["best_index"] and same(a["cand"], b["cand"]) and same(a["scores"], b["scores"]), (m.id, lvl, kind)
    print(m.id, "level", lvl, "winners", [r["best_index"] for r in rows], "likelihoods", [float(r["best_score"]) for r in rows])
    top = lec.topk_of(rows)
    for b, r in enumerate(rows):
        assert np.array_equal(top[b], r["index"]) and r["best_index"] >= 0, (m.id, lvl, b)
    if (m.id, lvl) in lec.TIED:
        assert all((r["scores"] == 0).all() and r["index"].tolist() == list(range(egc.RELOC_K)) for r in rows), (m.id, lvl)
    else:
        assert rows[0]["best_score"] > psc.SEES_THE_MAP, (m.id, lvl, rows[0]["best_score"])
        assert not same(rows[0]["scores"], rows[1]["scores"]) and not same(rows[0]["scores"], rows[2]["scores"])


def test_the_picks_hold_and_the_moved_drops_are_named(oracle_mod):
    assert len(lec.PICKS) <= lec.MAX_PICKS and lec.search_picks(oracle_mod) == lec.PICKS
    dropped = []
    for m, name, lvl in lec.RELOC_MOVED:
        rows = lec.expected_reloc_moved(oracle_mod, m, name, lvl, "ho")
        if rows is None:
            dropped.append((m.id, name, lvl))
            continue
        for kind in oracle_kinds()[1:]:
            for a, b in zip(rows, lec.expected_reloc_moved(oracle_mod, m, name, lvl, kind)):
                assert a["best_index"] == b["best_index"] and same(a["scores"], b["scores"]), (m.id, name, lvl, kind)
        print(m.id, name, "level", lvl, "winners", [r["best_index"] for r in rows], "likelihoods", [float(r["best_score"]) for r in rows])
    print("moved relocalisation cases the reference does not define:", dropped)
    assert tuple(dropped) == tuple(lec.MOVED_DROPPED) and len(dropped) <= lec.MAX_DROPS


@pytest.mark.parametrize("m,name", [(m, name) for m in lec.RELOC_MOVED_MAPS for name in mec.READER_MOVES],
                         ids=["%s-%s" % (m.id, name) for m in lec.RELOC_MOVED_MAPS for name in mec.READER_MOVES])
def test_the_move_changes_the_batch_scores(oracle_mod, m, name):
    half = lec.BATCH_HALVES[0]
    o = mec.reader_checker(oracle_mod, "ho", m, name)
    moved = lec.expected_batch(oracle_mod, m, 0, half, "ho", o=o, tag=("moved", name))
    stay = lec.expected_batch(oracle_mod, m, 0, half, "ho")
    assert not same(moved[0][1], stay[0][1]), (m.id, name)
