"""CPU pin of tests/entry_geometry_cases.py, no device: the cases of tests/test_gpu_entry_geometries.py on the checkers alone, so
that its comparisons cannot be vacuous.  Both checkers give the same bits on every cast, ray, window and relocalisation case and
read nothing the reference does not define; the frames are the ones frame_cases counts; the published origin is the numpy frame
statement's; the casts hit and miss, along both axes where the map is not square; the windows see the map; and the expected casts
change when the origin's components are swapped or another level's reciprocal is used.

Where the conditions of the issue cannot be met, they are narrowed for the maps concerned and for nothing else:

  * "a tenth of the general poses' rays hit at half the diagonal" holds on the 64 x 64 and 96 x 40 frames.  On the others a ray of
    half the diagonal that starts inside the room ends off the level whatever the seed (cast_cases.poses takes 16 of its 20
    general poses from the truth as they are): 90 x 24 leaves a cone of some ten degrees either side of the x axis, 4 .. 6 % of
    the rays; the deep maps' loops run 170 (333 x 90) and 180 (256 x 256) cells from nothing, under 1 %.  There the tenth is
    demanded at the added range, 0.45 of the shorter side (entry_geometry_cases.range_maxes); at half the diagonal at least one
    ray hits and a tenth miss.
  * "hits with |dy| > |dx| and with |dx| > |dy| on maps with sx != sy": at half the diagonal no ray along the shorter axis has
    both ends on the level (range_maxes says why), on any of these maps; demanded at the added range.
  * "the edge pose half a cell below row 0 hits on level 0 of every frame": on 90 x 24 half the diagonal is longer than half the
    width, the pose stands at the middle column and the beam table holds no direction between 15 and 31 degrees off the axis from
    it; demanded at the range the tenth is demanded at.
"""
import numpy as np
import pytest

import cast_cases
import entry_geometry_cases as eg
import frame_cases as fc
import window_cases
from conftest import bits, oracle_kinds
from support import same

MAPS = pytest.mark.parametrize("m", eg.MAPS, ids=eg.MAP_IDS)


def same_rays(got, want):
    (d, h), (rd, rh) = got, want
    has = rd >= 0
    return same(d, rd) and same(h[has], rh[has]) and bool(np.isnan(h[~has]).all())


def test_the_list_is_the_issues():
    assert [(m.frame, m.geom) for m in eg.MAPS if m.kind == "frame"] == [(f, g) for g in fc.GEOMETRIES for f in fc.FRAMES]
    assert fc.GEOMETRIES == [(64, 64, 2), (90, 24, 2), (96, 40, 3)] and len(fc.FRAMES) == 8
    deep = [m for m in eg.MAPS if m.kind == "deep"]
    assert [m.geom for m in deep] == [(333, 90, 6), (90, 333, 6), (256, 256, 8)]
    assert [deep[0].dims(l) for l in range(6)] == [(333, 90), (166, 45), (83, 22), (41, 11), (20, 5), (10, 2)]
    assert deep[2].dims(7) == (2, 2)
    assert sorted(m.id for m in eg.MAPS if m.planes_too) == sorted([eg.map_of(None, (333, 90, 6)).id] +
                                                                    [eg.map_of(fc.FRAMES[1], g).id for g in fc.GEOMETRIES])
    assert eg.FANS == (1, 63, 64, 65, 200) and eg.N_BEAMS == 200 and eg.N_RAYS == 500
    assert eg.WINDOWS == ((3, 2, 1), (40, 0, 0)) and eg.SCAN_LENS == (1, 65, 200)
    assert (eg.RELOC_HALF, eg.RELOC_K, eg.RELOC_ANGLE) == ((4, 4, 3), 8, 0.05)


def test_the_frames_are_what_frame_cases_counts():
    counts = {}
    for frame in fc.FRAMES:
        facts = fc.frame_facts(frame, fc.GEOMETRIES[0])
        assert any(facts.values()) == (frame != fc.CONTROL), (frame, facts)
        for k, v in facts.items():
            counts[k] = counts.get(k, 0) + int(v)
    assert all(v >= 2 for v in counts.values()), counts
    facts = fc.frame_facts(eg.SENSITIVE_FRAME, fc.GEOMETRIES[0])
    assert facts["unequal translations"] and facts["fractional translation"] and facts["inverse is not the cell length"], facts


@MAPS
def test_metadata_is_the_numpy_frame_statement(oracle_mod, m):
    """origin = world_coords_numpy of (0, 0) minus half a cell, on every level, by both checkers"""
    lv = fc.frame_numpy((m.resolution, m.start), m.geom)
    for kind in oracle_kinds():
        o = m.checker(oracle_mod, kind)
        for lvl in range(m.levels):
            w = fc.world_coords_numpy(lv[lvl], np.zeros(3, np.float32))
            half = np.float32(lv[lvl]["cell"]) * np.float32(0.5)
            want = (float(np.float32(w[0] - half)), float(np.float32(w[1] - half)), float(lv[lvl]["cell"]))
            assert cast_cases.metadata(o, lvl) == want, (kind, lvl, cast_cases.metadata(o, lvl), want)
            assert o.level_info(lvl)[:2] == m.dims(lvl)


@MAPS
def test_both_checkers_agree_on_every_cast_and_ray(oracle_mod, m):
    kinds = oracle_kinds()
    for lvl in range(m.levels):
        c = eg.level_case(oracle_mod, m, lvl)
        res = np.float32(c["meta"][2])
        first = eg.expected(oracle_mod, m, lvl, kinds[0])
        for kind in kinds[1:]:
            assert np.array_equal(m.checker(oracle_mod, kind).occupancy_grid(lvl), c["grid"]), (kind, lvl)
            other = eg.expected(oracle_mod, m, lvl, kind)
            assert same_rays(other["rays"], first["rays"]), (kind, lvl, "rays")
            for name in eg.RANGES:
                assert same_rays(other["cast"][name][:2], first["cast"][name][:2]), (kind, lvl, name)
        for name in eg.RANGES:
            rd, rh, _ = first["cast"][name]
            has = rd >= 0
            assert (rd[~has] == -res).all() and np.isnan(rh[~has]).all() and np.isfinite(rh[has]).all(), (lvl, name)
            # (the nearer "outside" poses stand a metre off the level: less than a cell at 1 m cells, and truncation takes them in)
            assert not has[c["fam"]["outside"].stop - 1].any() and not has[c["fam"]["nonfinite"]].any(), (lvl, name)
            if name in ("zero", "two_diagonals"):
                assert not has.any(), (lvl, name)   # no step is walked; every end point off the level
    for kind in kinds:
        assert m.checker(oracle_mod, kind).undefined_reads() <= 0, kind


@MAPS
def test_casts_hit_and_miss_along_both_axes(oracle_mod, m):
    """the conditions of the module docstring on every level of at least 8 cells in both axes; on a smaller one only what the
    reference gives (test_both_checkers_agree_on_every_cast_and_ray), its hits counted here"""
    for lvl in range(m.levels):
        ok, fig = eg.cast_conditions(oracle_mod, m, lvl)
        print(m.id, "level", lvl, m.dims(lvl), "seed", eg.cast_seed(m, lvl), "tenth at", eg.tenth_at(m), fig)
        if min(m.dims(lvl)) >= eg.MIN_SIDE:
            assert ok, (m.id, lvl, fig)
            continue
        c = eg.level_case(oracle_mod, m, lvl)
        for name in ("short_side", "half_diagonal"):
            rd = eg.expected(oracle_mod, m, lvl, "ho")["cast"][name][0]
            g = c["fam"]["general"]
            hits = int((rd[g] >= 0).sum())
            assert hits == fig[name]["hits"] and hits + fig[name]["misses"] == rd[g].size, (m.id, lvl, name, "hits", hits)


def test_the_recorded_picks_are_the_searched_ones(oracle_mod):
    assert eg.search_picks(oracle_mod) == eg.PICKS


@MAPS
def test_windows_see_the_map(oracle_mod, m):
    centre, pts = m.scan(oracle_mod)
    assert pts.shape == (200, 2) and np.isfinite(centre).all()
    step = eg.window_step(m)
    for half in eg.WINDOWS:
        poses = window_cases.window_poses(centre, step, half)
        assert len(np.unique(poses[:, 0])) == 2 * half[0] + 1, (half, "the window's columns collapse in fp32")
    for lvl in range(m.levels):
        for half in eg.WINDOWS:
            for n in eg.SCAN_LENS:
                first = eg.expected_window(oracle_mod, m, lvl, half, n, "ho")
                for kind in oracle_kinds()[1:]:
                    other = eg.expected_window(oracle_mod, m, lvl, half, n, kind)
                    assert same(other[0], first[0]) and same(other[1], first[1]), (kind, lvl, half, n)
        res = eg.expected_window(oracle_mod, m, lvl, (3, 2, 1), 200, "ho")[1]
        print(m.id, "level", lvl, "distinct residuals of the (3, 2, 1) window:", np.unique(res).size)
        if min(m.dims(lvl)) >= eg.MIN_SIDE:
            assert np.unique(res).size >= 3 and not (res == np.float32(200.0)).all(), (lvl, np.unique(res)[:5])
    assert m.checker(oracle_mod, "ho").undefined_reads() == 0


def reloc_kind(oracle_mod, m, lvl):
    """"filled": K places, each a finite candidate, a finite winner; "tied": at least K window scores share the best value, so
    the expected K are the window's first indices in order"""
    r = eg.expected_reloc(oracle_mod, m, lvl, "ho")
    for kind in oracle_kinds()[1:]:
        other = eg.expected_reloc(oracle_mod, m, lvl, kind)
        for key in ("scores", "top", "start", "cand", "cov", "lh0", "best_pose"):
            assert same(other[key], r[key]), (m.id, lvl, kind, key)
        assert np.array_equal(other["index"], r["index"]) and other["best_index"] == r["best_index"], (m.id, lvl, kind)
    assert (r["index"] >= 0).all() and np.isfinite(r["cand"]).all() and r["best"] >= 0 and np.isfinite(r["best_pose"]).all()
    if eg.tied_places(r) >= eg.RELOC_K:
        assert r["index"].tolist() == list(np.flatnonzero(r["scores"] == np.nanmax(r["scores"]))[:eg.RELOC_K]), (m.id, lvl)
        return "tied"
    assert np.isfinite(r["best_score"]) and r["best_score"] > 0 and len(set(r["index"].tolist())) == eg.RELOC_K
    return "filled"


def test_relocalisation_cases_fill_their_places_or_tie(oracle_mod):
    kinds = {}
    for m in eg.MAPS:
        for lvl in eg.reloc_levels(m):
            kinds[m.id, lvl] = reloc_kind(oracle_mod, m, lvl)
            want = "tied" if m.kind == "deep" and lvl == m.levels - 1 else "filled"   # 10 x 2, 2 x 10 and 2 x 2 cells
            assert kinds[m.id, lvl] == want, (m.id, lvl, kinds[m.id, lvl])
    print(kinds)
    assert len(kinds) == len(eg.MAPS) + len(eg.DEEP) and {"tied", "filled"} == set(kinds.values())


@pytest.mark.parametrize("geom", fc.GEOMETRIES, ids=fc.gid)
def test_swapped_origins_and_a_foreign_reciprocal_change_the_casts(oracle_mod, geom):
    """the numpy statement of getDist equals the checker on the first 65 beams of both ranges that hit; with the origin's two
    components swapped, and with level 1's reciprocal on level 0 (and level 0's on level 1), it does not"""
    m = eg.map_of(eg.SENSITIVE_FRAME, geom)
    cases = [eg.level_case(oracle_mod, m, lvl) for lvl in (0, 1)]
    for lvl, c in enumerate(cases):
        ox, oy, res = (np.float32(v) for v in c["meta"])
        assert ox != oy
        inv = np.float32(1.0) / res
        other = np.float32(1.0) / np.float32(cases[1 - lvl]["meta"][2])
        assert inv != other
        changed = {"origin": 0, "reciprocal": 0}
        for name in ("short_side", "half_diagonal"):
            begin, end = cast_cases.cast_rays(c["poses"], c["angles"][:65], c["ranges"][name])
            want = eg.expected(oracle_mod, m, lvl, "ho")["cast"][name][0][:, :65].reshape(-1)
            got = eg.numpy_rays(c["grid"], (ox, oy), res, inv, begin, end)
            assert same(got, want), (lvl, name, int((bits(got) != bits(want)).sum()))
            changed["origin"] += int((bits(eg.numpy_rays(c["grid"], (oy, ox), res, inv, begin, end)) != bits(want)).sum())
            changed["reciprocal"] += int((bits(eg.numpy_rays(c["grid"], (ox, oy), res, other, begin, end)) != bits(want)).sum())
        print(m.id, "level", lvl, "rays changed:", changed)
        assert changed["origin"] >= 1 and changed["reciprocal"] >= 1, (lvl, changed)


def test_copy_boxes_fit_their_levels_and_miss_the_alignment():
    geom = eg.COPY_DEEP
    assert geom == (333, 90, 6)
    seen = [set() for _ in range(geom[2])]
    for names, boxes in eg.copy_rounds(geom):
        assert boxes.shape == (geom[2], 4)
        for lvl, (name, (x0, y0, x1, y1)) in enumerate(zip(names, boxes)):
            sx, sy = geom[0] >> lvl, geom[1] >> lvl
            assert x1 < x0 or y1 < y0 or (0 <= x0 <= x1 < sx and 0 <= y0 <= y1 < sy), (lvl, name)   # empty, or inside
            seen[lvl].add(name)
    for lvl in range(geom[2]):
        sx, sy = geom[0] >> lvl, geom[1] >> lvl
        every = eg.level_boxes(sx, sy)
        assert seen[lvl] == set(every), lvl
        assert {"corner 00", "last cell", "whole level", "all but the rim", "empty"} <= set(every), lvl
        assert sy < 12 or len(every) == len(eg.copy_tests.hand_boxes(sx, sy)) + 1, lvl   # from 41 x 11 down some do not fit
        x0, y0, x1, y1 = every["odd start, odd width"]       # every level of this pyramid is wide enough
        assert x0 % 2 == 1 and (x1 - x0 + 1) % 2 == 1 and x1 - x0 + 1 >= 3, (lvl, every["odd start, odd width"])
    assert [(geom[0] >> l) % 4 for l in range(geom[2])] == [1, 2, 3, 1, 0, 2]   # row starts off the 16-byte grid on five levels
