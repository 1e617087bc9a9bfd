"""The CPU pin of the window-move cases (tests/shift_cases.py): what makes the GPU comparison of tests/test_gpu_shift_map.py
meaningful.  The reference has no move; the GPU tests hold a moved context to a checker created with the new start coordinates
and loaded with the moved cells.  For every case this file checks, with both checkers (the restatement and, where it is built,
the reference's own headers):

* the conditions of the case: the plan model accepts it with the displacement the case names, and for 64 cell centres per level
  the cell map_coords_pose gives in the new frame is the old cell plus d_l -- so "the cells keep their world position" is a
  statement about whole cells and the comparison against shift_planes() is the right one;
* the two checkers agree bit for bit on the moved map: download_level, occupancy_grid, one match from the case's start pose and
  the planes after one update_by_scan;
* an update with an empty scan advances a checker's counters like any scan (the counters-carried variant of the GPU test
  rests on it): after N empty updates the stamps one real update writes are those it writes after N real ones.
"""
import numpy as np
import pytest

import frame_cases as fc
import shift_cases as sc
from conftest import bits, oracle_kinds
from support import same

F = np.float32
KINDS = oracle_kinds()
MAPS = pytest.mark.parametrize("m", sc.MAPS, ids=[m.id for m in sc.MAPS])
NAMES = pytest.mark.parametrize("name", sc.SHIFT_NAMES)


@MAPS
def test_conditions_of_the_cases(oracle_mod, m):
    old = m.checker(oracle_mod, "ho")
    rng = np.random.default_rng(2102)
    for name in sc.SHIFT_NAMES:
        new_start, refusal, d0, lv = sc.case_plan(m, name)
        assert refusal == sc.OK, (m.id, name, refusal)
        kx, ky = sc.shift_of(m.geom, name)
        assert d0 == (kx << (m.levels - 1), ky << (m.levels - 1)), (m.id, name, d0)
        new = oracle_mod.Oracle("ho", m.resolution, m.geom[0], m.geom[1], m.geom[2], (float(new_start[0]), float(new_start[1])))
        for lvl in range(m.levels):
            sx, sy = m.dims(lvl)
            assert new.level_info(lvl)[:2] == (sx, sy)
            assert (lv[lvl][0], lv[lvl][1]) == (d0[0] >> lvl, d0[1] >> lvl)
            cells = np.stack([rng.integers(0, sx, 64), rng.integers(0, sy, 64)], 1)
            cells[:4] = [[0, 0], [sx - 1, 0], [0, sy - 1], [sx - 1, sy - 1]]
            for cx, cy in cells:
                world = old.world_coords_pose(lvl, np.array([cx, cy, 0.0], F))   # the centre of old cell (cx, cy)
                p = new.map_coords_pose(lvl, world)
                got = (int(np.floor(p[0] + F(0.5))), int(np.floor(p[1] + F(0.5))))
                assert got == (cx + lv[lvl][0], cy + lv[lvl][1]), (m.id, name, lvl, (cx, cy), p)
                assert abs(p[0] - got[0]) < 1e-3 and abs(p[1] - got[1]) < 1e-3, (m.id, name, lvl, p)   # far from half a cell
        new.close()


@NAMES
@MAPS
def test_checkers_agree_on_the_moved_map(oracle_mod, m, name):
    start, pts = sc.case_scan(oracle_mod, m)
    res = []
    for kind in KINDS:
        o = sc.moved_checker(oracle_mod, kind, m, name)
        planes = [o.download_level(lvl) for lvl in range(m.levels)]
        grids = [o.occupancy_grid(lvl) for lvl in range(m.levels)]
        match = o.match(start, pts)
        o.update_by_scan(start, pts)
        after = [o.download_level(lvl) for lvl in range(m.levels)]
        assert o.undefined_reads() <= 0, (m.id, name, kind)
        res.append((planes, grids, match, after))
        o.close()
    _, d0, _ = sc.case_plan(m, name)[1:]
    want = sc.shifted_levels(sc.old_planes(oracle_mod, m), d0)
    for lvl in range(m.levels):   # what was loaded is what the checker holds
        assert same(res[0][0][lvl][0], want[lvl][0]) and np.array_equal(res[0][0][lvl][1], want[lvl][1]), (m.id, name, lvl)
    for other in res[1:]:
        for lvl in range(m.levels):
            assert same(other[0][lvl][0], res[0][0][lvl][0]) and np.array_equal(other[0][lvl][1], res[0][0][lvl][1]), (m.id, name, lvl)
            assert np.array_equal(other[1][lvl], res[0][1][lvl]), (m.id, name, lvl)
            assert same(other[3][lvl][0], res[0][3][lvl][0]) and np.array_equal(other[3][lvl][1], res[0][3][lvl][1]), (m.id, name, lvl)
        assert same(other[2][0], res[0][2][0]) and same(other[2][1], res[0][2][1]), (m.id, name)
    if name == "zero":
        for lvl in range(m.levels):   # the map before the move, through another checker
            assert same(res[0][0][lvl][0], sc.old_planes(oracle_mod, m)[lvl][0])


@NAMES
@MAPS
def test_the_batch_of_start_poses_is_defined_and_the_checkers_agree(oracle_mod, m, name):
    """the 65 start poses of the GPU test's batch: the restatement reads no map value at a NaN coordinate for any of them
    (shift_cases.batch_starts keeps only such draws), and both checkers give the same poses and covariances"""
    starts = sc.batch_starts(oracle_mod, m, name)
    assert starts.shape == (65, 3) and len({tuple(s) for s in bits(starts)}) == 65
    _, pts = sc.case_scan(oracle_mod, m)
    res = []
    for kind in KINDS:
        o = sc.moved_checker(oracle_mod, kind, m, name)
        res.append([o.match(s, pts) for s in starts])
        assert o.undefined_reads() <= 0, (m.id, name, kind)
        o.close()
    for other in res[1:]:
        for (p, c), (rp, rc) in zip(other, res[0]):
            assert same(p, rp) and same(c, rc), (m.id, name)


@pytest.mark.parametrize("kind", KINDS)
def test_an_empty_update_advances_the_counters_like_any_scan(oracle_mod, kind):
    m = sc.MAPS[1]
    start, pts = sc.case_scan(oracle_mod, m)
    n = 3
    out = []
    for empty in (False, True):
        o = oracle_mod.Oracle(kind, m.resolution, m.geom[0], m.geom[1], m.geom[2], m.start)
        for k in range(n):
            o.update_by_scan(start, np.zeros((0, 2), F) if empty else pts[: 50 + k])
        fc.upload(o, m.geom)   # the same cells under either history
        o.match(start, pts)    # (the coarser levels update from the containers the last match retained)
        o.update_by_scan(start, pts)
        out.append([o.download_level(lvl) for lvl in range(m.levels)])
        o.close()
    for lvl in range(m.levels):
        assert same(out[0][lvl][0], out[1][lvl][0]) and np.array_equal(out[0][lvl][1], out[1][lvl][1]), lvl
        stamps = out[0][lvl][1]
        assert stamps.max() == 3 * n + 2, (lvl, stamps.max())   # the occupied mark of update n + 1: counter 3 n, + 2
