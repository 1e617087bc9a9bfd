"""What the reference does on reset(), stated once on the CPU, and that tests/reset_cases.py's history is what it claims to be.

GridMapBase::reset only clears the cells: currUpdateIndex is not rewound, MapRepMultiMap::dataContainers survive, and
HectorSlamProcessor::reset sets lastMapUpdatePose to FLT_MAX.  tests/test_gpu_reset.py compares a device context with checkers
that went through the same history and the same reset, so these facts are what its expected stamps rest on.
"""
import numpy as np
import pytest

import moved_entry_cases as mec
import reset_cases as rc
import topk_rule
from conftest import bits, oracle_kinds

F = np.float32
MAP_IDS = [m.id for m in rc.MAPS]
ALL = [(m, v) for m in rc.MAPS for v in rc.VARIANTS]
ALL_IDS = ["%s-%s" % (m.id, v) for m, v in ALL]


def same_planes(a, b):
    return all(np.array_equal(bits(x[0]), bits(y[0])) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))


def flat(x):
    """every array of a nested expectation, in order"""
    if x is None:
        return []
    if isinstance(x, (int, float, np.integer, np.floating)):
        return [np.atleast_1d(np.asarray(x))]
    if isinstance(x, np.ndarray):
        return [np.atleast_1d(x)]
    if isinstance(x, dict):
        return [a for k in sorted(x) for a in flat(x[k])]
    return [a for y in x for a in flat(y)]


# ---- 1: the two checkers agree through history, reset and after-sequence ------------------------------------------------------------
@pytest.mark.parametrize("m,variant", ALL, ids=ALL_IDS)
def test_restatement_and_reference_agree_through_the_whole_case(oracle_mod, m, variant):
    if "hr" not in oracle_kinds():
        pytest.skip("oracle/_ref is not built")
    a, b = rc.run_checker(oracle_mod, "ho", m, variant), rc.run_checker(oracle_mod, "hr", m, variant)
    for key in ("before", "blank", "first_update", "rebuilt"):
        assert same_planes(a[key], b[key]), key
    for key in ("readers_blank", "readers_rebuilt"):
        for x, y in zip(flat(a[key]), flat(b[key])):
            assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), key
    assert np.array_equal(bits(a["gate_last"]), bits(b["gate_last"])) and a["gate_count"] == b["gate_count"]


# ---- 2: what reset() clears and what it keeps ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", oracle_kinds())
@pytest.mark.parametrize("m,variant", ALL, ids=ALL_IDS)
def test_reset_clears_the_cells_and_keeps_the_counters(oracle_mod, m, variant, kind):
    r = rc.run_checker(oracle_mod, kind, m, variant)
    for lvl, (lo, st) in enumerate(r["blank"]):
        assert (bits(lo) == 0).all() and (st == -1).all(), lvl
    n = r["index_before"] + 1   # updates up to the reset: currUpdateIndex = 3 n
    assert n >= 8
    for lvl, (lo, st) in enumerate(r["first_update"]):   # (a level of a few cells may take no mark at all)
        assert set(np.unique(st).tolist()) <= {-1, 3 * n + 1, 3 * n + 2} and (lvl > 1 or (st == 3 * n + 1).any()), (lvl, np.unique(st), n)
    assert r["index_after"] == r["index_before"] + 6


# ---- 3: the containers of the coarse levels survive ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", oracle_kinds())
@pytest.mark.parametrize("m", rc.MAPS, ids=MAP_IDS)
def test_update_right_after_reset_takes_the_container_matched_before_it(oracle_mod, m, kind):
    """MapRepMultiMap::updateByScan hands level i > 0 dataContainers[i - 1] (MapRepMultiMap.h:143), which only matchData
    refills (:127): an update right behind reset() marks the coarse levels with the scan matched BEFORE the reset.  A fresh
    checker, whose containers are empty, marks nothing there"""
    t = mec.trajectory(oracle_mod, m)
    used, fresh = (mec.old_checker(oracle_mod, kind, m, planes=[]) for _ in range(2))
    used.match(t.world[3], t.scans[3])
    used.update_by_scan(t.world[3], t.scans[3])
    used.guard.reset()
    if used.o is not used.guard:
        used.o.reset()
    for o in (used, fresh):
        o.update_by_scan(t.world[0], t.scans[0][:40])
    model = mec.old_checker(oracle_mod, kind, m, planes=[])   # what the rule above says: level 0 scan 0, coarse levels scan 3
    model.update_by_scan(np.zeros(3, F), np.zeros((0, 2), F))
    model.match(t.world[3], t.scans[3])
    model.update_by_scan(t.world[0], t.scans[0][:40])
    (u, f, w) = (mec.levels_of(o, m.levels) for o in (used, fresh, model))
    assert np.array_equal(bits(u[0][0]), bits(f[0][0]))   # (level 0: the cells agree, the stamps do not: the counter went on)
    assert same_planes(u, w)
    for lvl in range(1, m.levels):   # (a level of a few cells may take no mark from either)
        assert (f[lvl][1] == -1).all() and (lvl > 1 or (u[lvl][1] != -1).any()), lvl
    for o in (used, fresh, model):
        o.close()


# ---- 4: the blank map ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", oracle_kinds())
@pytest.mark.parametrize("m", rc.MAPS, ids=MAP_IDS)
def test_blank_map_is_an_edge_of_its_own(oracle_mod, m, kind):
    r = rc.run_checker(oracle_mod, kind, m, "plain")["readers_blank"]
    q = rc.reader_inputs(oracle_mod, m)
    assert all(x is not None for x in r["match"])
    for (pose, cov), start in zip(r["match"] + [r["single"]], list(q["poses"]) + [q["centre"]]):
        # H == 0: the step is skipped on every level.  What is left of MapRepMultiMap::matchData is the trip to the level's
        # map frame and back, coarsest level first (ScanMatcher.h:57, :96-99).  That is NOT the start pose bit for bit: each
        # trip costs a few ulps (measured: up to 15 on the three maps), so "returns its start pose" holds to 16 fp32 ulps of
        # the largest coordinate per level only.  The device is held to the checker's bits, not to the start pose
        assert np.abs(pose.astype(np.float64) - start).max() <= 16 * m.levels * np.spacing(F(np.abs(start).max())), (pose, start)
        assert (cov == 0).all(), cov   # the covariance handed back is H of level 0 (ScanMatcher.h:90): exactly 0, every entry
    o = m.checker(oracle_mod, kind)   # (the map's own checker for its frame; H is asked of a cleared checker below)
    blank = mec.old_checker(oracle_mod, kind, m, planes=[])
    for lvl in range(m.levels):
        H, dTr = blank.hessian_derivs(lvl, o.map_coords_pose(lvl, q["centre"]), q["pts"] * F(1.0 / 2 ** lvl))
        assert (H == 0).all() and (dTr == 0).all(), (lvl, H, dTr)   # every gradient is 0 on a map of 0.5
    blank.close()
    for lvl in range(m.levels):
        lh, res = r["window"][lvl]
        # every beam that ends on the level reads 0.5, so the scores of a window tie wherever its poses keep the same beams on
        # the level; a pose that sends some off it scores lower (0.4175 on level 1 of 64 x 64).  Level 0 of 64 x 64 ties outright
        assert len(lh) == 7 * 5 * 3 and 0.0 <= float(np.nanmax(lh)) <= 0.5, lvl
        tied = bool((bits(lh) == bits(lh[0])).all())
        assert tied or (m.id, lvl) != (rc.MAPS[0].id, 0)
        for k in rc.TOPK:
            idx, _ = topk_rule.topk(lh, k)
            if tied:   # decided by index alone
                assert np.array_equal(idx, np.arange(k)), (lvl, k, idx)
            else:      # the first k of the poses that score 0.5, in index order
                assert np.array_equal(idx, np.flatnonzero(lh == lh.max())[:k]) or (lh == lh.max()).sum() < k, (lvl, k, idx)
        assert (r["grid"][lvl] == -1).all()
        for n, x in zip(rc.CSR_LENS, r["score"][lvl][0]):
            assert np.isnan(x) == (n == 0)


@pytest.mark.parametrize("m,variant", ALL, ids=ALL_IDS)
def test_rows_the_reference_does_not_define_are_the_recorded_ones(oracle_mod, m, variant):
    r = rc.run_checker(oracle_mod, "ho", m, variant)
    assert all(x is not None for x in r["readers_blank"]["match"])
    rows = tuple(k for k, x in enumerate(r["readers_rebuilt"]["match"]) if x is None)
    assert rows == rc.PICKS.get(("undefined", m.id, variant), ()), rows
    assert len(rows) <= 2 and len(rc.PICKS) <= 3


# ---- 5: the history is what it claims to be --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,variant", ALL, ids=ALL_IDS)
def test_history_leaves_every_unit_dirty(oracle_mod, m, variant):
    r = rc.run_checker(oracle_mod, "ho", m, variant)
    ops = rc.history(oracle_mod, m, variant)
    assert ops[-1][0] == "gated"   # the last step: no host query between it and the reset
    first = r["flags"][0]
    assert first.sum() >= 1 and (~first).sum() >= 1, first
    assert all(f.all() for f in r["flags"][1:])
    assert 8 <= sum(op[0] == "update" for op in ops) <= 12
    assert [op[0] for op in ops].index("export") < [op[0] for op in ops].index("gated")
    _, left = rc.serial_model(ops, m.levels)
    taken, _ = rc.serial_model(rc.after_sequence(oracle_mod, m), m.levels, left)
    assert len(taken) == 6
    for lvl in range(m.levels):   # level l takes generation 1 again in update l + 1 after the reset, 4095 in the one before
        col = [s[lvl] for s in taken]
        assert col[lvl] == 1 and (lvl == 0 or col[lvl - 1] == rc.SERIAL_MAX), (lvl, col)
    assert max(s[m.levels - 1] for s in taken) >= 4096 - m.levels
    counter = 3 * (r["index_before"] + 1)
    ahead = any(int(st.max()) > counter for _, st in r["before"])
    assert ahead == (variant == "frozen"), [int(st.max()) for _, st in r["before"]]
    assert (not np.array_equal(bits(r["start"]), bits(np.asarray(m.start, F)))) == (variant == "moved")
    assert any((st != -1).any() for _, st in r["before"])


# ---- 6: the group case ------------------------------------------------------------------------------------------------------------------
def test_group_case_keeps_its_counters_across_the_reset(oracle_mod):
    """tests/test_gpu_reset.py's group: four scans matched and applied, reset(), four more.  Both checkers agree; the stamps behind
    the reset continue the count of the four in front of it, and the first match behind it runs on a blank map"""
    rs = [rc.group_case(oracle_mod, kind) for kind in oracle_kinds()]
    r = rs[-1]
    for other in rs[:-1]:
        assert same_planes(other["end"], r["end"]) and np.array_equal(bits(other["poses"]), bits(r["poses"]))
        assert np.array_equal(bits(other["covs"]), bits(r["covs"]))
    n = sum(len(ks) for ks in rc.GROUP_SCANS)
    assert r["index"] == n - 1 and len(r["poses"]) == n
    assert all((bits(lo) == 0).all() and (st == -1).all() for lo, st in r["blank"])
    first = 3 * len(rc.GROUP_SCANS[0])
    for lvl, (lo, st) in enumerate(r["end"]):
        known = st[st != -1]
        assert known.size and known.min() > first and known.max() <= 3 * n, (lvl, known.min(), known.max())
    assert (r["covs"][len(rc.GROUP_SCANS[0])] == 0).all()   # H == 0 on the blank map
