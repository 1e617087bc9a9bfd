"""CPU pin of tests/order_cases.py, the inputs of tests/test_gpu_update_order.py: on every order case the plain-C++ restatement
("ho") equals the reference headers compiled unmodified ("hr") bit for bit, and -- on the checker alone -- the conditions hold
that give the GPU tests their teeth: from the priors of 4 and 9 clear_fan updates the two beam orders of every scan give maps
that DIFFER in at least 100 cells (so a kernel that reverts always, never, or by the wrong key cannot give both), and the
saturate sequence puts at least 100 cells at the 50.0 clamp.

Measured here (level-0 cells whose bits differ, given order against reversed / against the permutation; same after 4 and after
9 prior updates): fan 627 / 541, fan_sub (1024 beams) 306 / 207, pattern 122 / 112, pattern_cut (4095 beams) 122 / 113; after
0, 3, 5 or 10 prior updates every one of them is 0.  Cells at the clamp after 30 updates: fan 2538, fan_sub 841, pattern and
pattern_cut 150 (none before the 23rd update)."""
import numpy as np
import pytest

import order_cases as oc
from conftest import bits
from support import kind

ALL_CASES = oc.DENSE_CASES + oc.KEYED_CASES
MIN_CELLS = 100


def same_snapshots(a, b, what):
    assert len(a) == len(b)
    for k, (sa, sb) in enumerate(zip(a, b)):
        for lvl in range(oc.LEVELS):
            assert np.array_equal(sa[lvl][1], sb[lvl][1]), (what, k, lvl, "update index")
            assert np.array_equal(bits(sa[lvl][0]), bits(sb[lvl][0])), (what, k, lvl, int((bits(sa[lvl][0]) != bits(sb[lvl][0])).sum()))


@pytest.mark.parametrize("map_name", list(oc.MAPS))
def test_restatement_equals_reference_on_every_order_case(oracle_mod, map_name):
    if not oracle_mod.available("hr"):
        pytest.skip("oracle/_ref not built")
    for case in ALL_CASES:
        for prior in oc.PRIORS:
            for order in oc.ORDERS:
                cell, scans = oc.order_sequence(case, prior, order)
                ho, hr = (oc.run_reference(oracle_mod, k, map_name, cell, scans)[1] for k in ("ho", "hr"))
                same_snapshots(ho, hr, (map_name, case, prior, order))
        cell, scans = oc.saturate_sequence(case)
        ho, hr = (oc.run_reference(oracle_mod, k, map_name, cell, scans)[1] for k in ("ho", "hr"))
        same_snapshots(ho, hr, (map_name, case, "saturate"))


@pytest.mark.parametrize("case", ALL_CASES)
def test_beam_order_shows_in_the_checker_from_the_two_priors_only(oracle_mod, kind, case):
    for prior in (0, 3) + oc.PRIORS:
        last = {}
        for order in oc.ORDERS:
            cell, scans = oc.order_sequence(case, prior, order)
            last[order] = oc.run_reference(oracle_mod, kind, "main", cell, scans)[1][-1]
        rev, perm = oc.cells_that_differ(last["given"], last["reversed"]), oc.cells_that_differ(last["given"], last["permuted"])
        print(f"{kind} {case}: after {prior} clear_fan updates the reversed order differs in {rev} cells, the permuted one in {perm}")
        if prior in oc.PRIORS:
            assert rev >= MIN_CELLS and perm >= MIN_CELLS, (case, prior, rev, perm)
            for order in oc.ORDERS:  # the orders change the log-odds' last bits only: the same cells are touched the same way
                assert np.array_equal(last[order][0][1], last["given"][0][1]), (case, prior, order)
        else:
            assert rev == 0 and perm == 0, (case, prior, rev, perm)  # why the room scenes could not see the rule


@pytest.mark.parametrize("case", ALL_CASES)
def test_saturate_reaches_the_clamp_in_the_checker(oracle_mod, kind, case):
    cell, scans = oc.saturate_sequence(case)
    assert len(scans) == oc.N_SATURATE
    snaps = oc.run_reference(oracle_mod, kind, "main", cell, scans)[1]
    at_clamp = [int((s[0][0] >= 50.0).sum()) for s in snaps]
    print(f"{kind} {case}: cells at or above 50.0 after each update: {at_clamp}")
    assert at_clamp[-1] >= MIN_CELLS and at_clamp[21] == 0, at_clamp
    assert float(snaps[-1][0][0].max()) < 50.0 + 2.2  # one occupied step past 50 at the most: the clamp held for 7 updates


def test_scan_shapes():
    assert oc.clear_fan().shape == oc.mixed_fan().shape == (oc.N_FAN, 2) and oc.N_FAN >= oc.DENSE_MIN
    assert len(oc.mixed_subsample()) == oc.N_SUB < oc.DENSE_MIN
    assert len(oc.pattern_cut()) == oc.DENSE_MIN - 1 and len(oc.pattern_scan()) >= oc.DENSE_MIN
    r = np.hypot(*oc.mixed_fan().T)
    assert r.min() >= 6.0 and r.max() <= 30.0
    r = np.hypot(*oc.clear_fan().T)
    assert r.min() >= 34.0 and r.max() <= 36.0
    for case in ALL_CASES:
        g = oc.scan_of(case, "given")
        assert np.array_equal(oc.scan_of(case, "reversed"), g[::-1])
        p = oc.scan_of(case, "permuted")
        assert not np.array_equal(p, g) and np.array_equal(np.sort(p.view(np.uint64).ravel()), np.sort(g.view(np.uint64).ravel()))


def test_pattern_sequence_holds_what_it_promises():
    seq, info = oc.pattern_sequence()
    cells = set(oc.pattern_cells())
    assert {(63, 48), (64, 48), (95, 48), (96, 48)} <= cells and len(cells) >= MIN_CELLS
    sx = oc.MAPS["main"][0]
    word = lambda c: (c[1] * sx + c[0]) >> 5  # noqa: E731
    (a0, b0), (a1, b1), (a2, b2) = info["pairs"]
    assert word(a0) != word(b0) and word(a1) != word(b1) and word(a2) == word(b2) and a2 != b2
    for k, (a, b) in enumerate(info["pairs"]):
        i = info["abab%d" % k]
        assert seq[i:i + 64] == [a, b] * 32
    assert seq[info["abab0"]:info["abab0"] + 128] == [a0, b0] * 64
    # the 200-beam run of one cell spans wavefront boundaries
    i = info["run"]
    assert seq[i:i + 200] == [info["run_cell"]] * 200 and seq[i - 1] != info["run_cell"] and (i + 199) // 64 - i // 64 >= 3
    # runs broken by both kinds of skipped beam, and a whole wavefront of skipped beams
    broken = seq[info["broken"]:info["last_lane"]]
    assert oc.OUTSIDE in broken and oc.BEGIN in broken
    run = [j for j in range(len(seq) - 64) if j % 64 == 0 and all(c == oc.OUTSIDE for c in seq[j:j + 64])]
    assert run, "no wavefront of the end-cell pass is all skipped beams"
    # a run that starts in the last lane of a wavefront
    i = info["last_lane"]
    assert i % 64 == 63 and seq[i:i + 10] == [info["lane_cell"]] * 10 and seq[i - 1] != info["lane_cell"]
    # the tail: one cell, 4096 beams
    assert seq[info["tail"]:] == [info["tail_cell"]] * oc.N_TAIL and len(seq) == info["tail"] + oc.N_TAIL
    # every cell of the set is ended in, both in front of the first crossers and behind them
    crossers = set(oc.pattern_crossers())
    assert not (crossers & cells)
    first_x = min(j for j, c in enumerate(seq) if c in crossers)
    last_x = max(j for j, c in enumerate(seq) if c in crossers)
    ended = {c for c in seq if isinstance(c, tuple)} - crossers
    assert ended == cells
    assert first_x < info["run"] and last_x == info["tail"] - 1
    assert {c for c in seq[first_x:last_x] if isinstance(c, tuple)} >= cells  # ended in between two rounds of crossers
    # the end points hit the chosen cells
    pts = oc.pattern_scan()
    sx0, sy0 = oc.PATTERN_SENSOR
    for c, p in zip(seq, pts):
        if isinstance(c, tuple):
            assert (int(np.floor(sx0 + p[0] + 0.5)), int(np.floor(sy0 + p[1] + 0.5))) == c
