"""Inputs for the beam-ORDER tests of updateByScan (OccGridMapBase.h:121-260, cell rules GridMapLogOdds.h:135-156).

The reference walks the beams of a scan one after the other, and its result depends on their order in one place: a cell that
an earlier beam crossed (updateSetFree) and a later beam ends in is reverted and then set occupied, lo + f - f + occ; a cell
that is ended in first and crossed later is lo + occ.  In fp32 (lo + f) - f == lo unless lo + f leaves lo's binade, so the rule
shows in the bits only for cells that sit just above -2, -4, -8 ...: with the factors 0.4 / 0.9 (f = log(0.4 / 0.6) = -0.405)
that is after 4 free-only updates (-1.62 -> -2.03) and after 9 (-3.65 -> -4.05).  The scans here put a disc of cells into
exactly those states and then end beams in cells that other beams of the same scan cross, in several orders.

Pure numpy; shared by the CPU pin (tests/test_update_order_reference.py: restatement == reference headers, and the reference's
own two orders DO differ) and the GPU tests (tests/test_gpu_update_order.py).  Everything is generated from fixed seeds.

Geometry: resolution 0.05, two levels (level 1 takes the scaled container), the sensor at a cell centre with theta 0, so
robot-frame end point (dx, dy) (level-0 cell units) ends in cell sensor + (round(dx), round(dy)).
"""
import numpy as np

from edge_cases import world_pose_of_cell

RES = 0.05
FACTOR_FREE, FACTOR_OCC = 0.4, 0.9
LEVELS = 2
# "main": rows of 128 cells (a multiple of 64: the keyed apply pass takes its aligned form; scans of >= 4096 beams the byte-map
# form); "narrow": rows of 120 cells (the keyed apply pass takes its unaligned form, the byte-map form's 32 x 8-cell blocks
# straddle the right edge, bitmap words straddle rows)
MAPS = {"main": (128, 96), "narrow": (120, 96)}
FAN_SENSOR = (40, 40)
# pattern_scan's cell set contains x = 95 / 96, which no disc around (40, 40) reaches on these maps: it has a sensor cell
# of its own, and its priors are clear_fan updates from there
PATTERN_SENSOR = (80, 48)
PRIORS = (4, 9)          # clear_fan updates before the scan under test
ORDERS = ("given", "reversed", "permuted")
N_FAN = 8192
N_SUB = 1024             # the keyed form's subsample of mixed_fan (< 4096)
N_TAIL = 4096
DENSE_MIN = 4096         # scans of at least this many beams take the byte-map form (HSM_MERGED_MARK_MAX)
N_SATURATE = 30          # 23 occupied updates reach the 50.0 clamp: 23 * log(9) = 50.5
OUTSIDE, BEGIN = -1, -2  # pattern_scan's two kinds of skipped beam


def sensor_pose(map_name, cell):
    sx, sy = MAPS[map_name]
    return world_pose_of_cell(RES, sx, sy, float(cell[0]), float(cell[1]), 0.0)


def clear_fan():
    """8192 beams ending 34 .. 36 cells out: frees the disc inside that radius (k updates leave it at k * log_odds_free) and
    ends in no cell of it"""
    rng = np.random.default_rng(4001)
    a = np.linspace(-np.pi, np.pi, N_FAN, endpoint=False) + rng.uniform(0, 1e-3)
    r = rng.uniform(34.0, 36.0, N_FAN)
    return np.stack([r * np.cos(a), r * np.sin(a)], 1).astype(np.float32)


def mixed_fan():
    """8192 beams ending 6 .. 30 cells out in random directions: most cells of the disc are crossed by some beams and ended in by
    others, in an order that has nothing to do with the geometry"""
    rng = np.random.default_rng(4002)
    a = rng.uniform(-np.pi, np.pi, N_FAN)
    r = rng.uniform(6.0, 30.0, N_FAN)
    return np.stack([r * np.cos(a), r * np.sin(a)], 1).astype(np.float32)


def in_orders(pts):
    """the scan in given order, reversed, and in one fixed random permutation"""
    perm = np.random.default_rng(4003).permutation(len(pts))
    return {"given": np.ascontiguousarray(pts), "reversed": np.ascontiguousarray(pts[::-1]), "permuted": np.ascontiguousarray(pts[perm])}


def mixed_subsample():
    return np.ascontiguousarray(mixed_fan()[:: N_FAN // N_SUB])


def pattern_cells():
    """the cell set: the sensor's row and its two neighbours, 22 columns on either side of the sensor, 8 .. 29 cells out.
    Holds (63, 64) and (95, 96), neighbours across a 32-cell bitmap word boundary of a 128-cell row."""
    sx0, sy0 = PATTERN_SENSOR
    return [(x, y) for y in (sy0 - 1, sy0, sy0 + 1) for x in list(range(51, 73)) + list(range(88, 110))]


def pattern_crossers():
    """end cells 31 columns out on either side, rows -4 .. +4: these beams cross every cell of the set and end in none"""
    sx0, sy0 = PATTERN_SENSOR
    return [(sx0 + s * 31, sy0 + dy) for s in (-1, 1) for dy in range(-4, 5)]


def pattern_sequence():
    """-> (end cells [(x, y)] with OUTSIDE / BEGIN for the skipped beams, info).  In beam order:
      sweep 1     every ordinary cell of the set once, the nearest first: ended in BEFORE anything crosses it
      ABAB        two cells in turn, 128 beams: the pair (63, 64) across a bitmap word, then (95, 96), then a pair inside one word
      crossers    beams that end further out and cross the whole set
      run         one cell 200 times: the run spans four wavefronts
      broken      runs of one cell / of two cells of one bitmap word, interrupted by skipped beams of both kinds
      last lane   filler up to beam 64 m + 63, then a run that starts in that last lane of a wavefront
      sweep 2     every cell of the set once more, in another order: ended in AFTER the crossers
      crossers    again, reversed
      tail        4096 beams that all end in one cell
    so every cell of the set is crossed by beams before and after beams that end in it, the given order ends in the swept
    cells first and the reversed order crosses them first."""
    rng = np.random.default_rng(4004)
    cells = pattern_cells()
    sy0 = PATTERN_SENSOR[1]
    pairs = [((63, sy0), (64, sy0)), ((95, sy0), (96, sy0)), ((66, sy0 - 1), (67, sy0 - 1))]
    run_cell, broken_a, broken_b, lane_cell, tail_cell = (60, sy0 + 1), (100, sy0 + 1), (101, sy0 + 1), (58, sy0 - 1), (104, sy0 - 1)
    special = {c for p in pairs for c in p} | {run_cell, broken_a, broken_b, lane_cell, tail_cell}
    assert special <= set(cells)
    ordinary = [c for c in cells if c not in special]
    sx0 = PATTERN_SENSOR[0]
    seq = sorted(ordinary, key=lambda c: (abs(c[0] - sx0), c[1], c[0]))  # near to far: no beam crosses a cell swept before it
    info = {"pairs": pairs, "run_cell": run_cell, "lane_cell": lane_cell, "tail_cell": tail_cell}
    for k, (a, b) in enumerate(pairs):
        info["abab%d" % k] = len(seq)
        seq += [a, b] * (64 if k < 2 else 32)
    crossers = pattern_crossers()
    seq += crossers
    info["run"] = len(seq)
    seq += [run_cell] * 200
    info["broken"] = len(seq)
    seq += ([broken_a] * 5 + [OUTSIDE] + [broken_a] * 5 + [BEGIN] + [broken_a] * 3 + [OUTSIDE, BEGIN] + [broken_a, broken_b, OUTSIDE,
            broken_b, broken_a, BEGIN] + [broken_b] * 4 + [BEGIN] * 3 + [broken_a, broken_a] + [OUTSIDE] * 130 + [broken_b])  # (130: one wavefront of the end-cell pass holds skipped beams only)
    k = 0
    while len(seq) % 64 != 63:
        seq.append(ordinary[k % len(ordinary)])
        k += 1
    info["last_lane"] = len(seq)
    seq += [lane_cell] * 10
    seq += [cells[i] for i in rng.permutation(len(cells))]
    seq += crossers[::-1]
    info["tail"] = len(seq)
    seq += [tail_cell] * N_TAIL
    return seq, info


def pattern_scan():
    """pattern_sequence() as robot-frame end points from PATTERN_SENSOR (a quarter cell of jitter: the level-0 cell stays the
    chosen one); OUTSIDE ends 60 columns to the right (off both maps on both levels), BEGIN in the sensor's cell"""
    rng = np.random.default_rng(4005)
    seq, _ = pattern_sequence()
    sx0, sy0 = PATTERN_SENSOR
    base = np.array([(60.0, 3.0) if c == OUTSIDE else (0.0, 0.0) if c == BEGIN else (c[0] - sx0, c[1] - sy0) for c in seq], np.float64)
    return (base + rng.uniform(-0.25, 0.25, base.shape)).astype(np.float32)


def pattern_cut():
    """the keyed form's share of pattern_scan: everything in front of the tail and as much of the tail as stays below 4096 beams"""
    return np.ascontiguousarray(pattern_scan()[:DENSE_MIN - 1])


_SCANS = {"fan": mixed_fan, "fan_sub": mixed_subsample, "pattern": pattern_scan, "pattern_cut": pattern_cut}
SENSORS = {"fan": FAN_SENSOR, "fan_sub": FAN_SENSOR, "pattern": PATTERN_SENSOR, "pattern_cut": PATTERN_SENSOR}
DENSE_CASES, KEYED_CASES = ("fan", "pattern"), ("fan_sub", "pattern_cut")
_cache = {}


def scan_of(case, order="given"):
    if case not in _cache:
        _cache[case] = in_orders(_SCANS[case]())
    return _cache[case][order]


def order_sequence(case, prior, order):
    """-> (sensor cell, [scans]): `prior` clear_fan updates, then the case's scan in `order`"""
    if "clear" not in _cache:
        _cache["clear"] = clear_fan()
    return SENSORS[case], [_cache["clear"]] * prior + [scan_of(case, order)]


def saturate_sequence(case="fan"):
    """the scan and its reverse in turn, 30 updates: the cells beams end in pass 50.0 at the 23rd"""
    return SENSORS[case], [scan_of(case, "given"), scan_of(case, "reversed")] * (N_SATURATE // 2)


def new_reference(oracle_mod, kind, map_name):
    sx, sy = MAPS[map_name]
    o = oracle_mod.Oracle(kind, RES, sx, sy, LEVELS)
    o.set_update_factor_free(FACTOR_FREE)
    o.set_update_factor_occupied(FACTOR_OCC)
    return o


def run_reference(oracle_mod, kind, map_name, cell, scans):
    """the checker `kind` over the sequence -> (the checker, [after every update: [(log-odds, update index) per level]]); every
    level is driven with the container scaled to it, which is what matchData's setFrom retains (MapRepMultiMap.h:127,143)"""
    o = new_reference(oracle_mod, kind, map_name)
    pose = sensor_pose(map_name, cell)
    snaps = []
    for pts in scans:
        o.build_map(pose[None, :], [pts])
        snaps.append([o.download_level(lvl) for lvl in range(LEVELS)])
    return o, snaps


def cells_that_differ(a, b):
    """level-0 cells whose log-odds bits differ between two snapshots"""
    return int((a[0][0].view(np.uint32) != b[0][0].view(np.uint32)).sum())
