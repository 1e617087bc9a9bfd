"""hsm_occupied_points* and hsm_align_map on every map state the suite has: the cases.

The entries' own tests (tests/test_gpu_occupied_points.py, tests/test_gpu_align_map.py) run on maps that never moved, were never
reset, have a resolution with an exact reciprocal, three levels at most, and align from level 0 on one search level.  Here the
same entries get

  * extraction: the eight frames of frame_cases.FRAMES on 90 x 24 x 2 and 96 x 40 x 3 and entry_geometry_cases' three deep
    pyramids down to 10 x 2, 2 x 10 and 2 x 2 cells; every level, every in (1, 3), four boxes a level (whole, odd start and odd
    width, the last column -- one cell wide: the dividing form with w == 1 --, the last row), caps either side of the kept count;
  * extraction on moved maps: moved_entry_cases.MAP_LAYOUTS under READER_MOVES, and x4_y-1 on the deep map;
  * alignment: both contexts hold the same map, src_level 0 and 1, the search levels of entry_geometry_cases.reloc_levels, and
    one pair each on 96 x 40 x 3 and (333, 90, 6) whose src has moved by x3_y-2 after its planes went in.

The expected points have three statements that must agree bit for bit: points_cases.occupied_points_model with
points_cases.world_from_map of the geometry tuple; the CPU checker's own cells (occupancy_grid == 100, row-major) through its
world_coords_pose times fp32 1 / resolution; and, on the device, getWorldCoordsPose times getScaleToMap.

Pure numpy; the checker module (oracle.pyoracle) is handed in; starts no device on import.  Shared by the CPU pin
(tests/test_points_states_reference.py) and the GPU tests (tests/test_gpu_points_states.py).  Nothing is chosen at run time:
EVERY holds the thinning of each alignment case, PICKS the guesses that had to be searched on the CPU.
"""
import numpy as np

import entry_geometry_cases as egc
import frame_cases as fc
import moved_entry_cases as mec
import newer_entry_cases as nec
import points_cases as pc
import shift_cases as sc
from test_window_model import reference_relocalize

F = np.float32
_cache = {}

# ---- the maps ----------------------------------------------------------------------------------------------------------------------
GEOMETRIES = ((90, 24, 2), (96, 40, 3))
MAPS = [m for m in egc.MAPS if m.kind == "deep" or m.geom in GEOMETRIES]
MAP_LAYOUTS = [(m, "quad") for m in MAPS] + [(m, "plane") for m in MAPS if m.planes_too]
MAP_LAYOUT_IDS = ["%s-%s" % (m.id, layout) for m, layout in MAP_LAYOUTS]
EVERY = (1, 3)
SMALL_LEVEL = 64     # cells: below this the double loop of points_cases.brute_force is run against kept_cells


def planes(pyoracle, m):
    """[(log-odds, stamps)] per level: the shared checker's, never changed"""
    return sc.old_planes(pyoracle, m)


def geometry(m, start=None):
    return nec.geometry_of(m, start)


def level_boxes(sx, sy):
    """[(name, box)] of a level: the whole level, entry_geometry_cases' odd start and odd width where the level is wide enough,
    the last column (w == 1) and the last row"""
    out = [("whole", None)]
    odd = egc.level_boxes(sx, sy).get("odd start, odd width")
    if odd is not None:
        out.append(("odd start, odd width", odd))
    return out + [("last column", (sx - 1, 0, sx - 1, sy - 1)), ("last row", (0, sy - 1, sx - 1, sy - 1))]


def caps(kept):
    return (kept + 3, kept - 1) if kept > 1 else (kept + 3,)


def level_runs(lo):
    """[(box name, box, every, cap)] of a level with the log-odds `lo`"""
    sy, sx = lo.shape
    return [(name, box, every, cap) for name, box in level_boxes(sx, sy) for every in EVERY
            for cap in caps(len(pc.kept_cells(lo, box, every)))]


def frame_of(geom, lvl):
    """(affine, scale) of the model"""
    return pc.world_from_map(geom, lvl), pc.scale_to_map(geom)


def model(lo, geom, lvl, box, every, cap):
    affine, scale = frame_of(geom, lvl)
    return pc.occupied_points_model(lo, box, every, cap, affine, scale)


def checker_points(o, lvl, resolution, box=None):
    """the checker's own statement: the cells of occupancy_grid(lvl) == 100 inside `box` in row-major order, each
    world_coords_pose(lvl, (x, y, 0))[:2] times fp32 1 / resolution -> (cells int64 [n, 2], points float32 [n, 2])"""
    grid = np.asarray(o.occupancy_grid(lvl))
    sy, sx = grid.shape
    x0, y0, x1, y1 = pc.clamp_box(box, sx, sy)
    scale = F(F(1.0) / F(resolution))
    ys, xs = np.nonzero(grid[y0:y1 + 1, x0:x1 + 1] == 100) if x1 >= x0 else (np.zeros(0, np.int64),) * 2
    cells = np.stack([xs + x0, ys + y0], axis=1).astype(np.int64).reshape(-1, 2)
    pts = [(np.asarray(o.world_coords_pose(lvl, F([x, y, 0])), F)[:2] * scale).astype(F) for x, y in cells]
    return cells, np.asarray(pts, F).reshape(-1, 2)


def probe_cells(lo, n=6):
    """a handful of cells of a level for the device's own statement: the corners, and occupied cells spread over the rank order"""
    sy, sx = lo.shape
    occ = pc.kept_cells(lo, None, 1)
    pick = occ[np.linspace(0, len(occ) - 1, min(n, len(occ))).astype(np.int64)] if len(occ) else occ
    return np.concatenate([np.array([[0, 0], [sx - 1, 0], [0, sy - 1], [sx - 1, sy - 1]], np.int64), pick])


# ---- the faults the frames are there to see ----------------------------------------------------------------------------------------
def fused_points(cells_xy, affine, scale):
    """points_cases.cell_points with a fused multiply-add, two ways -> (contracted, fused):
    contracted  what a contracting compiler makes of t0 + (l00 * x + l01 * y) as written: fma(l00, x, l01 * y), then + t0.  Every
                map hsm_create makes has l01 == l10 == 0, so the addend is an exact zero and the bits are the unfused ones;
    fused       the affine written as a single fused multiply-add per coordinate, fma(l00, x, t0) (+ the exact zero): the
                product is not rounded before the translation is added.
    Emulated in float64, where the product of two fp32 numbers is exact and the sum with a third keeps more bits than fp32
    rounds to (the cases' exponents lie within a few binades of each other), then rounded to fp32"""
    l00, l10, l01, l11, t0, t1 = (F(v) for v in affine)
    x, y = cells_xy[:, 0].astype(F), cells_xy[:, 1].astype(F)

    def fma(a, b, c):
        return (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(F)
    wx = (t0 + fma(x, l00, (l01 * y).astype(F))).astype(F)
    wy = (t1 + fma(y, l11, (l10 * x).astype(F))).astype(F)
    wx2 = fma(x, l00, (t0 + (l01 * y).astype(F)).astype(F))
    wy2 = fma(y, l11, (t1 + (l10 * x).astype(F)).astype(F))
    return (np.stack([(wx * F(scale)).astype(F), (wy * F(scale)).astype(F)], axis=1),
            np.stack([(wx2 * F(scale)).astype(F), (wy2 * F(scale)).astype(F)], axis=1))


# ---- moved maps ------------------------------------------------------------------------------------------------------------------
MOVED_CASES = [(m, layout, name) for m, layout in mec.MAP_LAYOUTS for name in mec.READER_MOVES] + \
              [(mec.DEEP, layout, "x4_y-1") for layout in ("quad", "plane")]
MOVED_IDS = ["%s-%s-%s" % (m.id, layout, name) for m, layout, name in MOVED_CASES]
MOVED_MAPS = sorted({(m.id, name): (m, name) for m, _, name in MOVED_CASES}.values(), key=lambda c: (c[0].id, c[1]))
# one_left keeps one cell of the coarsest level, in a corner of the window.  On the frame maps that corner lies outside
# frame_cases.room, whose walls stand 3 coarsest cells inside the map: no occupied cell survives on any level, and the extraction
# of every level has to give [0, 0] and write nothing.  On every other moved map a cell survives on level 0
NOTHING_SURVIVES = frozenset((m.id, "one_left") for m in (mec.M64, mec.M96))
STREAM_CASES =[(mec.M96, "quad", "x3_y-2"), (mec.DEEP, "plane", "x4_y-1")]   # extraction, move, extraction on a caller's stream


def moved_case(pyoracle, m, name):
    """-> dict(start: the plan's new start, d0, geom: the geometry tuple at that start, planes: shifted_levels of the old ones)"""
    key = ("moved", m.id, name)
    if key not in _cache:
        new, refusal, d0, _ = mec.case_plan(m, name)
        assert refusal == sc.OK, (m.id, name, refusal)
        _cache[key] = dict(start=new, d0=d0, geom=geometry(m, new), planes=sc.shifted_levels(planes(pyoracle, m), d0))
    return _cache[key]


# ---- alignment -------------------------------------------------------------------------------------------------------------------
ALIGN_FRAMES = (egc.SENSITIVE_FRAME, fc.FAR, nec.ORIGIN_OUTSIDE, fc.CONTROL)
ALIGN_MAPS = [egc.map_of(f, (96, 40, 3)) for f in ALIGN_FRAMES] + [egc.map_of(None, (333, 90, 6)), egc.map_of(None, (256, 256, 8))]
SRC_LEVELS = (0, 1)
ALIGN_MOVE = "x3_y-2"
MIN_POINTS, MAX_POINTS = 40, 1100
# the guess: src_in_dst off the identity, x and y in cells of the search level.  The first is every case's unless PICKS names another
GUESSES = ((0.3, -0.2, 0.02), (0.3, -0.2, 0.002), (-0.4, 0.25, -0.02), (0.3, -0.2, 0.0))
# case id -> index into GUESSES where the reference does not define the case at GUESSES[0] or finds no winner there; searched on
# the CPU by search_picks(), held by tests/test_points_states_reference.py.  At most MAX_PICKS entries
# The far frame: 0.02 rad about a world origin 80 m away carries every point 1.6 m, two thirds of the 2.4 m map, and every
# likelihood of the window is 0; at 0.002 rad the points stay on the map
PICKS = {"res0.025_start-50_37-96x40_L3-src0-search2": 1, "res0.025_start-50_37-96x40_L3-src1-search2": 1}
MAX_PICKS = 3
# the thinning per (map id, src_level, moved), so that 40 < points <= 1100: 96 x 40 x 3 holds 524 / 260 occupied cells on levels
# 0 / 1 (488 on level 0 after the move), (256, 256, 8) 912 / 665, (333, 90, 6) 1537 / 425 (470 after the move)
EVERY_OF = {(m.id, s, None): 1 for m in ALIGN_MAPS for s in SRC_LEVELS}
EVERY_OF.update({("333x90_L6", 0, None): 2, (mec.M96.id, 0, ALIGN_MOVE): 1, (mec.DEEP.id, 0, ALIGN_MOVE): 1})


class AlignCase:
    def __init__(self, m, src_level, search_level, moved=None):
        self.m, self.src_level, self.search_level, self.moved = m, src_level, search_level, moved
        self.id = "%s-src%d-search%d%s" % (m.id, src_level, search_level, "-src_moved_" + moved if moved else "")

    @property
    def every(self):
        return EVERY_OF[self.m.id, self.src_level, self.moved]


ALIGN_CASES = [AlignCase(m, s, lvl) for m in ALIGN_MAPS for s in SRC_LEVELS for lvl in egc.reloc_levels(m)] + \
              [AlignCase(mec.M96, 0, mec.M96.levels - 1, ALIGN_MOVE), AlignCase(mec.DEEP, 0, egc.DEEP_RELOC_LEVEL, ALIGN_MOVE)]
ALIGN_IDS = [c.id for c in ALIGN_CASES]
# The deep maps searched on their coarsest level, 10 x 2 and 2 x 2 cells: every point at every pose of the window is off the level
# (limx = sx - 2 = 0 ...), all 567 likelihoods are 0 and tie, the first k window places are matched from starts metres away and
# the winner's level-0 likelihood is 0 as well, at every guess of GUESSES.  That is the reference's answer, defined and finite, and
# the device has to give its bits; every other case must see the map (a winner's likelihood above SEES_THE_MAP)
ALL_ZERO = frozenset(c.id for c in ALIGN_CASES if c.m.kind == "deep" and c.search_level == c.m.levels - 1)
SEES_THE_MAP = 0.3
# (333, 90, 6) moved by x3_y-2 keeps 26 of its 90 rows (moved_entry_cases.LOSES_TRACK): the 470 points of that strip do not pin
# the pose, and the reference's matches leave the identity by metres; its winner's likelihood is 0.065.  Defined and finite, and
# the device has to give its bits: the case stays, and the CPU pin asserts that it is the only one of its kind
WANDERS = frozenset(c.id for c in ALIGN_CASES if c.moved and c.m is mec.DEEP)


def align_step(pyoracle, c):
    return egc.reloc_step(pyoracle, c.m, c.search_level)


def align_guess(pyoracle, c, pick=None):
    gx, gy, ga = GUESSES[PICKS.get(c.id, 0) if pick is None else pick]
    cell = align_step(pyoracle, c)[0]
    return F([gx * cell, gy * cell, ga])


def align_src(pyoracle, c):
    """what src holds when the alignment is queued -> (planes, geometry tuple)"""
    if c.moved:
        mv = moved_case(pyoracle, c.m, c.moved)
        return mv["planes"], mv["geom"]
    return planes(pyoracle, c.m), geometry(c.m)


def align_points(pyoracle, c):
    """the model's points of the case: what the extraction tests hold the device to -> (points, (written, kept))"""
    src_planes, geom = align_src(pyoracle, c)
    return model(src_planes[c.src_level][0], geom, c.src_level, None, c.every, MAX_POINTS)


def align_reference(pyoracle, kind, c, pts, pick=None):
    """reference_relocalize on dst's checker (the map's own: dst never moves) fed `pts`; the restatement goes first and counts the
    reads the reference does not define -> the result, or None where the case is not defined, has no finite winner, or has a
    winner of likelihood 0 outside ALL_ZERO"""
    o = c.m.checker(pyoracle, "ho")
    u0 = o.undefined_reads()
    args = (None, align_guess(pyoracle, c, pick), pts, align_step(pyoracle, c), egc.RELOC_HALF, egc.RELOC_K)
    r = reference_relocalize(o, *args, search_level=c.search_level)
    if o.undefined_reads() != u0 or r["best_index"] < 0 or not np.isfinite(r["best_pose"]).all() or not np.isfinite(r["best_score"]):
        return None
    if (r["best_score"] == 0) != (c.id in ALL_ZERO):
        return None
    return r if kind == "ho" else reference_relocalize(c.m.checker(pyoracle, kind), *args, search_level=c.search_level)


def expected_align(pyoracle, kind, c):
    """the reference's answer on the model's points, cached"""
    key = ("align", kind, c.id)
    if key not in _cache:
        r = align_reference(pyoracle, kind, c, align_points(pyoracle, c)[0])
        assert r is not None, (c.id, "the reference does not define this alignment: see search_picks()")
        _cache[key] = r
    return _cache[key]


def search_picks(pyoracle):
    """-> the PICKS dict for the present cases (run on the CPU when an input changes; the result is recorded above)"""
    picks = {}
    for c in ALIGN_CASES:
        pts = align_points(pyoracle, c)[0]
        pick = next((k for k in range(len(GUESSES)) if align_reference(pyoracle, "ho", c, pts, k) is not None), None)
        if pick != 0:
            picks[c.id] = pick
    return picks
