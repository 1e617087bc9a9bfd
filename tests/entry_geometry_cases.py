"""The cast, window and copy entries on maps that are not square, centred 3-level pyramids of 0.05 m cells: the cases.

hsm_ray_distances_device / hsm_cast_scans*, hsm_score_window* / hsm_window_poses_device / hsm_select_topk_device /
hsm_relocalize* and hsm_copy_map / hsm_copy_map_boxes came after the suite's geometry files (rectangular maps, deep pyramids,
map frames), and their own tests run on conftest.pyramid_scene: x and y translations equal whole numbers of cells, an exact
1 / resolution, sx == sy, every level's width a multiple of 4.  Here the same entries get

  * the eight frames of frame_cases.FRAMES on its three geometries (64 x 64 x 2, 90 x 24 x 2, 96 x 40 x 3), on the room of
    frame_cases.map_planes, and
  * three of deep_cases' pyramids, with the maps deep_cases.case builds: (333, 90, 6) and (90, 333, 6) -- levels 83 / 41 cells
    wide and 45 / 11 high on the way down to 10 x 2 -- and (256, 256, 8), whose coarsest level is 2 x 2 cells.

Pure numpy; the checker module (oracle.pyoracle) is handed in.  Shared by the CPU pin (tests/test_entry_geometries_reference.py)
and the GPU tests (tests/test_gpu_entry_geometries.py).  Everything comes from fixed seeds and nothing is chosen at run time:
PICKS records the seeds that had to be searched on the CPU.

numpy_rays is a third statement of DistanceMeasurementProvider::getDist (HectorMapTools.h:133-234) next to the two checkers,
with the four numbers of the CoordinateTransformer as arguments of their own: the CPU pin holds it to the checkers and then
hands it a swapped origin and another level's reciprocal, the faults the GPU test is there to see.
"""
import numpy as np

import cast_cases
import deep_cases
import frame_cases as fc
import test_gpu_copy_map as copy_tests   # hand_boxes, random_planes (neither module starts a device on import)
import test_gpu_window as window_tests  # oracle_window
import window_cases
from test_window_model import reference_relocalize

F32 = np.float32
FRAME_MAPS = [(frame, geom) for geom in fc.GEOMETRIES for frame in fc.FRAMES]
DEEP = [(333, 90, 6), (90, 333, 6), (256, 256, 8)]
assert all(g in deep_cases.GEOMETRIES for g in DEEP)
SENSITIVE_FRAME = fc.FRAMES[1]   # inexact scale, inexact and unequal translations
PLANE_LAYOUT_TOO = ("frame", SENSITIVE_FRAME), ("deep", (333, 90, 6))   # the maps that run in the plane layout as well

N_BEAMS = 200                    # the beam table; a fan is its first n angles
FANS = (1, 63, 64, 65, 200)
N_RAYS = 500
RANGES = ("zero", "sub_cell", "short_side", "half_diagonal", "two_diagonals")
SHORT_SIDE = 0.45                # of the level's shorter side: see range_maxes
TENTH_AT_HALF_DIAGONAL = [(64, 64, 2), (96, 40, 3)]   # the frame geometries whose rays of half a diagonal hit often enough
MIN_SIDE = 8                     # the conditions of the CPU pin hold on levels at least this many cells in both axes

WINDOWS = ((3, 2, 1), (40, 0, 0))
SCAN_LENS = (1, 65, 200)
WINDOW_STEP_CELLS, WINDOW_STEP_ANGLE = (0.5, 0.7), 0.013   # of the level-0 cell: 80 m centres and 0.0125 m steps in the far frame
RELOC_HALF, RELOC_K, RELOC_ANGLE = (4, 4, 3), 8, 0.05      # 9 * 9 * 7 = 567 hypotheses, steps of one cell of the search level
DEEP_RELOC_LEVEL = 2             # the deep maps' second search level, next to the coarsest one

# ("cast", map id, level) -> seed of cast_cases.poses where the level's own number did not meet the conditions of
# tests/test_entry_geometries_reference.py; searched on the CPU by search_picks()
PICKS = {}
_cache = {}


class _Truth:
    """what cast_cases.poses asks of a scene: world poses on the map"""

    def __init__(self, query_truth):
        self.query_truth = query_truth


class Map:
    """one map of the list: a frame on a geometry (kind "frame"), or a deep pyramid with its built map (kind "deep")"""

    def __init__(self, frame, geom):
        self.frame, self.geom = frame, geom
        self.kind = "deep" if frame is None else "frame"
        self.id = deep_cases.gid(geom) if frame is None else fc.fid(frame) + "-" + fc.gid(geom)
        self.levels = geom[2]
        self.resolution = deep_cases.RES if frame is None else frame[0]
        self.start = (0.5, 0.5) if frame is None else frame[1]
        self.planes_too = (self.kind, geom if frame is None else frame) in PLANE_LAYOUT_TOO

    def dims(self, lvl):
        return self.geom[0] >> lvl, self.geom[1] >> lvl

    def case(self):
        """the deep geometry's scene (deep_cases.case), made once"""
        assert self.kind == "deep"
        if ("case", self.geom) not in _cache:
            _cache["case", self.geom] = deep_cases.case(self.geom)
        return _cache["case", self.geom]

    def checker(self, pyoracle, kind):
        """the shared checker that holds the map; nobody changes it"""
        if self.kind == "frame":
            return fc.checker(pyoracle, kind, self.frame, self.geom)
        if ("checker", kind, self.geom) not in _cache:
            _cache["checker", kind, self.geom] = deep_cases.built_oracle(pyoracle, kind, self.case())
        return _cache["checker", kind, self.geom]

    def upload(self, pyoracle, g):
        """the map into a device context"""
        o = self.checker(pyoracle, "ho")
        for lvl in range(self.levels):
            g.upload_level(lvl, *o.download_level(lvl))
        return g

    def truth(self, pyoracle):
        """16 world poses on the map: frame_cases.map_poses through the checker's world_coords_pose, or the case's own"""
        if self.kind == "deep":
            return np.asarray(self.case().query_truth, F32)
        o = self.checker(pyoracle, "ho")
        return np.stack([o.world_coords_pose(0, p) for p in fc.map_poses(self.geom, 16, 40)]).astype(F32)

    def scan(self, pyoracle):
        """(the window's centre, a scan of 200 beams in level-0 cells): the start pose and the end points of frame_cases.pair,
        or the first hint of the deep case and every fifth or so beam of its scan (the whole fan)"""
        if self.kind == "deep":
            c = self.case()
            pts = np.asarray(c.query_scans[0], F32)
            pick = np.linspace(0, len(pts) - 1, SCAN_LENS[-1]).astype(np.int64)
            return np.asarray(c.query_init[0], F32), np.ascontiguousarray(pts[pick])
        _, start, pts = fc.pair(self.checker(pyoracle, "ho"), self.frame, self.geom, SCAN_LENS[-1])
        return np.asarray(start, F32), np.ascontiguousarray(pts, F32)


MAPS = [Map(frame, geom) for frame, geom in FRAME_MAPS] + [Map(None, geom) for geom in DEEP]
MAP_IDS = [m.id for m in MAPS]


def map_of(frame, geom):
    return next(m for m in MAPS if m.frame == frame and m.geom == geom)


# ---- casts and rays -----------------------------------------------------------------------------------------------------------------
def range_maxes(grid, meta):
    """cast_cases.range_maxes with "8m" replaced by half the level's diagonal: 8 m means nothing at 1.0 m or 0.025 m cells.
    And one more, 0.45 of the shorter side: a ray of half the diagonal of a level a times as long as it is high (a > 1) that
    runs more along y than along x spans hypot(a, 1) / (2 sqrt 2) of the height at the least -- 1.37 of it at a = 3.75 (90 x 24,
    333 x 90), 0.92 at a = 2.4 (96 x 40, from poses that stand a quarter of the height inside) -- so every such ray ends off
    the level and is refused.  On these maps the rays that walk the row stride as their major step and hit something are the
    ones of this range"""
    r = cast_cases.range_maxes(grid, meta)
    sy, sx = grid.shape
    r["half_diagonal"] = 0.5 * float(np.hypot(sx * meta[2], sy * meta[2]))
    r["short_side"] = SHORT_SIDE * min(sx, sy) * meta[2]
    return {name: r[name] for name in RANGES}


def cast_seed(m, lvl):
    return PICKS.get(("cast", m.id, lvl), lvl)


def level_case(pyoracle, m, lvl, seed=None):
    """grid, metadata, the 37 poses of cast_cases.poses in the level's own metadata, their families, the beam table, the range
    maxima and the 500 mixed rays of a level; no expected value"""
    key = ("level", m.id, lvl, seed)
    if key not in _cache:
        o = m.checker(pyoracle, "ho")
        grid, meta = o.occupancy_grid(lvl), cast_cases.metadata(o, lvl)
        # (cast_cases.poses draws four different occupied cells for its wall family: a level that holds fewer -- the 2 x 2
        # one has three -- offers all its cells instead, and its wall poses stand on four cells of whatever kind)
        cells = grid if (grid == 100).sum() >= 4 else np.full_like(grid, 100)
        poses, fam = cast_cases.poses(_Truth(m.truth(pyoracle)), cells, meta, cast_seed(m, lvl) if seed is None else seed)
        begin, end = cast_cases.mixed_rays(grid, meta, N_RAYS, 100 + lvl)
        _cache[key] = dict(grid=grid, meta=meta, poses=poses, fam=fam, angles=cast_cases.beam_table(N_BEAMS),
                           ranges=range_maxes(grid, meta), begin=begin, end=end)
    return _cache[key]


def expected(pyoracle, m, lvl, kind):
    """the checker's answers of a level: {"cast": {range name: (ranges [37, 200], hit [37, 200, 2], range_max)}, "rays": (dist,
    hit)}; a shorter fan is the first n columns.  Computed once per kind and shared"""
    key = ("expected", m.id, lvl, kind)
    if key not in _cache:
        c = level_case(pyoracle, m, lvl)
        cast = {name: cast_cases.expected_cast(kind, c["grid"], c["meta"], c["poses"], c["angles"], r) + (r,)
                for name, r in c["ranges"].items()}
        _cache[key] = dict(cast=cast, rays=cast_cases.expected_rays(kind, c["grid"], c["meta"], c["begin"], c["end"]))
    return _cache[key]


def numpy_rays(grid, origin, scale, inv_scale, begin, end):
    """getDist ray by ray in numpy fp32 -> dist [n] (-scale without a hit).  The CoordinateTransformer's numbers are arguments
    of their own: the checkers take (origin, resolution) and form the reciprocal themselves"""
    grid = np.asarray(grid)
    sy, sx = grid.shape
    flat = grid.reshape(-1)
    b, e = np.asarray(begin, F32).reshape(-1, 2), np.asarray(end, F32).reshape(-1, 2)
    o, inv = np.asarray(origin, F32), F32(inv_scale)
    fb, fe = ((b - o) * inv).astype(F32), ((e - o) * inv).astype(F32)
    out = np.full(len(b), F32(scale) * F32(-1.0), F32)
    ok = np.isfinite(fb).all(1) & np.isfinite(fe).all(1) & (np.abs(fb) < 2e9).all(1) & (np.abs(fe) < 2e9).all(1)
    for r in np.flatnonzero(ok):
        x0, y0, x1, y1 = int(fb[r, 0]), int(fb[r, 1]), int(fe[r, 0]), int(fe[r, 1])   # truncation
        if not (0 <= x0 < sx and 0 <= y0 < sy and 0 <= x1 < sx and 0 <= y1 < sy):
            continue
        dx, dy = x1 - x0, y1 - y0
        off_x, off_y = (1 if dx > 0 else -1), (1 if dy > 0 else -1) * sx
        if abs(dx) >= abs(dy):
            da, db, off_a, off_b = abs(dx), abs(dy), off_x, off_y
        else:
            da, db, off_a, off_b = abs(dy), abs(dx), off_y, off_x
        offset, err = y0 * sx + x0, da // 2
        for _ in range(min(da, 5000)):
            if flat[offset] == 100:
                fx, fy = F32(x0 - offset % sx), F32(y0 - offset // sx)
                out[r] = F32(scale) * F32(int(np.sqrt(F32(F32(fx * fx) + F32(fy * fy)))))
                break
            offset += off_a
            err += db
            if err >= da:
                offset += off_b
                err -= da
    return out


def hit_directions(c, name, rd):
    """of the general poses' rays at the range `name` (rd: their expected ranges): (hits, misses, hits with |dy| > |dx|, hits
    with |dx| > |dy|), the steps counted in cells of the level"""
    g = c["fam"]["general"]
    begin, end = cast_cases.cast_rays(c["poses"][g], c["angles"], c["ranges"][name])
    ox, oy, res = c["meta"]
    inv = F32(1.0) / F32(res)
    with np.errstate(invalid="ignore", over="ignore"):
        cb = np.trunc((begin - F32([ox, oy])) * inv)
        ce = np.trunc((end - F32([ox, oy])) * inv)
    d = np.abs(ce - cb)
    has = rd[g].reshape(-1) >= 0
    return dict(hits=int(has.sum()), misses=int((~has).sum()), steep=int((has & (d[:, 1] > d[:, 0])).sum()),
                flat=int((has & (d[:, 0] > d[:, 1])).sum()))


def tenth_at(m):
    return "half_diagonal" if m.kind == "frame" and m.geom in TENTH_AT_HALF_DIAGONAL else "short_side"


def cast_conditions(pyoracle, m, lvl, seed=None):
    """what the CPU pin demands of a level at least MIN_SIDE cells in both axes (its docstring says why it is this) ->
    (ok, the figures per range)"""
    c = level_case(pyoracle, m, lvl, seed)
    fig = {}
    for name in ("short_side", "half_diagonal"):
        rd, _ = cast_cases.expected_cast("ho", c["grid"], c["meta"], c["poses"], c["angles"], c["ranges"][name])
        fig[name] = hit_directions(c, name, rd)
        fig[name]["below_row_0"] = int((rd[c["fam"]["edge"].start + 4] >= 0).sum())   # the edge pose half a cell below row 0
    f = fig[tenth_at(m)]
    n = f["hits"] + f["misses"]
    ok = 10 * f["hits"] >= n and 10 * f["misses"] >= n
    ok = ok and fig["half_diagonal"]["hits"] >= 1 and 10 * fig["half_diagonal"]["misses"] >= n
    if m.geom[0] != m.geom[1]:
        ok = ok and fig["short_side"]["steep"] > 0 and fig["short_side"]["flat"] > 0
    if lvl == 0 and m.kind == "frame":
        ok = ok and f["below_row_0"] >= 1
    return ok, fig


def search_picks(pyoracle):
    """-> the PICKS dict for the present generators (run on the CPU when a generator changes; the result is recorded above)"""
    picks = {}
    for m in MAPS:
        for lvl in range(m.levels):
            if min(m.dims(lvl)) < MIN_SIDE:
                continue
            seed = next((s for s in [lvl] + list(range(200)) if cast_conditions(pyoracle, m, lvl, s)[0]), None)
            if seed != lvl:
                picks["cast", m.id, lvl] = seed
    return picks


# ---- windows -------------------------------------------------------------------------------------------------------------------------
def window_step(m):
    return (WINDOW_STEP_CELLS[0] * m.resolution, WINDOW_STEP_CELLS[1] * m.resolution, WINDOW_STEP_ANGLE)


def expected_window(pyoracle, m, lvl, half, n, kind):
    key = ("window", m.id, lvl, half, n, kind)
    if key not in _cache:
        centre, pts = m.scan(pyoracle)
        poses = window_cases.window_poses(centre, window_step(m), half)
        _cache[key] = window_tests.oracle_window(m.checker(pyoracle, kind), lvl, poses, pts[:n])
    return _cache[key]


def reloc_levels(m):
    return [m.levels - 1] + ([DEEP_RELOC_LEVEL] if m.kind == "deep" else [])


def reloc_step(pyoracle, m, lvl):
    cell = m.checker(pyoracle, "ho").level_info(lvl)[2]
    return (float(cell), float(cell), RELOC_ANGLE)


def expected_reloc(pyoracle, m, lvl, kind):
    """reference_relocalize of tests/test_window_model.py on the map's window centre and scan, searched on level lvl.  The
    restatement goes first and counts the reads the reference does not define; the reference itself runs on a defined case only"""
    key = ("reloc", m.id, lvl, kind)
    if key not in _cache:
        centre, pts = m.scan(pyoracle)
        step = reloc_step(pyoracle, m, lvl)
        if kind != "ho":
            expected_reloc(pyoracle, m, lvl, "ho")
        o = m.checker(pyoracle, kind)
        u0 = o.undefined_reads()
        r = reference_relocalize(o, None, centre, pts, step, RELOC_HALF, RELOC_K, search_level=lvl)
        assert o.undefined_reads() == u0, (m.id, lvl, "the reference does not define this relocalisation")
        _cache[key] = r
    return _cache[key]


def tied_places(r):
    """how many window scores equal the best one"""
    s = r["scores"]
    return int((s == np.nanmax(s)).sum())


# ---- copies --------------------------------------------------------------------------------------------------------------------------
COPY_DEEP, COPY_FRAME = (333, 90, 6), (SENSITIVE_FRAME, (96, 40, 3))


def level_boxes(sx, sy):
    """the boxes of tests/test_gpu_copy_map.hand_boxes that fit a level of sx x sy cells (an empty box fits every level), and one
    with an odd x0 and an odd width on a level wide enough for it: no row of it starts or ends on a 16-byte boundary of an
    even-width level, and on an odd-width level the phase changes from row to row besides"""
    out = {}
    for name, (x0, y0, x1, y1) in copy_tests.hand_boxes(sx, sy).items():
        empty = x1 < x0 or y1 < y0
        if empty or (0 <= x0 <= x1 < sx and 0 <= y0 <= y1 < sy):
            out[name] = (x0, y0, x1, y1)
    if sx >= 4:
        w = min(sx - 1, 23)
        w -= int(w % 2 == 0)
        out["odd start, odd width"] = (1, min(1, sy - 1), w, sy - 1)   # columns 1 .. w: w cells
    return out


def copy_rounds(geom=COPY_DEEP):
    """[(names per level, boxes [levels, 4])]: hsm_copy_map_boxes takes one box per level, so round j takes the j-th box of
    every level's list (shorter lists start again); every box of every level is in some round"""
    per_level = [list(level_boxes(geom[0] >> lvl, geom[1] >> lvl).items()) for lvl in range(geom[2])]
    rounds = []
    for j in range(max(len(b) for b in per_level)):
        pick = [b[j % len(b)] for b in per_level]
        rounds.append(([name for name, _ in pick], np.array([box for _, box in pick], np.int32)))
    return rounds


def prior_planes(geom, lvl):
    """what the destination holds in front of a box copy: random planes of its own"""
    rng = np.random.default_rng(9100 + lvl + geom[0])
    return copy_tests.random_planes(rng, geom[0] >> lvl, geom[1] >> lvl)
