"""Inputs for the RESTORED-STAMP tests of updateByScan: levels uploaded with hsm_upload_level whose stamp plane holds values at or
ahead of the context's update counter, then integrated.

The reference's cell rules read the stored stamp (OccGridMapBase.h bresenhamCellFree / bresenhamCellOcc): with F, O the scan's
free and occupied marks (counter + 1, + 2) and s the cell's stamp in front of the scan,
    s >= O   the cell stays as it is;
    s == F   (possible through an upload only) a crossing does nothing; an end applies unsetFree (l -= f) -- whether or not the
             scan crossed the cell first --, then the occupied update, stamp O;
    s <  F   the usual rule (order_cases.py).
Every update test before this one had every stamp below the counter.

Pure numpy, fixed seeds; shared by the CPU pin (tests/test_stamp_reference.py) and the GPU tests
(tests/test_gpu_restored_stamps.py).

Geometry: the two smallest of border_cases.GEOMETRIES, (64, 64, 2) -- rows a multiple of 64 cells: apply_box's aligned body --
and (90, 24, 2) -- the other body, partial quad tiles on both levels.  Resolution 0.05, the sensor at a cell centre with theta
0 (order_cases' convention).  The scans are order_cases' pattern scan from that sensor: cells ended in before they are crossed,
crossed before they are ended in, ended in by several beams, OUTSIDE and BEGIN beams, a wavefront of skipped beams only.

Planes: per level the cells scan 0 ends in (E), the cells it only crosses (C) and the rest each take (stamp, log-odds) pairs in
turn from a list, along a seeded permutation -- so every class the tests ask for holds enough touched cells on both levels.
Stamps are relative to the counter U at upload time (0, or 15 after W = 5 warm-up updates):
    -1, U-1, U          below every mark
    U+1, U+2            scan 0's free / occupied mark
    U+3, U+4, U+5       the counter after scan 0, scan 1's marks
    U+10, U+11          scan M = 3's marks: these cells thaw partway through the batch of 8
    1 << 20             frozen for the whole test
Log-odds: young cells in +-2.5; k free updates for k in 4, 5, 9, 10, 19, 20 (next to -2, -4, -8, where (l + f) - f != l and
l - f leaves the binade); 49.6, 50.0, 50.5 (unsetFree on a stored free mark takes them across the `< 50.0f` test)."""
import numpy as np

import border_cases as bc
import order_cases as oc
from edge_cases import world_pose_of_cell
from support import upload_planes

RES = oc.RES
FACTOR_FREE, FACTOR_OCC = oc.FACTOR_FREE, oc.FACTOR_OCC
GEOMETRIES = bc.GEOMETRIES[:2]
assert GEOMETRIES == [(64, 64, 2), (90, 24, 2)]
LEVELS = 2
SENSORS = {(64, 64, 2): (32, 32), (90, 24, 2): (45, 12)}
WARM = 5                       # warm-up updates of the warmed counter
COUNTERS = (0, 3 * WARM)       # U at upload time
ORDERS = ("given", "reversed")
BATCH, M_THAW = 8, 3
FAR = 1 << 20
DENSE_BEAMS = 4096             # HSM_MERGED_MARK_MAX's default: the byte-map form from this many beams on
# the batch's sensor cells, as offsets from the geometry's sensor (scan 0 is the single-scan cases' pose)
BATCH_SHIFTS = ((0, 0), (1, 0), (1, 1), (0, 1), (0, 0), (-1, -1), (-1, 0), (1, -1))
# the movement gate of the gated entries: a move of one cell (0.05 m) is rejected, a diagonal one (0.0707 m) accepted
GATE_MIN_DIST, GATE_MIN_ANGLE = 0.06, 0.5

STAMP_CLASSES = ("minus1", "U-1", "U", "U+1", "U+2", "U+3", "U+4", "U+5", "thaw_free", "thaw_occ", "far")
LO_CLASSES = ("young", "binade", "clamp")
# (stamp class, log-odds class) in turn over the cells scan 0 ends in ...
_E_LIST = [("U+1", "clamp"), ("U+1", "young"), ("U+1", "binade"), ("minus1", "binade"), ("U+1", "clamp"), ("U+2", "young"),
           ("U+1", "binade"), ("thaw_free", "young"), ("U+1", "clamp"), ("U", "clamp"), ("U+1", "young"), ("far", "young"),
           ("U+4", "clamp"), ("thaw_occ", "binade"), ("U+1", "binade"), ("U-1", "binade")]
# ... over the cells it only crosses ...
_C_LIST = [("U+1", "young"), ("far", "young"), ("U+2", "binade"), ("U+1", "binade"), ("thaw_free", "binade"), ("minus1", "young"),
           ("U+1", "clamp"), ("thaw_occ", "young"), ("far", "clamp"), ("U+2", "young"), ("U+1", "young"), ("U+4", "binade")]
# ... and over the cells it does not touch (later scans of the batch reach some of them)
_R_LIST = [(s, l) for s in STAMP_CLASSES for l in LO_CLASSES]
_cache = {}


def gid(g):
    return bc.gid(g)


def dims(geom, lvl):
    return geom[0] >> lvl, geom[1] >> lvl


def stamp_value(name, U):
    return {"minus1": -1, "U-1": U - 1, "U": U, "U+1": U + 1, "U+2": U + 2, "U+3": U + 3, "U+4": U + 4, "U+5": U + 5,
            "thaw_free": U + 3 * M_THAW + 1, "thaw_occ": U + 3 * M_THAW + 2, "far": FAR}[name]


def sensor_pose(geom, shift=(0, 0)):
    cx, cy = SENSORS[geom]
    return world_pose_of_cell(RES, geom[0], geom[1], float(cx + shift[0]), float(cy + shift[1]), 0.0)


def map_pose(geom, lvl, shift=(0, 0)):
    """the sensor's map coordinates on level lvl (the checkers' getMapCoordsPose gives these bits: pinned by the CPU test)"""
    cx, cy = SENSORS[geom]
    f = np.float32(1.0 / 2 ** lvl)
    return np.array([(cx + shift[0]) * f, (cy + shift[1]) * f, 0.0], np.float32)


# ---- scans --------------------------------------------------------------------------------------------------------------------------
def _in_order(pts, order):
    return np.ascontiguousarray(pts if order == "given" else pts[::-1])


def keyed_scan(order="given"):
    """order_cases' pattern scan below the byte-map threshold (4095 beams)"""
    return _in_order(oc.pattern_cut(), order)


def dense_scan(order="given"):
    """the same with one more beam of the tail: 4096 beams, the shortest scan that takes the byte-map form"""
    return _in_order(oc.pattern_scan()[:DENSE_BEAMS], order)


def short_scan(order="given"):
    """the pattern in front of its tail and 64 beams of the tail: the batch's scans"""
    _, info = oc.pattern_sequence()
    return _in_order(oc.pattern_scan()[:info["tail"] + 64], order)


def warm_scan():
    """four beams: what the warm-up updates integrate (the upload replaces both planes afterwards)"""
    return np.float32([[3.0, 0.2], [0.1, 3.0], [-3.0, 0.3], [0.2, -3.0]])


def batch(geom, order="given"):
    """-> (poses [8, 3], [scans]): the short scan from eight sensor cells next to each other"""
    poses = np.stack([sensor_pose(geom, s) for s in BATCH_SHIFTS])
    return poses, [short_scan(order)] * BATCH


# ---- the update as numpy ------------------------------------------------------------------------------------------------------------
def touches(geom, lvl, pose_map, pts_level):
    """-> (first_free, first_occ): per cell of level lvl the lowest index of a beam that crosses it / ends in it, n where none
    does.  updateByScan's beam geometry at theta 0 (OccGridMapBase.h:137-207): end = (int)(t + p + 0.5), skipped when it is the
    begin cell or either lies off the map; the line's step i sits i major steps and (da / 2 + i * db) / da minor steps out."""
    sx, sy = dims(geom, lvl)
    p = np.asarray(pts_level, np.float32)
    n = len(p)
    t = np.asarray(pose_map, np.float32)
    assert t[2] == 0.0
    ex = ((t[0] + p[:, 0]) + np.float32(0.5)).astype(np.float32)
    ey = ((t[1] + p[:, 1]) + np.float32(0.5)).astype(np.float32)
    x1, y1 = np.trunc(ex).astype(np.int64), np.trunc(ey).astype(np.int64)
    x0, y0 = int(np.float32(t[0] + np.float32(0.5))), int(np.float32(t[1] + np.float32(0.5)))
    valid = ~((x1 == x0) & (y1 == y0)) & (x1 >= 0) & (x1 < sx) & (y1 >= 0) & (y1 < sy)
    valid &= 0 <= x0 < sx and 0 <= y0 < sy
    dx, dy = x1 - x0, y1 - y0
    adx, ady = np.abs(dx), np.abs(dy)
    xmaj = adx >= ady
    da, db = np.where(xmaj, adx, ady), np.where(xmaj, ady, adx)
    sgx, sgy = np.where(dx > 0, 1, -1), np.where(dy > 0, 1, -1)
    first_free = np.full(sx * sy, n, np.int64)
    first_occ = np.full(sx * sy, n, np.int64)
    idx = np.arange(n)
    np.minimum.at(first_occ, (y1 * sx + x1)[valid], idx[valid])
    for i in range(int(da[valid].max()) if valid.any() else 0):
        m = valid & (da > i)
        q = (da[m] // 2 + i * db[m]) // da[m]
        cx = x0 + np.where(xmaj[m], i * sgx[m], q * sgx[m])
        cy = y0 + np.where(xmaj[m], q * sgy[m], i * sgy[m])
        np.minimum.at(first_free, cy * sx + cx, idx[m])
    return first_free.reshape(sy, sx), first_occ.reshape(sy, sx)


def model_update(lo, ui, first_free, first_occ, n, mark_free, f, o, blind):
    """one scan on one level -> (log-odds, stamps).  blind: the rule of map_update.h's header comment with the stored stamp
    ignored -- what the apply passes did before they read it; else the reference's rule (the module docstring)."""
    lo, ui = lo.copy(), ui.copy()
    F, O = mark_free, mark_free + 1
    occ, fre = first_occ < n, first_free < n
    frozen = np.zeros_like(occ) if blind else ui >= O
    stored = np.zeros_like(occ) if blind else ui == F
    e = occ & ~frozen
    l = lo[e]
    sf = stored[e]
    rev = (first_free[e] < first_occ[e]) & ~sf
    l = np.where(rev, ((l + f).astype(np.float32) - f).astype(np.float32), l)
    l = np.where(sf, (l - f).astype(np.float32), l)
    l = np.where(l < np.float32(50.0), (l + o).astype(np.float32), l)
    lo[e] = l
    ui[e] = O
    c = fre & ~occ & ~frozen & ~stored
    lo[c] = (lo[c] + f).astype(np.float32)
    ui[c] = F
    return lo, ui


def log_odds_steps():
    """(f, o) as the levels hold them, GridMapLogOdds.h:196-200: logf of the fp32 odds p / (1 - p) -- here the float64 logarithm
    rounded once (numpy's own float32 log is an ulp off for 0.4; the CPU test pins these bits against the checkers)"""
    def step(p):
        odds = np.float32(p) / (np.float32(1.0) - np.float32(p))
        return np.float32(np.log(np.float64(odds)))
    return step(FACTOR_FREE), step(FACTOR_OCC)


# ---- planes -------------------------------------------------------------------------------------------------------------------------
def _lo_value(cls, rng):
    if cls == "young":
        return np.float32(rng.uniform(-2.5, 2.5))
    if cls == "clamp":
        return np.float32(rng.choice([49.6, 50.0, 50.5]))
    f = np.float32(np.log(0.4 / 0.6))
    l = np.float32(0.0)
    for _ in range(int(rng.choice([4, 5, 9, 10, 19, 20]))):
        l = np.float32(l + f)
    return l


def class_planes(geom):
    """per level (stamp class index [sy, sx], log-odds [sy, sx]); the same for both counters"""
    key = ("classes", geom)
    if key not in _cache:
        out = []
        for lvl in range(LEVELS):
            sx, sy = dims(geom, lvl)
            rng = np.random.default_rng(7301 + 13 * lvl + geom[0])
            ff, fo = touches(geom, lvl, map_pose(geom, lvl), keyed_scan() * np.float32(1.0 / 2 ** lvl))
            n = len(keyed_scan())
            ended, crossed = (fo < n).reshape(-1), ((ff < n) & ~(fo < n)).reshape(-1)
            cls = np.zeros(sx * sy, np.int32)
            lo = np.zeros(sx * sy, np.float32)
            for sel, combos in ((ended, _E_LIST), (crossed, _C_LIST), (~ended & ~crossed, _R_LIST)):
                cells = rng.permutation(np.flatnonzero(sel))
                for j, c in enumerate(cells):
                    s, l = combos[j % len(combos)]
                    cls[c] = STAMP_CLASSES.index(s)
                    lo[c] = _lo_value(l, rng)
            out.append((cls.reshape(sy, sx), lo.reshape(sy, sx)))
        _cache[key] = out
    return _cache[key]


def planes(geom, U):
    """per level (log-odds [sy, sx] float32, stamps [sy, sx] int32) for a level whose counter is U at upload time"""
    vals = np.array([stamp_value(s, U) for s in STAMP_CLASSES], np.int32)
    return [(lo.copy(), vals[cls]) for cls, lo in class_planes(geom)]


def upload(m, geom, U):
    """the planes into a checker (pyoracle.Oracle) or a device context (capi.MapRepMultiMap)"""
    return upload_planes(m, planes(geom, U))


# ---- the checkers -------------------------------------------------------------------------------------------------------------------
def new_checker(pyoracle, kind, geom):
    o = pyoracle.Oracle(kind, RES, geom[0], geom[1], geom[2])
    o.set_update_factor_free(FACTOR_FREE)
    o.set_update_factor_occupied(FACTOR_OCC)
    return o


def checker_update(o, pose, pts):
    """one updateByScan on every level, each with the container scaled to it (matchData's setFrom, MapRepMultiMap.h:127,143)"""
    o.build_map(np.asarray(pose, np.float32)[None, :], [pts])


def restored_checker(pyoracle, kind, geom, U):
    """a checker whose counter is U (U / 3 warm-up updates) with the planes for U uploaded"""
    o = new_checker(pyoracle, kind, geom)
    for _ in range(U // 3):
        checker_update(o, sensor_pose(geom), warm_scan())
    return upload(o, geom, U)


def snapshot(o):
    return [o.download_level(lvl) for lvl in range(LEVELS)]


def run_checker(pyoracle, kind, geom, U, poses, scans):
    """-> (the checker, [its planes after every scan])"""
    o = restored_checker(pyoracle, kind, geom, U)
    snaps = []
    for pose, pts in zip(poses, scans):
        checker_update(o, pose, pts)
        snaps.append(snapshot(o))
    return o, snaps


SINGLE_CASES = ("keyed", "dense")


def case_scans(geom, case, order):
    """-> (poses, scans) of "keyed", "dense" (one scan from the sensor) or "batch" (eight)"""
    if case == "batch":
        return batch(geom, order)
    return sensor_pose(geom)[None, :], [keyed_scan(order) if case == "keyed" else dense_scan(order)]
