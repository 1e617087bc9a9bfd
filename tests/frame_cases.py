"""Inputs for the map-FRAME tests: maps that do not start at (0.5, 0.5) and cell lengths whose reciprocal is inexact.

Every other case module builds its maps at start coordinates (0.5, 0.5) and a resolution of 0.05, 0.1 or 0.125: there the
translation of mapTworld is a whole number of cells, equal in x and y on a square map, the world origin is the map centre and
worldTmap is exactly (cell length, -offset).  The frames below break each of these (FRAMES says which one breaks what;
tests/test_frame_reference.py counts it), on maps whose CELLS are the same in every frame: the room is drawn in cell
coordinates, poses and scans are generated in map coordinates and carried to the world by the checker's own
world_coords_pose.  So whatever differs between two frames' results comes from the frame alone.

Pure numpy; shared by the CPU pin (tests/test_frame_reference.py) and the GPU tests (tests/test_gpu_map_frames.py).
Everything comes from fixed seeds; PICKS records the seeds that had to be searched on the CPU.

frame_numpy / map_coords_numpy / world_coords_numpy are a third statement of GridMapBase::setMapTransformation and the two
pose conversions (GridMapBase.h:226-239, :265-280, MapRepMultiMap.h:48-69), written from the header in numpy fp32.
"""
import numpy as np

import border_cases as bc
from support import upload_planes

_F = np.float32
CONTROL = (0.125, (0.5, 0.5))
FAR = (0.025, (-50.0, 37.0))
FRAMES = [
    (0.025, (0.5, 0.5)),      # the node's default resolution
    (0.03, (0.3, 0.7)),       # inexact scale, inexact and unequal translations
    (0.05, (0.0, 1.0)),       # world origin on a map corner: all world x >= 0, all y <= 0
    (0.1, (-0.25, 1.5)),      # world origin outside the map
    (0.07, (1.0, 0.0)),       # the inverse transform is exactly the cell length; the opposite corner
    (1.0, (0.7, 0.2)),        # scale exactly 1
    FAR,                      # world coordinates of about 80 m on a 64-cell map
    CONTROL,                  # the frame the suite already has
]
GEOMETRIES = list(bc.GEOMETRIES[0:2]) + [(96, 40, 3)]   # the third: two coarser levels to confuse
SCAN_SIZES = (1, 63, 64, 65) + bc.LIST_SIZES            # bc.LIST_SIZES starts with 300
MAP_SEED = 8101
# (frame index, geometry, scan size) -> seed, where seed 0 gave a case the reference does not define or a start pose that
# does not move; searched on the CPU by search_picks() (tests/test_frame_reference.py asserts every pick still holds)
PICKS = {(0, (90, 24, 2), 1): 1, (1, (64, 64, 2), 1): 2, (1, (90, 24, 2), 1): 2, (1, (96, 40, 3), 1): 1, (2, (64, 64, 2), 1): 4,
         (2, (90, 24, 2), 1): 4, (2, (96, 40, 3), 1): 1, (3, (64, 64, 2), 1): 1, (3, (90, 24, 2), 1): 2, (3, (96, 40, 3), 1): 1,
         (4, (90, 24, 2), 1): 4, (4, (96, 40, 3), 1): 1, (5, (90, 24, 2), 1): 1, (5, (96, 40, 3), 1): 1, (6, (90, 24, 2), 1): 2,
         (6, (96, 40, 3), 1): 1, (7, (90, 24, 2), 1): 1}  # only one-beam scans needed one: their H is all but singular
_cache = {}


def fid(frame):
    return "res%g_start%g_%g" % (frame[0], frame[1][0], frame[1][1])


gid = bc.gid
dims = bc.dims


# ---- the third statement of the frame -------------------------------------------------------------------------------------------
def frame_numpy(frame, geom):
    """per level a dict: cell, scale, m = (l00, l01, l10, l11, t0, t1) of mapTworld, w = the same of worldTmap, off = the offset"""
    f = _F
    res, (sx0, sy0) = f(frame[0]), (f(frame[1][0]), f(frame[1][1]))
    offx = f(f(res * f(geom[0])) * sx0)      # MapRepMultiMap.h:53-57: totalMapSize * startCoords
    offy = f(f(res * f(geom[1])) * sy0)
    out = []
    for _ in range(geom[2]):
        s = f(f(1) / res)                    # GridMapBase.h:270
        # :272  Scaling(s, s) * Translation(off): linear diag(s, s), translation (s * offx, s * offy)
        m = (s, f(0), f(0), s, f(s * offx), f(s * offy))
        # :279  the 2 x 2 inverse by cofactors over the determinant, translation = (-linear^-1) * t
        det = f(f(m[0] * m[3]) - f(m[2] * m[1]))
        inv = f(f(1) / det)
        l00, l01, l10, l11 = f(m[3] * inv), f(-m[1] * inv), f(-m[2] * inv), f(m[0] * inv)
        t0 = f(f(-l00 * m[4]) + f(-l01 * m[5]))
        t1 = f(f(-l10 * m[4]) + f(-l11 * m[5]))
        out.append({"cell": res, "scale": s, "m": m, "w": (l00, l01, l10, l11, t0, t1), "off": (offx, offy)})
        res = f(res * f(2))                  # MapRepMultiMap.h:68
    return out


def _apply(a, x, y):
    f = _F
    return f(f(f(a[0] * x) + f(a[1] * y)) + a[4]), f(f(f(a[2] * x) + f(a[3] * y)) + a[5])


def map_coords_numpy(lv, world):
    w = np.asarray(world, _F)
    x, y = _apply(lv["m"], w[0], w[1])
    return np.array([x, y, w[2]], _F)


def world_coords_numpy(lv, mp):
    p = np.asarray(mp, _F)
    x, y = _apply(lv["w"], p[0], p[1])
    return np.array([x, y, p[2]], _F)


def frame_facts(frame, geom):
    """the four facts of level 0 that make a frame worth having -> dict of bools"""
    lv = frame_numpy(frame, geom)[0]
    m, w = lv["m"], lv["w"]
    return {"unequal translations": bool(m[4] != m[5]),
            "fractional translation": bool(m[4] != np.floor(m[4]) or m[5] != np.floor(m[5])),
            "inverse is not the cell length": bool(w[0] != _F(frame[0])),
            "inverse translation is not -offset": bool(w[4] != -lv["off"][0] or w[5] != -lv["off"][1])}


# ---- the maps: one room, drawn in cell coordinates --------------------------------------------------------------------------------
def room(geom, lvl=0):
    """(x0, y0, x1, y1) of the walls in coordinates of level lvl"""
    m = 3.0 * 2 ** (geom[2] - 1)
    k = 1.0 / 2 ** lvl
    return m * k, m * k, (geom[0] - m) * k, (geom[1] - m) * k


def map_planes(geom):
    """per level (log-odds [sy, sx], update index): walls of +2 that fall off over about a cell into free space of -1, plus a
    jitter of a few hundredths that makes every cell's value its own"""
    key = ("map", geom)
    if key not in _cache:
        rng = np.random.default_rng(MAP_SEED + geom[0] + geom[2])
        planes = []
        for lvl in range(geom[2]):
            sx, sy = dims(geom, lvl)
            x0, y0, x1, y1 = room(geom, lvl)
            X, Y = np.meshgrid(np.arange(sx, dtype=np.float64), np.arange(sy, dtype=np.float64))
            inside = (X >= x0) & (X <= x1) & (Y >= y0) & (Y <= y1)
            d_in = np.minimum(np.minimum(X - x0, x1 - X), np.minimum(Y - y0, y1 - Y))
            d_out = np.hypot(np.maximum(np.maximum(x0 - X, X - x1), 0), np.maximum(np.maximum(y0 - Y, Y - y1), 0))
            d = np.where(inside, d_in, d_out)
            base = 3.0 * np.exp(-(d / 1.2) ** 2) - 1.0
            lo = (base + rng.uniform(-0.04, 0.04, (sy, sx))).astype(_F)
            while True:  # fp32 holds about a million values in that band: draw the few cells that collide again
                _, first, count = np.unique(lo, return_index=True, return_counts=True)
                if (count == 1).all():
                    break
                again = np.ones(lo.size, bool)
                again[first] = False
                again = again.reshape(sy, sx)
                lo[again] = (base[again] + rng.uniform(-0.04, 0.04, int(again.sum()))).astype(_F)
            assert np.unique(lo).size == lo.size, "two cells share a value"
            planes.append((lo, np.zeros((sy, sx), np.int32)))
        _cache[key] = planes
    return _cache[key]


def upload(m, geom):
    """the same planes into a checker or a device context: both have upload_level"""
    return upload_planes(m, map_planes(geom))


def new_oracle(pyoracle, kind, frame, geom, factors=None):
    o = pyoracle.Oracle(kind, frame[0], geom[0], geom[1], geom[2], frame[1])
    if factors:
        o.set_update_factor_free(factors[0])
        o.set_update_factor_occupied(factors[1])
    return upload(o, geom)


def checker(pyoracle, kind, frame, geom):
    """one shared checker per kind, frame and geometry; the tests that share it leave its map unchanged"""
    key = ("oracle", kind, frame, geom)
    if key not in _cache:
        _cache[key] = new_oracle(pyoracle, kind, frame, geom)
    return _cache[key]


# ---- poses and scans, generated in map coordinates ----------------------------------------------------------------------------------
def map_poses(geom, n, seed):
    """n level-0 map poses inside the room, 2.5 cells and more from its walls"""
    rng = np.random.default_rng(8200 + 31 * seed + geom[0])
    x0, y0, x1, y1 = room(geom)
    return np.stack([rng.uniform(x0 + 2.5, x1 - 2.5, n), rng.uniform(y0 + 2.5, y1 - 2.5, n), rng.uniform(-3.1, 3.1, n)], 1).astype(_F)


def scan_from(geom, pose_map, n, seed=0):
    """n robot-frame end points (level-0 cell units) of beams over 264 degrees that end on the room's walls, seen from the
    level-0 map pose `pose_map`"""
    rng = np.random.default_rng(8300 + 17 * seed + n)
    px, py, th = (float(v) for v in pose_map)
    a = (np.linspace(-2.3, 2.3, n) if n > 1 else np.array([0.3])) + rng.uniform(-1e-3, 1e-3, n)
    c, s = np.cos(a + th), np.sin(a + th)
    x0, y0, x1, y1 = room(geom)
    with np.errstate(divide="ignore"):
        tx = np.where(c > 0, (x1 - px) / c, (x0 - px) / c)
        ty = np.where(s > 0, (y1 - py) / s, (y0 - py) / s)
    t = np.minimum(tx, ty)
    return np.ascontiguousarray(np.stack([t * np.cos(a), t * np.sin(a)], 1).astype(_F))


def seed_of(frame, geom, n):
    return PICKS.get((FRAMES.index(frame), geom, n), 0)


def pair(o, frame, geom, n, seed=None):
    """(true world pose, start world pose, level-0 end points) of the case of n beams: the scan is drawn from a map pose, the
    start sits 0.3 .. 0.6 cell and 0.02 .. 0.05 rad off it; both reach the world through the checker's world_coords_pose"""
    seed = seed_of(frame, geom, n) if seed is None else seed
    rng = np.random.default_rng(8400 + 13 * seed + n)
    true_map = map_poses(geom, 1, 100 * seed + n)[0]
    pts = scan_from(geom, true_map, n, seed)
    off = rng.uniform(0.3, 0.6, 3) * rng.choice([-1.0, 1.0], 3)
    start_map = (true_map.astype(np.float64) + [off[0], off[1], off[2] / 12.0]).astype(_F)
    return o.world_coords_pose(0, true_map), o.world_coords_pose(0, start_map), pts


def pairs(pyoracle, frame, geom, sizes=SCAN_SIZES):
    """[(tag, start world pose, level-0 end points)] for every scan size, cached"""
    key = ("pairs", frame, geom)
    if key not in _cache:
        o = checker(pyoracle, "ho", frame, geom)
        _cache[key] = {n: pair(o, frame, geom, n) for n in SCAN_SIZES}
    return [("n%d" % n, _cache[key][n][1], _cache[key][n][2]) for n in sizes]


def level_pts(pts, lvl):
    """the container MapRepMultiMap::matchData hands level lvl (setFrom(.., 0.5) per level: exact)"""
    return np.ascontiguousarray(np.asarray(pts, _F) * _F(1.0 / 2 ** lvl))


def geometry_poses(pyoracle, frame, geom, lvl, n=40):
    """n map poses of level lvl and n world poses: over the room, the corners of the map, +-0"""
    o = checker(pyoracle, "ho", frame, geom)
    mp = map_poses(geom, n, 7 + lvl).copy()
    mp[:, :2] *= _F(1.0 / 2 ** lvl)
    sx, sy = dims(geom, lvl)
    mp[:6] = [[0, 0, 0], [-0.0, -0.0, -0.0], [sx - 1, sy - 1, 1.0], [sx - 1, 0, -2.0], [0.5, sy - 0.5, 3.0], [1e-3, -1e-3, 0.1]]
    world = np.stack([o.world_coords_pose(lvl, p) for p in mp])
    rng = np.random.default_rng(8500 + lvl)
    world[n // 2:, :2] += (rng.uniform(-0.5, 0.5, (n - n // 2, 2)) * frame[0]).astype(_F)  # not on the image of a map pose
    return mp, np.ascontiguousarray(world, _F)


def defined_and_moving(pyoracle, frame, geom, n, seed):
    """what PICKS is searched for: the reference defines every result of the case (no NaN coordinate is ever read, all
    poses finite) and the full match moves the start pose"""
    o = checker(pyoracle, "ho", frame, geom)
    u0 = o.undefined_reads()
    _, w, pts = pair(o, frame, geom, n, seed)
    res = [o.match(w, pts)[0]]
    for lvl in range(geom[2]):
        res += [o.match_level(lvl, w, level_pts(pts, lvl), it)[0] for it in range(4)]
    return o.undefined_reads() == u0 and all(np.isfinite(r).all() for r in res) and not np.array_equal(res[0].view(np.uint32), w.view(np.uint32))


def search_picks(pyoracle):
    """-> the PICKS dict for the present generators (run on the CPU when a generator changes; the result is recorded above)"""
    picks = {}
    for fi, frame in enumerate(FRAMES):
        for geom in GEOMETRIES:
            for n in SCAN_SIZES:
                seed = next(s for s in range(200) if defined_and_moving(pyoracle, frame, geom, n, s))
                if seed:
                    picks[(fi, geom, n)] = seed
    return picks


# ---- a batch of start poses, in map order and shuffled ------------------------------------------------------------------------------
def batch(pyoracle, frame, geom, count, n):
    """count start world poses around the n-beam case's true pose (a cloud of +-0.6 cell, +-0.05 rad) over its one scan"""
    o = checker(pyoracle, "ho", frame, geom)
    true_w, _, pts = pair(o, frame, geom, n)
    true_map = o.map_coords_pose(0, true_w)
    rng = np.random.default_rng(8600 + count + n)
    d = rng.uniform(-1.0, 1.0, (count, 3)) * [0.6, 0.6, 0.05]
    starts = np.stack([o.world_coords_pose(0, (true_map.astype(np.float64) + d[k]).astype(_F)) for k in range(count)])
    return np.ascontiguousarray(starts, _F), pts


# ---- the tile sort -----------------------------------------------------------------------------------------------------------------
ORDER_FRAME, ORDER_GEOM, ORDER_N = FRAMES[1], GEOMETRIES[1], 64


def _part1by1_6(v):
    v = v & 0x3F
    v = (v | (v << 4)) & 0x30F
    v = (v | (v << 2)) & 0x333
    v = (v | (v << 1)) & 0x555
    return v


def tile_shift(geom):
    shift = 0
    while (64 << shift) < max(geom[0], geom[1]):
        shift += 1
    return shift


def tile_keys(geom, map_xy):
    """the Morton key of the tile each level-0 map coordinate falls in (64 x 64 tiles over the level, coordinates clamped)"""
    shift = tile_shift(geom)
    c = np.clip(np.asarray(map_xy, np.float64), 0.0, 1.0e6).astype(np.int64)
    tx, ty = np.minimum(c[:, 0] >> shift, 63), np.minimum(c[:, 1] >> shift, 63)
    return np.array([_part1by1_6(int(a)) | (_part1by1_6(int(b)) << 1) for a, b in zip(tx, ty)])


def order_case(pyoracle):
    """(start world poses [64, 3], their level-0 map coordinates by the checker, by the checker with the two translations
    swapped): poses all over the ORDER_GEOM map, none within 0.01 cell of a tile border"""
    o = checker(pyoracle, "ho", ORDER_FRAME, ORDER_GEOM)
    rng = np.random.default_rng(8700)
    T = 1 << tile_shift(ORDER_GEOM)
    mp = np.zeros((ORDER_N, 3), _F)
    k = 0
    while k < ORDER_N:
        p = rng.uniform([1.0, 1.0], [ORDER_GEOM[0] - 1.0, ORDER_GEOM[1] - 1.0])
        if min(np.abs(p / T - np.round(p / T))) * T > 0.01:
            mp[k, :2] = p
            k += 1
    world = np.stack([o.world_coords_pose(0, p) for p in mp])
    back = np.stack([o.map_coords_pose(0, w) for w in world])
    m = frame_numpy(ORDER_FRAME, ORDER_GEOM)[0]["m"]
    swapped = back.copy()
    swapped[:, 0] += m[5] - m[4]
    swapped[:, 1] += m[4] - m[5]
    return np.ascontiguousarray(world, _F), back, swapped


# ---- update sequences and the SLAM log ----------------------------------------------------------------------------------------------
FACTORS = (0.4, 0.9)
N_TRAJ, N_LOG, LOG_BEAMS = 6, 12, 300
GATE_CELLS, GATE_ANGLE = 1.5, 0.1   # the distance threshold is GATE_CELLS * resolution: metres that scale with the frame


def trajectory(pyoracle, frame, geom, count, beams, step=(0.55, 0.2, 0.045)):
    """count map poses along a line through the room's middle, their world poses (by the checker) and a scan from each"""
    o = checker(pyoracle, "ho", frame, geom)
    x0, y0, x1, y1 = room(geom)
    p0 = np.array([x0 + 4.0, (y0 + y1) / 2 - 1.0, 0.1])
    mp = np.stack([p0 + k * np.array(step) for k in range(count)]).astype(_F)
    world = np.ascontiguousarray(np.stack([o.world_coords_pose(0, p) for p in mp]), _F)
    sizes = beams if isinstance(beams, (list, tuple)) else [beams] * count
    scans = [scan_from(geom, mp[k], sizes[k], 50 + k) for k in range(count)]
    return mp, world, scans


def thresholds(frame):
    return float(_F(GATE_CELLS * frame[0])), GATE_ANGLE


def slam_log(pyoracle, frame, geom):
    """(world poses [12, 3] the scans were drawn from, hint deltas [12, 3] in fp32, 12 scans of 300 beams)"""
    _, world, scans = trajectory(pyoracle, frame, geom, N_LOG, LOG_BEAMS)
    deltas = np.zeros((N_LOG, 3), _F)
    deltas[1:] = world[1:] - world[:-1]
    return world, deltas, scans


def raw_log(pyoracle, frame, geom):
    """the log as a laser on a moving mount sees it -> (world poses, hint deltas, ranges [12, 300] in metres, tf rows [12, 12],
    angle_min, angle_increment, (range_min, range_max, range_cutoff), (sqr_min, sqr_max, z_min, z_max)).  The mount is a
    translation of up to 1.5 cells that differs from scan to scan, so every scan has an origo of its own"""
    o = checker(pyoracle, "ho", frame, geom)
    mp, world, _ = trajectory(pyoracle, frame, geom, N_LOG, LOG_BEAMS)
    deltas = np.zeros((N_LOG, 3), _F)
    deltas[1:] = world[1:] - world[:-1]
    rng = np.random.default_rng(8900)
    res = float(frame[0])
    n = LOG_BEAMS
    a0, inc = -2.3, float(_F(4.6 / (n - 1)))
    x0, y0, x1, y1 = room(geom)
    ranges, rows = np.empty((N_LOG, n), _F), np.empty((N_LOG, 12), np.float64)
    for k in range(N_LOG):
        t = rng.uniform(-1.5, 1.5, 2)  # cells, in the robot's frame
        px, py, th = (float(v) for v in mp[k])
        lx, ly = px + np.cos(th) * t[0] - np.sin(th) * t[1], py + np.sin(th) * t[0] + np.cos(th) * t[1]
        a = a0 + inc * np.arange(n)
        c, s = np.cos(a + th), np.sin(a + th)
        with np.errstate(divide="ignore"):
            tx = np.where(c > 0, (x1 - lx) / c, (x0 - lx) / c)
            ty = np.where(s > 0, (y1 - ly) / s, (y0 - ly) / s)
        ranges[k] = (np.minimum(tx, ty) * res).astype(_F)
        rows[k] = [1, 0, 0, t[0] * res, 0, 1, 0, t[1] * res, 0, 0, 1, 0]
    ranges[:, 7::53] = np.inf  # a few beams the conversion drops
    lim = (float(_F(0.5 * res)), float(_F(300.0 * res)), float(_F(300.0 * res)))
    gates = (float(_F((0.2 * res) ** 2)), float(_F((300.0 * res) ** 2)), -1.0, 1.0)
    return world, deltas, ranges, rows, a0, inc, lim, gates


def convert_log(o, raw):
    """the node's projectLaser + rosPointCloudToDataContainer per scan, by the checker -> ([end points], origos [12, 2])"""
    _, _, ranges, rows, a0, inc, lim, gates = raw
    conts, origos = [], np.empty((len(ranges), 2), _F)
    for k in range(len(ranges)):
        cloud = o.project_laser(ranges[k], a0, inc, lim[0], lim[1], lim[2])
        pts, origos[k] = o.point_cloud_to_container(cloud, rows[k], gates[0], gates[1], gates[2], gates[3], o.scale_to_map())
        conts.append(np.ascontiguousarray(pts, _F).reshape(-1, 2))
    return conts, origos


def reference_loop(o, frame, world, deltas, scans, origos=None):
    """HectorSlamProcessor::update per scan on a checker of its own (its map changes) -> (poses, covariances, gate decisions);
    the decisions by the checker's own poseDifferenceLargerThan from lastMapUpdatePose = FLT_MAX"""
    thr = thresholds(frame)
    o.proc_set_thresholds(*thr)
    last = np.full(3, np.finfo(_F).max, _F)
    pose = world[0].copy()
    poses, covs, flags = [], [], []
    for k in range(len(scans)):
        o.proc_update(scans[k], (pose + deltas[k]).astype(_F), np.zeros(2, _F) if origos is None else origos[k], False)
        pose, cov = o.proc_last_pose()
        go = o.pose_difference_larger_than(pose, last, thr[0], thr[1])
        if go:
            last = pose.copy()
        poses.append(pose.copy())
        covs.append(cov.copy())
        flags.append(go)
    return np.array(poses), np.array(covs), np.array(flags)
