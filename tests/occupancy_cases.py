"""Inputs for the changed-cells export of the published grid (hsm_occupancy_changes*; tests/test_gpu_occupancy_changes.py).

Geometry: a 3-level pyramid of 100 x 76, 50 x 38 and 25 x 19 cells -- widths that are a multiple of 4, even but no multiple of 4,
and odd, so the 4-cell groups of the export kernel start at every phase of a row.  Resolution 0.125 and start (0.5, 0.5) as in
tests/border_cases.py, whose construction this reuses: a world pose that is a multiple of a cell has an EXACT map pose on every
level, and at theta = 0 an end point p lands on map coordinate e + p, so a scan can be aimed at a column or row by number.
Scans have 16 - 181 beams.  Pure numpy, fixed seeds."""
import numpy as np

import border_cases as bc

RES = bc.RES
START = bc.START
GEOM = (100, 76, 3)
LEVELS = GEOM[2]
POISON = 55
_F = np.float32


def dims(lvl):
    return GEOM[0] >> lvl, GEOM[1] >> lvl


def world_pose(mx, my, theta=0.0):
    """the world pose whose level-0 map pose is (mx, my, theta); exact for multiples of a cell (border_cases.exact_world_pose)"""
    return np.array([(mx - GEOM[0] * 0.5) * RES, (my - GEOM[1] * 0.5) * RES, theta], _F)


def aimed_scan(robot, targets):
    """level-0 end points (robot frame, theta = 0) that land on the map coordinates `targets`"""
    t = np.asarray(targets, _F).reshape(-1, 2)
    return np.ascontiguousarray(t - np.asarray(robot, _F)[None, :2])


def edge_scans():
    """name -> (world pose, scan): scans whose end cells lie in column 0, the last column, row 0 and the last row of level 0,
    and one whose box starts at an odd column (its begin cell, the lowest x of the scan)"""
    sx, sy = dims(0)
    n = 24
    ys = np.linspace(3.0, sy - 4.0, n)
    xs = np.linspace(3.0, sx - 4.0, n)
    out = {}
    r = (40.0, 30.0)
    out["column 0"] = (world_pose(*r), aimed_scan(r, np.stack([np.zeros(n), ys], 1)))
    out["last column"] = (world_pose(*r), aimed_scan(r, np.stack([np.full(n, sx - 1.0), ys], 1)))
    out["row 0"] = (world_pose(*r), aimed_scan(r, np.stack([xs, np.zeros(n)], 1)))
    out["last row"] = (world_pose(*r), aimed_scan(r, np.stack([xs, np.full(n, sy - 1.0)], 1)))
    r = (41.0, 31.0)  # begin cell (41, 31); level 1: (int)(20.5 + 0.5) = 21, (int)(15.5 + 0.5) = 16
    fan = np.stack([np.linspace(47.0, 66.0, 16), np.linspace(33.0, 52.0, 16)], 1)
    out["odd x"] = (world_pose(*r), aimed_scan(r, fan))
    return out


def room_scans(count, beams=181, seed=11):
    """`count` posed scans of a loop in a room that fits the map (tests/rect_cases.py's scene at this geometry)"""
    import rect_cases
    _, poses, scans = rect_cases.scene(GEOM[0], GEOM[1], count, beams, seed, res=RES, grow=0.9)
    return np.ascontiguousarray(poses, _F), [np.ascontiguousarray(s, _F) for s in scans]


def zero_cell_scans():
    """two one-beam-wide scans from (40, 30): the first ends in cell (60, 30) and crosses (50, 30), the second ends IN (50, 30).
    With update factors 0.4 / 0.6 the log-odds of (50, 30) is free + occupied = exactly 0 (the two are each other's negative)"""
    r = (40.0, 30.0)
    a = aimed_scan(r, [[60.0, 30.0]] * 16)
    b = aimed_scan(r, [[50.0, 30.0]] * 16)
    return world_pose(*r), a, b


def special_planes():
    """per level (log-odds, update index): zeros except four cells per level -- NaN, -0.0, +inf, -inf -- and a sprinkle of
    finite values; and where the four are: (y, x) per level"""
    rng = np.random.default_rng(415)
    planes, where = [], []
    for lvl in range(LEVELS):
        sx, sy = dims(lvl)
        lo = np.zeros((sy, sx), _F)
        idx = rng.choice(sx * sy, 40, replace=False)
        lo.reshape(-1)[idx] = rng.uniform(-2, 2, 40).astype(_F)
        cells = [(1, 1), (sy - 1, sx - 1), (2, sx - 2), (sy - 2, 0)]
        for (y, x), v in zip(cells, (np.nan, -0.0, np.inf, -np.inf)):
            lo[y, x] = v
        planes.append((lo, np.zeros((sy, sx), np.int32)))
        where.append(cells)
    return planes, where


def inside(box, inner):
    """inner (x0, y0, x1, y1) lies in box; an empty inner lies in anything"""
    if inner[2] < inner[0]:
        return True
    return box[2] >= box[0] and box[0] <= inner[0] and box[1] <= inner[1] and box[2] >= inner[2] and box[3] >= inner[3]


def union(boxes):
    out = [0, 0, -1, -1]
    for b in boxes:
        if b[2] < b[0]:
            continue
        out = [int(v) for v in b] if out[2] < out[0] else [min(out[0], b[0]), min(out[1], b[1]), max(out[2], b[2]), max(out[3], b[3])]
    return out


def hull_of(mask):
    """the box of the True cells of mask [sy, sx], (0, 0, -1, -1) where there is none"""
    ys, xs = np.nonzero(mask)
    if ys.size == 0:
        return [0, 0, -1, -1]
    return [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())]
