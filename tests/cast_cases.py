"""The cases of the expected-scan tests (hsm_cast_scans*, hsm_ray_distances_device), built on the CPU and shared by
test_cast_scans_reference.py (which holds the two CPU checkers to each other on them, and asserts what the GPU test relies on) and
test_gpu_cast_scans.py.

The ray of beam i at sensor pose (px, py, theta), restated in numpy fp32 -- one rounding per operation, no fused multiply-add,
sin and cos from the host libm through the checker (pyoracle.libm_sincosf), never numpy's:

    a = theta + angles[i];  (s, c) = sincosf(a);  begin = (px, py);  end = (px + range_max * c, py + range_max * s)

and the expected answer is DistanceMeasurementProvider::getDist of that ray on the level's published grid with the level's own
metadata.  A ray with a non-finite coordinate is "without a hit" by the library's stated rule (capi.h); the checkers are not asked.
"""
import numpy as np

from oracle import pyoracle

B = 37                       # a ragged last workgroup in either launch shape
BEAMS = (1, 63, 64, 65, 1081)
F32 = np.float32


def metadata(o, level):
    """(origin_x, origin_y, resolution) of a level as the node publishes them: the floats of capi.map_metadata"""
    _, _, cell, _ = o.level_info(level)
    w = o.world_coords_pose(level, np.zeros(3, F32))
    half = F32(cell) * F32(0.5)
    return float(F32(w[0]) - half), float(F32(w[1]) - half), float(cell)


def beam_table(n=1081):
    """n sensor-frame angles: the node's fp32 running sum over 270 degrees, with exact multiples of pi/4, duplicates and one
    unsorted stretch planted at the front (so that every fan length of BEAMS has some)"""
    inc = F32(np.deg2rad(270.0) / 1080.0)
    t = np.empty(max(n, 64), F32)
    a = F32(-np.deg2rad(135.0))
    for i in range(t.size):
        t[i] = a
        a = F32(a + inc)  # angle += angle_increment
    quarter = F32(np.pi / 4)
    t[0:9] = [F32(k) * quarter for k in (0, 1, -1, 2, -2, 3, -3, 4, -4)]
    t[9:12] = t[1:4]                      # duplicates
    t[12:15] = t[12]
    t[20:40] = t[20:40][::-1].copy()      # an unsorted stretch
    return t[:n].copy()


def cell_centre(meta, cx, cy):
    ox, oy, res = meta
    return [ox + (cx + 0.5) * res, oy + (cy + 0.5) * res]


def poses(sc, grid, meta, seed):
    """(poses [B, 3], families): name -> slice of the poses"""
    rng = np.random.default_rng(seed)
    sy, sx = grid.shape
    ox, oy, res = meta
    truth = np.asarray(sc.query_truth, F32)
    general = np.concatenate([truth[:16], truth[:4] + rng.normal(0, [0.3, 0.3, 0.5], (4, 3))]).astype(F32)
    occ = np.argwhere(grid == 100)
    pick = occ[rng.choice(len(occ), 4, replace=False)]
    # on a wall cell, 0.15 cells from its right-hand border: a third of a cell crosses it for some beams (one step, on the wall)
    wall = np.array([cell_centre(meta, cx + 0.35, cy) + [rng.uniform(-3, 3)] for cy, cx in pick], F32)
    edge = np.array([cell_centre(meta, 0, 0) + [0.7], cell_centre(meta, sx - 1, 0) + [2.5], cell_centre(meta, 0, sy - 1) + [-0.6],
                     cell_centre(meta, sx - 1, sy - 1) + [-2.4],
                     [ox + 0.5 * sx * res, oy - 0.51 * res, 1.5]], F32)  # (half a cell below row 0 truncates INTO row 0)
    outside = np.array([[ox - 1.0, oy + 0.5 * sy * res, 0.0], [ox + (sx + 3) * res, oy + 0.5 * sy * res, 3.0],
                        [ox + 0.5 * sx * res, oy - 1.51 * res, 1.5], [1e9, -1e9, 0.3]], F32)
    c = truth[0]
    nonfinite = np.array([[c[0], c[1], np.nan], [c[0], c[1], np.inf], [np.nan, c[1], 0.2], [c[0], -np.inf, 0.2]], F32)
    all_poses = np.concatenate([general, wall, edge, outside, nonfinite]).astype(F32)
    fam, at = {}, 0
    for name, block in (("general", general), ("wall", wall), ("edge", edge), ("outside", outside), ("nonfinite", nonfinite)):
        fam[name] = slice(at, at + len(block))
        at += len(block)
    assert len(all_poses) == B
    return all_poses, fam


def range_maxes(grid, meta):
    sy, sx = grid.shape
    res = meta[2]
    diag = float(np.hypot(sx * res, sy * res))
    return {"zero": 0.0, "sub_cell": 0.3 * res, "8m": 8.0, "two_diagonals": 2.0 * diag}


def cast_rays(poses_world, angles, range_max, kind="ho"):
    """(begin [B*n, 2], end [B*n, 2]) of every beam of every pose, fp32 in the order the header states"""
    p = np.asarray(poses_world, F32).reshape(-1, 3)
    ang = np.asarray(angles, F32).reshape(-1)
    a = (p[:, 2:3] + ang[None, :]).astype(F32)
    with np.errstate(invalid="ignore"):
        s, c = pyoracle.libm_sincosf(a.reshape(-1), kind)
        s, c = s.reshape(a.shape), c.reshape(a.shape)
        r = F32(range_max)
        ex = p[:, 0:1] + r * c
        ey = p[:, 1:2] + r * s
    begin = np.broadcast_to(p[:, None, :2], a.shape + (2,)).reshape(-1, 2)
    end = np.stack([ex, ey], -1).astype(F32).reshape(-1, 2)
    return np.ascontiguousarray(begin, F32), np.ascontiguousarray(end, F32)


def expected_rays(kind, grid, meta, begin, end):
    """(dist [n], hit [n, 2] NaN without a hit): the checker's getDist; a ray with a non-finite coordinate by the stated rule"""
    begin, end = np.asarray(begin, F32).reshape(-1, 2), np.asarray(end, F32).reshape(-1, 2)
    bad = ~(np.isfinite(begin).all(1) & np.isfinite(end).all(1))
    b, e = begin.copy(), end.copy()
    b[bad] = e[bad] = [meta[0], meta[1]]
    dist, hit = pyoracle.ray_distances(kind, grid, (meta[0], meta[1]), meta[2], b, e)
    dist[bad] = F32(meta[2]) * F32(-1.0)
    hit[bad] = np.nan
    return dist, hit


def expected_cast(kind, grid, meta, poses_world, angles, range_max):
    """(ranges [B, n], hit [B, n, 2])"""
    Bn, n = len(poses_world), len(angles)
    dist, hit = expected_rays(kind, grid, meta, *cast_rays(poses_world, angles, range_max, kind))
    return dist.reshape(Bn, n), hit.reshape(Bn, n, 2)


def mixed_rays(grid, meta, n, seed):
    """arbitrary rays of a level: begins in and slightly around it, any direction and length, zero-length and axis-parallel ones"""
    rng = np.random.default_rng(seed)
    sy, sx = grid.shape
    ox, oy, res = meta
    ext = np.array([sx * res, sy * res])
    begin = (np.array([ox, oy]) + rng.uniform(-0.05, 1.05, (n, 2)) * ext).astype(F32)
    ang = rng.uniform(0, 2 * np.pi, n)
    end = (begin + np.stack([np.cos(ang), np.sin(ang)], 1) * (rng.uniform(0.0, 0.6, n) * ext.max())[:, None]).astype(F32)
    end[:40] = begin[:40]
    end[40:80, 1] = begin[40:80, 1]
    end[80:120, 0] = begin[80:120, 0]
    return begin, end


# ---- the cap of 5000 steps: the smallest map that reaches it --------------------------------------------------------------------
CAP_SX, CAP_SY, CAP_RES, CAP_WALL = 6000, 16, 0.05, 5600
CAP_FAR_CELLS, CAP_NEAR_CELLS = 5420, 4920          # range_max in cells: the end cell is the same for a beam and its near twin
CAP_ANGLES = np.array([0.0, 0.0005, -0.0005, 0.001, -0.001], F32)  # along the corridor: at most six rows over 5420 cells


def cap_logodds():
    """a wall CAP_WALL cells out and a free corridor to it; unknown cells elsewhere"""
    lo = np.zeros((CAP_SY, CAP_SX), F32)
    lo[:, CAP_WALL:CAP_WALL + 3] = 2.0
    lo[2:14, 0:CAP_WALL] = -1.0
    return lo


def cap_grid():
    lo = cap_logodds()
    return np.where(lo > 0, 100, np.where(lo < 0, 0, -1)).astype(np.int8)


def cap_poses(meta):
    """(far, near): beams along +x from cells 181..559 of row 8 -- the wall is 5041..5419 steps away, behind the cap -- and the
    same beams started 500 cells closer"""
    cols = np.array([181, 200, 333, 480, 559], np.int64)
    far = np.array([cell_centre(meta, cx, 8) + [0.0] for cx in cols], F32)
    near = np.array([cell_centre(meta, cx + 500, 8) + [0.0] for cx in cols], F32)
    return far, near


CAP_EDGE_CELLS = 5300


def cap_edge_poses(meta):
    """either side of the cap's last step, beams of CAP_EDGE_CELLS cells: from cell 600 the wall is step 5000 (never looked at),
    from cell 601 it is step 4999 (the last one that is)"""
    return np.array([cell_centre(meta, 600, 8) + [0.0], cell_centre(meta, 601, 8) + [0.0]], F32)
