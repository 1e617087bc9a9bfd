"""Inputs and the host model of a merge of two pyramids under a rigid transform (hsm_merge_map, hsm_merge_map_box).

Pure numpy and math; shared by the CPU pins (tests/test_merge_model.py, tests/test_merge_map_abi.py) and the GPU tests
(tests/test_gpu_merge_map.py).  The reference has no such call: the operation is pinned by the rule of include/hector_mi355/capi.h,
which merge_model() restates cell by cell in numpy float32 -- one rounded operation per numpy call, so nothing is fused.

A geometry is (resolution, size_x, size_y, levels, (start_x, start_y)): hsm_create's arguments.  The pairs:
  LOCAL   src 48 x 44 with its own start coordinates into dst 70 x 52, 3 levels: dst's widths 70, 35, 17 are no multiples of 4
          (head and tail cells, the 16-byte phase changes from row to row), more than one 16-row tile, sizes that differ
  SAME    the same geometry on both sides
The transforms (tx, ty, theta): identity, whole- and half-cell translations (ties of floorf(m + 0.5f)), quarter turn, 0.3, -2.1,
one that leaves src half outside dst, one that misses dst (empty boxes).

On the GPU the maps are built by the product's own updates from hector_slam_amd.synth scans (build_scans); the model tests,
which have no device, take synthetic_planes() instead.
"""
import math

import numpy as np

F = np.float32
RES = 0.1
LEVELS = 3
DST_GEOM = (RES, 70, 52, LEVELS, (0.5, 0.5))
SRC_GEOM = (RES, 48, 44, LEVELS, (0.4, 0.55))
PAIRS = {"local": (DST_GEOM, SRC_GEOM), "same": (DST_GEOM, DST_GEOM)}

TRANSFORMS = [
    ("identity", (0.0, 0.0, 0.0)),
    ("whole_cells", (0.8, -0.4, 0.0)),          # SAME: 8 and -4 cells of level 0, 2 and -1 of level 2
    ("half_cells", (0.25, 0.15, 0.0)),           # SAME: 2.5 and 1.5 cells of level 0, as near as fp32 has them: ties
    ("quarter_turn", (0.3, -0.2, math.pi / 2)),
    ("theta_0.3", (-0.45, 0.33, 0.3)),
    ("theta_-2.1", (0.6, 0.5, -2.1)),
    ("half_outside", (3.2, -1.1, 0.3)),
    ("misses", (40.0, 25.0, 0.3)),
]
CASES = [(pair, name, F(t)) for pair in PAIRS for name, t in TRANSFORMS]
CASE_IDS = ["%s-%s" % (pair, name) for pair, name, _ in CASES]
EMPTY = (0, 0, -1, -1)


# ---- geometry -------------------------------------------------------------------------------------------------------------------------
def level_size(geom, level):
    return geom[1] >> level, geom[2] >> level


def level_scale(geom, level):
    """1 / cell length as hsm_level_info reports it: hsm_create doubles the fp32 resolution per level and inverts it in fp32"""
    cell = F(geom[0])
    for _ in range(level):
        cell = F(cell * F(2.0))
    return F(F(1.0) / cell)


def offsets(geom):
    """hsm_create's offsets in fp32: (resolution * size) * start per axis"""
    res, sx, sy, _, start = geom
    return (F(F(F(res) * F(sx)) * F(start[0])), F(F(F(res) * F(sy)) * F(start[1])))


def affine(geom_dst, geom_src, level, t):
    """(c, s, bx, by) in double: src map coordinates of dst's cell (x, y) are (c x + s y + bx, -s x + c y + by).  math.cos and
    math.sin: the C library's doubles, as the host side of the entry uses them"""
    tx, ty, th = (float(F(v)) for v in t)
    c, s = math.cos(th), math.sin(th)
    od, os_ = offsets(geom_dst), offsets(geom_src)
    scale = float(level_scale(geom_dst, level))
    ux, uy = -float(od[0]) - tx, -float(od[1]) - ty
    bx = scale * ((c * ux + s * uy) + float(os_[0]))
    by = scale * ((-s * ux + c * uy) + float(os_[1]))
    return c, s, bx, by


def _grown_bounds(px, py, sx, sy):
    x0, x1 = max(math.floor(min(px)) - 1.0, 0.0), min(math.ceil(max(px)) + 1.0, float(sx - 1))
    y0, y1 = max(math.floor(min(py)) - 1.0, 0.0), min(math.ceil(max(py)) + 1.0, float(sy - 1))
    if not (x0 <= x1 and y0 <= y1):
        return EMPTY
    return int(x0), int(y0), int(x1), int(y1)


def merge_box(geom_dst, geom_src, level, t):
    """the dst cells a merge visits on `level`: the corners of src's level rectangle through the inverse affine, their bounding
    box from floor to ceil, grown by one cell, clamped; EMPTY where it misses the level"""
    c, s, bx, by = affine(geom_dst, geom_src, level, t)
    ssx, ssy = level_size(geom_src, level)
    px, py = [], []
    for k in range(4):
        qx = ((ssx - 0.5) if k & 1 else -0.5) - bx
        qy = ((ssy - 0.5) if k & 2 else -0.5) - by
        px.append(c * qx - s * qy)
        py.append(s * qx + c * qy)
    return _grown_bounds(px, py, *level_size(geom_dst, level))


def merge_src_box(geom_dst, geom_src, level, t):
    """the src cells that the cells of merge_box map back to (what the staged route copies): the same construction the other way"""
    box = merge_box(geom_dst, geom_src, level, t)
    if box[2] < box[0]:
        return EMPTY
    c, s, bx, by = affine(geom_dst, geom_src, level, t)
    px, py = [], []
    for k in range(4):
        x = (box[2] + 0.5) if k & 1 else (box[0] - 0.5)
        y = (box[3] + 0.5) if k & 2 else (box[1] - 0.5)
        px.append((c * x + s * y) + bx)
        py.append((-s * x + c * y) + by)
    return _grown_bounds(px, py, *level_size(geom_src, level))


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def sampled(src_logodds, geometry_dst, geometry_src, level, src_in_dst, box):
    """steps 1-3 for the dst cells of `box` (not empty) -> (v, ix, iy, inside): the sampled log-odds, 0 outside src and for a NaN
    or an infinity, and the src cell each dst cell reads (valid where inside)"""
    src = np.asarray(src_logodds, F)
    c, s, bx, by = (F(v) for v in affine(geometry_dst, geometry_src, level, src_in_dst))
    x0, y0, x1, y1 = box
    with np.errstate(over="ignore", invalid="ignore"):
        x = np.arange(x0, x1 + 1, dtype=F)[None, :]
        y = np.arange(y0, y1 + 1, dtype=F)[:, None]
        mx = ((c * x).astype(F) + (s * y).astype(F)).astype(F) + bx
        my = ((F(-s) * x).astype(F) + (c * y).astype(F)).astype(F) + by
        assert mx.dtype == F and my.dtype == F
        rx, ry = np.floor(mx + F(0.5)), np.floor(my + F(0.5))
    ssy, ssx = src.shape
    inside = (rx >= 0) & (rx < ssx) & (ry >= 0) & (ry < ssy)
    ix, iy = np.where(inside, rx, 0).astype(np.int64), np.where(inside, ry, 0).astype(np.int64)
    v = np.where(inside, src[iy, ix], F(0.0)).astype(F)
    v = np.where(np.isfinite(v), v, F(0.0)).astype(F)
    return v, ix, iy, inside


def combine(old, v):
    """step 4: what the sampled v makes of dst's log-odds `old`"""
    with np.errstate(over="ignore", invalid="ignore"):
        both = (old + v).astype(F)
    up = np.where(old < F(50.0), np.fmin(both, F(50.0)), old)
    return np.where(v < 0, both, np.where(v > 0, up, old)).astype(F)


def merge_model(dst_logodds, src_logodds, geometry_dst, geometry_src, level, src_in_dst, visit=None):
    """-> (dst's new log-odds [sy, sx] float32, box): steps 1-4 of the cell rule over the box, in numpy float32.
    visit: the cells to visit instead of the box (the test that the box misses no cell visits the whole level)"""
    d = np.array(dst_logodds, F, copy=True)
    box = merge_box(geometry_dst, geometry_src, level, src_in_dst)
    x0, y0, x1, y1 = box if visit is None else visit
    if x1 < x0:
        return d, box
    v, _, _, _ = sampled(src_logodds, geometry_dst, geometry_src, level, src_in_dst, (x0, y0, x1, y1))
    d[y0:y1 + 1, x0:x1 + 1] = combine(d[y0:y1 + 1, x0:x1 + 1], v)
    return d, box


def merge_pyramid(dst_planes, src_planes, geometry_dst, geometry_src, src_in_dst):
    """[(log-odds, box)] per level"""
    return [merge_model(dst_planes[lvl], src_planes[lvl], geometry_dst, geometry_src, lvl, src_in_dst)
            for lvl in range(geometry_dst[3])]


def synthetic_planes(geom, seed):
    """log-odds per level as maps hold them: mostly unknown (0), free space, walls, saturated cells either side of 50 and a -0.0"""
    rng = np.random.default_rng(seed)
    out = []
    for lvl in range(geom[3]):
        sx, sy = level_size(geom, lvl)
        lo = np.zeros((sy, sx), F)
        free = rng.random((sy, sx)) < 0.45
        lo[free] = (F(-0.4054651) * rng.integers(1, 9, (sy, sx)).astype(F))[free]
        occ = rng.random((sy, sx)) < 0.12
        lo[occ] = (F(2.1972246) * rng.integers(1, 6, (sy, sx)).astype(F))[occ]
        lo[rng.random((sy, sx)) < 0.02] = F(49.5)
        lo[rng.random((sy, sx)) < 0.02] = F(50.5)
        lo[rng.random((sy, sx)) < 0.01] = F(-60.0)
        lo[0, 0] = F(-0.0)
        lo[sy - 1, sx - 1] = F(3.0)   # the far corner cell is known on every level
        out.append(lo)
    return out


# ---- the scans the GPU tests build their maps from ----------------------------------------------------------------------------------
def build_scans(seed, n_scans=6, n_beams=181):
    """[(world pose float32 [3], end points float32 [n, 2] in level-0 cells)]: a 4 m x 3 m room seen from a short arc round the
    world origin, so that both maps of a pair hold walls and free space"""
    from hector_slam_amd import synth
    world = synth.World.make(4.0, 3.0, n_boxes=3, seed=seed, box_min=2.0, box_max=5.0, keep_clear=0.2)
    rng = np.random.default_rng(seed + 1)
    scale = float(F(1.0) / F(RES))
    out = []
    for k in range(n_scans):
        a = 2.0 * math.pi * k / n_scans
        pose = np.array([0.5 * math.cos(a), 0.4 * math.sin(a), a + 0.5], F)
        out.append((pose, synth.make_scan(world, pose, n_beams, scale, rng, range_max=30.0)))
    return out
