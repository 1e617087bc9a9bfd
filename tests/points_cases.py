"""The rule of hsm_occupied_points* (include/hector_mi355/capi.h) restated in numpy, and the planes the tests extract from.

Pure numpy; shared by the CPU pins (tests/test_points_model.py) and the GPU tests (tests/test_gpu_occupied_points.py,
tests/test_gpu_align_map.py).  A cell of the clamped box is occupied when its log-odds is > 0 (NaN and +-0 are not); occupied
cells are ranked in row-major order of the box; rank r is kept when r % every == 0; kept cell j < max_points is written as the
level's world-from-map transform of (x, y), t0 + (l00 * x + l01 * y) with one rounding per numpy call, times the scale to the
map.  A geometry is merge_cases': (resolution, size_x, size_y, levels, (start_x, start_y)).
"""
import numpy as np

import merge_cases as mc

F = np.float32
EMPTY = (0, 0, -1, -1)
BIG_GEOM = (0.05, 300, 210, 1, (0.4, 0.6))   # 63 000 cells: widths and heights that are no multiple of 4, 64 or the tile


def clamp_box(bbox, sx, sy):
    """the inclusive box (None: the whole level) clamped to the level; EMPTY where nothing is left"""
    if bbox is None:
        return 0, 0, sx - 1, sy - 1
    x0, y0, x1, y1 = (int(v) for v in bbox)
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, sx - 1), min(y1, sy - 1)
    return EMPTY if x1 < x0 or y1 < y0 else (x0, y0, x1, y1)


def box_cells(box):
    return max(box[2] - box[0] + 1, 0) * max(box[3] - box[1] + 1, 0)


def world_from_map(geom, level):
    """(l00, l10, l01, l11, t0, t1) float32 of `level`: hsm_create's transforms, operation for operation (the map-from-world
    scaling and offsets, inverted by cofactors)"""
    s = mc.level_scale(geom, level)
    off = mc.offsets(geom)
    m00, m10, m01, m11, mt0, mt1 = s, F(0.0), F(0.0), s, F(s * off[0]), F(s * off[1])
    det = F(F(m00 * m11) - F(m10 * m01))
    inv = F(F(1.0) / det)
    l00, l10, l01, l11 = F(m11 * inv), F(F(-m10) * inv), F(F(-m01) * inv), F(m00 * inv)
    t0 = F(F(F(-l00) * mt0) + F(F(-l01) * mt1))
    t1 = F(F(F(-l10) * mt0) + F(F(-l11) * mt1))
    return l00, l10, l01, l11, t0, t1


def scale_to_map(geom):
    return F(F(1.0) / F(geom[0]))


def cell_points(cells_xy, affine, scale):
    """float32 [n, 2]: the points of cells [n, 2] (x, y)"""
    l00, l10, l01, l11, t0, t1 = (F(v) for v in affine)
    x, y = cells_xy[:, 0].astype(F), cells_xy[:, 1].astype(F)
    wx = (t0 + ((l00 * x).astype(F) + (l01 * y).astype(F)).astype(F)).astype(F)
    wy = (t1 + ((l10 * x).astype(F) + (l11 * y).astype(F)).astype(F)).astype(F)
    out = np.stack([(wx * F(scale)).astype(F), (wy * F(scale)).astype(F)], axis=1)
    assert out.dtype == F
    return out


def kept_cells(logodds, bbox, every):
    """int64 [kept, 2]: (x, y) of the kept cells of the box, in rank order"""
    lo = np.asarray(logodds, F)
    sy, sx = lo.shape
    x0, y0, x1, y1 = clamp_box(bbox, sx, sy)
    if x1 < x0:
        return np.zeros((0, 2), np.int64)
    with np.errstate(invalid="ignore"):
        ys, xs = np.nonzero(lo[y0:y1 + 1, x0:x1 + 1] > F(0.0))   # row-major: y outer, x inner
    return np.stack([xs + x0, ys + y0], axis=1)[::every].astype(np.int64)


def occupied_points_model(logodds, bbox, every, max_points, affine, scale):
    """-> (points float32 [written, 2], (written, kept))"""
    cells = kept_cells(logodds, bbox, every)
    kept = len(cells)
    written = min(kept, max_points)
    return cell_points(cells[:written], affine, scale), (written, kept)


def brute_force(logodds, bbox, every, max_points):
    """the rule as a double loop -> ([(x, y)] written, (written, kept))"""
    lo = np.asarray(logodds, F)
    sy, sx = lo.shape
    if bbox is None:
        bbox = (0, 0, sx - 1, sy - 1)
    out, rank, kept = [], 0, 0
    for y in range(max(bbox[1], 0), min(bbox[3], sy - 1) + 1):
        for x in range(max(bbox[0], 0), min(bbox[2], sx - 1) + 1):
            v = float(lo[y, x])
            if v > 0.0:   # False for NaN, +0 and -0
                if rank % every == 0:
                    if kept < max_points:
                        out.append((x, y))
                    kept += 1
                rank += 1
    return out, (len(out), kept)


def random_plane(sx, sy, seed):
    """log-odds as no map holds them, so that every branch of the test is met: about 15 % positive, free cells, NaN, +0, -0,
    infinities of either sign, and a denormal either side of zero"""
    rng = np.random.default_rng(seed)
    lo = np.zeros((sy, sx), F)
    u = rng.random((sy, sx))
    lo[u < 0.15] = (F(0.8472979) * rng.integers(1, 9, (sy, sx)).astype(F))[u < 0.15]
    free = (u >= 0.15) & (u < 0.55)
    lo[free] = (F(-0.4054651) * rng.integers(1, 9, (sy, sx)).astype(F))[free]
    lo[(u >= 0.55) & (u < 0.58)] = F(np.nan)
    lo[(u >= 0.58) & (u < 0.62)] = F(-0.0)
    lo[(u >= 0.62) & (u < 0.63)] = F(np.inf)
    lo[(u >= 0.63) & (u < 0.64)] = F(-np.inf)
    lo[(u >= 0.64) & (u < 0.645)] = F(1e-45)
    lo[(u >= 0.645) & (u < 0.65)] = F(-1e-45)
    return lo


# the boxes of the GPU test on the 300 x 210 plane: (name, box)
BOXES = [
    ("single_cell", (17, 23, 17, 23)),
    ("single_row", (0, 101, 299, 101)),
    ("part_of_a_row", (31, 7, 95, 7)),
    ("single_column", (299, 0, 299, 209)),
    ("inner", (13, 9, 270, 190)),
    ("over_two_edges", (-5, -3, 40, 21)),
    ("over_the_far_edges", (250, 180, 400, 300)),
    ("misses", (400, 0, 500, 10)),
    ("misses_below", (0, -9, 299, -1)),
    ("empty", EMPTY),
]
