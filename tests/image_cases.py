"""The rules of hsm_map_extents*, hsm_map_image* and hsm_map_tiles* (include/hector_mi355/capi.h) in numpy, each next to a plain
double-loop transcription of the reference loop it restates, and the planes, poses and tile sizes the tests run them on.

Pure numpy; shared by the CPU pins (tests/test_map_image_model.py) and the GPU tests (tests/test_gpu_map_image.py).  One cell
rule: a log-odds < 0 is free, > 0 occupied, anything else (+0, -0, NaN) unknown -- what publishMap writes as 0 / 100 / -1
(HectorMappingRos.cpp:449-468).  Image bytes: free 255, occupied 0, unknown 127.  A cell is KNOWN when it is free or occupied.
Everything is integer and comparison work: no tolerance anywhere.  A geometry is merge_cases': (resolution, size_x, size_y,
levels, (start_x, start_y))."""
import math

import numpy as np

import merge_cases as mc
import points_cases as pc

F = np.float32
EMPTY = (0, 0, -1, -1)
BIG_GEOM = pc.BIG_GEOM          # one level of 300 x 210 cells: no multiple of 4 or 64 either way
PYRAMID_GEOM = mc.DST_GEOM      # 70 x 52, 35 x 26, 17 x 13
CLAMP = F(1073741824.0)         # 2^30: where the entries clamp a map coordinate in front of the conversion to int


# ---- the cell rule ---------------------------------------------------------------------------------------------------------------
def published(logodds):
    """publishMap's grid of a plane: int8 [sy, sx]"""
    lo = np.asarray(logodds, F)
    with np.errstate(invalid="ignore"):
        return np.where(lo < 0, 0, np.where(lo > 0, 100, -1)).astype(np.int8)


def image_bytes(logodds):
    lo = np.asarray(logodds, F)
    with np.errstate(invalid="ignore"):
        return np.where(lo < 0, 255, np.where(lo > 0, 0, 127)).astype(np.uint8)


# ---- extents -----------------------------------------------------------------------------------------------------------------------
def extents_model(logodds):
    """(x0, y0, x1, y1) inclusive over the known cells, EMPTY without one"""
    ys, xs = np.nonzero(published(logodds) != -1)
    return EMPTY if ys.size == 0 else (int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()))


def extents_loop_grid_map_base(logodds):
    """GridMapBase::getMapExtends (hector_slam_lib/map/GridMapBase.h:334-383), its loops and its test `getValue() != 0.0f` on the
    log-odds themselves -> (found, xMax, yMax, xMin, yMin).  (A NaN compares unequal to 0: this loop calls it known.)"""
    lo = np.asarray(logodds, F)
    size_y, size_x = lo.shape
    lower_start, upper_start = -1, 10000
    x_max = y_max = lower_start
    x_min = y_min = upper_start
    for x in range(size_x):
        for y in range(size_y):
            if float(lo[y, x]) != 0.0:
                x_max, x_min = max(x_max, x), min(x_min, x)
                y_max, y_min = max(y_max, y), min(y_min, y)
    found = x_max != lower_start and y_max != lower_start and x_min != upper_start and y_min != upper_start
    return found, x_max, y_max, x_min, y_min


def extents_loop_map_tools(grid):
    """HectorMapTools::getMapExtends (hector_map_tools/HectorMapTools.h:241-290) on a published int8 grid
    -> (found, topLeft (x, y), bottomRight (x, y)): bottomRight is one past the last known cell"""
    height, width = grid.shape
    data = grid.reshape(-1)
    lower_start, upper_start = -1, 10000000
    x_max = y_max = lower_start
    x_min = y_min = upper_start
    for y in range(height):
        for x in range(width):
            if data[x + y * width] != -1:
                x_max, x_min = max(x_max, x), min(x_min, x)
                y_max, y_min = max(y_max, y), min(y_min, y)
    found = x_max != lower_start and y_max != lower_start and x_min != upper_start and y_min != upper_start
    return found, (x_min, y_min), (x_max + 1, y_max + 1)


# ---- the image of a cell box -------------------------------------------------------------------------------------------------------
def image_model(logodds, crop=None):
    """uint8 [hgt, w]: the clamped crop (None: the whole level), row 0 its top map row; (0, 0) where the crop misses the level"""
    lo = np.asarray(logodds, F)
    x0, y0, x1, y1 = pc.clamp_box(crop, lo.shape[1], lo.shape[0])
    if x1 < x0:
        return np.zeros((0, 0), np.uint8)
    return np.ascontiguousarray(image_bytes(lo[y0:y1 + 1, x0:x1 + 1])[::-1])


def image_loop_full(grid):
    """map_to_image_node's full image (hector_compressed_map_transport/src/map_to_image_node.cpp:98-140) of a published int8 grid"""
    size_y, size_x = grid.shape
    map_data = grid.reshape(-1)
    img = np.full(size_x * size_y, 77, np.uint8)
    size_y_rev = size_y - 1
    for y in range(size_y_rev, -1, -1):
        idx_map_y = size_x * (size_y_rev - y)
        idx_img_y = size_x * y
        for x in range(size_x):
            v = map_data[idx_map_y + x]
            if v == -1:
                img[idx_img_y + x] = 127
            elif v == 0:
                img[idx_img_y + x] = 255
            elif v == 100:
                img[idx_img_y + x] = 0
    return img.reshape(size_y, size_x)


# ---- tiles ---------------------------------------------------------------------------------------------------------------------------
def metadata(geom, level):
    """(origin_x, origin_y, resolution) float32 of `level`: the OccupancyGrid metadata the node publishes
    (HectorMappingRos.cpp:546-553): getWorldCoords(0, 0) - cell * 0.5f per axis, the cell length"""
    _, _, _, _, t0, t1 = pc.world_from_map(geom, level)
    cell = F(geom[0])
    for _ in range(level):
        cell = F(cell * F(2.0))
    half = F(cell * F(0.5))
    return F(F(t0) - half), F(F(t1) - half), cell


def _axis_lo(p, origin, inv, tile, size):
    """map_to_image_node.cpp:147-193 for one axis -> the window's first cell (its last: lo + tile - 1, as tile <= size)"""
    with np.errstate(over="ignore"):
        m = F(F(F(p) - origin) * inv)  # getC2Coords, HectorMapTools.h:89-92: fp32, subtraction then multiplication
    m = min(max(m, -CLAMP), CLAMP)     # (the entries' definition where the reference's cast is undefined)
    lo = int(math.trunc(float(m))) - tile // 2
    lo = max(lo, 0)
    hi = lo + tile
    if hi > size:
        lo -= hi - size
        hi = size
    lo = max(lo, 0)
    assert hi - lo == tile
    return lo


def tile_box(meta, pose, tile_w, tile_h, sx, sy):
    """the inclusive cell box of the tile of `pose`; EMPTY for a non-finite x or y"""
    ox, oy, res = (F(v) for v in meta)
    inv = F(F(1.0) / res)  # CoordinateTransformer::setTransforms, HectorMapTools.h:64
    if not (math.isfinite(float(pose[0])) and math.isfinite(float(pose[1]))):
        return EMPTY
    lx = _axis_lo(pose[0], ox, inv, tile_w, sx)
    ly = _axis_lo(pose[1], oy, inv, tile_h, sy)
    return lx, ly, lx + tile_w - 1, ly + tile_h - 1


def tiles_model(logodds, meta, poses, tile_w, tile_h):
    """-> (tiles uint8 [B, tile_h, tile_w], boxes int32 [B, 4])"""
    lo = np.asarray(logodds, F)
    sy, sx = lo.shape
    img = image_bytes(lo)
    p = np.asarray(poses, F).reshape(-1, 3)
    tiles = np.full((len(p), tile_h, tile_w), 127, np.uint8)
    boxes = np.zeros((len(p), 4), np.int32)
    for b in range(len(p)):
        x0, y0, x1, y1 = boxes[b] = tile_box(meta, p[b], tile_w, tile_h, sx, sy)
        if x1 >= x0:
            tiles[b] = img[y0:y1 + 1, x0:x1 + 1][::-1]
    return tiles, boxes


def tile_loop(grid, meta, pose, tile_w, tile_h):
    """map_to_image_node's tile image (map_to_image_node.cpp:143-235) of a published int8 grid, statement for statement, with the
    entries' two definitions in front: a non-finite position gives 127 throughout and the empty box, a finite map coordinate is
    clamped to +-2^30 before the cast.  -> (tile uint8 [tile_h, tile_w], box)"""
    size_y, size_x = grid.shape
    if not (math.isfinite(float(pose[0])) and math.isfinite(float(pose[1]))):
        return np.full((tile_h, tile_w), 127, np.uint8), EMPTY
    origo = (F(meta[0]), F(meta[1]))
    inv_scale = F(F(1.0) / F(meta[2]))
    with np.errstate(over="ignore"):
        rob_map = [F(F(F(pose[k]) - origo[k]) * inv_scale) for k in (0, 1)]
    rob_mapi = [int(math.trunc(float(min(max(v, -CLAMP), CLAMP)))) for v in rob_map]
    half = (tile_w // 2, tile_h // 2)
    min_c = [rob_mapi[0] - half[0], rob_mapi[1] - half[1]]
    for k in (0, 1):
        if min_c[k] < 0:
            min_c[k] = 0
    max_c = [min_c[0] + tile_w, min_c[1] + tile_h]
    for k, size in ((0, size_x), (1, size_y)):
        if max_c[k] > size:
            diff = max_c[k] - size
            min_c[k] -= diff
            max_c[k] = size
    for k in (0, 1):
        if min_c[k] < 0:
            min_c[k] = 0
    dims = (max_c[0] - min_c[0], max_c[1] - min_c[1])
    map_data = grid.reshape(-1)
    img = np.full(dims[0] * dims[1], 77, np.uint8)
    y_img = max_c[1] - 1
    for y in range(min_c[1], max_c[1]):
        idx_map_y = y_img * size_x
        y_img -= 1
        idx_img_y = (y - min_c[1]) * dims[0]
        for x in range(min_c[0], max_c[0]):
            v = map_data[idx_map_y + x]
            img[idx_img_y + (x - min_c[0])] = {0: 255, -1: 127, 100: 0}[int(v)]
    return img.reshape(dims[1], dims[0]), (min_c[0], min_c[1], max_c[0] - 1, max_c[1] - 1)


# ---- planes ------------------------------------------------------------------------------------------------------------------------
def planes():
    """name -> log-odds [210, 300] of BIG_GEOM's level"""
    _, sx, sy, _, _ = BIG_GEOM
    out = {"random_1": pc.random_plane(sx, sy, 1), "random_2": pc.random_plane(sx, sy, 2),
           "all_zero": np.zeros((sy, sx), F), "all_nan": np.full((sy, sx), np.nan, F)}
    known = pc.random_plane(sx, sy, 3)
    with np.errstate(invalid="ignore"):
        known[~((known < 0) | (known > 0))] = F(-0.4054651)
    out["all_known"] = known
    for name, (y, x) in {"cell_0_0": (0, 0), "cell_last_x": (0, sx - 1), "cell_last_y": (sy - 1, 0), "cell_last": (sy - 1, sx - 1),
                         "cell_middle": (sy // 2, sx // 2)}.items():
        lo = np.zeros((sy, sx), F)
        lo[y, x] = F(0.8472979) if (x + y) % 2 else F(-0.4054651)
        out[name] = lo
    return out


NAN_FREE = ("all_zero", "all_known", "cell_0_0", "cell_last_x", "cell_last_y", "cell_last", "cell_middle")


def pyramid_scans():
    """[(world pose, end points in level-0 cells)] that build PYRAMID_GEOM's three levels (merge_cases' room)"""
    return mc.build_scans(7)


def pyramid_planes(oracle_mod, kind="ho"):
    """the log-odds of the three levels after those updates on a CPU checker, whose updates are the product's bit for bit"""
    res, sx, sy, levels, start = PYRAMID_GEOM
    o = oracle_mod.Oracle(kind, res, sx, sy, levels, start)
    o.set_update_factor_free(0.4)
    o.set_update_factor_occupied(0.9)
    scans = pyramid_scans()
    o.build_map([p for p, _ in scans], [s for _, s in scans])
    return [np.asarray(o.download_level(lvl)[0], F).reshape(mc.level_size(PYRAMID_GEOM, lvl)[::-1]) for lvl in range(levels)]


def node_published(oracle_mod, logodds):
    """the grid the reference's node publishes for these log-odds (oracle/node_shim.cpp publishMap, as tests/test_node_rows.py
    takes it) where that checker is built; the restated rule otherwise"""
    if oracle_mod.available("node"):
        node = oracle_mod.NodeRef()
        cells, _ = node.publish_map(0.1, logodds)
        node.close()
        return cells
    return published(logodds)


# ---- poses and tile sizes -------------------------------------------------------------------------------------------------------------
def world_of(meta, mx, my):
    """a world position whose map coordinate on `meta` is about (mx, my) (cell units, corner-based as the image node's)"""
    return [float(meta[0]) + mx * float(meta[2]), float(meta[1]) + my * float(meta[2])]


def poses(meta, sx, sy):
    """float32 [n, 3]: the positions the tiles are cut around, on a level of sx x sy cells with this metadata"""
    at = lambda mx, my: world_of(meta, mx, my) + [0.3]  # noqa: E731
    out = [at(sx / 2 + 0.5, sy / 2 + 0.5),                                                         # the centre
           at(0.5, 0.5), at(sx - 0.5, 0.5), at(0.5, sy - 0.5), at(sx - 0.5, sy - 0.5),           # the corners
           at(-40.0, sy / 2), at(sx + 40.0, sy / 2), at(sx / 2, -40.0), at(sx / 2, sy + 40.0),   # outside on each side
           at(-3.0, -7.0), at(sx + 9.0, sy + 2.0), at(-5.0, sy + 5.0), at(sx + 1.0, -1.0),       # ... and diagonally
           at(32.0, 32.0), at(33.0, 31.0), at(float(sx), float(sy)), at(0.0, 0.0),               # on cell boundaries
           at(-0.5, 40.0), at(40.0, -0.25), at(-0.999, -0.001),                                   # in (-1, 0): cell 0, not -1
           at(17.3, 101.9), at(211.6, 13.2)]
    out += [[1e30, 0.0, 0.0], [0.0, -1e30, 0.0], [-1e30, 1e30, 0.0], [3e38, -3e38, 1.0],          # finite and far: the edge windows
            [np.nan, 0.0, 0.0], [0.0, np.nan, 0.0], [np.inf, 0.0, 0.0], [0.0, -np.inf, 0.0], [-np.inf, np.nan, 0.0],
            [0.0, 0.0, np.nan]]                                                                    # (theta is not read)
    return np.asarray(out, F)


def tile_sizes(sx, sy):
    """(tile_w, tile_h): the reference's window, the smallest, two odd ones, and the level itself"""
    return [(64, 64), (1, 1), (5, 3), (7, 64), (sx, sy)] if sx >= 64 and sy >= 64 else [(1, 1), (5, 3), (min(7, sx), sy), (sx, sy)]
