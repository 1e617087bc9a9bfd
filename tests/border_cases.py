"""Inputs for the map-EDGE tests of the sampler every matcher, scorer and probe kernel shares (interpMapValueWithDerivatives,
OccGridMapUtil.h:287-347; the kernels' copy of it is beam_sample.h cell_coord / sample_fetch and the texel-cache re-gather of
gn_match_exact.h): map coordinates that land EXACTLY on 0, -0.0, a subnormal, an integer, dims - 2 and one ulp either side of it,
far outside, and beams that cross the border between two Gauss-Newton steps -- on maps whose every cell, border cells and
corners included, holds a value of its own, so that a sampler that reads the wrong border cell or lets a beam at lim + 1 ulp
in changes M and both gradients.

Pure numpy; shared by the CPU pin (tests/test_border_reference.py: restatement == reference headers == a plain numpy
restatement written in that test) and the GPU tests (tests/test_gpu_border_sampling.py).  Everything comes from fixed seeds.

Geometry: resolution 0.125 (scale_to_map = 8) and start coordinates (0.5, 0.5), so the world -> map transform is exact for
poses that are multiples of a cell: world ((8 - sx / 2) / 8, (8 - sy / 2) / 8, 0) is map pose (8, 8, 0) on level 0 and
(4, 4, 0) on level 1 (check_exact_pose asserts it).  At theta = 0 the rotation is exact (1 * px - 0 * py), so the end point
p = v - e lands on e + p: on v itself wherever v - e is representable -- every value of the list except -0.0 and the two
subnormals, which e = 8 turns into +0.0 (reached() says what a list really hits).  Those three are reached from the map-frame
poses (0, 0, 0) and (-0.0, -0.0, +-0.0) of ZERO_POSES, which only the entries that take a map-frame pose can be given.
"""
import numpy as np

from support import upload_planes

RES = 0.125
START = (0.5, 0.5)
LEVELS = 2
GEOMETRIES = [(64, 64, 2), (90, 24, 2), (24, 90, 2)]  # (sx, sy, levels); 90 % 4 != 0: partial quad tiles; a pair of transposes
EXACT_MAP_POSE = (8.0, 8.0)   # level 0; level l: / 2^l
MAP_SEED, BAND_SEED = 6101, 6102
THETAS = (0.3, -1.2, 1.5707, -1.5708, 3.1415, -3.14159, 2.2)  # near +-pi/2 and pi: the rotation swaps / flips the axes
# map-frame poses that reach -0.0 and the subnormals (e + r is -0.0 only if both are): +0 / -0 in every component
ZERO_POSES = np.array([[0.0, 0.0, 0.0], [-0.0, -0.0, 0.0], [-0.0, -0.0, -0.0], [-0.0, 0.0, -0.0], [0.0, -0.0, 0.0]], np.float32)
LIST_SIZES = (300, 560, 720, 1081, 1300, 1920)  # the 5 / 9 / 13 / 17-row texel-cache instantiations, a streamed tail, a dense scan
N_VALUES = 20
N_EXACT = N_VALUES * N_VALUES
K_CROSS = 3          # the crossing cases are followed through match_level(.., it) for it = 0 .. K_CROSS
MIN_CROSSINGS = 8    # in each direction, on level 0
_F = np.float32
_cache = {}


def gid(g):
    return "%dx%d_L%d" % g


def dims(geom, lvl):
    return geom[0] >> lvl, geom[1] >> lvl


def lims(geom, lvl):
    """(limx, limy) = dims - 2 (MapDimensionProperties.h:70-74)"""
    sx, sy = dims(geom, lvl)
    return _F(sx - 2), _F(sy - 2)


def map_planes(geom):
    """per level (log-odds [sy, sx], update index): every cell a pseudo-random log-odds of its own in [-2, 2]"""
    key = ("map", geom)
    if key not in _cache:
        rng = np.random.default_rng(MAP_SEED + geom[0])
        planes = []
        for lvl in range(geom[2]):
            sx, sy = dims(geom, lvl)
            lo = rng.uniform(-2.0, 2.0, (sy, sx)).astype(_F)
            assert np.unique(lo).size == lo.size, "two cells share a value"
            planes.append((lo, np.zeros((sy, sx), np.int32)))
        _cache[key] = planes
    return _cache[key]


def upload(m, geom):
    """the same planes into a checker (pyoracle.Oracle) or a device context (capi.MapRepMultiMap): both have upload_level"""
    return upload_planes(m, map_planes(geom))


def new_oracle(pyoracle, kind, geom):
    return upload(pyoracle.Oracle(kind, RES, geom[0], geom[1], geom[2], START), geom)


def axis_values(lim):
    """the 20 coordinates of one axis, lim = size - 2 of that axis and level"""
    lim = _F(lim)
    sub = np.array([1], np.uint32).view(_F)[0]  # the smallest positive subnormal
    v = [0.0, -0.0, sub, -sub, 1.0, lim, np.nextafter(lim, _F(np.inf)), np.nextafter(lim, _F(-np.inf)), lim + _F(1), lim + _F(2),
         -1.0, -0.5, 0.5, lim - _F(0.5), lim / _F(2), 2.0 ** 23 + 0.5, 3e9, -3e9, 1e30, -1e30]
    v = np.array(v, _F)
    assert v.size == N_VALUES and np.unique(v.view(np.uint32)).size == N_VALUES
    return v


def inside_axis(v, lim):
    """the reference's test, MapDimensionProperties.h:65-68: outside when v < 0 or v > dims - 2 (so -0.0 is inside)"""
    v = np.asarray(v, _F)
    return ~((v < _F(0)) | (v > _F(lim)))


def n_inside_exact(geom, lvl):
    """how many of the 400 exact coordinates the reference samples: worked out from the value list alone"""
    lx, ly = lims(geom, lvl)
    return int(inside_axis(axis_values(lx), lx).sum()) * int(inside_axis(axis_values(ly), ly).sum())


def exact_coords(geom, lvl):
    """the cross product of the two axes' values: 400 map coordinates of level lvl, x-major"""
    lx, ly = lims(geom, lvl)
    vx, vy = axis_values(lx), axis_values(ly)
    return np.ascontiguousarray(np.stack([np.repeat(vx, N_VALUES), np.tile(vy, N_VALUES)], 1))


def exact_map_pose(lvl, theta=0.0):
    f = _F(1.0 / 2 ** lvl)
    return np.array([EXACT_MAP_POSE[0] * f, EXACT_MAP_POSE[1] * f, theta], _F)


def exact_world_pose(geom, theta=0.0):
    """the world pose whose map pose is exact_map_pose(lvl) on every level: map = world * 8 + size / 2 on level 0"""
    return np.array([(EXACT_MAP_POSE[0] - geom[0] * 0.5) * RES, (EXACT_MAP_POSE[1] - geom[1] * 0.5) * RES, theta], _F)


def corner_world_pose(geom):
    """the world pose of map pose (0, 0, 0) on every level: from there an end point IS its map coordinate"""
    return np.array([-geom[0] * 0.5 * RES, -geom[1] * 0.5 * RES, 0.0], _F)


def check_exact_pose(o, geom):
    for lvl in range(geom[2]):
        got = o.map_coords_pose(lvl, exact_world_pose(geom))
        assert np.array_equal(got.view(np.uint32), exact_map_pose(lvl).view(np.uint32)), (geom, lvl, got)
        got = o.map_coords_pose(lvl, corner_world_pose(geom))
        assert np.array_equal(got.view(np.uint32), np.zeros(3, _F).view(np.uint32)), (geom, lvl, got)


def end_points(coords, pose_map):
    """robot-frame end points (units of the pose's level) that the transform of `pose_map` takes to `coords`: exactly v - e at
    theta = 0 (see reached()), the float64 inverse rotation rounded to fp32 otherwise"""
    c = np.asarray(coords, _F)
    e = np.asarray(pose_map, _F)
    with np.errstate(over="ignore"):
        d = np.stack([c[:, 0] - e[0], c[:, 1] - e[1]], 1).astype(_F)
    if e[2] == 0:
        return np.ascontiguousarray(d)
    th = float(e[2])
    cs, sn = np.cos(-th), np.sin(-th)
    d64 = np.stack([c[:, 0].astype(np.float64) - float(e[0]), c[:, 1].astype(np.float64) - float(e[1])], 1)
    return np.ascontiguousarray(np.stack([cs * d64[:, 0] - sn * d64[:, 1], sn * d64[:, 0] + cs * d64[:, 1]], 1).astype(_F))


def transform(pose_map, pts, sincos=None):
    """the map coordinates of the beams, the fp32 expression of OccGridMapUtil.h:80 and of the kernels: t + (c * x + (-s) * y).
    sincos: (sin, cos) of the pose's angle from the host libm (pyoracle.libm_sincosf); None: theta must be +-0"""
    pm = np.asarray(pose_map, _F)
    if sincos is None:
        assert pm[2] == 0
        s, c = _F(pm[2]), _F(1.0)  # sinf(+-0) = +-0
    else:
        s, c = _F(sincos[0]), _F(sincos[1])
    x, y = pts[:, 0], pts[:, 1]
    with np.errstate(over="ignore", invalid="ignore"):
        tx = pm[0] + (c * x + (-s) * y)
        ty = pm[1] + (s * x + c * y)
    return np.stack([tx, ty], 1).astype(_F)


def reached(coords, pose_map):
    """bool per point: the theta = 0 transform of end_points(coords, pose) gives back the coordinate bit for bit"""
    got = transform(pose_map, end_points(coords, pose_map))
    return (got.view(np.uint32) == np.asarray(coords, _F).view(np.uint32)).all(1)


def band_coords(geom, lvl, n, seed=0):
    """n map coordinates within +-2 cells of the four borders and the four corners, the eight regions in turn"""
    rng = np.random.default_rng(BAND_SEED + 97 * seed + 7 * lvl + geom[0])
    lx, ly = (float(v) for v in lims(geom, lvl))
    k = np.arange(n) % 8
    lo_x, hi_x = rng.uniform(-2, 2, n), lx + rng.uniform(-2, 2, n)
    lo_y, hi_y = rng.uniform(-2, 2, n), ly + rng.uniform(-2, 2, n)
    any_x, any_y = rng.uniform(-2, lx + 2, n), rng.uniform(-2, ly + 2, n)
    x = np.choose(k, [lo_x, hi_x, any_x, any_x, lo_x, hi_x, lo_x, hi_x])
    y = np.choose(k, [any_y, any_y, lo_y, hi_y, lo_y, lo_y, hi_y, hi_y])
    return np.stack([x, y], 1).astype(_F)


def level_list(geom, lvl, n, pose_map=None, seed=0):
    """n end points in units of level lvl for `pose_map` (default: the exact pose of that level): the 400 exact coordinates first
    (n < 400: an evenly spaced n of them), then band points"""
    pm = exact_map_pose(lvl) if pose_map is None else np.asarray(pose_map, _F)
    ex = exact_coords(geom, lvl)
    if n < N_EXACT:
        ex = ex[np.linspace(0, N_EXACT - 1, n).astype(int)]
    parts = [end_points(ex, pm)]
    if n > N_EXACT:
        parts.append(end_points(band_coords(geom, lvl, n - N_EXACT, seed), pm))
    return np.ascontiguousarray(np.concatenate(parts))


def pyramid_list(geom, n, theta=0.0, seed=0):
    """n level-0 end points for a whole-pyramid match from exact_world_pose: alternately a point aimed at level 0's edges and one
    aimed at level 1's (level-0 coordinates = 2 x the level-1 ones, exact; the matcher scales them back by 0.5, exact)"""
    a = level_list(geom, 0, (n + 1) // 2, exact_map_pose(0, theta), seed)
    b = level_list(geom, 1, n // 2, exact_map_pose(1, theta), seed + 1) * _F(2)
    out = np.empty((n, 2), _F)
    out[0::2], out[1::2] = a, b
    return out


def in_orders(pts):
    """as built: the exact points in lanes 0 .. 63 of the first (cached) rows; reversed: in the last rows (streamed ones in a list
    longer than 17 rows), and lane 0 / lane 63 hold other points"""
    return {"built": np.ascontiguousarray(pts), "reversed": np.ascontiguousarray(pts[::-1])}


def inside(geom, lvl, coords):
    lx, ly = lims(geom, lvl)
    return inside_axis(coords[:, 0], lx) & inside_axis(coords[:, 1], ly)


# ---- beams that cross the border between two Gauss-Newton steps ---------------------------------------------------------------
CROSS_SEEDS = (1, 3)      # picked on the CPU: test_border_reference.py asserts the crossing counts of both on every geometry
N_CROSS = 720


def crossing_case(geom, seed, n=N_CROSS):
    """(start world pose, n level-0 end points): a start a few tenths of a cell from the exact pose; 100 of the exact points and
    n - 100 band points for the exact pose, so most beams start within a fraction of a cell of a border"""
    rng = np.random.default_rng(7000 + seed)
    w = exact_world_pose(geom).astype(np.float64)
    w[:2] += rng.uniform(-0.45, 0.45, 2) * RES
    w[2] += rng.uniform(-0.01, 0.01)
    pm = exact_map_pose(0)
    pts = np.concatenate([end_points(band_coords(geom, 0, n - 100, seed), pm), level_list(geom, 0, 100)])
    return w.astype(_F), np.ascontiguousarray(pts)


def step_poses(o, lvl, begin_world, pts_level, k_max=K_CROSS):
    """map-frame estimates in front of GN steps 0 .. k_max + 1 of match_level, from the poses match_level(.., it) returns"""
    poses = [o.map_coords_pose(lvl, begin_world)]
    for it in range(k_max + 1):
        poses.append(o.map_coords_pose(lvl, o.match_level(lvl, begin_world, pts_level, it)[0]))
    return poses


def count_crossings(pyoracle, o, geom, lvl, begin_world, pts_level, k_max=K_CROSS):
    """-> (in -> out, out -> in, in -> out with the same truncated cell): beams whose bounds test changes between consecutive
    steps.  The third count is the texel-cache forms' hard case: the cell offset stays, the EFFECTIVE offset (zero texel) changes"""
    poses = step_poses(o, lvl, begin_world, pts_level, k_max)
    n_out = n_in = n_same = 0
    prev = None
    for pm in poses[:-1]:  # the estimates the steps are evaluated at
        s, c = (v[0] for v in pyoracle.libm_sincosf(pm[2:3], o.kind))
        co = transform(pm, pts_level, (s, c))
        ins = inside(geom, lvl, co)
        with np.errstate(invalid="ignore"):
            cell = np.trunc(np.clip(co.astype(np.float64), -1e9, 1e9))
        if prev is not None:
            out_now = prev[0] & ~ins
            n_out += int(out_now.sum())
            n_in += int((~prev[0] & ins).sum())
            n_same += int((out_now & (prev[1] == cell).all(1)).sum())
        prev = (ins, cell)
    return n_out, n_in, n_same


# ---- the guard: no case may make the reference index its grid with (int)NaN -----------------------------------------------------
def checker(pyoracle, kind, geom):
    key = ("oracle", kind, geom)
    if key not in _cache:
        _cache[key] = new_oracle(pyoracle, kind, geom)
    return _cache[key]


def run_checked(pyoracle, kind, geom, op):
    """op(checker) on the checker `kind`.  The restatement runs it first and must count no undefined read (a NaN coordinate:
    where the reference headers would crash) before the reference-compiled checker is given the same input"""
    ho = checker(pyoracle, "ho", geom)
    r = op(ho)
    assert ho.undefined_reads() == 0, (gid(geom), "the case has no reference result")
    return r if kind == "ho" else op(checker(pyoracle, kind, geom))
