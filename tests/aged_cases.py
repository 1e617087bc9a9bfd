"""Inputs for the AGED-map tests: maps whose log-odds sit where every long-lived map ends up -- free space far below -87
(getGridProbability subnormal or +0), walls at the 50.0 clamp (probability exactly 1.0f) -- and Gauss-Newton steps whose
Hessian is neither regular nor all zero: one diagonal entry exactly 0, every entry +0 by underflow, a determinant that
underflows, a rotation step beyond the +-0.2 clamp, a final angle normalize_angle has to wrap, a nearly singular H whose step
throws the pose off the map.

Pure numpy; shared by the CPU pin (tests/test_aged_reference.py) and the GPU tests (tests/test_gpu_aged_maps.py).  Everything
comes from fixed seeds; the searches that picked the solve cases are find() below (the CPU pin re-runs them and
asserts that the committed picks are what they return).

Geometry: the two smallest shapes of border_cases.GEOMETRIES with partial quad tiles and a second level, at its RES and START.
Start poses are multiples of 1/8 cell on level 0, so world -> map -> world is exact and a skipped step returns the start pose
bit for bit.
"""
import numpy as np

import border_cases as bc
from support import upload_planes

RES, START = bc.RES, bc.START
GEOMETRIES = [bc.GEOMETRIES[0], bc.GEOMETRIES[1]]  # (64, 64, 2), (90, 24, 2)
FAMILIES = ("wall_x", "wall_y", "deep_free", "saturated", "mixed", "tiny")
DEFINED = FAMILIES[:-1]    # `tiny` is the family on which the reference has no defined result
MAP_SEED = 8800
SCAN_SEED = 8900
SCAN_SIZES = tuple(sorted({1, 2, 3, 63, 64, 65, 300} | set(bc.LIST_SIZES)))
POSE_THETAS = (0.1, 2.2, 1.5, 0.7)   # the four start poses of a geometry; positive: normalize_angle returns them bit for bit
WALL_LO, FREE_LO = 50.0, -95.0
_F = np.float32
_cache = {}
gid, dims = bc.gid, bc.dims


# ---- the value families: (geom, level, seed) -> a log-odds plane [sy, sx] ---------------------------------------------------------
def wall_at(size0, lvl=0):
    """first of the three wall columns / rows of an axis of size0 level-0 cells: 5/8 of the way, even on level 0 so that level
    1's wall begins at exactly half the coordinate"""
    return ((5 * size0) // 8 // 2 * 2) >> lvl


def _rng(family, geom, lvl, seed):
    return np.random.default_rng(MAP_SEED + 1000 * FAMILIES.index(family) + 100 * seed + 10 * lvl + geom[0])


def plane(family, geom, lvl, seed=0):
    sx, sy = dims(geom, lvl)
    rng = _rng(family, geom, lvl, seed)
    if family in ("wall_x", "wall_y"):
        lo = np.full((sy, sx), FREE_LO, _F)
        if family == "wall_x":
            lo[:, wall_at(geom[0], lvl):wall_at(geom[0], lvl) + 3] = WALL_LO
        else:
            lo[wall_at(geom[1], lvl):wall_at(geom[1], lvl) + 3, :] = WALL_LO
        return lo
    if family == "deep_free":     # probabilities subnormal or +0
        return rng.uniform(-103.5, -86.0, (sy, sx)).astype(_F)
    if family == "saturated":     # probabilities exactly 1.0f, 1 - ulp, 1 - 2 ulp or subnormal
        return rng.choice(np.array([WALL_LO, FREE_LO, 17.0, 16.0], _F), (sy, sx), p=[0.3, 0.4, 0.15, 0.15]).astype(_F)
    if family == "mixed":         # regular H whose per-beam terms span about 60 binades
        lo = rng.choice(np.array([-95.0, -30.0, 0.0, 17.0, 50.0], _F), (sy, sx)).astype(_F)
        young = rng.random((sy, sx)) < 1.0 / 3.0
        return np.where(young, rng.uniform(-2.5, 2.5, (sy, sx)), lo).astype(_F)
    if family == "tiny":          # H ~ 1e-34: the determinant underflows, the solve goes non-finite
        return rng.uniform(-50.0, -40.0, (sy, sx)).astype(_F)
    raise KeyError(family)


def planes(family, geom, seed=0):
    key = ("planes", family, geom, seed)
    if key not in _cache:
        _cache[key] = [(plane(family, geom, lvl, seed), np.zeros(dims(geom, lvl)[::-1], np.int32)) for lvl in range(geom[2])]
    return _cache[key]


def upload(m, family, geom, seed=0):
    """the family's planes into a checker (pyoracle.Oracle) or a device context (capi.MapRepMultiMap)"""
    return upload_planes(m, planes(family, geom, seed))


def prob_plane(pyoracle, family, geom, lvl, kind="ho"):
    """the level's probability plane (getGridProbability of the log-odds, host libm): what gn_f64.relaxed_factors samples"""
    lo = planes(family, geom)[lvl][0]
    return pyoracle.libm_expf(lo.reshape(-1), kind)[1].reshape(lo.shape)


def checker(pyoracle, kind, family, geom):
    key = ("oracle", kind, family, geom)
    if key not in _cache:
        _cache[key] = upload(pyoracle.Oracle(kind, RES, geom[0], geom[1], geom[2], START), family, geom)
    return _cache[key]


# ---- start poses and scans ----------------------------------------------------------------------------------------------------
def map_pose0(geom, k, theta=None):
    """level-0 map-frame start pose k (0 .. 3): multiples of 1/8 cell a little off the map's centre"""
    th = POSE_THETAS[k] if theta is None else theta
    return np.array([geom[0] / 2 - 1.75 + 0.625 * k, geom[1] / 2 - 0.25 + 0.375 * k, th], _F)


def map_pose(geom, lvl, k, theta=None):
    p = map_pose0(geom, k, theta)
    p[:2] *= _F(1.0 / 2 ** lvl)
    return p


def world_pose(geom, k, theta=None):
    p = map_pose0(geom, k, theta)
    return np.array([(p[0] - _F(geom[0] * 0.5)) * _F(RES), (p[1] - _F(geom[1] * 0.5)) * _F(RES), p[2]], _F)


def reach(geom):
    """half-width in level-0 cells of the square the end points are drawn from: beyond the short side of the 90 x 24 map, so
    part of every scan reads the zero texel"""
    return 0.3 * max(geom[0], geom[1])


def scan(geom, n, seed=0):
    """n level-0 end points, uniform in +-reach cells; the first three within +-3 cells (the 1, 2 and 3-beam scans stay on the map)"""
    rng = np.random.default_rng(SCAN_SEED + 131 * seed + geom[0])
    pts = rng.uniform(-reach(geom), reach(geom), (max(n, 3), 2))
    pts[:3] = rng.uniform(-3.0, 3.0, (3, 2))
    return np.ascontiguousarray(pts[:n].astype(_F))


def level_scan(geom, lvl, n, seed=0):
    return scan(geom, n, seed) * _F(1.0 / 2 ** lvl)  # exact


def tile(pts, n_min):
    """the short list repeated until it has at least n_min beams: repeats keep H's zero / non-zero pattern"""
    reps = -(-n_min // pts.shape[0])
    return np.ascontiguousarray(np.tile(pts, (reps, 1)))


def aimed(family, geom, k):
    """three level-0 end points that pose k's transform takes to the near edge of the wall (half and a quarter of a cell in
    front of it) and into its far edge: a one-beam scan already has the non-zero diagonal entry"""
    pm = map_pose0(geom, k)
    ax = 0 if family == "wall_x" else 1
    c = np.repeat(pm[None, :2], 3, 0).astype(np.float64)
    c[:, ax] = wall_at(geom[ax]) + np.array([-0.5, -0.25, 2.5])
    c[:, 1 - ax] += np.array([0.3, -1.2, 0.7])
    return bc.end_points(c.astype(_F), pm)


def family_scan(family, geom, k, n, seed):
    """the n-beam level-0 scan of a (pose k, seed) pair; on the wall families its first three beams are aimed at the wall"""
    pts = scan(geom, n, seed)
    if family in ("wall_x", "wall_y"):
        pts[:min(n, 3)] = aimed(family, geom, k)[:min(n, 3)]
    return pts


def pairs(geom):
    """the (pose index, scan length, scan seed) pairs of the one-evaluation and matcher tests: every scan length once, from
    63 beams on from a second pose and seed as well"""
    out = [(k % 4, n, k) for k, n in enumerate(SCAN_SIZES)]
    return out + [((k + 2) % 4, n, 20 + k) for k, n in enumerate(SCAN_SIZES) if n >= 63]


# ---- the reference's products in numpy fp32, every intermediate kept -------------------------------------------------------------
def beam_terms(pyoracle, family, geom, lvl, pose_map, pts, kind="ho"):
    """OccGridMapUtil.h:64-104 and :287-347 per beam in numpy fp32 -> (fac [n, 5] = M, gx, gy, rotDeriv, funVal; prods [n, 12] =
    the nine H products in row-major order and the three dTr products; blend [n, 4] = the four products of the bilinear blend)"""
    f = _F
    lo = planes(family, geom)[lvl][0]
    sy, sx = lo.shape
    prob = pyoracle.libm_expf(lo.reshape(-1), kind)[1]
    pm = np.asarray(pose_map, f)
    s, c = (v[0] for v in pyoracle.libm_sincosf(pm[2:3], kind))
    co = bc.transform(pm, pts, (s, c))
    n = pts.shape[0]
    fac, blend = np.zeros((n, 5), f), np.zeros((n, 4), f)
    with np.errstate(under="ignore"):
        for k in range(n):
            x, y = co[k]
            if not (x < f(0) or x > f(sx - 2) or y < f(0) or y > f(sy - 2)):
                ix, iy = int(x), int(y)
                fx, fy = f(x - f(ix)), f(y - f(iy))
                i = iy * sx + ix
                i0, i1, i2, i3 = prob[i], prob[i + 1], prob[i + sx], prob[i + sx + 1]
                xi, yi = f(f(1) - fx), f(f(1) - fy)
                blend[k] = (f(i0 * xi), f(i1 * fx), f(i2 * xi), f(i3 * fx))
                fac[k, 0] = f(f(f(blend[k, 0] + blend[k, 1]) * yi) + f(f(blend[k, 2] + blend[k, 3]) * fy))
                fac[k, 1] = -f(f(f(i0 - i1) * xi) + f(f(i2 - i3) * fx))
                fac[k, 2] = -f(f(f(i0 - i2) * yi) + f(f(i1 - i3) * fy))
        px, py = pts[:, 0], pts[:, 1]
        fac[:, 3] = ((-s * px - c * py) * fac[:, 1] + (c * px - s * py) * fac[:, 2]).astype(f)
        fac[:, 4] = f(1) - fac[:, 0]
        g = fac[:, 1:4]
        prods = np.concatenate([(g[:, r] * g[:, cc]).astype(f)[:, None] for r, cc in
                                ((0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2))]
                               + [(g[:, r] * fac[:, 4]).astype(f)[:, None] for r in range(3)], 1)
    return fac, prods, blend


def n_subnormal(*arrays):
    """how many values are fp32 subnormals (non-zero, exponent field 0)"""
    n = 0
    for a in arrays:
        b = np.ascontiguousarray(a, _F).view(np.uint32) & np.uint32(0x7fffffff)
        n += int(((b != 0) & (b < 0x00800000)).sum())
    return n


# ---- the Gauss-Newton solve in numpy fp32, and a replay of the reference's iteration with it ---------------------------------------
def gn_step(H, dTr):
    """ScanMatcher.h:194-221 on one (H [3, 3], dTr [3]) in numpy fp32, Eigen's cofactor inverse and coefficient product in the
    order the kernels and both checkers use -> (step [3] after the clamp or None where the zero-diagonal test skips it,
    unclamped rotation step, det)"""
    f = _F
    H = np.asarray(H, f).reshape(3, 3)
    b = np.asarray(dTr, f)
    if not (H[0, 0] != 0 and H[1, 1] != 0):
        return None, f(0), f(0)
    with np.errstate(all="ignore"):
        def cof(i, j):
            i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            return f(f(H[i1, j1] * H[i2, j2]) - f(H[i1, j2] * H[i2, j1]))
        c00, c10, c20 = cof(0, 0), cof(1, 0), cof(2, 0)
        det = f(f(c00 * H[0, 0]) + f(f(c10 * H[1, 0]) + f(c20 * H[2, 0])))
        invdet = f(f(1) / det)
        inv = np.array([[f(cof(c, r) * invdet) for c in range(3)] for r in range(3)], f)  # inverse(r, c) = cofactor(c, r) / det
        s = np.array([f(f(inv[r, 0] * b[0]) + f(f(inv[r, 1] * b[1]) + f(inv[r, 2] * b[2]))) for r in range(3)], f)
    raw = s[2]
    if s[2] > f(0.2):
        s[2] = f(0.2)
    elif s[2] < f(-0.2):
        s[2] = f(-0.2)
    return s, raw, det


def replay(o, lvl, begin_world, pts_level, max_iter):
    """ScanMatcher::matchData (ScanMatcher.h:54-190) with the checker's hessian_derivs per step and gn_step above -> (final
    world pose, H of the last step column major [9], records); a record = (estimate in front of the step, H, dTr, step or None,
    unclamped rotation step, det).  test_aged_reference.py asserts that this equals the checker's own match_level bit for bit"""
    est = o.map_coords_pose(lvl, begin_world)
    recs = []
    H = np.zeros((3, 3), _F)
    for _ in range(max_iter + 1):
        H, d = o.hessian_derivs(lvl, est, pts_level)
        s, raw, det = gn_step(H, d)
        recs.append((est.copy(), H, d, s, raw, det))
        if s is not None:
            with np.errstate(all="ignore"):
                est = (est + s).astype(_F)
    est[2] = o.normalize_angle(est[2])
    return o.world_coords_pose(lvl, est), np.ascontiguousarray(H.T).reshape(9), recs


def classify(o, geom, lvl, begin_world, pts_level, max_iter):
    """what the solve of one case goes through -> dict of counts; 'undefined': the checker `o` (the restatement) read the map
    with a NaN coordinate, the reference has no result"""
    u0 = o.undefined_reads()
    pose, _, recs = replay(o, lvl, begin_world, pts_level, max_iter)
    sx, sy = dims(geom, lvl)
    last = recs[-1][0] if recs[-1][3] is None else (recs[-1][0] + recs[-1][3])
    big = [r for r in recs if r[3] is not None and np.isfinite(r[3]).all() and np.abs(r[3][:2]).max() > 1000]
    with np.errstate(invalid="ignore"):
        off = bool(np.isfinite(last).all() and not (-reach(geom) <= last[0] <= sx + reach(geom) and -reach(geom) <= last[1] <= sy + reach(geom)))
    return {"undefined": o.undefined_reads() > u0, "finite": bool(np.isfinite(pose).all()),
            "clamp+": sum(1 for r in recs if r[3] is not None and r[4] > _F(0.2)),
            "clamp-": sum(1 for r in recs if r[3] is not None and r[4] < _F(-0.2)),
            "skipped": sum(1 for r in recs if r[3] is None),
            "wrap": bool(np.isfinite(last[2]) and abs(float(last[2]) - float(o.normalize_angle(last[2]))) > 1.0),
            "ill": bool(big and off and np.isfinite(pose).all() and recs[-1][3] is None and not np.asarray(recs[-1][1]).any())}


# ---- the solve cases: `mixed` and `saturated` maps ---------------------------------------------------------------------------------
START_ANGLES = (3.1415, -3.14159, 7.0, -100.0, 119.99)  # the last three: normalize_angle wraps, sincosf's middle range
SOLVE_FAMILIES = ("mixed", "saturated")
SOLVE_ITERS = 3


def short_case(geom, seed):
    """a scan of 2 .. 6 beams within +-8 cells of a start pose whose angle cycles through START_ANGLES and POSE_THETAS: few
    beams make H badly conditioned, so the rotation step leaves +-0.2 rad"""
    rng = np.random.default_rng(9100 + seed)
    n = 2 + seed % 5
    angles = START_ANGLES + POSE_THETAS
    w = world_pose(geom, seed % 4, angles[seed % len(angles)])
    return w, np.ascontiguousarray(rng.uniform(-8.0, 8.0, (n, 2)).astype(_F))


def collinear_case(geom, seed):
    """3 .. 6 beams on one ray from the sensor, a thousandth of a cell off it: H is nearly singular but its determinant does
    not vanish"""
    rng = np.random.default_rng(9500 + seed)
    n = 3 + seed % 4
    phi = rng.uniform(-np.pi, np.pi)
    r = rng.uniform(1.5, 9.0, n)
    off = rng.uniform(-1e-3, 1e-3, n)
    pts = np.stack([r * np.cos(phi) - off * np.sin(phi), r * np.sin(phi) + off * np.cos(phi)], 1)
    return world_pose(geom, seed % 4), np.ascontiguousarray(pts.astype(_F))


def angle_cases(geom):
    """regular solves from the five start angles: 300-beam scans"""
    return [(f"angle {th}", world_pose(geom, k % 4, th), scan(geom, 300, 40 + k)) for k, th in enumerate(START_ANGLES)]


def find(pyoracle, family, geom, make, want, n_want, seeds=range(400)):
    """the search loop: the first n_want seeds whose case (level 0, SOLVE_ITERS iterations) is defined in the reference and
    has classify()[want]"""
    o = checker(pyoracle, "ho", family, geom)
    out = []
    for seed in seeds:
        w, pts = make(geom, seed)
        c = classify(o, geom, 0, w, pts, SOLVE_ITERS)
        if not c["undefined"] and c["finite"] and c[want]:
            out.append(seed)
            if len(out) == n_want:
                break
    return out


# What find() returned when the cases were chosen (test_aged_reference.py re-runs the searches and asserts these lists):
# (family, sx) -> seeds of short_case whose iteration clamps a rotation step at +0.2 / at -0.2, seeds of collinear_case whose
# iteration takes a finite step of more than 1000 cells, ends off the map and sees only all-zero H from there on.  `mixed` maps
# rarely let such a step stay finite (about one seed in 600), so that search runs over ILL_SEEDS.
PICKS = {
    ("mixed", 64): {"clamp+": [2, 3, 4, 7], "clamp-": [6, 11, 12, 15], "ill": [282, 986, 1284, 1360]},
    ("mixed", 90): {"clamp+": [3, 11, 12, 17], "clamp-": [1, 2, 3, 10], "ill": [444, 876, 2276, 2478]},
    ("saturated", 64): {"clamp+": [6, 7, 13, 16], "clamp-": [0, 2, 3, 6], "ill": [8, 81, 92, 93]},
    ("saturated", 90): {"clamp+": [1, 3, 7, 8], "clamp-": [2, 5, 6, 8], "ill": [83, 89, 115, 133]},
}
N_PICK = 4
ILL_SEEDS = range(3000)


def search(pyoracle, family, geom):
    """the searches behind PICKS"""
    return {"clamp+": find(pyoracle, family, geom, short_case, "clamp+", N_PICK),
            "clamp-": find(pyoracle, family, geom, short_case, "clamp-", N_PICK),
            "ill": find(pyoracle, family, geom, collinear_case, "ill", N_PICK, ILL_SEEDS)}


def solve_cases(family, geom):
    """(name, start world pose, level-0 end points) of a solve family: the five start angles, the clamped and the
    ill-conditioned picks"""
    p = PICKS[(family, geom[0])]
    out = angle_cases(geom)
    for seed in sorted(set(p["clamp+"]) | set(p["clamp-"])):
        out.append((f"short {seed}",) + short_case(geom, seed))
    for seed in p["ill"]:
        out.append((f"collinear {seed}",) + collinear_case(geom, seed))
    return out
