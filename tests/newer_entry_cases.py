"""The two newest families of entries on maps that are not square, centred 3-level pyramids: the cases.

hsm_covariance_batch_device / hsm_covariance_batch / hsm_match_cov_batch_device and hsm_merge_map / hsm_merge_map_box came after
the suite's geometry files; their own tests run on conftest.pyramid_scene and on two 3-level pairs at resolution 0.1.  Here
they get

  * covariance: four of frame_cases' frames (inexact scale and unequal translations, world origin outside the map, the far
    frame, the control) on 90 x 24 x 2 and 96 x 40 x 3, and entry_geometry_cases' three deep pyramids down to 10 x 2, 2 x 10 and
    2 x 2 cells, where limx = sx - 2 is 0 and every sigma point is off the map; per map and level the CSR case, the border case
    and the shared batches of tests/test_gpu_covariance_batch.py, on the map's own 200-beam scan;
  * merge: PAIRS below -- an inexact scale with a start outside the map, the far frame (bx, by of thousands of cells), six and
    eight levels down to 10 x 2 / 2 x 10 and 2 x 2 cells, and a strip of 2050 tiles, one tile across, that sends the kernel's
    tile loop on its second trip -- and merges between contexts of which one or both have moved (hsm_shift_map).

Pure numpy; the checker module (oracle.pyoracle) is handed in.  Shared by the CPU pin (tests/test_newer_entries_reference.py)
and the GPU tests (tests/test_gpu_newer_entries.py).  Everything comes from fixed seeds and nothing is chosen at run time: PICKS
records what had to be searched on the CPU (nothing so far).
"""
import math

import numpy as np

import entry_geometry_cases as egc
import frame_cases as fc
import merge_cases as mc
import moved_entry_cases as mec
import shift_cases as sc
from test_gpu_covariance_batch import reference   # (the module starts no device on import)

F = np.float32

# ("cov", map id, level, case) -> seed, where the level's own seed gave a case the reference does not define; searched on the
# CPU (tests/test_newer_entries_reference.py asserts that every case is defined and that this table stays short)
PICKS = {}
_cache = {}

# ---- covariance: the maps -------------------------------------------------------------------------------------------------------------
ORIGIN_OUTSIDE = fc.FRAMES[3]
assert egc.SENSITIVE_FRAME == (0.03, (0.3, 0.7)) and ORIGIN_OUTSIDE == (0.1, (-0.25, 1.5))
COV_FRAMES = (egc.SENSITIVE_FRAME, ORIGIN_OUTSIDE, fc.FAR, fc.CONTROL)
COV_GEOMETRIES = ((90, 24, 2), (96, 40, 3))
COV_MAPS = [egc.map_of(frame, geom) for geom in COV_GEOMETRIES for frame in COV_FRAMES] + [egc.map_of(None, geom) for geom in egc.DEEP]
COV_MAP_LAYOUTS = [(m, "quad") for m in COV_MAPS] + [(m, "plane") for m in COV_MAPS if m.planes_too]
COV_IDS = ["%s-%s" % (m.id, layout) for m, layout in COV_MAP_LAYOUTS]
TREE_MAPS = [m for m in COV_MAPS if m.frame in (egc.SENSITIVE_FRAME, fc.FAR) or m.geom == (333, 90, 6)]
TREE_MAP_LAYOUTS = [(m, layout) for m, layout in COV_MAP_LAYOUTS if m in TREE_MAPS]
LH_MAPS = [m for m in COV_MAPS if m.frame == egc.SENSITIVE_FRAME or m.geom == (256, 256, 8)]
CHAIN_MAPS = [egc.map_of(egc.SENSITIVE_FRAME, (96, 40, 3)), egc.map_of(None, (333, 90, 6))]

CSR_LENS = (0, 1, 63, 64, 65, 128, 129, 0, 181)   # tests/test_gpu_covariance_batch.py's, all within the 200-beam scan
SHARED_BATCHES = (1, 3, 4, 5)
BORDER_ANGLES = (0.3, -2.0, 1.2, 2.9, 0.8, 2.2, -0.7, -2.4, -3.1)
SMALL_SIDE = 4                                    # a level with a side below this takes the five poses that fit


def cov_seed(m, lvl, case):
    return PICKS.get(("cov", m.id, lvl, case), 2700 + lvl)


def scan_pose(pyoracle, m):
    """the world pose the map's scan was taken from: the deep case's first truth, the frame's pair of 200 beams"""
    if m.kind == "deep":
        return m.truth(pyoracle)[0]
    return np.asarray(fc.pair(m.checker(pyoracle, "ho"), m.frame, m.geom, egc.SCAN_LENS[-1])[0], F)


def truth_poses(pyoracle, m):
    """Map.truth(), the scan's own pose first: 17 world poses on the map"""
    return np.concatenate([scan_pose(pyoracle, m)[None], m.truth(pyoracle)]).astype(F)


def csr_case(pyoracle, m, lvl):
    """nine hypotheses of the nine scan lengths, each scan n beams spread over the whole fan of the map's 200 (one beam: the
    shortest, which ends on the map on the coarse levels too).  Even rows stand
    at the scan's own pose; odd rows half a level-0 cell and 0.02 rad (one sigma) off a truth pose -- on a frame map another pose
    of Map.truth(), inside the same room; on a deep map the scan's own, the others stand elsewhere on the loop and see other
    walls -> (poses [9, 3], scans)"""
    rng = np.random.default_rng(cov_seed(m, lvl, "csr"))
    truth, (_, pts) = truth_poses(pyoracle, m), m.scan(pyoracle)
    poses, scans = [], []
    for k, n in enumerate(CSR_LENS):
        off = rng.normal(0, [0.5 * m.resolution, 0.5 * m.resolution, 0.02])
        other = k if m.kind == "frame" and n > 1 else 0   # (the one beam needs its own pose to end on the map)
        poses.append(truth[0] if k % 2 == 0 else truth[other].astype(np.float64) + off)
        pick = np.linspace(0, len(pts) - 1, n).astype(np.int64) if n != 1 else np.array([np.argmin(np.hypot(pts[:, 0], pts[:, 1]))])
        scans.append(np.ascontiguousarray(pts[pick]))
    return np.asarray(poses, F), scans


def border_map_poses(dims):
    """map-frame poses of a level of dims = (sx, sy) cells.  A level of at least SMALL_SIDE cells both ways: one cell inside each
    limit and each corner of [0, lim], lim = size - 2 per axis (the +-1.5-cell sigma points leave, the pose does not), and one
    off the centre with an angle near -pi: test_gpu_covariance_batch.border_case's with its constants taken per axis.  A smaller
    level: the centre cell and the four positions half a cell from each limit"""
    sx, sy = dims
    limx, limy, midx, midy = float(sx - 2), float(sy - 2), sx / 2.0, sy / 2.0
    if min(sx, sy) < SMALL_SIDE:
        xy = [(midx, midy), (0.5, midy), (limx - 0.5, midy), (midx, 0.5), (midx, limy - 0.5)]
    else:
        lo, hx, hy = 1.0, limx - 1.0, limy - 1.0
        xy = [(lo, midy), (hx, midy), (midx, lo), (midx, hy), (lo, lo), (hx, lo), (lo, hy), (hx, hy),
              (midx + 0.1 * limx, midy - 0.2 * limy)]
    return np.array([(x, y, a) for (x, y), a in zip(xy, BORDER_ANGLES)], F)


def border_case(pyoracle, m, lvl):
    """border_map_poses as WORLD poses through the checker, each with the whole scan -> (poses, scans, the map poses)"""
    o = m.checker(pyoracle, "ho")
    maps = border_map_poses(m.dims(lvl))
    poses = np.stack([o.world_coords_pose(lvl, p) for p in maps]).astype(F)
    _, pts = m.scan(pyoracle)
    return poses, [pts] * len(maps), maps


def shared_case(pyoracle, m, lvl, B):
    """B hypotheses around the scan's own pose over the one scan -> (poses [B, 3], scan)"""
    rng = np.random.default_rng(cov_seed(m, lvl, "shared") + 10 * B)
    d = rng.normal(0, [0.5 * m.resolution, 0.5 * m.resolution, 0.02], (B, 3))
    return (scan_pose(pyoracle, m).astype(np.float64)[None] + d).astype(F), m.scan(pyoracle)[1]


def cov_level_case(pyoracle, m, lvl):
    """the inputs of a level, made once: dict(csr, border, shared = {B: (poses, scan)})"""
    key = ("cov", m.id, lvl)
    if key not in _cache:
        _cache[key] = dict(csr=csr_case(pyoracle, m, lvl), border=border_case(pyoracle, m, lvl),
                           shared={B: shared_case(pyoracle, m, lvl, B) for B in SHARED_BATCHES})
    return _cache[key]


def cov_batches(pyoracle, m, lvl):
    """[(name, poses, scans)] of a level: what the reference-order tests run"""
    c = cov_level_case(pyoracle, m, lvl)
    out = [("csr", c["csr"][0], c["csr"][1]), ("border", c["border"][0], c["border"][1])]
    return out + [("shared x%d" % B, p, [s] * B) for B, (p, s) in c["shared"].items()]


def expected_cov(pyoracle, m, lvl, kind, o=None, tag=None):
    """{batch name: reference(...)} of a level by the map's shared checker (or by `o`, cached under the caller's tag)"""
    key = ("cov expected", m.id, lvl, kind, tag)
    if key not in _cache:
        o = m.checker(pyoracle, kind) if o is None else o
        _cache[key] = {name: reference(o, lvl, p, s) for name, p, s in cov_batches(pyoracle, m, lvl)}
    return _cache[key]


# ---- the chain (hsm_match_cov_batch_device) on the map's 200-beam scan -----------------------------------------------------------------
CHAIN_GROUPS, CHAIN_K = 3, 4   # two groups of the whole scan from wide starts and a group whose scans are all empty


def chain_case(pyoracle, m):
    """-> (starts [12, 3], scans): test_gpu_covariance_batch.ChainBuffers' shape scaled to the map's scan"""
    rng = np.random.default_rng(2750)
    w0, pts = m.scan(pyoracle)
    init, scans = [], []
    for gi in range(CHAIN_GROUPS):
        d = rng.uniform(-1, 1, (CHAIN_K, 3)) * [0.6 * m.resolution, 0.6 * m.resolution, 0.05]
        init.append(w0.astype(np.float64)[None] + d)
        scans += [pts if gi == 0 else pts[:129] if gi == 1 else pts[:0]] * CHAIN_K
    return np.concatenate(init).astype(F), scans


# ---- merge: the pairs ------------------------------------------------------------------------------------------------------------------
STRIP_ROWS = 16 * 2049 + 5
PAIRS = {
    "frames": ((0.03, 96, 40, 3, (0.3, 0.7)), (0.03, 90, 24, 3, (-0.25, 1.5))),
    "far": ((fc.FAR[0], 64, 64, 2, fc.FAR[1]), (fc.FAR[0], 48, 44, 2, (0.5, 0.5))),
    "deep": ((mc.RES, 333, 90, 6, (0.5, 0.5)), (mc.RES, 90, 333, 6, (0.4, 0.55))),
    "tiny": ((mc.RES, 256, 256, 8, (0.5, 0.5)), (mc.RES, 256, 256, 8, (0.5, 0.5))),
    "strip": ((mc.RES, 24, STRIP_ROWS, 1, (0.5, 0.5)), (mc.RES, 24, STRIP_ROWS, 1, (0.5, 0.5))),
}
# the pairs whose two windows lie apart in the world: there the translation carries src's centre onto dst's besides
ALIGNED = ("frames", "far")
PAIR_TRANSFORMS = ("identity", "quarter_turn", "theta_0.3", "theta_-2.1", "half_outside")
STRIP_TRANSFORMS = ("identity", "theta_0.3")
READS_MIN_SIDE = 40    # a match, a score and a cast are compared on pairs with this many cells both ways at level 0
STRIP_STRIDE = 97      # the CPU pin's affine check takes every 97th inside cell of the strip


def level0_centre(geom):
    """the world point of the centre of a geometry's window, in double from hsm_create's fp32 offsets"""
    off = mc.offsets(geom)
    return np.array([geom[1] * 0.5 * float(F(geom[0])) - float(off[0]), geom[2] * 0.5 * float(F(geom[0])) - float(off[1])])


def transform(pair, name):
    """merge_cases' transform `name` for a pair: its translation was written in metres for cells of merge_cases.RES and is
    rescaled to the pair's cells; on the ALIGNED pairs src's centre is carried onto dst's first -> float32 [3]"""
    gd, gs = PAIRS[pair]
    tx, ty, th = dict(mc.TRANSFORMS)[name]
    k = float(F(gd[0])) / mc.RES
    t = np.array([tx * k, ty * k])
    if pair in ALIGNED:
        c, s = math.cos(float(F(th))), math.sin(float(F(th)))
        cs = level0_centre(gs)
        t = t + level0_centre(gd) - np.array([c * cs[0] - s * cs[1], s * cs[0] + c * cs[1]])
    return F([t[0], t[1], th])


MERGE_CASES = [(pair, name) for pair in PAIRS for name in (STRIP_TRANSFORMS if pair == "strip" else PAIR_TRANSFORMS)]
MERGE_IDS = ["%s-%s" % c for c in MERGE_CASES]


def merge_layouts(pair, name):
    return ("quad", "plane") if pair != "strip" or name == "identity" else ("quad",)


MERGE_RUNS = [(pair, name, layout) for pair, name in MERGE_CASES for layout in merge_layouts(pair, name)]
MERGE_RUN_IDS = ["%s-%s-%s" % r for r in MERGE_RUNS]


def pair_planes(pair):
    """(dst's log-odds per level, src's): frame_cases.map_planes where the geometry is one of its own, merge_cases.synthetic_planes
    otherwise.  Made once, never changed"""
    if ("planes", pair) not in _cache:
        out = []
        for k, g in enumerate(PAIRS[pair]):
            own = pair in ALIGNED and (g[1], g[2], g[3]) in fc.GEOMETRIES
            out.append([lo for lo, _ in fc.map_planes((g[1], g[2], g[3]))] if own else mc.synthetic_planes(g, 2800 + 7 * k + g[1]))
        _cache["planes", pair] = tuple(out)
    return _cache["planes", pair]


def merge_case(pair, name):
    """-> dict(gd, gs, t, dst, src, model = [(log-odds, box)] per level), made once"""
    key = ("merge", pair, name)
    if key not in _cache:
        gd, gs = PAIRS[pair]
        dst, src = pair_planes(pair)
        t = transform(pair, name)
        _cache[key] = dict(gd=gd, gs=gs, t=t, dst=dst, src=src, model=mc.merge_pyramid(dst, src, gd, gs, t))
    return _cache[key]


def box_tiles(box):
    """merge_box_tiles of map_merge_kernels.h restated: (a row's 4-cell slots, w / 4 + 1, in blocks of 16) x (rows in tiles of 16)"""
    if box[2] < box[0]:
        return 0
    slots, rows = (box[2] - box[0] + 1) // 4 + 1, box[3] - box[1] + 1
    return ((slots + 15) // 16) * ((rows + 15) // 16)


MAX_GRID = 2048   # the workgroups of one level: more tiles than this and a workgroup takes a second one


def conditions(case, what):
    """every level's box is non-empty and the model changes at least one cell on level 0"""
    for lvl, (lo, box) in enumerate(case["model"]):
        assert box != mc.EMPTY, (what, lvl, "an empty box")
    changed = int((case["model"][0][0].view(np.uint32) != case["dst"][0].view(np.uint32)).sum())
    assert changed > 0, (what, "the merge changes nothing on level 0")
    return changed


assert box_tiles((0, 0, 23, STRIP_ROWS - 1)) == 2050 > MAX_GRID

# ---- merge: moved contexts -------------------------------------------------------------------------------------------------------------
MOVED_MAPS = (mec.M96, mec.DEEP)
MOVED_MOVES = ("x3_y-2", "one_left")
MOVED_SIDES = ("src", "dst", "both")
# x3_y-2 keeps most of the window: merge_cases' theta_0.3, rescaled.  one_left keeps one cell of the coarsest level, in a corner,
# and puts a moved window a whole window away from one that stayed: there the translation carries src's window onto dst's and
# nothing turns, so the cells that survived the move land on the level and the merge changes some
MOVED_TRANSFORMS = {"x3_y-2": ("theta_0.3", False), "one_left": ("identity", True)}
MOVED_CASES = [(m, move, side) for m in MOVED_MAPS for move in MOVED_MOVES for side in MOVED_SIDES]
MOVED_IDS = ["%s-%s-%s_moved" % (m.id, move, side) for m, move, side in MOVED_CASES]
MOVED_RUNS = [(m, move, side, layout) for m, move, side in MOVED_CASES for layout in ("quad", "plane")]
MOVED_RUN_IDS = ["%s-%s-%s_moved-%s" % (m.id, move, side, layout) for m, move, side, layout in MOVED_RUNS]


def geometry_of(m, start=None):
    s = m.start if start is None else start
    return (m.resolution, m.geom[0], m.geom[1], m.geom[2], (float(F(s[0])), float(F(s[1]))))


def moved_transform(m, move, gd, gs):
    name, aligned = MOVED_TRANSFORMS[move]
    tx, ty, th = dict(mc.TRANSFORMS)[name]
    k = float(F(m.resolution)) / mc.RES
    t = np.array([tx * k, ty * k])
    if aligned:
        assert th == 0.0
        t = t + level0_centre(gd) - level0_centre(gs)
    return F([t[0], t[1], th])


def moved_case(pyoracle, m, move, side):
    """a merge between two contexts on the map's geometry of which `side` has moved by `move` after its planes went in.
    dst holds the map's own log-odds, src synthetic planes; all stamps -1.  -> dict(gd, gs: the geometry tuples with the moved
    side's start replaced by the plan's, t, start, d0, old_dst, old_src: the planes as uploaded, dst, src: what the contexts
    hold when the merge is queued, model)"""
    key = ("moved", m.id, move, side)
    if key not in _cache:
        new, refusal, d0, _ = mec.case_plan(m, move)
        assert refusal == sc.OK, (m.id, move, refusal)
        old_dst = [lo for lo, _ in sc.old_planes(pyoracle, m)]
        old_src = mc.synthetic_planes(geometry_of(m), 2900 + m.geom[0])
        minus = lambda planes: [(lo, np.full(lo.shape, -1, np.int32)) for lo in planes]   # noqa: E731
        shifted = lambda planes: [lo for lo, _ in sc.shifted_levels(minus(planes), d0)]   # noqa: E731
        dst = shifted(old_dst) if side in ("dst", "both") else old_dst
        src = shifted(old_src) if side in ("src", "both") else old_src
        gd = geometry_of(m, new if side in ("dst", "both") else None)
        gs = geometry_of(m, new if side in ("src", "both") else None)
        t = moved_transform(m, move, gd, gs)
        _cache[key] = dict(gd=gd, gs=gs, t=t, start=new, d0=d0, old_dst=old_dst, old_src=old_src, dst=dst, src=src,
                           model=mc.merge_pyramid(dst, src, gd, gs, t))
    return _cache[key]


def moved_side_checker(pyoracle, m, move, moved):
    """the checker whose world-to-map transform a side of a moved case has: the moved map's or the map's own"""
    return mec.reader_checker(pyoracle, "ho", m, move) if moved else m.checker(pyoracle, "ho")
