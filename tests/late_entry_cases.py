"""The image entries (hsm_map_extents*, hsm_map_image*, hsm_map_tiles*) and the batched relocalisation entries
(hsm_score_windows_batch_device, hsm_select_topk_groups_device, hsm_relocalize_batch*) on every map and map state the suite has:
the cases.

Both families came after the last pass over the geometries; their own tests run on one 300 x 210 level, the 70 x 52 x 3 pyramid
and conftest.pyramid_scene.  Here they get

  * images    entry_geometry_cases.MAPS -- eight frames on 64 x 64 x 2, 90 x 24 x 2 and 96 x 40 x 3, and the deep pyramids down to
              10 x 2, 2 x 10 and 2 x 2 cells --, every level: six crops, tile sizes clipped to the level, image_cases.poses on the
              level's own metadata and a few SENSITIVE poses per level, world positions whose fp32 map coordinate lies at or next
              to an integer (sensitive_poses: a search in numpy fp32 from fixed inputs, the same on every machine);
  * states    the same entries after hsm_shift_map (points_state_cases.MOVED_CASES), after hsm_reset of a used context, after a
              whole hsm_copy_map and after hsm_merge_map, each with an extents call in front so that the accumulators were used;
  * batches   per map one CSR batch of five windows over the map's 200-beam scan, lengths (200, 65, 0, 1, 64), one centre with
              an infinite angle, windows of 105, 81, 1, 63 and 65 hypotheses, every level;
  * chains    per map and search level of entry_geometry_cases.reloc_levels one relocalisation batch of three rows; the same
              batches on moved maps (moved_entry_cases.reader_checker) and after a reset.

The faults the cases are there to see are stated in numpy next to the models (faulty_box, zeroed_extents, slot_fault,
row_fault); the CPU pin shows that each changes an expected value.

Pure numpy; the checker module (oracle.pyoracle) is handed in; starts no device on import.  Shared by the CPU pin
(tests/test_late_entries_reference.py) and the GPU tests (tests/test_gpu_late_entries.py).  Nothing is chosen at run time:
PICKS records what had to be searched on the CPU.
"""
import numpy as np

import cast_cases
import entry_geometry_cases as egc
import frame_cases as fc
import image_cases as ic
import merge_cases as mc
import moved_entry_cases as mec
import newer_entry_cases as nec
import points_cases as pc
import points_state_cases as psc
import reset_cases
import shift_cases
import test_gpu_window as window_tests   # oracle_window, SENTINEL (the module starts no device on import)
import topk_rule
import window_cases
from test_window_model import reference_relocalize

F = np.float32
_cache = {}

MAPS = egc.MAPS
MAP_LAYOUTS = [(m, "quad") for m in MAPS] + [(m, "plane") for m in MAPS if m.planes_too]
MAP_LAYOUT_IDS = ["%s-%s" % (m.id, layout) for m, layout in MAP_LAYOUTS]
PADS = (67, 66, 64)   # where a device output starts in its guarded block: an odd address, an even one off 4, a multiple of 4
# ("reloc", map id, level, row) -> index into SECOND_CENTRES (row 1) or THIRD_LENS (row 2) where the first choice gave a row the
# reference does not define; searched on the CPU by search_picks(), held by tests/test_late_entries_reference.py.  The two long
# deep maps searched on level 2 (83 x 22 and 22 x 83 cells): the first 129 beams of their scan see one side of the loop only, and
# a match from one of the eight starts ends on a NaN; 150 beams reach round the corner
PICKS = {("reloc", "333x90_L6", 2, 2): 1, ("reloc", "90x333_L6", 2, 2): 1}
MAX_PICKS = 3
# the moved relocalisation cases (map id, move, level) the reference does not define, by name; at most MAX_DROPS
MOVED_DROPPED = ()
MAX_DROPS = 2


def geometry(m, start=None):
    """the geometry tuple image_cases and points_cases take"""
    return nec.geometry_of(m, start)


def planes(pyoracle, m):
    """[(log-odds, stamps)] per level: the shared checker's, never changed"""
    return shift_cases.old_planes(pyoracle, m)


# ---- 1: images on every geometry ----------------------------------------------------------------------------------------------------
NODE_MAPS = (egc.map_of(egc.SENSITIVE_FRAME, (96, 40, 3)), egc.map_of(None, (333, 90, 6)))   # also held to the reference's node
FAULTS = ("swapped_origin", "other_level_reciprocal", "level0_cell", "fused")
SENSITIVE_CELLS = 24      # integer map coordinates tried per axis
SENSITIVE_ULPS = (0, -1, 1, -2, 2, -3, 3)


def crops(sx, sy):
    """[(name, crop)] of a level; the GPU test adds the extents box itself"""
    out = [("whole", None)]
    odd = egc.level_boxes(sx, sy).get("odd start, odd width")
    if odd is not None:
        out.append(("odd start, odd width", odd))
    return out + [("last column", (sx - 1, 0, sx - 1, sy - 1)), ("last row", (0, sy - 1, sx - 1, sy - 1)),
                  ("overhangs two sides", (sx // 2, sy // 2, sx + 5, sy + 3))]


def tile_sizes(sx, sy):
    """image_cases.tile_sizes with every size clipped to the level (the entries refuse a larger tile), duplicates dropped, and a
    tile the level's full width and up to three rows high: its rows start at three different phases of the output's 4-byte
    groups, so the cut into head, groups and tail differs from row to row"""
    out = []
    for tw, th in ic.tile_sizes(sx, sy) + [(sx, 3)]:
        size = (min(tw, sx), min(th, sy))
        if size not in out:
            out.append(size)
    return out


def inexact_reciprocal(m):
    """fp32 1 / resolution times the resolution is not 1"""
    res = F(m.resolution)
    return float(F(F(1.0) / res)) * float(res) != 1.0


def held_to_faults(m):
    """the maps on whose every level each fault that changes a number must change a box: the frame maps with an inexact
    reciprocal, and the far frame"""
    return m.kind == "frame" and (inexact_reciprocal(m) or m.frame == fc.FAR)


def fault_changes_a_number(fault, geom, lvl):
    """whether the fault hands tile_box another number on this level at all"""
    ox, oy, _ = ic.metadata(geom, lvl)
    if fault == "swapped_origin":
        return bool(ox != oy)
    if fault == "other_level_reciprocal":
        return geom[3] > 1
    if fault == "level0_cell":
        return lvl > 0
    return True


def _fused_coordinate(p, origin, inv):
    """(p - origin) * inv contracted into one fused multiply-add, fma(p, inv, -(origin * inv)): the product origin * inv rounded to
    fp32, p * inv - that in float64 (exact but for the last rounding), rounded to fp32 once"""
    with np.errstate(over="ignore", invalid="ignore"):
        return F(np.float64(F(p)) * np.float64(inv) - np.float64(F(origin * inv)))


def faulty_box(fault, geom, lvl, pose, tile_w, tile_h, sx, sy):
    """image_cases.tile_box of a kernel with one of the faults:
    swapped_origin          origin_x and origin_y exchanged
    other_level_reciprocal  the reciprocal of the next coarser level's cell (of the next finer one on the coarsest level)
    level0_cell             a cell length that was not doubled level by level: level 0's, in the half cell of the origin and in
                            the reciprocal
    fused                   image_cases._axis_lo on a map coordinate from a single fused multiply-add"""
    ox, oy, res = ic.metadata(geom, lvl)
    if fault == "swapped_origin":
        return ic.tile_box((oy, ox, res), pose, tile_w, tile_h, sx, sy)
    if fault == "other_level_reciprocal":
        other = lvl + 1 if lvl + 1 < geom[3] else lvl - 1
        return ic.tile_box((ox, oy, ic.metadata(geom, other)[2]), pose, tile_w, tile_h, sx, sy)
    if fault == "level0_cell":
        _, _, _, _, t0, t1 = pc.world_from_map(geom, lvl)
        cell = F(geom[0])
        half = F(cell * F(0.5))
        return ic.tile_box((F(F(t0) - half), F(F(t1) - half), cell), pose, tile_w, tile_h, sx, sy)
    assert fault == "fused"
    if not (np.isfinite(pose[0]) and np.isfinite(pose[1])):
        return ic.EMPTY
    inv = F(F(1.0) / res)
    lx = ic._axis_lo(_fused_coordinate(pose[0], ox, inv), F(0.0), F(1.0), tile_w, sx)   # (m - 0) * 1 == m: the model's clamps
    ly = ic._axis_lo(_fused_coordinate(pose[1], oy, inv), F(0.0), F(1.0), tile_h, sy)
    return lx, ly, lx + tile_w - 1, ly + tile_h - 1


def _ulps(v, n):
    for _ in range(abs(n)):
        v = np.nextafter(F(v), F(np.inf if n > 0 else -np.inf))
    return F(v)


def sensitive_poses(geom, lvl, sx, sy):
    """float32 [n, 3]: world positions whose fp32 map coordinate lies at or next to an integer, so that the truncation turns on
    the last bit of origin, reciprocal and rounding.  Per axis the positions origin + k * cell for up to SENSITIVE_CELLS whole
    k inside the level, each moved by SENSITIVE_ULPS; of these the first per fault and axis whose 1 x 1 tile a faulty kernel
    puts elsewhere (where there is one), and the two ends of the axis in any case.  The other coordinate is the level's centre"""
    key = ("sensitive", geom, lvl)
    if key in _cache:
        return _cache[key]
    meta = ic.metadata(geom, lvl)
    mid = ic.world_of(meta, sx / 2 + 0.25, sy / 2 + 0.25)
    out = []

    def pose_of(axis, v):
        p = [mid[0], mid[1], 0.1]
        p[axis] = v
        return F(p)

    for axis, size in ((0, sx), (1, sy)):
        cells = sorted({int(k) for k in np.linspace(1, size - 1, min(size - 1, SENSITIVE_CELLS))})
        cands = [pose_of(axis, _ulps(F(np.float64(meta[axis]) + k * np.float64(meta[2])), u)) for k in cells for u in SENSITIVE_ULPS]
        boxes = [ic.tile_box(meta, p, 1, 1, sx, sy) for p in cands]
        out += [cands[0], cands[len(cands) - len(SENSITIVE_ULPS)]]
        for fault in FAULTS:
            hit = next((p for p, box in zip(cands, boxes) if faulty_box(fault, geom, lvl, p, 1, 1, sx, sy) != box), None)
            if hit is not None:
                out.append(hit)
    poses = np.unique(np.asarray(out, F).reshape(-1, 3), axis=0)
    _cache[key] = poses
    return poses


def faults_seen(geom, lvl, poses, sx, sy):
    """{fault: how many of `poses` a faulty kernel gives another 1 x 1 box}"""
    meta = ic.metadata(geom, lvl)
    return {fault: sum(faulty_box(fault, geom, lvl, p, 1, 1, sx, sy) != ic.tile_box(meta, p, 1, 1, sx, sy) for p in poses)
            for fault in FAULTS}


def image_level(geom, lvl, sx, sy):
    """what the image entries are asked on a level of this geometry: dict(meta, poses, sizes, crops)"""
    key = ("image level", geom, lvl)
    if key not in _cache:
        meta = ic.metadata(geom, lvl)
        poses = np.concatenate([ic.poses(meta, sx, sy), sensitive_poses(geom, lvl, sx, sy)]).astype(F)
        _cache[key] = dict(meta=meta, poses=poses, sizes=tile_sizes(sx, sy), crops=crops(sx, sy))
    return _cache[key]


def checker_metadata(o, lvl):
    """cast_cases.metadata as float32"""
    return tuple(F(v) for v in cast_cases.metadata(o, lvl))


# ---- 2: images across map state -----------------------------------------------------------------------------------------------------
MOVED_CASES, MOVED_IDS, MOVED_MAPS = psc.MOVED_CASES, psc.MOVED_IDS, psc.MOVED_MAPS
RESET_LAYOUTS = reset_cases.MAP_LAYOUTS
COPY_MAP = egc.map_of(*egc.COPY_FRAME)
MERGE_CASE = ("frames", "theta_0.3")


def zeroed_extents(logodds):
    """the box of an extents call whose four accumulators (min column | min flat index | min -column | min -flat index) start at 0
    instead of at none: the two minima are pinned to 0, the negated maxima are not touched, and a level without a known cell
    is not seen to be empty"""
    want = ic.extents_model(logodds)
    return (0, 0, 0, 0) if want == ic.EMPTY else (0, 0, want[2], want[3])


def margin_planes(log_odds):
    """the planes with their first columns and rows unknown (an eighth of either side, one cell at the least): the hull of the
    known cells does not start at cell (0, 0), so an accumulator that starts at 0 shows"""
    out = []
    for lo in log_odds:
        lo = np.array(lo, F)
        sy, sx = lo.shape
        lo[:, :max(1, sx // 8)] = F(0.0)
        lo[:max(1, sy // 8), :] = F(0.0)
        out.append(lo)
    return out


def copy_case(pyoracle):
    """the whole copy on entry_geometry_cases.COPY_FRAME: dst holds the map, src synthetic planes with an unknown margin
    -> dict(geom, dst, src)"""
    if "copy" not in _cache:
        geom = geometry(COPY_MAP)
        _cache["copy"] = dict(geom=geom, dst=[lo for lo, _ in planes(pyoracle, COPY_MAP)],
                              src=margin_planes(mc.synthetic_planes(geom, 3300)))
    return _cache["copy"]


def merge_cases_of_this_file():
    """{name: dict(gd, gs, t, dst, src, model)}: newer_entry_cases.merge_case("frames", "theta_0.3") as it stands -- every cell of
    its dst is known before and after, so its hull starts at (0, 0) whatever the accumulators held -- and the same pair and
    transform with an unknown margin on dst, which the merge leaves unknown where src does not reach"""
    if "merge" not in _cache:
        case = nec.merge_case(*MERGE_CASE)
        dst = margin_planes(case["dst"])
        margin = dict(case, dst=dst, model=mc.merge_pyramid(dst, case["src"], case["gd"], case["gs"], case["t"]))
        _cache["merge"] = {"committed": case, "margin": margin}
    return _cache["merge"]


def state_cases(pyoracle):
    """[(name, [log-odds per level of a context the case reads])] of every moved, reset, copied and merged case"""
    out = [("moved %s %s" % (m.id, name), [lo for lo, _ in psc.moved_case(pyoracle, m, name)["planes"]]) for m, name in MOVED_MAPS]
    out += [("reset %s" % m.id, [np.zeros_like(lo) for lo, _ in planes(pyoracle, m)]) for m in reset_cases.MAPS]
    out.append(("copied", copy_case(pyoracle)["src"]))
    out.append(("merged", [lo for lo, _ in merge_cases_of_this_file()["margin"]["model"]]))
    return out


# ---- 3: batched window scores -------------------------------------------------------------------------------------------------------
BATCH_LENS = (200, 65, 0, 1, 64)
BATCH_HALVES = egc.WINDOWS + ((0, 0, 0), (31, 0, 0), (32, 0, 0))   # 105, 81, 1, 63 and 65 hypotheses
# the centres: the scan's own, and four neighbours off it by fractions of a level-0 cell and hundredths of a radian
BATCH_OFFSETS = ((0.0, 0.0, 0.0), (0.3, -0.2, 0.02), (-0.45, 0.15, -0.03), (0.2, 0.4, 0.01), (-0.15, -0.35, 0.04))
INF_ROW = 1               # this neighbour's angle is inf: held to the single call's bits, which the reference does not define
EMPTY_ROW = BATCH_LENS.index(0)
EMPTY_NAN = 0xFFC00000    # the likelihood of a window whose scan is empty
SENTINEL = window_tests.SENTINEL
assert [window_cases.window_count(h) for h in BATCH_HALVES] == [105, 81, 1, 63, 65]


def batch_case(pyoracle, m):
    """-> (centres [5, 3], scans, step)"""
    key = ("batch", m.id)
    if key not in _cache:
        centre, pts = m.scan(pyoracle)
        res = m.resolution
        centres = (centre.astype(np.float64)[None] + np.array(BATCH_OFFSETS) * [res, res, 1.0]).astype(F)
        centres[INF_ROW, 2] = np.inf
        _cache[key] = (centres, [np.ascontiguousarray(pts[:n]) for n in BATCH_LENS], egc.window_step(m))
    return _cache[key]


def shared_level(m):
    """the level the shared-scan form runs on"""
    return min(1, m.levels - 1)


def expected_batch(pyoracle, m, lvl, half, kind, o=None, tag=None, scan_of=lambda b: b):
    """[(likelihood [W], residual [W]) per window] by the map's shared checker (or by `o`, cached under the caller's tag); None
    for the window around the infinite angle.  scan_of: which scan window b is scored against"""
    key = ("batch expected", m.id, lvl, half, kind, tag)
    if key not in _cache:
        centres, scans, step = batch_case(pyoracle, m)
        o = m.checker(pyoracle, kind) if o is None else o
        _cache[key] = [None if b == INF_ROW else
                       window_tests.oracle_window(o, lvl, window_cases.window_poses(centres[b], step, half), scans[scan_of(b)])
                       for b in range(len(centres))]
    return _cache[key]


def slot_fault(scores, fill=SENTINEL):
    """what a kernel that starts window b at slot b * (W rounded up to 64) leaves in an output of [B, W] filled with `fill`"""
    B, W = scores.shape
    w64 = -(-W // 64) * 64
    out = np.full(B * W, fill, F)
    for b in range(B):
        n = max(0, min(W, B * W - b * w64))
        out[b * w64:b * w64 + n] = scores[b, :n]
    return out.reshape(B, W)


def row_fault(b):
    """a kernel that takes window b's scan from row b - 1 of the offsets"""
    return (b - 1) % len(BATCH_LENS)


# ---- 4: the batched relocalisation --------------------------------------------------------------------------------------------------
RELOC_ROWS = 3
SECOND_CENTRES = ((0.3, -0.2, 0.01), (-0.25, 0.35, -0.01), (0.15, 0.1, 0.0))   # row 1's centre off row 0's, in search-level cells
THIRD_LENS = (129, 150, 160)                                                     # row 2's beams
RELOC_CASES = [(m, lvl) for m in MAPS for lvl in egc.reloc_levels(m)]
RELOC_IDS = ["%s-search%d" % (m.id, lvl) for m, lvl in RELOC_CASES]
TIED = frozenset((m.id, lvl) for m, lvl in RELOC_CASES if m.kind == "deep" and lvl == m.levels - 1)   # 10 x 2, 2 x 10, 2 x 2
RELOC_MOVED_MAPS = (mec.M96, mec.DEEP)
RELOC_MOVED = [(m, name, lvl) for m in RELOC_MOVED_MAPS for name in mec.READER_MOVES for lvl in egc.reloc_levels(m)]
RELOC_MOVED_IDS = ["%s-%s-search%d" % (m.id, name, lvl) for m, name, lvl in RELOC_MOVED]
RESET_MAP = mec.M96


def reloc_rows(pyoracle, m, lvl, picks=None):
    """-> (centres [3, 3], scans, step): the map's scan at its centre (entry_geometry_cases.expected_reloc's case), the same scan
    around a second centre a fraction of a search-level cell away, the scan's first 129 beams at the first centre"""
    picks = PICKS if picks is None else picks
    centre, pts = m.scan(pyoracle)
    step = egc.reloc_step(pyoracle, m, lvl)
    gx, gy, ga = SECOND_CENTRES[picks.get(("reloc", m.id, lvl, 1), 0)]
    second = (centre.astype(np.float64) + [gx * step[0], gy * step[1], ga]).astype(F)
    n = THIRD_LENS[picks.get(("reloc", m.id, lvl, 2), 0)]
    return np.stack([centre, second, centre]).astype(F), [pts, pts, np.ascontiguousarray(pts[:n])], step


def reference_row(guard, o, lvl, centre, scan, step):
    """reference_relocalize of one row: the restatement `guard` first, which counts the reads the reference does not define; the
    checker `o` only on a defined row -> the result, or None"""
    u0 = guard.undefined_reads()
    r = reference_relocalize(guard, None, centre, scan, step, egc.RELOC_HALF, egc.RELOC_K, search_level=lvl)
    if guard.undefined_reads() != u0:
        return None
    return r if o is guard else reference_relocalize(o, None, centre, scan, step, egc.RELOC_HALF, egc.RELOC_K, search_level=lvl)


def expected_reloc_batch(pyoracle, m, lvl, kind):
    """[reference result per row]; row 0 is entry_geometry_cases.expected_reloc's"""
    key = ("reloc batch", m.id, lvl, kind)
    if key not in _cache:
        centres, scans, step = reloc_rows(pyoracle, m, lvl)
        rows = [egc.expected_reloc(pyoracle, m, lvl, kind)]
        for b in (1, 2):
            r = reference_row(m.checker(pyoracle, "ho"), m.checker(pyoracle, kind), lvl, centres[b], scans[b], step)
            assert r is not None, (m.id, lvl, b, "the reference does not define this row: see search_picks()")
            rows.append(r)
        _cache[key] = rows
    return _cache[key]


def expected_reloc_moved(pyoracle, m, name, lvl, kind):
    """the same rows on the moved map's checker (the world does not move with the window) -> [result per row], or None where
    the reference does not define one of them"""
    key = ("reloc moved", m.id, name, lvl, kind)
    if key not in _cache:
        centres, scans, step = reloc_rows(pyoracle, m, lvl)
        o = mec.reader_checker(pyoracle, kind, m, name)
        rows = [reference_row(o.guard, o.o, lvl, centres[b], scans[b], step) for b in range(RELOC_ROWS)]
        _cache[key] = None if any(r is None for r in rows) else rows
    return _cache[key]


def stacked(rows):
    """the reference's rows as the batch's outputs: {key of test_gpu_relocalize_batch.BatchBuffers.KEYS: array}"""
    nan3 = np.full(3, np.nan, F)
    return dict(cand=np.stack([r["cand"] for r in rows]), cov=np.stack([r["cov"] for r in rows]),
                lh0=np.stack([r["lh0"] for r in rows]), cand_index=np.stack([r["index"] for r in rows]).astype(np.int32),
                best_pose=np.stack([nan3 if r["best_pose"] is None else r["best_pose"] for r in rows]).astype(F),
                best_score=np.array([r["best_score"] for r in rows], F), best_index=np.array([r["best_index"] for r in rows], np.int32))


def topk_of(rows):
    """the grouped top-K's rows by tests/topk_rule.py from the reference's window scores"""
    return np.stack([topk_rule.topk(r["scores"], egc.RELOC_K)[0] for r in rows]).astype(np.int32)


def search_picks(pyoracle):
    """-> the PICKS dict for the present cases (run on the CPU when an input changes; the result is recorded above)"""
    picks = {}
    for m, lvl in RELOC_CASES:
        guard = m.checker(pyoracle, "ho")
        for b, choices in ((1, SECOND_CENTRES), (2, THIRD_LENS)):
            for k in range(len(choices)):
                centres, scans, step = reloc_rows(pyoracle, m, lvl, {("reloc", m.id, lvl, b): k})
                if reference_row(guard, guard, lvl, centres[b], scans[b], step) is not None:
                    break
            else:
                k = None
            if k != 0:
                picks["reloc", m.id, lvl, b] = k
    return picks
