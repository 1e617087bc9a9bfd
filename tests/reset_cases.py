"""hsm_reset of a context that has been USED: the cases.

The suite resets a context in four places, each on a square, centred, never-moved map that the host has just queried.  Here a
context gets a history that leaves every unit dirty, is reset with no host look in between, read on the blank map, rebuilt by
six updates and read again.  history() is a fixed list of steps; each names the state it is there for:

  load      the map's planes through upload_level; the frozen variant's stamps lie ahead of every counter the history reaches
            (FROZEN_STAMP), so uploaded_stamp_max selects the stamp-aware apply form up to the reset
  match, update   eight host matchData + updateByScan pairs, and on the two small maps one 1081-beam (keyed form) and one
            5000-beam scan (byte-map form) besides: cells, stamps, probability / texel planes, retained containers
  shift     (moved variant) hsm_shift_map by MOVE, between the host updates
  batches   matcher caches: 1024 scans under a sorting batch order (a cached permutation where the form takes one), a raw-ranges
            batch (a cached sensor geometry) and a batch wider and longer than anything after the reset (grown buffers)
  export    one hsm_occupancy_changes_device per level, so the gated call below leaves a partial publish box pending
  serial    hsm_debug_set_update_serial(level, 4093 - level): level l's key generation wraps in update l + 1 after the reset
  gated     hsm_update_by_scans_device_gated of two scans, one accepted and one rejected: the LAST step.  No host query follows,
            so the gate's count and the update boxes are still on the device when hsm_reset runs

The checkers ("ho" always, "hr" where built) go through the same history and the same reset(): the reference keeps its update
counters and its retained containers through a reset, and the expected stamps show that.  The reference has no window move:
at a shift step the checker is replaced by moved_entry_cases.moved() -- created at the new start, its counters advanced by
one empty update per update so far, loaded with the shifted cells.  The key generation is the device's own: serial_model
restates how it advances (one per scan handed to a device-side call, accepted or not; one per non-empty host update).

Pure numpy; the checker module (oracle.pyoracle) is handed in.  Shared by tests/test_reset_reference.py and
tests/test_gpu_reset.py.  Nothing is chosen at run time; PICKS records what had to be searched on the CPU.
"""
import numpy as np

import cast_cases
import frame_cases as fc
import moved_entry_cases as mec
import select_rule
import shift_cases as sc
from test_gpu_covariance_batch import reference as cov_reference   # (the module starts no device on import)
from test_window_model import reference_relocalize
import test_gpu_score_batch as tsb
import test_gpu_window as tw
import window_cases
from test_gpu_slam_scans_device import Gate

F = np.float32
ZERO2 = np.zeros(2, F)
FLT_MAX = np.finfo(np.float32).max
# ("undefined", map id, variant) -> the hypotheses of reader_inputs whose match the reference does not define on the REBUILT map
# (on the blank map every match is defined); searched on the CPU, held by tests/test_reset_reference.py.  Levels 4 and 5 of the
# deep map are 20 x 5 and 10 x 2 cells: a start a fraction of a cell off sends the one-beam estimate to NaN there
PICKS = {("undefined", "333x90_L6", "moved"): (1,)}
_cache = {}

MAPS = mec.MAPS                      # 64 x 64 x 2 centred, 96 x 40 x 3 in the sensitive frame, (333, 90, 6)
MAP_LAYOUTS = mec.MAP_LAYOUTS        # the latter two in the plane layout as well
VARIANTS = ("plain", "moved", "frozen")
MOVE = "x1"                          # one coarsest-level cell along x: a move every map takes (shift_cases)
FROZEN_STAMP = 1000                  # ahead of 3 * (updates of a whole case): those cells stay frozen until the reset
KEYED_BEAMS, DENSE_BEAMS = 1081, 5000
SERIAL_MAX = 4095                    # kSerialMax of csrc/update_types.h
GATED = (5, 6)                       # the trajectory's scans of the gated call: 0.4 cell apart, the second is rejected
AFTER_HOST, AFTER_DEVICE, AFTER_GATED = (0, 1), (2, 3), (4, 7)   # the six updates after the reset (4 and 7: 3.6 cells apart)
CSR_LENS = (0, 1, 63, 64, 65, 181, 200, 200)   # eight hypotheses: something to rank
WINDOW_HALF, TOPK = window_cases.WINDOWS[0], (1, 8)
CAST_BEAMS, N_RAYS, N_RANGE_SCANS = 65, 100, 3
CASES = [(m, layout, v) for m, layout in MAP_LAYOUTS for v in VARIANTS]
CASE_IDS = ["%s-%s-%s" % (m.id, layout, v) for m, layout, v in CASES]


def start_planes(pyoracle, m, variant):
    """what `load` uploads: the map's log-odds; stamps -1, or FROZEN_STAMP on every known cell (frozen variant)"""
    out = []
    for lo, _ in sc.old_planes(pyoracle, m):
        st = np.full(lo.shape, -1, np.int32)
        if variant == "frozen":
            st[lo != 0] = FROZEN_STAMP
        out.append((lo.copy(), st))
    return out


def dense_scans(m):
    """(map pose index of the trajectory, scan) of the keyed and the byte-map form on the two small maps; none on the deep one"""
    if m.kind != "frame":
        return []
    mp = mec.line_poses(m).astype(F)
    return [(1, np.ascontiguousarray(fc.scan_from(m.geom, mp[1], KEYED_BEAMS, 91), F)),
            (2, np.ascontiguousarray(fc.scan_from(m.geom, mp[2], DENSE_BEAMS, 92), F))]


def history(pyoracle, m, variant):
    """the steps up to the reset -> [(name, arguments ...)]"""
    key = ("history", m.id, variant)
    if key in _cache:
        return _cache[key]
    t = mec.trajectory(pyoracle, m)
    pair = lambda w, s: [("match", w, s), ("update", w, s)]   # noqa: E731
    ops = [("load", start_planes(pyoracle, m, variant))]
    for k in range(4):
        ops += pair(t.world[k], t.scans[k])
    for k, s in dense_scans(m):
        ops += pair(t.world[k], s)
    if variant == "moved":
        ops.append(("shift", MOVE))
    for k in range(4, 8):
        ops += pair(t.world[k], t.scans[k])
    ops += [("batches",), ("export",), ("serial",),
            ("gated", t.world[list(GATED)].copy(), [t.scans[k] for k in GATED])]
    _cache[key] = ops
    return ops


def after_sequence(pyoracle, m):
    """the six updates after the reset: two host pairs, one device-side call of two scans, one gated call of two (both pass)"""
    t = mec.trajectory(pyoracle, m)
    ops = []
    for k in AFTER_HOST:
        ops += [("match", t.world[k], t.scans[k]), ("update", t.world[k], t.scans[k])]
    ops.append(("device", t.world[list(AFTER_DEVICE)].copy(), [t.scans[k] for k in AFTER_DEVICE]))
    ops.append(("gated", t.world[list(AFTER_GATED)].copy(), [t.scans[k] for k in AFTER_GATED]))
    return ops


def serial_model(ops, levels, serial=None):
    """the key generation each level's updates take -> ([per update: [serial per level]], the serials left behind).  `serial`:
    None until a serial step sets it (what came before is then of no account)"""
    taken = []
    for op in ops:
        if op[0] == "serial":
            serial = [4093 - lvl for lvl in range(levels)]
        n = {"update": 1 if op[0] == "update" and len(op[2]) else 0, "device": 0, "gated": 0}.get(op[0], 0)
        if op[0] in ("device", "gated"):
            n = len(op[2])
        for _ in range(n):
            if serial is not None:
                serial = [1 if s + 1 > SERIAL_MAX else s + 1 for s in serial]
                taken.append(list(serial))
    return taken, serial


class Model:
    """a checker (moved_entry_cases.Checker: "ho" in front of `kind`) going through the steps, with what the reference keeps
    on its own but does not show: the number of updates (getUpdateIndex = updates - 1), the gate, the window's start"""

    def __init__(self, pyoracle, kind, m, variant):
        self.py, self.kind, self.m = pyoracle, kind, m
        self.o = mec.old_checker(pyoracle, kind, m, planes=[])
        self.updates, self.start = 0, np.asarray(m.start, F)
        self.gate = Gate(self.o, mec.trajectory(pyoracle, m).thresholds)
        self.flags = []

    def update_index(self, lvl=0):
        return self.updates - 1

    def planes(self):
        return mec.levels_of(self.o, self.m.levels)

    def step(self, op):
        name = op[0]
        if name == "load":
            for guard_or_own in {id(self.o.guard): self.o.guard, id(self.o.o): self.o.o}.values():
                for lvl, (lo, st) in enumerate(op[1]):
                    guard_or_own.upload_level(lvl, lo, st)
        elif name == "match":
            return self.o.match(op[1], op[2])
        elif name == "update":
            self.o.update_by_scan(op[1], op[2])
            self.o.on_map_updated()
            self.updates += 1
        elif name == "device":
            self.o.build_map(op[1], op[2])
            self.updates += len(op[2])
        elif name == "gated":
            f = self.gate.walk(op[1])
            self.o.build_map(op[1][f], [s for s, go in zip(op[2], f) if go])
            self.updates += int(f.sum())
            self.flags.append(f)
        elif name == "shift":
            new, refusal, _, _ = mec.case_plan(self.m, op[1])
            assert refusal == sc.OK
            moved = mec.moved(self.py, self.kind, self.m, op[1], self.planes(), self.updates)
            self.o.close()
            self.o, self.start = moved, np.asarray(new, F)
            self.gate.o = moved
        elif name == "reset":
            self.o.guard.reset()
            if self.o.o is not self.o.guard:
                self.o.o.reset()
            self.gate.last = F([FLT_MAX] * 3)   # HectorSlamProcessor::reset: lastMapUpdatePose; the count of applied scans stays
        return None

    def close(self):
        self.o.close()


# ---- the readers: asked on the blank map and again on the rebuilt one ------------------------------------------------------------------
def reader_inputs(pyoracle, m):
    """none of it taken from a result: the map's start pose and 200-beam scan, eight hypotheses of CSR_LENS around it, a window,
    map-frame states per level.  (After a move by MOVE the start pose is still inside the window.)"""
    key = ("inputs", m.id)
    if key not in _cache:
        centre, pts = m.scan(pyoracle)
        rng = np.random.default_rng(3100)
        res = m.resolution
        cloud = (centre.astype(np.float64) + rng.uniform(-1, 1, (len(CSR_LENS), 3)) * [0.6 * res, 0.6 * res, 0.05]).astype(F)
        cloud[0] = centre
        states = [rng.uniform(-1, 1, (8, 3)) * [1.5, 1.5, 0.1] for _ in range(m.levels)]
        near = int(np.argmin(np.hypot(pts[:, 0], pts[:, 1])))   # the one beam: the shortest, which ends on the coarse levels too
        # three raw LaserScans: the scan's own ranges over a fan (moved_entry_cases.reader_inputs' way), a few beams dropped
        n = len(pts)
        r = np.hypot(pts[:, 0], pts[:, 1]).astype(np.float64) * res
        ranges = (r[None, :] * rng.uniform(0.97, 1.03, (N_RANGE_SCANS, n))).astype(F)
        ranges[:, 7::53] = np.inf
        ranges[1, ::9] = 0.0
        starts = (centre.astype(np.float64) + rng.uniform(-1, 1, (N_RANGE_SCANS, 3)) * [0.6 * res, 0.6 * res, 0.03]).astype(F)
        # the same scans through the node's tf path: a mount per scan (moved_entry_cases.raw_log's way and limits)
        from ranges_tf_cases import rigid_rows
        rng_tf = np.random.default_rng(3102)
        tf_rows = np.stack([rigid_rows(rng_tf, tilt=0.05, shift=1.5 * res) for _ in range(N_RANGE_SCANS)])
        tf_lim = (float(F(0.5 * res)), float(F(400.0 * res)), float(F(400.0 * res)))
        tf_gates = (float(F((0.2 * res) ** 2)), float(F((400.0 * res) ** 2)), -1.0, 1.0)
        _cache[key] = dict(centre=centre, pts=pts, poses=cloud,
                           scans=[np.ascontiguousarray(pts[:n] if n != 1 else pts[near:near + 1]) for n in CSR_LENS],
                           step=(0.5 * res, 0.7 * res, 0.013), state_offsets=states, angles=cast_cases.beam_table(CAST_BEAMS)[:CAST_BEAMS],
                           ranges=ranges, starts=starts, tf_rows=tf_rows, tf_lim=tf_lim, tf_gates=tf_gates, laser=(-2.3, float(F(4.6 / (n - 1))), float(F(0.5 * res)), float(F(400.0 * res))))
    return _cache[key]


def expected_readers(pyoracle, m, o):
    """the answers of checker `o` (a moved_entry_cases.Checker) to reader_inputs; every match is one the reference defines"""
    q = reader_inputs(pyoracle, m)

    def match_if_defined(p, s):
        """None where the restatement reads the map at a NaN coordinate or ends on one: the reference indexes its grid with
        (int)NaN there.  Such a row is left out of the batches; tests/test_reset_reference.py holds the rows to PICKS"""
        u = o.guard.undefined_reads()
        res = o.guard.match(p, s)
        if o.guard.undefined_reads() != u or not np.isfinite(res[0]).all():
            return None
        return res if o.o is o.guard else o.o.match(p, s)

    out = dict(match=[match_if_defined(p, s) for p, s in zip(q["poses"], q["scans"])], score=[], window=[], states=[], grid=[],
               cov=[], cast=[], rays=[], best=[])
    out["single"] = o.match(q["centre"], q["pts"])   # (last: the container the next host update finds retained is the scan's)
    wposes = window_cases.window_poses(q["centre"], q["step"], WINDOW_HALF)
    for lvl in range(m.levels):
        out["score"].append(tsb.reference(o, lvl, q["poses"], q["scans"]))
        out["window"].append(tw.oracle_window(o, lvl, wposes, q["pts"]))
        st = (o.map_coords_pose(lvl, q["centre"]).astype(np.float64) + q["state_offsets"][lvl]).astype(F)
        pl = q["pts"] * F(1.0 / 2 ** lvl)
        out["states"].append((st, o.likelihood_states(lvl, st, pl), o.residual_states(lvl, st, pl), o.covariance_for_poses(lvl, st, pl)))
        grid, meta = o.occupancy_grid(lvl), cast_cases.metadata(o, lvl)
        out["grid"].append(grid)
        out["cov"].append(cov_reference(o, lvl, q["poses"], q["scans"]))
        reach = 0.45 * min(m.dims(lvl)) * meta[2]   # entry_geometry_cases.SHORT_SIDE of the level's shorter side
        out["cast"].append((reach,) + cast_cases.expected_cast(o.kind, grid, meta, q["poses"], q["angles"], reach))
        begin, end = cast_cases.mixed_rays(grid, meta, N_RAYS, 300 + lvl)
        out["rays"].append((begin, end) + cast_cases.expected_rays(o.kind, grid, meta, begin, end))
        out["best"].append(select_rule.select_best(out["score"][lvl][0], groups=2, group_size=len(CSR_LENS) // 2))
    a0, inc, rmin, rmax = q["laser"]
    conts = [o.laser_scan_to_container(x, a0, inc, rmin, rmax, o.scale_to_map()) for x in q["ranges"]]
    out.update(conts=conts, counts=np.array([len(c) for c in conts], np.int32), ranges_match=[o.match(s, c) for s, c in zip(q["starts"], conts)])
    out["tf"] = []   # (container, origo, match): projectLaser + rosPointCloudToDataContainer + matchData per scan
    for x, T, s in zip(q["ranges"], q["tf_rows"], q["starts"]):
        pts, origo = o.point_cloud_to_container(o.project_laser(x, a0, inc, *q["tf_lim"]), T, *q["tf_gates"], o.scale_to_map())
        assert len(pts) > 100, (m.id, "a scan of the tf batch keeps too few beams", len(pts))
        out["tf"].append((pts, origo, o.match(s, pts, origo)))
    # the chains: match -> score (on the coarsest level) -> select, match -> sigma-point covariance (level 0) -> select, over
    # the hypotheses whose match the reference defines, as one group
    rows = [k for k, x in enumerate(out["match"]) if x is not None]
    matched, scans = np.stack([out["match"][k][0] for k in rows]), [q["scans"][k] for k in rows]
    lvl = m.levels - 1
    score, cov = tsb.reference(o, lvl, matched, scans), cov_reference(o, 0, matched, scans)
    out["chain"] = dict(rows=rows, score=score, cov=cov, score_best=select_rule.select_best(score[0], groups=1, group_size=len(rows)),
                        cov_best=select_rule.select_best(np.asarray(cov["lh"], F).reshape(-1), groups=1, group_size=len(rows)))
    cell = float(o.level_info(lvl)[2])
    out["reloc_level"], out["reloc_step"] = lvl, (cell, cell, 0.05)
    u0 = o.guard.undefined_reads()
    args = (None, q["centre"], q["pts"], out["reloc_step"], mec.RELOC_HALF, mec.RELOC_K)
    out["reloc"] = reference_relocalize(o.guard, *args, search_level=lvl)   # the restatement first: it counts, the reference dies
    assert o.guard.undefined_reads() == u0, (m.id, "the reference does not define this relocalisation")
    if o.o is not o.guard:
        out["reloc"] = reference_relocalize(o.o, *args, search_level=lvl)
    o.match(q["centre"], q["pts"])   # (last again: the container the next host update finds retained is the scan's)
    return out


def run_checker(pyoracle, kind, m, variant):
    """the whole case on a checker of its own -> dict(before: planes at reset time, index_before, start, blank: planes after the
    reset, readers_blank, rebuilt: planes after the six updates, readers_rebuilt, index_after, gate_last, gate_count,
    flags: the gated calls' decisions, history's first, first_update: the planes after the first update behind the reset).  Cached"""
    key = ("run", kind, m.id, variant)
    if key in _cache:
        return _cache[key]
    md = Model(pyoracle, kind, m, variant)
    for op in history(pyoracle, m, variant):
        md.step(op)
    r = dict(before=md.planes(), index_before=md.update_index(), start=md.start.copy(), gate_count_before=md.gate.count)
    md.step(("reset",))
    r["blank"] = md.planes()
    r["readers_blank"] = expected_readers(pyoracle, m, md.o)
    first = True
    for op in after_sequence(pyoracle, m):
        md.step(op)
        if first and op[0] == "update":
            r["first_update"], first = md.planes(), False
    r["rebuilt"] = md.planes()
    r["readers_rebuilt"] = expected_readers(pyoracle, m, md.o)
    r.update(index_after=md.update_index(), gate_last=md.gate.last.copy(), gate_count=md.gate.count, flags=[f.copy() for f in md.flags])
    md.close()
    _cache[key] = r
    return r


# ---- a group of two replicas: process_scan, reset of both members, process_scan again ---------------------------------------------------
GROUP_MAP = mec.M64
GROUP_SCANS = ((0, 1, 2, 3), (4, 5, 6, 7))   # the trajectory's scans in front of and behind the reset


def group_case(pyoracle, kind):
    """HectorSlamProcessor::update's two halves per scan on one checker (match at the hint, update at the matched pose), reset()
    in between -> dict(poses, covs: one row per scan, before / blank / end: planes, index)"""
    key = ("group", kind)
    if key not in _cache:
        m = GROUP_MAP
        t = mec.trajectory(pyoracle, m)
        md = Model(pyoracle, kind, m, "plain")
        md.step(("load", start_planes(pyoracle, m, "plain")))
        poses, covs, r = [], [], {}
        for part, ks in enumerate(GROUP_SCANS):
            for k in ks:
                p, c = md.step(("match", t.world[k], t.scans[k]))
                assert np.isfinite(p).all(), (k, p)
                md.step(("update", p, t.scans[k]))
                poses.append(p)
                covs.append(c)
            if part == 0:
                r["before"] = md.planes()
                md.step(("reset",))
                r["blank"] = md.planes()
        r.update(poses=np.stack(poses), covs=np.stack(covs), end=md.planes(), index=md.update_index())
        md.close()
        _cache[key] = r
    return _cache[key]
