"""The device-resident entries across a window move (hsm_shift_map): the cases.

tests/shift_cases.py and tests/test_gpu_shift_map.py hold the move itself to the reference; around it they run the oldest
entries only.  Here are the inputs for everything newer on a context that HAS moved: the device-side updates (plain, gated,
with origos) queued right in front of a move, the device SLAM loop split by a move, and the map readers on a moved frame.

Pure numpy; the checker module (oracle.pyoracle) is handed in.  Shared by the CPU pin (tests/test_moved_entries_reference.py)
and the GPU tests (tests/test_gpu_moved_entries.py).  The reference has no move: the checker of everything after one is
shift_cases.moved_checker -- created at the new start, loaded with shift_planes() of the old cells, its counters advanced by
one empty update per scan applied so far -- behind shift_cases.Guarded.

Maps: three of shift_cases.MAP_LAYOUTS (64 x 64 x 2 centred, quad; 96 x 40 x 3 in the sensitive frame and (333, 90, 6), quad
and plane).  Moves: x1 and x3_y-2 everywhere, one_left for the readers, x4_y-1 on the deep map besides (EXTRA_MOVES).  A trajectory per map: eight posed scans of at most 200
end points, 4 + 4 around the move, with fp32 hint deltas and a pair of gate thresholds.  trajectory() asserts its own
conditions (run_case), so an input that drifts fails on the CPU instead of passing as a comparison that shows nothing.
"""
import numpy as np

import cast_cases
import entry_geometry_cases as egc
import frame_cases as fc
import shift_cases as sc
from test_gpu_slam_scans_device import Gate

F = np.float32
ZERO2 = np.zeros(2, F)

M64 = egc.map_of(sc.CENTRED_FRAME, (64, 64, 2))
M96 = egc.map_of(egc.SENSITIVE_FRAME, (96, 40, 3))
DEEP = egc.map_of(None, sc.DEEP)
MAPS = [M64, M96, DEEP]
MAP_LAYOUTS = [(M64, "quad"), (M96, "quad"), (M96, "plane"), (DEEP, "quad"), (DEEP, "plane")]
assert all(any(m is m2 and l == l2 for m2, l2 in sc.MAP_LAYOUTS) for m, l in MAP_LAYOUTS)
MAP_LAYOUT_IDS = ["%s-%s" % (m.id, layout) for m, layout in MAP_LAYOUTS]
MOVES = ("x1", "x3_y-2")
READER_MOVES = ("x3_y-2", "one_left")
N_SCANS, SPLIT, MAX_BEAMS = 8, 4, 200

# the robot's way along its line, in level-0 cells, and the gate's distance threshold in cells.  Where the reference keeps
# track the gate integrates scans 0, 2, 5, 7 and rejects 1, 3, 4, 6 with 0.4 cell and more to spare: two of either in each
# half, and scan 4, the first one after the move, is rejected by the pose scan 2 left behind (a gate that lost its pose in the
# move would integrate it).  Where the first match after the move jumps (LOSES_TRACK) the later poses keep their distances
# from one another and the gate integrates 4 and 7 and rejects 5 and 6
WAY = (0.0, 0.4, 2.8, 3.2, 4.0, 4.8, 5.2, 7.6)
GATE_CELLS, GATE_ANGLE = 1.6, 0.5
# (333, 90, 6) moved by (3, -2) coarsest cells keeps 26 of its 90 rows: levels 3, 4, 5 hold 3, 1 and 0 rows of the map, and on
# every line tried (x = 30 .. 220, y = 68 .. 82, four headings) the reference's first match after the move leaves the room by
# tens to thousands of cells and stays there.  That is the reference's answer on this map, defined and finite, and a device
# context has to give its bits; the case stays, and case_conditions asserts that it is the only one of its kind
LOSES_TRACK = {("333x90_L6", "x3_y-2")}
HEADING_STEP = 0.02
# the line's first level-0 cell and direction per map.  The frame maps: inside frame_cases.room.  The deep map: a line that
# stays inside the window under both moves ((3, -2) keeps the old rows 64 .. 89 and the old columns 0 .. 236), searched on the
# CPU by search_lines() among x = 40 .. 220 step 10, y = 68 .. 82 step 2 for the conditions of run_case
LINES = {M64.id: ((10.0, 30.0, 0.1), (0.94, 0.342)), M96.id: ((16.0, 19.0, 0.1), (0.94, 0.342)),
         DEEP.id: ((120.0, 74.0, 0.1), (1.0, 0.0))}
_cache = {}


class Checker(sc.Guarded):
    """shift_cases.Guarded with the calls of this file that change the map sent to both checkers as well"""

    def build_map(self, poses, scans, origo=ZERO2):
        self.guard.build_map(poses, scans, origo)
        if self.o is not self.guard:
            self.o.build_map(poses, scans, origo)

    def on_map_updated(self):
        self.guard.on_map_updated()
        if self.o is not self.guard:
            self.o.on_map_updated()

    def match(self, w, pts, origo=ZERO2):
        u = self.guard.undefined_reads()
        res = self.guard.match(w, pts, origo)
        assert self.guard.undefined_reads() == u and np.isfinite(res[0]).all(), ("the reference does not define this match", w)
        return res if self.o is self.guard else self.o.match(w, pts, origo)

    def update_by_scan(self, w, pts, origo=ZERO2):
        self.guard.update_by_scan(w, pts, origo)
        if self.o is not self.guard:
            self.o.update_by_scan(w, pts, origo)


# ---- the moves: shift_cases' by name, and one more for the deep map ---------------------------------------------------------------------
# (333, 90, 6) under x3_y-2 is a case where the reference loses track (LOSES_TRACK), and x1 runs along the x axis: one more,
# off the axis, that keeps 58 of the 90 rows (7, 3 and 1 on levels 3, 4, 5).  Searched on the CPU among (k, -1) coarsest cells,
# k = +-1 .. +-3 and 4, for run_case's and posed_case's conditions: on k = +-2, +-3 the reference jumps as on x3_y-2, on k = 1 it
# drifts past the gate's threshold on scan 6, on k = 4 it keeps track
EXTRA_MOVES = {"x4_y-1": (4, -1)}
DEEP_MOVES = MOVES + ("x4_y-1",)


def moves_of(m):
    return DEEP_MOVES if m is DEEP else MOVES


def shift_of(geom, name):
    return EXTRA_MOVES[name] if name in EXTRA_MOVES else sc.shift_of(geom, name)


def case_plan(m, name):
    """shift_cases.case_plan for the names of this file -> (new start, refusal, d0, levels)"""
    kx, ky = shift_of(m.geom, name)
    new = sc.start_for_shift(m.start, m.geom, kx, ky)
    return (new,) + sc.plan_model(m.resolution, m.geom[0], m.geom[1], m.geom[2], np.asarray(m.start, F), new)


def moved_checker(pyoracle, kind, m, name, planes=None, empty_updates=0):
    """shift_cases.moved_checker for the names of this file"""
    if name not in EXTRA_MOVES:
        return sc.moved_checker(pyoracle, kind, m, name, planes, empty_updates)
    new, refusal, d0, _ = case_plan(m, name)
    assert refusal == sc.OK, (m.id, name, refusal)
    o = pyoracle.Oracle(kind, m.resolution, m.geom[0], m.geom[1], m.geom[2], (float(new[0]), float(new[1])))
    o.set_update_factor_free(fc.FACTORS[0])
    o.set_update_factor_occupied(fc.FACTORS[1])
    for _ in range(empty_updates):
        o.update_by_scan(np.zeros(3, F), np.zeros((0, 2), F))
    for lvl, (lo, st) in enumerate(sc.shifted_levels(sc.old_planes(pyoracle, m) if planes is None else planes, d0)):
        o.upload_level(lvl, lo, st)
    return o


def old_checker(pyoracle, kind, m, planes=None, start=None):
    """a checker of its own at the map's start (or `start`) that holds the map's planes (or `planes`); the caller may change it"""
    planes = sc.old_planes(pyoracle, m) if planes is None else planes

    def make(k):
        o = pyoracle.Oracle(k, m.resolution, m.geom[0], m.geom[1], m.geom[2], m.start if start is None else start)
        o.set_update_factor_free(fc.FACTORS[0])
        o.set_update_factor_occupied(fc.FACTORS[1])
        for lvl, (lo, st) in enumerate(planes):
            o.upload_level(lvl, lo, st)
        return o
    return Checker(pyoracle, kind, make)


def moved(pyoracle, kind, m, name, planes=None, applied=0):
    """the checker of the moved map: one empty update per scan applied so far"""
    return Checker(pyoracle, kind, lambda k: moved_checker(pyoracle, k, m, name, planes, empty_updates=applied))


def levels_of(o, n):
    return [o.download_level(lvl) for lvl in range(n)]


# ---- the trajectory -------------------------------------------------------------------------------------------------------------------
class Trajectory:
    """world [8, 3] the scans were drawn from, scans (<= 200 end points, level-0 cells), deltas [8, 3] fp32 (hint k = pose k-1 +
    delta k, hint 0 = world 0), thresholds (metres, radians), origos [8, 2] for the entries that take one per scan"""

    def __init__(self, world, scans, thresholds, origos):
        self.world = np.ascontiguousarray(world, F)
        self.scans = [np.ascontiguousarray(s, F).reshape(-1, 2) for s in scans]
        self.deltas = np.zeros((len(scans), 3), F)
        self.deltas[1:] = self.world[1:] - self.world[:-1]
        self.thresholds, self.origos = thresholds, np.ascontiguousarray(origos, F)
        assert len(self.scans) == N_SCANS and all(0 < len(s) <= MAX_BEAMS for s in self.scans)


def line_poses(m, line=None):
    """the eight level-0 MAP poses of the old frame along the map's line"""
    (x, y, th), (ux, uy) = LINES[m.id] if line is None else line
    return np.array([[x + s * ux, y + s * uy, th + HEADING_STEP * k] for k, s in enumerate(WAY)], np.float64)


def trajectory(pyoracle, m, line=None):
    key = ("traj", m.id, line)
    if key in _cache:
        return _cache[key]
    o = m.checker(pyoracle, "ho")
    mp = line_poses(m, line).astype(F)
    world = np.stack([o.world_coords_pose(0, p) for p in mp]).astype(F)
    if m.kind == "frame":
        scans = [fc.scan_from(m.geom, mp[k], MAX_BEAMS, 70 + k) for k in range(N_SCANS)]
    else:
        from hector_slam_amd import synth
        c = m.case()
        s = float(F(1.0) / F(m.resolution))
        noise = np.random.default_rng(2201)
        scans = [synth.make_scan(c.world, world[k], MAX_BEAMS, s, noise, range_max=max(m.geom[:2]) * m.resolution) for k in range(N_SCANS)]
    rng = np.random.default_rng(2202)
    origos = rng.uniform(-1.5, 1.5, (N_SCANS, 2)).astype(F)   # level-0 cells, one per scan
    t = Trajectory(world, scans, (float(F(GATE_CELLS * m.resolution)), GATE_ANGLE), origos)
    _cache[key] = t
    return t


# ---- the trajectory as a laser on a moving, tilted mount sees it ------------------------------------------------------------------------
RAW = "raw"   # run_case(origos=RAW): the scans and origos are those the node's tf conversion makes of raw_log()


def raw_log(pyoracle, m):
    """the frame map's trajectory as raw LaserScans -> dict(ranges [8, 200] in metres, rows [8, 12], a0, inc, lim = (range_min,
    range_max, range_cutoff), gates = (sqr_min, sqr_max, z_min, z_max)).  The transforms are ranges_tf_cases.rigid_rows: a small
    roll and pitch, any yaw, a shift of up to 1.5 cells, a different one per scan; the ranges are what a laser at that place
    and heading measures to frame_cases.room, so the converted scan matches like the trajectory's own.  A few beams are inf
    (projectLaser drops them) and one scan has ranges below range_min"""
    key = ("raw", m.id)
    if key in _cache:
        return _cache[key]
    from ranges_tf_cases import rigid_rows
    assert m.kind == "frame"
    rng = np.random.default_rng(2204)
    res, n = float(m.resolution), MAX_BEAMS
    mp = line_poses(m)
    a0, inc = -2.3, float(F(4.6 / (n - 1)))
    x0, y0, x1, y1 = fc.room(m.geom)
    ranges, rows = np.empty((N_SCANS, n), F), np.empty((N_SCANS, 12), np.float64)
    for k in range(N_SCANS):
        rows[k] = T = rigid_rows(rng, tilt=0.05, shift=1.5 * res)
        yaw = np.arctan2(T[4], T[0])
        px, py, th = mp[k]
        lx = px + (np.cos(th) * T[3] - np.sin(th) * T[7]) / res
        ly = py + (np.sin(th) * T[3] + np.cos(th) * T[7]) / res
        a = a0 + inc * np.arange(n) + th + yaw
        c, s = np.cos(a), np.sin(a)
        with np.errstate(divide="ignore"):
            tx = np.where(c > 0, (x1 - lx) / c, (x0 - lx) / c)
            ty = np.where(s > 0, (y1 - ly) / s, (y0 - ly) / s)
        ranges[k] = (np.minimum(tx, ty) * res).astype(F)
    ranges[:, 7::53] = np.inf
    ranges[3, ::11] = F(0.1 * res)
    lim = (float(F(0.5 * res)), float(F(300.0 * res)), float(F(300.0 * res)))
    node_gates = (0.2 * res, 300.0 * res, -1.0, 1.0)   # the node's parameters; it squares the two distances itself
    gates = (float(F(node_gates[0] * node_gates[0])), float(F(node_gates[1] * node_gates[1])), -1.0, 1.0)
    _cache[key] = dict(ranges=ranges, rows=rows, a0=a0, inc=inc, lim=lim, gates=gates, node_gates=node_gates)
    return _cache[key]


def raw_trajectory(pyoracle, kind, m):
    """the Trajectory whose scans and origos are the checker's projectLaser + rosPointCloudToDataContainer of raw_log()"""
    key = ("raw traj", kind, m.id)
    if key not in _cache:
        raw, t0 = raw_log(pyoracle, m), trajectory(pyoracle, m)
        o = m.checker(pyoracle, kind)
        conts, origos = [], np.empty((N_SCANS, 2), F)
        for k in range(N_SCANS):
            cloud = o.project_laser(raw["ranges"][k], raw["a0"], raw["inc"], *raw["lim"])
            pts, origos[k] = o.point_cloud_to_container(cloud, raw["rows"][k], *raw["gates"], o.scale_to_map())
            conts.append(pts)
        _cache[key] = Trajectory(t0.world, conts, t0.thresholds, origos)
    return _cache[key]


# ---- the composed reference loop ---------------------------------------------------------------------------------------------------------
def composed_loop(segments, t, gate_of=Gate, origos=None):
    """HectorSlamProcessor::update composed of the checker's parts -- match on the hint, the gate (Gate.walk on the checker's
    own pose_difference_larger_than), update_by_scan + on_map_updated where the gate says so -- over segments [(make checker
    (planes of the checker before or None, scans applied so far) -> checker, number of scans)].  The gate's last pose and the
    pose the next hint starts from are carried from one segment's checker to the next in world coordinates, which do not move
    with the window.  -> dict(poses, covs, flags, planes per segment end, checkers, gate)"""
    poses, covs, flags, ends, checkers = [], [], [], [], []
    gate, pose, planes, k = None, t.world[0].copy(), None, 0
    for make, n in segments:
        o = make(planes, 0 if gate is None else gate.count)
        checkers.append(o)
        if gate is None:
            gate = gate_of(o, t.thresholds)
        gate.o = o
        for _ in range(n):
            hint = (pose + t.deltas[k]).astype(F)
            og = ZERO2 if origos is None else origos[k]
            pose, cov = o.match(hint, t.scans[k], og)
            go = bool(gate.walk(pose[None, :])[0])
            if go:
                o.update_by_scan(pose, t.scans[k], og)
                o.on_map_updated()
            poses.append(pose.copy())
            covs.append(cov.copy())
            flags.append(go)
            k += 1
        planes = levels_of(o, o.n_levels)
        ends.append(planes)
    return dict(poses=np.array(poses), covs=np.array(covs), flags=np.array(flags), ends=ends, checkers=checkers, gate=gate)


def segments_for(pyoracle, kind, m, name):
    """the two segments of a case: the map's own checker in the old frame, then (name given) the moved checker"""
    first = (lambda planes, applied: old_checker(pyoracle, kind, m), SPLIT)
    if name is None:
        return [(first[0], N_SCANS)]
    return [first, (lambda planes, applied: moved(pyoracle, kind, m, name, planes, applied), N_SCANS - SPLIT)]


def case_conditions(r, t, what):
    """the conditions of a trajectory, asserted (Checker.match has asserted that the reference defines every match already)"""
    f = r["flags"]
    assert np.isfinite(r["poses"]).all() and np.isfinite(r["covs"]).all(), what
    for seg in (f[:SPLIT], f[SPLIT:]):
        assert seg.sum() >= 2 and (~seg).sum() >= 2, (what, "the gate must both integrate and reject two scans in each half", f.astype(int))
    # the first scan after the move is not forced: no entry gets a force flag, and where the reference keeps track it is the
    # pose the gate carried that rejects it (a gate that had lost it -- FLT_MAX: everything passes -- would decide otherwise)
    err = np.linalg.norm((r["poses"] - t.world)[1:, :2], axis=1) / (t.thresholds[0] / GATE_CELLS)
    lost = bool((err > 5.0).any())   # three gate thresholds: a drift stays below, a jump is tens of cells and more
    assert lost == ((what[0], what[1]) in LOSES_TRACK), (what, "cells off the line", np.round(err, 2))
    if not lost:
        assert not f[SPLIT], (what, "scan 4 must be one that the carried gate rejects", f.astype(int))
    for g in r["checkers"]:
        assert g.guard.undefined_reads() == 0, what


def run_case(pyoracle, kind, m, name, origos=False, line=None):
    """the composed loop of a case (name None: no move), its conditions asserted; cached.  The checkers are closed, their planes kept"""
    key = ("run", kind, m.id, name, origos, line)
    if key not in _cache:
        t = raw_trajectory(pyoracle, kind, m) if origos == RAW else trajectory(pyoracle, m, line)
        r = composed_loop(segments_for(pyoracle, kind, m, name), t, origos=t.origos if origos else None)
        case_conditions(r, t, (m.id, name, kind))
        r["gate_last"], r["gate_count"] = r["gate"].last.copy(), r["gate"].count
        for o in r.pop("checkers"):
            o.close()
        del r["gate"]
        _cache[key] = r
    return _cache[key]


def search_lines(pyoracle, m, xs=range(40, 221, 10), ys=range(68, 83, 2)):
    """-> the first line (as LINES holds it) of the deep map that meets run_case's conditions under every move of MOVES, with and
    without origos (run on the CPU when a generator changes; the result is recorded in LINES)"""
    for y in ys:
        for x in xs:
            line = ((float(x), float(y), 0.1), (1.0, 0.0))
            try:
                for name in MOVES:
                    for og in (False, True):
                        run_case(pyoracle, "ho", m, name, og, line)
                return line
            except AssertionError:
                continue
    return None


# ---- given poses: the plain and the gated device-side update --------------------------------------------------------------------------------
def posed_case(pyoracle, kind, m, name, gated, origos=False):
    """the device-side updates at GIVEN poses (the composed loop's): every level sees the scan itself (Oracle.build_map), all
    eight scans (gated False) or those a Gate carried across the move lets through -> dict(poses, flags [8], planes before
    the move, moved [(lo, stamps)] = shifted_levels of them, end = the moved checker's planes after the second half,
    index = the update index of every level at the end, gate_last, gate_count, box_first / box_old / box_new per level)"""
    key = ("posed", kind, m.id, name, gated, origos)
    if key in _cache:
        return _cache[key]
    t = trajectory(pyoracle, m)
    poses = run_case(pyoracle, "ho", m, name)["poses"].copy()
    if (m.id, name) in LOSES_TRACK:   # the loop's poses are off the map there and an update at them marks nothing: the line's own
        poses[SPLIT:] = t.world[SPLIT:]
    a = old_checker(pyoracle, kind, m)
    gate = Gate(a, t.thresholds)
    f1 = gate.walk(poses[:SPLIT]) if gated else np.ones(SPLIT, bool)

    def apply(o, ks):
        for k in ks:
            o.build_map(poses[k:k + 1], [t.scans[k]], t.origos[k] if origos else ZERO2)

    first = levels_of(a, m.levels)
    apply(a, [k for k in range(SPLIT) if f1[k]])
    before = levels_of(a, m.levels)
    _, _, d0, _ = case_plan(m, name)
    b = moved(pyoracle, kind, m, name, before, int(f1.sum()))
    gate.o = b
    f2 = gate.walk(poses[SPLIT:]) if gated else np.ones(N_SCANS - SPLIT, bool)
    apply(b, [SPLIT + k for k in range(N_SCANS - SPLIT) if f2[k]])
    flags = np.concatenate([f1, f2])
    apply(a, [SPLIT + k for k in range(N_SCANS - SPLIT) if f2[k]])   # the same second half without a move: its cells in OLD coordinates
    unmoved_end = levels_of(a, m.levels)
    a.close()
    if gated:
        for seg in (f1, f2):
            assert seg.sum() >= 2 and (~seg).sum() >= 2, (m.id, name, flags.astype(int))
        assert not f2[0], (m.id, name, flags.astype(int))
    shifted, end = sc.shifted_levels(before, d0), levels_of(b, m.levels)
    # (index: lastUpdateIndex starts at -1 and counts every update, an empty one too)
    r = dict(poses=poses, flags=flags, before=before, moved=shifted, end=end, index=int(flags.sum()) - 1,
             gate_last=gate.last.copy(), gate_count=gate.count,
             box_first=[changed_box(x, y) for x, y in zip(first, before)],      # the first half's cells, old coordinates
             box_old=[changed_box(x, y) for x, y in zip(before, unmoved_end)],  # the second half's cells, old coordinates
             box_new=[changed_box(x, y) for x, y in zip(shifted, end)])         # the second half's cells, new coordinates
    assert b.guard.undefined_reads() == 0
    b.close()
    _cache[key] = r
    return r


def changed_box(before, after):
    """the smallest box x0, y0, x1, y1 around the cells whose log-odds or stamps differ ([0, 0, -1, -1]: none)"""
    (lo0, st0), (lo1, st1) = before, after
    ys, xs = np.nonzero((lo0.view(np.uint32) != lo1.view(np.uint32)) | (st0 != st1))
    return [0, 0, -1, -1] if len(xs) == 0 else [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())]


def union_box(a, b):
    if a[2] < a[0]:
        return list(b)
    if b[2] < b[0]:
        return list(a)
    return [min(a[0], b[0]), min(a[1], b[1]), max(a[2], b[2]), max(a[3], b[3])]


def shifted_box(box, d, dims):
    """a box moved by d = (dx, dy) cells and cut to a level of dims = (sx, sy)"""
    if box[2] < box[0]:
        return [0, 0, -1, -1]
    x0, y0, x1, y1 = max(box[0] + d[0], 0), max(box[1] + d[1], 0), min(box[2] + d[0], dims[0] - 1), min(box[3] + d[1], dims[1] - 1)
    return [x0, y0, x1, y1] if x1 >= x0 and y1 >= y0 else [0, 0, -1, -1]


# ---- the readers ------------------------------------------------------------------------------------------------------------------------
SCORE_LENS = (0, 1, 63, 64, 65, 200)
WINDOW_HALF, WINDOW_LENS = (3, 2, 1), (65, 200)
N_STATES, N_RAYS, N_RANGE_SCANS = 24, 200, 5
RELOC_HALF, RELOC_K = (2, 2, 1), 4


def reader_checker(pyoracle, kind, m, name):
    """the shared moved checker of the readers (nobody changes it)"""
    key = ("reader", kind, m.id, name)
    if key not in _cache:
        _cache[key] = moved(pyoracle, kind, m, name)
    return _cache[key]


def unmoved_checker(pyoracle, kind, m):
    """what a move that silently did nothing would leave: the OLD start and the UNSHIFTED planes"""
    return m.checker(pyoracle, kind)


def reader_inputs(pyoracle, m, name):
    """what the readers are asked on the moved map, none of it taken from a result: the map's start pose and scan, score
    hypotheses (a cloud around the start pose and two far poses per scan length), map-frame states per level, rays on the
    moved level's own metadata, five LaserScans of 200 ranges"""
    key = ("inputs", m.id, name)
    if key in _cache:
        return _cache[key]
    o = reader_checker(pyoracle, "ho", m, name)
    centre, pts = m.scan(pyoracle)
    rng = np.random.default_rng(2203)
    res = m.resolution
    poses, scans = [], []
    for n in SCORE_LENS:
        cloud = (centre.astype(np.float64) + rng.uniform(-1, 1, (4, 3)) * [2 * res, 2 * res, 0.05]).astype(F)
        far = np.stack([o.world_coords_pose(0, p) for p in F([[-50.0, 3.0, 0.1], [1e6, 1e6, 0.0]])])
        for p in np.concatenate([centre[None], cloud, far]).astype(F):
            poses.append(p)
            scans.append(pts[:n])
    states, rays = [], []
    for lvl in range(m.levels):
        c = o.map_coords_pose(lvl, centre).astype(np.float64)
        states.append((c + rng.uniform(-1, 1, (N_STATES, 3)) * [1.5, 1.5, 0.1]).astype(F))
        grid, meta = o.occupancy_grid(lvl), cast_cases.metadata(o, lvl)
        rays.append(cast_cases.mixed_rays(grid, meta, N_RAYS, 300 + lvl))
    # LaserScans: the scan's own end points as ranges and bearings would need the node's trigonometry; ranges of a fan instead
    n = MAX_BEAMS
    a0, inc = -2.3, float(F(4.6 / (n - 1)))
    r = np.hypot(pts[:, 0], pts[:, 1]).astype(np.float64) * res
    ranges = (r[None, :] * rng.uniform(0.97, 1.03, (N_RANGE_SCANS, n))).astype(F)
    ranges[:, 7::53] = np.inf
    ranges[1, ::9] = 0.0   # below range_min: dropped
    starts = (centre.astype(np.float64) + rng.uniform(-1, 1, (N_RANGE_SCANS, 3)) * [0.6 * res, 0.6 * res, 0.03]).astype(F)
    out = dict(centre=centre, pts=pts, poses=np.stack(poses), scans=scans, states=states, rays=rays, ranges=ranges, starts=starts,
               laser=(a0, inc, float(F(0.5 * res)), float(F(400.0 * res))), step=egc.window_step(m))
    _cache[key] = out
    return out


def expected_readers(pyoracle, kind, m, name, o=None, tag=None):
    """the checker's answers to reader_inputs on the moved map (o: another checker to ask instead, for the pin that the move
    matters, cached under the caller's tag).  Per level where it applies.  Every match among them is one the reference defines (Checker.match asserts it)"""
    assert (o is None) == (tag is None)
    key = ("expected", kind, m.id, name, tag)
    if key in _cache:
        return _cache[key]
    import test_gpu_score_batch as tsb
    import test_gpu_window as tw
    import window_cases
    from test_window_model import reference_relocalize
    q = reader_inputs(pyoracle, m, name)
    own = o is None
    o = reader_checker(pyoracle, kind, m, name) if own else o
    out = dict(score=[], window=[], states=[], rays=[], cov=[])
    wposes = window_cases.window_poses(q["centre"], q["step"], WINDOW_HALF)
    for lvl in range(m.levels):
        out["score"].append(tsb.reference(o, lvl, q["poses"], q["scans"]))
        out["window"].append({n: tw.oracle_window(o, lvl, wposes, q["pts"][:n]) for n in WINDOW_LENS})
        pl = q["pts"] * F(1.0 / 2 ** lvl)
        out["states"].append((o.likelihood_states(lvl, q["states"][lvl], pl), o.residual_states(lvl, q["states"][lvl], pl)))
        out["cov"].append(o.covariance_for_poses(lvl, q["states"][lvl], pl))
        grid, meta = o.occupancy_grid(lvl), cast_cases.metadata(o, lvl)
        out["rays"].append(cast_cases.expected_rays(kind, grid, meta, *q["rays"][lvl]))
    if own:
        a0, inc, rmin, rmax = q["laser"]
        conts = [o.laser_scan_to_container(r, a0, inc, rmin, rmax, o.scale_to_map()) for r in q["ranges"]]
        out["counts"] = np.array([len(c) for c in conts], np.int32)
        out["ranges_match"] = [o.match(s, c) for s, c in zip(q["starts"], conts)]
        out["conts"] = conts
        lvl = m.levels - 1
        cell = o.level_info(lvl)[2]
        out["reloc_level"], out["reloc_step"] = lvl, (float(cell), float(cell), 0.05)
        u0 = o.guard.undefined_reads()
        args = (None, q["centre"], q["pts"], out["reloc_step"], RELOC_HALF, RELOC_K)
        out["reloc"] = reference_relocalize(o.guard, *args, search_level=lvl)   # the restatement first: it counts, the reference dies
        assert o.guard.undefined_reads() == u0, (m.id, name, "the reference does not define this relocalisation")
        if o.o is not o.guard:
            out["reloc"] = reference_relocalize(o.o, *args, search_level=lvl)
    _cache[key] = out
    return out
