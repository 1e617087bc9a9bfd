"""The movement gate of HectorSlamProcessor::update on the device (hsm_update_by_scans_device_gated) and the whole per-scan loop
of the reference for a log of scans queued in one call (hsm_slam_scans_device), on the MI355X.  The bar is BIT-EXACT against the
CPU checkers ("hr": the unmodified reference, "ho": the restatement): every decision, every pose, the covariance of every
non-empty scan, the log-odds / update-index / probability planes of every level, the counters.

Inputs: a 512 x 512 (once 500 x 360) 3-level map, the first 24 of the 1081-beam build scans of the 16 m x 12 m room; the hint of
scan t + 1 is the last pose plus build_poses[t + 1] - build_poses[t].  Two threshold pairs: the reference's defaults (0.4, 0.13)
and (1.0, 0.3).  Every test that runs a gate first asserts that the reference both integrates and rejects at least 6 of the
24 scans, and that "ho" met no undefined read: a run that accepts everything would prove nothing about the gate.

What a forced scan (map_without_matching) does to the coarse levels -- they integrate the containers of the last MATCHED scan --
is the reference's HectorSlamProcessor::update and is held by the whole-loop tests against `proc_update`; the gated update at
GIVEN poses runs no matcher, every level sees the scan itself as in hsm_update_by_scans_device, and its yardstick is
`build_map` over the scans a Python loop over the checker's predicate (or the force flag) lets through.

Nothing here provokes a device fault."""
import numpy as np
import pytest

from conftest import bits
import support
from support import capi, dev, new_context, pack, stream_ptr

pytestmark = pytest.mark.gpu

RES = 0.05
HSM_ERR_INVALID = -1
ZERO2 = np.zeros(2, np.float32)
LEVELS = 3
N = 24
GEOMS = {"square": (512, 512), "rect": (500, 360)}
THRESHOLDS = {"default": (0.4, 0.13), "wide": (1.0, 0.3)}
FLT_MAX = np.finfo(np.float32).max


@pytest.fixture(scope="module")
def traj():
    from hector_slam_amd import synth
    sc = synth.make_scene(n_beams=1081, map_size=512, levels=LEVELS, resolution=RES, n_build=64, n_query=8, room=(16.0, 12.0), seed=2024)
    sc.poses = np.ascontiguousarray(sc.build_poses[:N], np.float32)
    sc.scans = [np.ascontiguousarray(s, np.float32) for s in sc.build_scans[:N]]
    sc.deltas = np.zeros((N, 3), np.float32)
    sc.deltas[1:] = sc.poses[1:] - sc.poses[:-1]  # fp32 differences; hint_k = pose_(k-1) + delta_k in fp32
    return sc


def new_ctx(capi, geom="square", layout="quad"):
    sx, sy = GEOMS[geom]
    return new_context(capi, RES, sx, sy, LEVELS, layout=layout)


def new_refs(oracle_mod, geom="square"):
    sx, sy = GEOMS[geom]
    return support.new_refs(oracle_mod, RES, sx, sy, LEVELS)


def host_path(capi, g, poses, scans, origo=ZERO2):
    """the parent path: per scan hsm_retain_scan (what matchData leaves for the coarse levels) + hsm_update_by_scan"""
    o = np.ascontiguousarray(origo, np.float32)
    for p, s in zip(np.asarray(poses, np.float32).reshape(-1, 3), scans):
        a = np.ascontiguousarray(s, np.float32).reshape(-1, 2)
        capi._check(g._lib.hsm_retain_scan(g._h, a.ctypes.data if a.size else None, a.shape[0], o), "hsm_retain_scan")
        g.updateByScan(a, p, o)


class Gate:
    """the Python loop over the checker's predicate: lastMapUpdatePose and the count, carried across calls"""

    def __init__(self, checker, thresholds):
        self.o, self.thr, self.last, self.count = checker, thresholds, np.float32([FLT_MAX] * 3), 0

    def walk(self, poses, force=None):
        flags = []
        for k, p in enumerate(np.asarray(poses, np.float32).reshape(-1, 3)):
            go = self.o.pose_difference_larger_than(p, self.last, self.thr[0], self.thr[1]) or bool(force is not None and force[k])
            flags.append(go)
            if go:
                self.last, self.count = p.copy(), self.count + 1
        return np.array(flags)


def gated(g, poses, scans, force=None, stream=None, thresholds=None):
    """hsm_update_by_scans_device_gated on torch buffers -> (the buffers, which must outlive the update; d_out_applied)"""
    import torch
    s = stream or torch.cuda.current_stream()
    if thresholds is not None:
        g.set_update_gate(*thresholds)
    with torch.cuda.stream(s):
        pts, offs = pack(scans)
        keep = [dev(np.asarray(poses, np.float32).reshape(-1, 3)), dev(pts if len(pts) else np.zeros((1, 2), np.float32)), dev(offs),
                None if force is None else dev(np.asarray(force, np.uint8)), torch.full((len(scans),), -7, dtype=torch.int32, device="cuda:0")]
        g.update_by_scans_device_gated(len(scans), keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), 0, 1081, None,
                                       0 if force is None else keep[3].data_ptr(), keep[4].data_ptr(), s.cuda_stream)
    return keep, keep[4]


def planes(g):
    return [g.download_level(l) + (g.download_prob(l),) for l in range(LEVELS)]


def assert_same_as_refs(oracle_mod, g, refs, what):
    for kind, o in refs.items():
        for lvl in range(LEVELS):
            (lo_g, ui_g), (lo_o, ui_o) = g.download_level(lvl), o.download_level(lvl)
            assert np.array_equal(ui_g, ui_o), (what, kind, lvl, int((ui_g != ui_o).sum()))
            assert np.array_equal(bits(lo_g), bits(lo_o)), (what, kind, lvl, int((bits(lo_g) != bits(lo_o)).sum()))
            _, prob = oracle_mod.libm_expf(lo_o.reshape(-1), "ho")
            assert np.array_equal(bits(g.download_prob(lvl)).reshape(-1), bits(prob)), (what, kind, lvl)
        if kind == "ho":
            assert o.undefined_reads() == 0, (what, o.undefined_reads())
    for lvl in range(LEVELS):
        assert g.debug_marks_nonzero(lvl) == (0, 0), (what, lvl)


def assert_same_as_ctx(g, h, what):
    for lvl, (a, b) in enumerate(zip(planes(g), planes(h))):
        assert np.array_equal(a[1], b[1]), (what, lvl, "update index", int((a[1] != b[1]).sum()))
        assert np.array_equal(bits(a[0]), bits(b[0])), (what, lvl, "log odds", int((bits(a[0]) != bits(b[0])).sum()))
        assert np.array_equal(bits(a[2]), bits(b[2])), (what, lvl, "probability")
        assert g.getUpdateIndex(lvl) == h.getUpdateIndex(lvl), (what, lvl, g.getUpdateIndex(lvl), h.getUpdateIndex(lvl))


def assert_same_matches(g, h, sc, what):
    pts, offs = pack(sc.query_scans)
    (pg, cg), (ph, ch) = g.match_batch(sc.query_init, pts, offs), h.match_batch(sc.query_init, pts, offs)
    assert np.isfinite(ph).all(), what
    assert np.array_equal(bits(pg), bits(ph)) and np.array_equal(bits(cg), bits(ch)), (what, int((bits(pg) != bits(ph)).sum()))


def assert_gate_is_exercised(flags, what):
    assert flags.sum() >= 6 and (~flags).sum() >= 6, (what, "the reference must both integrate and reject at least 6 scans", flags.astype(int))


def selected(seq, flags):
    return [x for x, f in zip(seq, flags) if f]


# ---- 1: the gated update at given poses ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["quad", "plane"])
@pytest.mark.parametrize("thr", list(THRESHOLDS))
def test_gated_update_at_given_poses(capi, oracle_mod, traj, thr, layout):
    sc, t = traj, THRESHOLDS[thr]
    geom = "rect" if (thr, layout) == ("wide", "plane") else "square"
    g, h, refs = new_ctx(capi, geom, layout), new_ctx(capi, geom, layout), new_refs(oracle_mod, geom)
    flags = None
    for kind, o in refs.items():
        f = Gate(o, t).walk(sc.poses)
        assert flags is None or np.array_equal(f, flags), "the two checkers disagree on a decision"
        flags = f
        o.build_map(sc.poses[flags], selected(sc.scans, flags))
    assert_gate_is_exercised(flags, thr)
    keep, applied = gated(g, sc.poses, sc.scans, thresholds=t)
    # the host path with a host gate (the parent's way)
    last = np.float32([FLT_MAX] * 3)
    for p, s in zip(sc.poses, sc.scans):
        if capi.pose_difference_larger_than(p, last, t[0], t[1]):
            host_path(capi, h, p[None, :], [s])
            last = p.copy()
    g.synchronize()
    assert np.array_equal(applied.cpu().numpy(), flags.astype(np.int32)), (applied.cpu().numpy(), flags.astype(int))
    assert_same_as_refs(oracle_mod, g, refs, thr)
    assert_same_as_ctx(g, h, thr)
    for lvl in range(LEVELS):
        assert g.getUpdateIndex(lvl) == int(flags.sum()) - 1  # lastUpdateIndex starts at -1
    assert_same_matches(g, h, sc, thr)
    del keep
    g.close()
    h.close()


# ---- 2: the state persists on the device and folds into the host's counters -----------------------------------------------------------
def test_state_persists_and_folds(capi, oracle_mod, traj):
    sc, t = traj, THRESHOLDS["default"]
    one, two, mix, refs = new_ctx(capi), new_ctx(capi), new_ctx(capi), new_refs(oracle_mod)
    gate = Gate(refs["ho"], t)
    flags = gate.walk(sc.poses)
    assert_gate_is_exercised(flags, "default")
    keep = [gated(one, sc.poses, sc.scans, thresholds=t), gated(two, sc.poses[:12], sc.scans[:12], thresholds=t),
            gated(two, sc.poses[12:], sc.scans[12:])]
    one.synchronize()
    two.synchronize()
    assert np.array_equal(np.concatenate([keep[1][1].cpu().numpy(), keep[2][1].cpu().numpy()]), flags.astype(np.int32))
    assert_same_as_ctx(two, one, "12 + 12 scans against 24")
    pose, total = two.update_gate_state()
    assert np.array_equal(bits(pose), bits(gate.last)) and total == gate.count == int(flags.sum())

    # gated -> host updateByScan -> ungated device update -> gated, queued back to back; the same sequence on the checkers
    t = THRESHOLDS["wide"]
    gates = {kind: Gate(o, t) for kind, o in refs.items()}
    want = []
    for kind, o in refs.items():
        gk = gates[kind]
        f1 = gk.walk(sc.poses[:8])
        o.build_map(sc.poses[:8][f1], selected(sc.scans[:8], f1))
        o.build_map(sc.poses[8:9], sc.scans[8:9])     # host update: no gate, lastMapUpdatePose untouched
        o.build_map(sc.poses[9:12], sc.scans[9:12])   # ungated device update
        f2 = gk.walk(sc.poses[12:])
        o.build_map(sc.poses[12:][f2], selected(sc.scans[12:], f2))
        want = np.concatenate([f1, f2])
    assert (~want).sum() >= 6 and want.sum() >= 6
    k1 = gated(mix, sc.poses[:8], sc.scans[:8], thresholds=t)
    host_path(capi, mix, sc.poses[8:9], sc.scans[8:9])
    pts, offs = pack(sc.scans[9:12])
    d = [dev(sc.poses[9:12]), dev(pts), dev(offs)]
    mix.update_by_scans_device(3, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 0, 1081, None, stream_ptr())
    k2 = gated(mix, sc.poses[12:], sc.scans[12:])
    mix.synchronize()
    assert np.array_equal(np.concatenate([k1[1].cpu().numpy(), k2[1].cpu().numpy()]), want.astype(np.int32))
    assert_same_as_refs(oracle_mod, mix, refs, "mixed sequence")
    pose, total = mix.update_gate_state()
    assert np.array_equal(bits(pose), bits(gates["ho"].last)) and total == gates["ho"].count
    for lvl in range(LEVELS):
        assert mix.getUpdateIndex(lvl) == int(want.sum()) + 4 - 1

    # after reset() the first scan is integrated again, whatever its pose
    mix.reset()
    pose, _ = mix.update_gate_state()
    assert np.array_equal(bits(pose), bits(np.float32([FLT_MAX] * 3)))
    k3 = gated(mix, sc.poses[23:24], sc.scans[23:24])
    mix.synchronize()
    assert k3[1].cpu().numpy().tolist() == [1]
    for o in refs.values():
        o.reset()
        o.build_map(sc.poses[23:24], sc.scans[23:24])
    for kind, o in refs.items():  # (reset keeps the update counters: compare the cells, not the stamps)
        for lvl in range(LEVELS):
            assert np.array_equal(bits(mix.download_level(lvl)[0]), bits(o.download_level(lvl)[0])), ("after reset", kind, lvl)
    del keep, k1, k2, k3, d
    for m in (one, two, mix):
        m.close()


# ---- 3: edge cases of the gate ----------------------------------------------------------------------------------------------------------
def test_edge_cases_of_the_gate(capi, oracle_mod, traj):
    sc, t = traj, THRESHOLDS["wide"]  # (at the defaults scan 7 passes the gate by itself)
    g, refs = new_ctx(capi), new_refs(oracle_mod)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    poses = sc.poses.copy()
    scans = list(sc.scans)
    force = np.zeros(N, np.uint8)
    poses[3] = [nan, nan, nan]      # never "larger": not integrated, no counter advances
    poses[5] = [inf, 1.0, 0.5]      # the distance is infinite: integrated, changes no cell, the counters advance
    force[7] = 1                    # map_without_matching: integrated whatever the gate says
    scans[10] = np.zeros((0, 2), np.float32)  # an empty scan at an accepted pose counts as an update
    flags = None
    for kind, o in refs.items():
        flags = Gate(o, t).walk(poses, force)
        o.build_map(poses[flags], selected(scans, flags))
    assert not flags[3] and flags[5] and flags[7] and flags[10], flags.astype(int)
    assert not Gate(refs["ho"], t).walk(poses)[7], "scan 7 would pass the gate anyway: forcing it shows nothing"
    assert_gate_is_exercised(flags, "edge cases")
    keep, applied = gated(g, poses[:5], scans[:5], force[:5], thresholds=t)
    g.synchronize()
    idx5 = g.getUpdateIndex(0)
    before = planes(g)
    keep2, applied2 = gated(g, poses[5:6], scans[5:6], force[5:6])
    g.synchronize()
    assert applied2.cpu().numpy().tolist() == [1] and g.getUpdateIndex(0) == idx5 + 1
    for lvl, (a, b) in enumerate(zip(before, planes(g))):
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b)), ("an infinite pose changed a plane", lvl)
    keep3, applied3 = gated(g, poses[6:], scans[6:], force[6:])
    g.synchronize()
    got = np.concatenate([applied.cpu().numpy(), applied2.cpu().numpy(), applied3.cpu().numpy()])
    assert np.array_equal(got, flags.astype(np.int32)), (got, flags.astype(int))
    assert_same_as_refs(oracle_mod, g, refs, "edge cases")
    for lvl in range(LEVELS):
        assert g.getUpdateIndex(lvl) == int(flags.sum()) - 1
    del keep, keep2, keep3
    g.close()


# ---- 4: the key generation wraps inside a gated call ------------------------------------------------------------------------------------
def test_key_generation_wrap_inside_a_gated_call(capi, oracle_mod, traj):
    sc, t = traj, THRESHOLDS["default"]
    g, refs = new_ctx(capi, "rect"), new_refs(oracle_mod, "rect")
    for lvl in range(LEVELS):
        capi._check(g._lib.hsm_debug_set_update_serial(g._h, lvl, 4095 - 5), "set serial")  # 5 below the wrap
    flags = None
    for o in refs.values():
        flags = Gate(o, t).walk(sc.poses)
        o.build_map(sc.poses[flags], selected(sc.scans, flags))
    assert_gate_is_exercised(flags, "wrap")
    assert flags[:5].any() and flags[5:].any()  # scans are integrated on both sides of the wrap
    keep, applied = gated(g, sc.poses, sc.scans, thresholds=t)
    g.synchronize()
    assert np.array_equal(applied.cpu().numpy(), flags.astype(np.int32))
    assert_same_as_refs(oracle_mod, g, refs, "across the wrap")
    del keep
    g.close()


# ---- 5: the whole loop --------------------------------------------------------------------------------------------------------------------
def reference_loop(o, sc, thresholds, force=None, scans=None, deltas=True):
    """HectorSlamProcessor::update x 24 on a checker -> (poses, covs, flags)"""
    scans = sc.scans if scans is None else scans
    o.proc_set_thresholds(*thresholds)
    gate = Gate(o, thresholds)
    poses, covs, flags = [], [], []
    pose = sc.poses[0].copy()
    for k in range(N):
        hint = (pose + sc.deltas[k]).astype(np.float32) if deltas else pose
        forced = bool(force is not None and force[k])
        o.proc_update(scans[k], hint, ZERO2, forced)
        pose, cov = o.proc_last_pose()
        flags.append(gate.walk(pose[None, :], [forced])[0])
        poses.append(pose.copy())
        covs.append(cov.copy())
    return np.array(poses), np.array(covs), np.array(flags)


def device_loop(g, sc, thresholds, splits=(N,), force=None, scans=None, deltas=True):
    import torch
    scans = sc.scans if scans is None else scans
    s = torch.cuda.Stream()
    g.set_update_gate(*thresholds)
    with torch.cuda.stream(s):
        pts, offs = pack(scans)
        d = {"start": dev(sc.poses[0]), "deltas": dev(sc.deltas), "pts": dev(pts), "offs": dev(offs),
             "force": None if force is None else dev(np.asarray(force, np.uint8)),
             "pose": torch.full((N, 3), -777.0, device="cuda:0"), "cov": torch.full((N, 9), -777.0, device="cuda:0"),
             "applied": torch.full((N,), -7, dtype=torch.int32, device="cuda:0")}
        k0 = 0
        for n in splits:
            g.slam_scans_device(n, d["start"].data_ptr() if k0 == 0 else d["pose"][k0 - 1].data_ptr(),
                                d["deltas"][k0:].data_ptr() if deltas else 0, d["pts"].data_ptr(), d["offs"][k0:].data_ptr(), 1081, None,
                                0 if force is None else d["force"][k0:].data_ptr(), d["pose"][k0:].data_ptr(), d["cov"][k0:].data_ptr(),
                                d["applied"][k0:].data_ptr(), s.cuda_stream)
            k0 += n
    s.synchronize()  # the one wait: the caller's stream is ordered behind everything the call queued
    return d["pose"].cpu().numpy(), d["cov"].cpu().numpy(), d["applied"].cpu().numpy(), d


def check_loop(capi, oracle_mod, sc, thresholds, what, geom="square", needs_both=True, python_loop=False, **kw):
    g, refs = new_ctx(capi, geom), new_refs(oracle_mod, geom)
    dkw = dict(kw)
    splits = dkw.pop("splits", (N,))
    poses, covs, applied, keep = device_loop(g, sc, thresholds, splits, **dkw)
    scans = kw.get("scans") or sc.scans
    for kind, o in refs.items():
        rp, rc, rf = reference_loop(o, sc, thresholds, **dkw)
        if needs_both:
            assert_gate_is_exercised(rf, (what, kind))
        assert np.linalg.norm(rp[-1, :2] - sc.poses[-1, :2]) < 0.01, (what, kind, "the reference lost track: the inputs drifted")
        assert np.array_equal(applied, rf.astype(np.int32)), (what, kind, applied, rf.astype(int))
        assert np.array_equal(bits(poses), bits(rp)), (what, kind, np.nonzero((bits(poses) != bits(rp)).any(axis=1))[0])
        for k in range(N):
            if len(scans[k]) > 0:
                assert np.array_equal(bits(covs[k]), bits(rc[k])), (what, kind, "covariance of scan", k)
    g.synchronize()
    assert_same_as_refs(oracle_mod, g, refs, what)
    if python_loop:  # the host loop of the Python glue on a second context
        sx, sy = GEOMS[geom]
        proc = capi.HectorSlamProcessor(RES, sx, sy, (0.5, 0.5), LEVELS)
        proc.setUpdateFactorFree(0.4)
        proc.setUpdateFactorOccupied(0.9)
        proc.setMapUpdateMinDistDiff(thresholds[0])
        proc.setMapUpdateMinAngleDiff(thresholds[1])
        pose = sc.poses[0].copy()
        force = kw.get("force")
        for k in range(N):
            hint = (pose + sc.deltas[k]).astype(np.float32) if kw.get("deltas", True) else pose
            proc.update(scans[k], hint, bool(force is not None and force[k]))
            pose = proc.getLastScanMatchPose().copy()
            assert np.array_equal(bits(pose), bits(poses[k])), (what, "python host loop, scan", k)
        assert_same_as_ctx(g, proc.mapRep, what)
        lp, total = g.update_gate_state()
        assert np.array_equal(bits(lp), bits(proc.lastMapUpdatePose)) and total == int(applied.sum())
        proc.mapRep.close()
    del keep
    g.close()


@pytest.mark.parametrize("thr", list(THRESHOLDS))
def test_whole_loop_is_bit_identical(capi, oracle_mod, traj, thr):
    check_loop(capi, oracle_mod, traj, THRESHOLDS[thr], thr, python_loop=True)


def test_whole_loop_split_in_two_calls(capi, oracle_mod, traj):
    check_loop(capi, oracle_mod, traj, THRESHOLDS["default"], "10 + 14", geom="rect", splits=(10, 14))


def test_whole_loop_with_a_forced_and_an_empty_scan(capi, oracle_mod, traj):
    force = np.zeros(N, np.uint8)
    force[7] = 1
    scans = list(traj.scans)
    scans[13] = np.zeros((0, 2), np.float32)
    # (at the defaults scan 7 passes the gate by itself; at (1.0, 0.3) the reference rejects it unless it is forced)
    check_loop(capi, oracle_mod, traj, THRESHOLDS["wide"], "forced + empty", python_loop=True, force=force, scans=scans)


def test_whole_loop_without_deltas(capi, oracle_mod, traj):
    check_loop(capi, oracle_mod, traj, THRESHOLDS["default"], "no deltas", deltas=False)


# ---- 6: capture ------------------------------------------------------------------------------------------------------------------------------
def test_both_entries_are_refused_during_capture(capi, traj):
    import torch
    sc = traj
    g = new_ctx(capi)
    keep, _ = gated(g, sc.poses[:4], sc.scans[:4], thresholds=THRESHOLDS["default"])
    g.synchronize()
    before, idx, state = planes(g), g.getUpdateIndex(0), g.update_gate_state()
    pts, offs = pack(sc.scans[4:8])
    d = [dev(sc.poses[4:8]), dev(pts), dev(offs), torch.zeros((4, 3), device="cuda:0"), torch.zeros(4, dtype=torch.int32, device="cuda:0")]
    s = torch.cuda.Stream()
    x = torch.zeros(8, device="cuda:0")
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        x.add_(1.0)
        for call in (lambda: g.update_by_scans_device_gated(4, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 0, 1081, None, 0,
                                                            d[4].data_ptr(), s.cuda_stream),
                     lambda: g.slam_scans_device(4, d[0].data_ptr(), 0, d[1].data_ptr(), d[2].data_ptr(), 1081, None, 0, d[3].data_ptr(), 0,
                                                 d[4].data_ptr(), s.cuda_stream)):
            with pytest.raises(capi.HsmError) as e:
                call()
            assert f"({HSM_ERR_INVALID})" in str(e.value) and "captur" in str(e.value), str(e.value)
        x.add_(1.0)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert x.cpu().numpy().tolist() == [2.0] * 8  # the capture ended normally
    g.synchronize()
    assert g.getUpdateIndex(0) == idx
    after = g.update_gate_state()
    assert np.array_equal(bits(after[0]), bits(state[0])) and after[1] == state[1]
    for a, b in zip(before, planes(g)):
        assert all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in zip(a, b)), "a refused call changed the map"
    g.slam_scans_device(4, d[0].data_ptr(), 0, d[1].data_ptr(), d[2].data_ptr(), 1081, None, 0, d[3].data_ptr(), 0, d[4].data_ptr(), s.cuda_stream)
    s.synchronize()
    g.synchronize()
    assert np.isfinite(d[3].cpu().numpy()).all()
    del keep
    g.close()
