"""The whole HectorSlamProcessor::update loop with one origo per scan (hsm_slam_scans_device_origos) and the one-call raw-log
entry (hsm_slam_ranges_tf_device, host form hsm_slam_ranges_tf: raw ranges and a transform per scan in; poses, covariances,
decisions and the map out), on the MI355X.  The bar is BIT-EXACT: every pose, the covariance of every non-empty scan, every
decision and the log-odds / update-index / probability planes of every level against `proc_update(pts_k, hint_k, origo_k,
force_k)` on the CPU checkers ("hr", "ho"), the containers against the reference node's own projectLaser +
rosPointCloudToDataContainer, and a fixed-mount log against the node's scanCallback.

What a wrong origo would corrupt: the begin cell of every free-space ray of the scan on every level -- and, for a forced scan,
the coarse levels must take the origo of the last MATCHED scan (the retained-origo rule, MapRepMultiMap.h:127,143), level 0 its
own.  The force mask puts forced scans behind matched scans of another origo and one first in the log.

Inputs: tests/origo_cases.py.  Nothing here provokes a device fault."""
import numpy as np
import pytest

from conftest import bits, oracle_kinds
from support import capi, dev, stream_ptr
import origo_cases as oc
from test_gpu_update_scans_origos import assert_same_as_ctx, assert_same_as_refs, new_ctx, pack, planes

pytestmark = pytest.mark.gpu

LEVELS, N = oc.LEVELS, oc.N
HSM_OK, HSM_ERR_INVALID, HSM_ERR_TOO_LARGE = 0, -1, -4
COV0 = -777.0


@pytest.fixture(scope="module")
def traj():
    return oc.trajectory()


@pytest.fixture(scope="module", autouse=True)
def guard(oracle_mod):
    for kind in oracle_kinds():
        oc.assert_the_reference_depends_on_the_origo(kind)


def outputs(n):
    import torch
    return {"pose": torch.full((n, 3), -777.0, device="cuda:0"), "cov": torch.full((n, 9), COV0, device="cuda:0"),
            "applied": torch.full((n,), -7, dtype=torch.int32, device="cuda:0"), "counts": torch.full((n,), -7, dtype=torch.int32, device="cuda:0")}


def device_loop(g, sc, thresholds, origos, splits=(N,), force=None):
    import torch
    s = torch.cuda.Stream()
    g.set_update_gate(*thresholds)
    with torch.cuda.stream(s):
        pts, offs = pack(sc.scans)
        d = {"start": dev(sc.poses[0]), "deltas": dev(sc.deltas), "pts": dev(pts), "offs": dev(offs), "origos": dev(origos),
             "force": None if force is None else dev(force), **outputs(N)}
        k0 = 0
        for n in splits:
            g.slam_scans_device_origos(n, d["start"].data_ptr() if k0 == 0 else d["pose"][k0 - 1].data_ptr(), d["deltas"][k0:].data_ptr(),
                                       d["pts"].data_ptr(), d["offs"][k0:].data_ptr(), 1081, d["origos"][k0:].data_ptr(),
                                       0 if force is None else d["force"][k0:].data_ptr(), d["pose"][k0:].data_ptr(),
                                       d["cov"][k0:].data_ptr(), d["applied"][k0:].data_ptr(), s.cuda_stream)
            k0 += n
    s.synchronize()
    return d["pose"].cpu().numpy(), d["cov"].cpu().numpy(), d["applied"].cpu().numpy(), d


def assert_loop_equals(got, ref, scans, what, force=None):
    """poses, decisions, and the covariance of every non-empty scan.  One exception: a scan forced BEFORE the first matched scan
    of the log repeats a lastScanMatchCov that nothing has written yet -- the reference never initialises that member
    (HectorSlamProcessor.h:147), so "hr" returns whatever its memory holds, a different value every run; the device and "ho"
    give zeros, and that row is compared against "ho" only."""
    (poses, covs, applied), (rp, rc, rf) = got, ref
    assert np.array_equal(applied, rf.astype(np.int32)), (what, applied, rf.astype(int))
    assert np.array_equal(bits(poses), bits(rp)), (what, np.nonzero((bits(poses) != bits(rp)).any(axis=1))[0])
    first_match = 0 if force is None else int(np.argmin(np.asarray(force) != 0))
    for k in range(len(scans)):
        if k < first_match and "hr" in what:
            continue
        if len(scans[k]) > 0:
            assert np.array_equal(bits(covs[k]), bits(rc[k])), (what, "covariance of scan", k)


# ---- 7: the SLAM loop with an origo per scan -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["default", "wide, forced", "wide, forced, 12 + 12"])
def test_slam_loop_with_an_origo_per_scan(capi, oracle_mod, traj, case):
    sc = traj
    t = oc.THRESHOLDS[case.split(",")[0]]
    force = oc.force_mask() if "forced" in case else None
    splits = (12, 12) if "12 + 12" in case else (N,)
    geom = "rect" if case == "default" else "square"
    g, refs = new_ctx(capi, geom), oc.new_refs(oracle_mod, geom)
    poses, covs, applied, keep = device_loop(g, sc, t, sc.origos, splits, force)
    for kind, o in refs.items():
        ref = oc.reference_loop(o, t, sc.scans, sc.origos, sc.poses[0], sc.deltas, force)
        oc.assert_gate_is_exercised(ref[2], (case, kind))
        assert np.linalg.norm(ref[0][-1, :2] - sc.poses[-1, :2]) < 0.01, (case, kind, "the reference lost track: the inputs drifted")
        assert_loop_equals((poses, covs, applied), ref, sc.scans, (case, kind), force)
        if force is not None:
            # the retained-origo rule is in play: each forced scan is integrated, and the last matched scan's origo is another one
            assert ref[2][force.astype(bool)].all() and not force[6] and not force[14]
            assert not np.array_equal(sc.origos[6], sc.origos[7]) and not np.array_equal(sc.origos[14], sc.origos[15])
    g.synchronize()
    assert_same_as_refs(oracle_mod, g, refs, case)
    if force is not None:
        # ... and it shows: with the forced scans' OWN origo on the coarse levels (what the ungated entry does) those levels differ
        h = new_ctx(capi, geom)
        pts, offs = pack(sc.scans)
        d = [dev(poses), dev(pts), dev(offs), dev(sc.origos), dev(applied.astype(np.uint8)), dev(np.zeros(N, np.int32))]
        h.set_update_gate(np.inf, np.inf)  # integrate exactly the scans the loop integrated, every level at the scan's own origo
        h.update_by_scans_device_gated_origos(N, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 0, 1081, d[3].data_ptr(),
                                              d[4].data_ptr(), d[5].data_ptr(), 0)
        h.synchronize()
        a, b = planes(g), planes(h)
        assert np.array_equal(bits(a[0][0]), bits(b[0][0])), "level 0 integrates every scan at its own origo"
        assert all((bits(a[l][0]) != bits(b[l][0])).any() for l in range(1, LEVELS)), "the coarse levels do not show the retained origo"
        del d
        h.close()
    del keep
    g.close()


# ---- 5 (gated and SLAM entries): no behaviour change ----------------------------------------------------------------------------------
@pytest.mark.parametrize("origo", [(3.25, -4.5), None], ids=["one pair", "null"])
@pytest.mark.parametrize("entry", ["gated", "slam"])
def test_equal_origos_give_the_gated_and_slam_parents_bit_for_bit(capi, traj, entry, origo):
    """d_origos filled with one pair X (or NULL) on one context, the parent entry with the host origo X (or NULL) on a twin:
    the same decisions, poses, covariances, gate state, boxes, counters and planes"""
    import torch
    sc, t = traj, oc.THRESHOLDS["wide"]
    force = oc.force_mask()
    g, h = new_ctx(capi, "rect"), new_ctx(capi, "rect")
    for m in (g, h):
        m.set_update_gate(*t)
        for lvl in range(LEVELS):
            m.take_dirty_bbox(lvl)
    s = stream_ptr()
    pts, offs = pack(sc.scans)
    d = {"poses": dev(sc.poses), "start": dev(sc.poses[0]), "deltas": dev(sc.deltas), "pts": dev(pts), "offs": dev(offs), "force": dev(force),
         "origos": None if origo is None else dev(np.tile(np.float32(origo), (N, 1)))}
    d_origos = 0 if origo is None else d["origos"].data_ptr()
    host = None if origo is None else np.float32(origo)
    og, oh = outputs(N), outputs(N)
    if entry == "gated":
        g.update_by_scans_device_gated_origos(N, d["poses"].data_ptr(), d["pts"].data_ptr(), d["offs"].data_ptr(), 0, 1081, d_origos,
                                              d["force"].data_ptr(), og["applied"].data_ptr(), s)
        h.update_by_scans_device_gated(N, d["poses"].data_ptr(), d["pts"].data_ptr(), d["offs"].data_ptr(), 0, 1081, host,
                                       d["force"].data_ptr(), oh["applied"].data_ptr(), s)
    else:
        g.slam_scans_device_origos(N, d["start"].data_ptr(), d["deltas"].data_ptr(), d["pts"].data_ptr(), d["offs"].data_ptr(), 1081, d_origos,
                                   d["force"].data_ptr(), og["pose"].data_ptr(), og["cov"].data_ptr(), og["applied"].data_ptr(), s)
        h.slam_scans_device(N, d["start"].data_ptr(), d["deltas"].data_ptr(), d["pts"].data_ptr(), d["offs"].data_ptr(), 1081, host,
                            d["force"].data_ptr(), oh["pose"].data_ptr(), oh["cov"].data_ptr(), oh["applied"].data_ptr(), s)
    torch.cuda.synchronize()
    assert g.last_launch_config() == h.last_launch_config()
    for k in ("applied", "pose", "cov"):
        a, b = og[k].cpu().numpy(), oh[k].cpu().numpy()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (entry, origo, k)
    applied = og["applied"].cpu().numpy()
    assert applied[force.astype(bool)].all() and (applied == 0).sum() >= 6, applied
    (pg, tg), (ph, th) = g.update_gate_state(), h.update_gate_state()
    assert np.array_equal(bits(pg), bits(ph)) and tg == th == int(applied.sum())
    for lvl in range(LEVELS):
        assert np.array_equal(g.last_update_bbox(lvl), h.last_update_bbox(lvl)), lvl
        assert np.array_equal(g.take_dirty_bbox(lvl), h.take_dirty_bbox(lvl)), lvl
    assert_same_as_ctx(g, h, (entry, origo))
    for lvl in range(LEVELS):
        assert g.debug_marks_nonzero(lvl) == (0, 0)
    del d
    g.close()
    h.close()


# ---- 9: the one-call raw entry, moving mount -----------------------------------------------------------------------------------------
def raw_call(g, sc, thresholds, r, T, a0, inc, shared, force=None, gates=None, start=True, stream=None, ws_bytes=None, k0=0):
    """hsm_slam_ranges_tf_device on torch buffers for scans k0 .. k0 + len(r) of the log -> (the buffers, the stream)"""
    import torch
    n = r.shape[1]
    s = stream or torch.cuda.Stream()
    g.set_update_gate(*thresholds)
    ga = oc.gate_args() if gates is None else gates
    with torch.cuda.stream(s):
        nbytes = g.slam_ranges_tf_workspace(len(r), n) if ws_bytes is None else ws_bytes
        d = {"start": dev(sc.poses[max(k0 - 1, 0)]), "deltas": dev(sc.deltas[k0:k0 + len(r)]), "ranges": dev(r), "T": dev(np.asarray(T, np.float64)),
             "force": None if force is None else dev(force), "ws": torch.full((max(nbytes, 8),), 0x5A, dtype=torch.uint8, device="cuda:0"),
             **outputs(len(r))}
        g.slam_ranges_tf_device(len(r), d["start"].data_ptr() if start else 0, d["deltas"].data_ptr() if start else 0, d["ranges"].data_ptr(),
                                n, a0, inc, 0.4, 30.0, 30.0, d["T"].data_ptr(), shared, *ga, g.getScaleToMap(),
                                0 if force is None else d["force"].data_ptr(), d["pose"].data_ptr(), d["cov"].data_ptr(),
                                d["applied"].data_ptr(), d["counts"].data_ptr(), d["ws"].data_ptr(), nbytes, s.cuda_stream)
    return d, s


def test_one_call_raw_entry_with_a_moving_mount(capi, oracle_mod, traj):
    if not oracle_mod.available("node"):
        pytest.skip("oracle/_ref/libhector_node_ref.so not built (no reference tree where the suite was built)")
    sc, t = traj, oc.THRESHOLDS["default"]
    r, T, a0, inc = oc.raw_log()
    force = np.zeros(N, np.uint8)
    force[11] = 1
    g, refs = new_ctx(capi), oc.new_refs(oracle_mod)
    node = oracle_mod.NodeRef(*oc.NODE_GATES0)
    conts, origos = [], np.empty((N, 2), np.float32)
    for k in range(N):
        pts, origos[k], _ = node.project_and_convert(r[k], a0, inc, 0.4, 30.0, 30.0, T[k], g.getScaleToMap())
        conts.append(np.ascontiguousarray(pts, np.float32).reshape(-1, 2))
    node.close()
    counts = np.array([len(c) for c in conts], np.int32)
    assert counts[5] == 0 and (np.delete(counts, 5) > 800).all() and len({tuple(bits(o)) for o in origos}) == N
    for lvl in range(LEVELS):  # the begin cell moves on every level
        assert len({tuple(np.floor(o * np.float32(0.5 ** lvl) + np.float32(0.5))) for o in origos}) >= 3, lvl
    d, s = raw_call(g, sc, t, r, T, a0, inc, False, force)
    s.synchronize()  # the one wait
    poses, covs, applied = d["pose"].cpu().numpy(), d["cov"].cpu().numpy(), d["applied"].cpu().numpy()
    assert np.array_equal(d["counts"].cpu().numpy(), counts)
    for kind, o in refs.items():
        ref = oc.reference_loop(o, t, conts, origos, sc.poses[0], sc.deltas, force)
        assert ref[2].sum() >= 6 and (~ref[2]).sum() >= 3, (kind, ref[2].astype(int))
        assert np.linalg.norm(ref[0][-1, :2] - sc.poses[-1, :2]) < 0.05, (kind, "the reference lost track: the inputs drifted")
        assert_loop_equals((poses, covs, applied), ref, conts, (kind,), force)
    # the scan that keeps no beam: its pose is its hint, its covariance row is left as hsm_match_batch_device leaves it
    assert np.array_equal(bits(poses[5]), bits((poses[4] + sc.deltas[5]).astype(np.float32))) and (covs[5] == COV0).all()
    g.synchronize()
    assert_same_as_refs(oracle_mod, g, refs, "one call, moving mount")
    # the host form: the same bits, and the node's origos
    h = new_ctx(capi)
    h.set_update_gate(*t)
    out = h.slam_ranges_tf(sc.poses[0], sc.deltas, r, a0, inc, 0.4, 30.0, 30.0, T, *oc.gate_args(), force=force,
                           cov=np.full((N, 9), COV0, np.float32))
    assert np.array_equal(bits(out["pose"]), bits(poses)) and np.array_equal(bits(out["cov"]), bits(covs))
    assert np.array_equal(out["applied"], applied) and np.array_equal(out["counts"], counts)
    assert np.array_equal(bits(out["origo"]), bits(origos))
    assert_same_as_ctx(g, h, "host form")
    del d
    g.close()
    h.close()


# ---- 10: the one-call raw entry, fixed mount, against the whole node -------------------------------------------------------------------
def test_one_call_raw_entry_with_a_fixed_mount_equals_the_node(capi, oracle_mod, traj):
    import torch
    from test_node_rows import laser_scan_messages
    if not oracle_mod.available("node"):
        pytest.skip("oracle/_ref/libhector_node_ref.so not built (no reference tree where the suite was built)")
    n_scans = 25
    scans, a0, inc = laser_scan_messages(n_scans)
    T = np.array([1, 0, 0, 0.12, 0, 1, 0, -0.05, 0, 0, 1, 0.3], np.float64)
    node = oracle_mod.NodeRef(map_size=512, levels=3, resolution=0.05, update_dist_thresh=0.05, update_angle_thresh=0.02, laser_transform=T)
    rp, rc = np.empty((n_scans, 3), np.float32), np.empty((n_scans, 9), np.float32)
    for k, r in enumerate(scans):
        rp[k], rc[k] = node.scan_callback(r, a0, inc, 0.4, 30.0)
    cells, lo, _ = node.node_map()
    g = new_ctx(capi)
    s = torch.cuda.Stream()  # a side stream, never synchronised between conversion and loop
    d, _ = raw_call(g, traj, (0.05, 0.02), np.stack(scans), T, a0, inc, True, gates=(np.float32(node.sqr_min), np.float32(node.sqr_max), -1.0, 1.0),
                    start=False, stream=s)
    s.synchronize()
    pose, cov = d["pose"].cpu().numpy(), d["cov"].cpu().numpy()
    assert np.array_equal(bits(pose), bits(rp)), np.nonzero((bits(pose) != bits(rp)).any(1))[0][:8]
    assert np.array_equal(bits(cov), bits(rc)), np.nonzero((bits(cov) != bits(rc)).any(1))[0][:8]
    g.synchronize()
    assert np.array_equal(bits(g.download_level(0)[0]), bits(lo))
    assert np.array_equal(g.occupancy_grid(0), cells) and (cells == 100).sum() > 200
    node.close()
    del d
    g.close()


# ---- 11: ordering, capture, validation ---------------------------------------------------------------------------------------------------
def test_matches_on_another_stream_are_ordered_around_the_call(capi, traj):
    """a batched match queued on another stream BEFORE the call reads the old map, one queued AFTER it reads the new map -- the
    contract of hsm_slam_scans_device; the yardsticks are the same matches on a twin context, waited for"""
    import torch
    sc, t = traj, oc.THRESHOLDS["default"]
    r, T, a0, inc = oc.raw_log()
    a, b = new_ctx(capi), new_ctx(capi)
    pts, offs = pack(sc.scans[:8])
    for m in (a, b):
        m.update_by_scans(sc.poses[:8], pts, offs)
        m.synchronize()
    B = 8
    qpts, qoffs = pack(sc.query_scans[:B])
    s2 = torch.cuda.Stream()

    def match_on(m, stream):
        with torch.cuda.stream(stream):
            d = {"begin": dev(sc.query_init[:B]), "pts": dev(qpts), "offs": dev(qoffs), "pose": torch.zeros((B, 3), device="cuda:0")}
            m.match_batch_device(B, d["begin"].data_ptr(), d["pts"].data_ptr(), d["offs"].data_ptr(), 1081, d["pose"].data_ptr(), 0, stream.cuda_stream)
        return d

    old_b = match_on(b, s2)
    s2.synchronize()
    db, sb = raw_call(b, sc, t, r[8:], T[8:], a0, inc, False, k0=8)
    sb.synchronize()
    b.synchronize()
    new_b = match_on(b, s2)
    s2.synchronize()
    old, new = old_b["pose"].cpu().numpy(), new_b["pose"].cpu().numpy()
    assert (bits(old) != bits(new)).any(), "the updates do not show in the matches: the checks below would be blind"
    # context a: nothing is waited for between the three calls
    before = match_on(a, s2)
    da, sa = raw_call(a, sc, t, r[8:], T[8:], a0, inc, False, k0=8)
    after = match_on(a, s2)
    s2.synchronize()
    sa.synchronize()
    assert np.array_equal(bits(before["pose"].cpu().numpy()), bits(old)), "a match queued before the call saw its updates"
    assert np.array_equal(bits(after["pose"].cpu().numpy()), bits(new)), "a match queued after the call did not see its updates"
    assert np.array_equal(bits(da["pose"].cpu().numpy()), bits(db["pose"].cpu().numpy()))
    assert_same_as_ctx(a, b, "ordering")
    del da, db
    a.close()
    b.close()


def test_new_entries_are_refused_during_capture(capi, traj):
    import torch
    sc = traj
    r, T, a0, inc = oc.raw_log()
    g = new_ctx(capi)
    warm, ws = raw_call(g, sc, oc.THRESHOLDS["default"], r[:4], T[:4], a0, inc, False)  # the geometry is known from here on
    ws.synchronize()
    g.synchronize()
    before, idx, state = planes(g), g.getUpdateIndex(0), g.update_gate_state()
    pts, offs = pack(sc.scans[4:8])
    d = [dev(sc.poses[4:8]), dev(pts), dev(offs), dev(sc.origos[4:8]), torch.full((4, 3), -5.0, device="cuda:0"),
         torch.full((4,), -5, dtype=torch.int32, device="cuda:0"), dev(r[4:8]), dev(T[4:8]),
         torch.zeros(g.slam_ranges_tf_workspace(4, 1081), dtype=torch.uint8, device="cuda:0")]
    s = torch.cuda.Stream()
    x = torch.zeros(8, device="cuda:0")
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        x.add_(1.0)
        for call in (lambda: g.update_by_scans_device_origos(4, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 0, 1081, d[3].data_ptr(), s.cuda_stream),
                     lambda: g.update_by_scans_device_gated_origos(4, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 0, 1081, d[3].data_ptr(), 0,
                                                                   d[5].data_ptr(), s.cuda_stream),
                     lambda: g.slam_scans_device_origos(4, d[0].data_ptr(), 0, d[1].data_ptr(), d[2].data_ptr(), 1081, d[3].data_ptr(), 0,
                                                        d[4].data_ptr(), 0, d[5].data_ptr(), s.cuda_stream),
                     lambda: g.slam_ranges_tf_device(4, d[0].data_ptr(), 0, d[6].data_ptr(), 1081, a0, inc, 0.4, 30.0, 30.0, d[7].data_ptr(), False,
                                                     *oc.gate_args(), g.getScaleToMap(), 0, d[4].data_ptr(), 0, d[5].data_ptr(), 0,
                                                     d[8].data_ptr(), d[8].numel(), s.cuda_stream)):
            with pytest.raises(capi.HsmError) as e:
                call()
            assert f"({HSM_ERR_INVALID})" in str(e.value) and "captur" in str(e.value), str(e.value)
        x.add_(1.0)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert x.cpu().numpy().tolist() == [2.0] * 8  # the capture ended normally and recorded nothing of ours
    g.synchronize()
    after = g.update_gate_state()
    assert g.getUpdateIndex(0) == idx and np.array_equal(bits(after[0]), bits(state[0])) and after[1] == state[1]
    assert (d[4].cpu().numpy() == -5.0).all() and (d[5].cpu().numpy() == -5).all() and (d[8].cpu().numpy() == 0).all()
    for a, b in zip(before, planes(g)):
        assert all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in zip(a, b)), "a refused call changed the map"
    del warm, d
    g.close()


def test_validation_leaves_outputs_and_map_untouched(capi, traj):
    import torch
    sc = traj
    r, T, a0, inc = oc.raw_log()
    g = new_ctx(capi)
    lib, n = g._lib, r.shape[1]
    need = g.slam_ranges_tf_workspace(4, n)
    d = {"ranges": dev(r[:4]), "T": dev(T[:4]), "ws": torch.full((need + 8,), 0x5A, dtype=torch.uint8, device="cuda:0"), **outputs(4)}
    s = stream_ptr()
    null = object()

    def call(count=4, n=n, h=g._h, ranges=None, tf=None, pose=None, ws=None, ws_bytes=need):
        p = lambda v, t: None if v is null else (t.data_ptr() if v is None else v)  # noqa: E731
        return lib.hsm_slam_ranges_tf_device(h, count, None, None, p(ranges, d["ranges"]), n, a0, inc, 0.4, 30.0, 30.0, p(tf, d["T"]), 0,
                                             *oc.gate_args(), g.getScaleToMap(), None, p(pose, d["pose"]), d["cov"].data_ptr(),
                                             d["applied"].data_ptr(), d["counts"].data_ptr(), p(ws, d["ws"]), ws_bytes, s)

    assert call(h=None) == HSM_ERR_INVALID
    assert call(count=-1) == HSM_ERR_INVALID and call(n=-1) == HSM_ERR_INVALID
    assert call(ranges=null) == HSM_ERR_INVALID and call(tf=null) == HSM_ERR_INVALID and call(pose=null) == HSM_ERR_INVALID
    assert call(tf=d["T"].data_ptr() + 4) == HSM_ERR_INVALID                  # transforms not 8-byte aligned
    assert call(ws=null) == HSM_ERR_INVALID and call(ws_bytes=need - 1) == HSM_ERR_INVALID
    assert call(ws=d["ws"].data_ptr() + 4) == HSM_ERR_INVALID and "workspace" in lib.hsm_last_error().decode()
    assert call(count=4096, n=1048575) == HSM_ERR_TOO_LARGE and call(count=1, n=1048576) == HSM_ERR_TOO_LARGE
    assert call(count=0) == HSM_OK and call(count=0, ranges=null, tf=null, ws=null, ws_bytes=0) == HSM_OK
    torch.cuda.synchronize()
    g.synchronize()
    assert (d["pose"].cpu().numpy() == -777.0).all() and (d["cov"].cpu().numpy() == COV0).all() and (d["ws"].cpu().numpy() == 0x5A).all()
    assert (d["applied"].cpu().numpy() == -7).all() and (d["counts"].cpu().numpy() == -7).all()
    assert g.getUpdateIndex(0) == -1 and (g.download_level(0)[1] == -1).all()
    # a misaligned origo array: refused, and the text names the entry the caller used
    og = dev(np.zeros((5, 2), np.float32))
    for name, args in (("hsm_update_by_scans_device_origos", (g._h, 4, d["pose"].data_ptr(), d["ranges"].data_ptr(), None, 8, 8, og.data_ptr() + 4, s)),
                       ("hsm_update_by_scans_device_gated_origos", (g._h, 4, d["pose"].data_ptr(), d["ranges"].data_ptr(), None, 8, 8,
                                                                    og.data_ptr() + 4, None, None, s)),
                       ("hsm_slam_scans_device_origos", (g._h, 4, None, None, d["ranges"].data_ptr(), d["counts"].data_ptr(), 8,
                                                         og.data_ptr() + 4, None, d["pose"].data_ptr(), None, None, s))):
        assert getattr(lib, name)(*args) == HSM_ERR_INVALID and lib.hsm_last_error().decode().startswith(name + ":"), lib.hsm_last_error()
    torch.cuda.synchronize()
    assert (d["pose"].cpu().numpy() == -777.0).all() and g.getUpdateIndex(0) == -1
    # the host form refuses the same way and writes nothing
    pose = np.full((4, 3), -9.0, np.float32)
    host = lambda count, n, rp, tp: lib.hsm_slam_ranges_tf(g._h, count, None, None, rp, n, a0, inc, 0.4, 30.0, 30.0, tp, 0, *oc.gate_args(),  # noqa: E731
                                                           g.getScaleToMap(), None, pose.ctypes.data, None, None, None, None)
    Th = np.ascontiguousarray(T[:4])
    assert host(4, n, None, Th.ctypes.data) == HSM_ERR_INVALID and host(4, n, r.ctypes.data, None) == HSM_ERR_INVALID
    assert host(-1, n, r.ctypes.data, Th.ctypes.data) == HSM_ERR_INVALID and host(1, 1048576, r.ctypes.data, Th.ctypes.data) == HSM_ERR_TOO_LARGE
    assert host(0, n, None, None) == HSM_OK and (pose == -9.0).all()
    # the same buffers in a valid call
    assert call() == HSM_OK
    torch.cuda.synchronize()
    g.synchronize()
    assert np.isfinite(d["pose"].cpu().numpy()).all() and (d["counts"].cpu().numpy() > 800).all() and g.getUpdateIndex(0) >= 0
    del d
    g.close()
