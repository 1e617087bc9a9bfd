"""hsm_update_by_scans_device / hsm_update_by_scans on the MI355X: posed scans that are already on the device, integrated in
order without a host trip.  The bar is the update path's: BIT-EXACT -- the log-odds and update-index planes of every level,
the probability plane, the counters, and matches run afterwards.

Two yardsticks, both on every test:
  * the CPU checkers' `build_map(poses, scans, origo)` -- "hr", the unmodified OccGridMapBase::updateByScan per level with the
    setFrom-scaled container, and "ho", the restatement, alongside (conftest.oracle_kinds());
  * a second context driven through hsm_retain_scan + hsm_update_by_scan, the host path: it also pins the texels (matches agree
    afterwards) and the mark planes.

The only input on which the reference is undefined is the NaN pose: (int)NaN is UB in C++; it is pinned to what x86 does
(cvttss2si gives INT_MIN, every beam fails the map test).  Nothing here provokes a device fault.
"""
import numpy as np
import pytest

from conftest import bits
import support
from support import capi, dev, new_context, pack

pytestmark = pytest.mark.gpu

RES = 0.05
HSM_ERR_INVALID = -1
ZERO2 = np.zeros(2, np.float32)
LEVELS = 3
GEOMS = {"square": (512, 512), "rect": (500, 360)}  # rect: rows that are no multiple of 64 cells, sx != sy on every level


@pytest.fixture(scope="module")
def traj():
    """64 posed 1081-beam scans along a loop in a 16 m x 12 m room, and a 5000-beam scan of the same room"""
    from hector_slam_amd import synth
    sc = synth.make_scene(n_beams=1081, map_size=512, levels=LEVELS, resolution=RES, n_build=64, n_query=64, room=(16.0, 12.0), seed=2024)
    sc.dense = synth.make_scan(sc.world, sc.build_poses[5], 5000, sc.scale_to_map, np.random.default_rng(7))
    assert len(sc.dense) > 4096 and max(len(s) for s in sc.build_scans) <= 1081
    return sc


def new_ctx(capi, geom, layout="quad"):
    sx, sy = GEOMS[geom]
    return new_context(capi, RES, sx, sy, LEVELS, layout=layout)


def new_refs(oracle_mod, geom):
    sx, sy = GEOMS[geom]
    return support.new_refs(oracle_mod, RES, sx, sy, LEVELS)


def ref_update(refs, poses, scans, origo=ZERO2):
    for o in refs.values():
        o.build_map(np.asarray(poses, np.float32).reshape(-1, 3), scans, origo)


def host_path(capi, g, poses, scans, origo=ZERO2):
    """the parent path: per scan hsm_retain_scan (what matchData leaves for the coarse levels) + hsm_update_by_scan"""
    o = np.ascontiguousarray(origo, np.float32)
    for p, s in zip(np.asarray(poses, np.float32).reshape(-1, 3), scans):
        a = np.ascontiguousarray(s, np.float32).reshape(-1, 2)
        capi._check(g._lib.hsm_retain_scan(g._h, a.ctypes.data if a.size else None, a.shape[0], o), "hsm_retain_scan")
        g.updateByScan(a, p, o)


def device_update(g, poses, scans=None, shared=None, max_beams=0, origo=None, stream=None):
    """hsm_update_by_scans_device on torch buffers (CSR scans, or one shared scan); returns the buffers (they must outlive the update)"""
    import torch
    s = stream or torch.cuda.current_stream()
    poses = np.asarray(poses, np.float32).reshape(-1, 3)
    with torch.cuda.stream(s):
        d_p = dev(poses)
        if shared is None:
            pts, offs = pack(scans)
            d_pts, d_offs = dev(pts if len(pts) else np.zeros((1, 2), np.float32)), dev(offs)
            g.update_by_scans_device(len(poses), d_p.data_ptr(), d_pts.data_ptr(), d_offs.data_ptr(), 0, max_beams, origo, s.cuda_stream)
        else:
            a = np.asarray(shared, np.float32).reshape(-1, 2)
            d_pts, d_offs = dev(a if len(a) else np.zeros((1, 2), np.float32)), None
            g.update_by_scans_device(len(poses), d_p.data_ptr(), d_pts.data_ptr(), 0, len(a), max_beams, origo, s.cuda_stream)
    return d_p, d_pts, d_offs


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
    for lvl in range(LEVELS):
        assert g.debug_marks_nonzero(lvl) == (0, 0), (what, lvl)


def assert_same_as_ctx(g, h, what):
    for lvl, (a, b) in enumerate(zip(planes(g), planes(h))):
        assert np.array_equal(a[1], b[1]), (what, lvl, "update index", int((a[1] != b[1]).sum()))
        assert np.array_equal(bits(a[0]), bits(b[0])), (what, lvl, "log odds", int((bits(a[0]) != bits(b[0])).sum()))
        assert np.array_equal(bits(a[2]), bits(b[2])), (what, lvl, "probability")
        assert g.getUpdateIndex(lvl) == h.getUpdateIndex(lvl), (what, lvl, g.getUpdateIndex(lvl), h.getUpdateIndex(lvl))


def assert_same_matches(g, h, sc, what):
    """a batched match of the 64 query scans gives the same bits on both contexts (the texels the updates wrote)"""
    pts, offs = pack(sc.query_scans)
    (pg, cg), (ph, ch) = g.match_batch(sc.query_init, pts, offs), h.match_batch(sc.query_init, pts, offs)
    assert np.isfinite(ph).all(), what
    assert np.array_equal(bits(pg), bits(ph)) and np.array_equal(bits(cg), bits(ch)), (what, int((bits(pg) != bits(ph)).sum()))


def check_all(capi, oracle_mod, g, h, refs, what):
    g.synchronize()
    assert_same_as_refs(oracle_mod, g, refs, what)
    assert_same_as_ctx(g, h, what)


# ---- 3: a trajectory in one call ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["quad", "plane"])
@pytest.mark.parametrize("geom", list(GEOMS))
def test_trajectory_in_one_call_is_bit_identical(capi, oracle_mod, traj, geom, layout):
    sc = traj
    g, h, refs = new_ctx(capi, geom, layout), new_ctx(capi, geom, layout), new_refs(oracle_mod, geom)
    keep = device_update(g, sc.build_poses, sc.build_scans, max_beams=1081)
    host_path(capi, h, sc.build_poses, sc.build_scans)
    ref_update(refs, sc.build_poses, sc.build_scans)
    check_all(capi, oracle_mod, g, h, refs, f"{geom} {layout}")
    for lvl in range(LEVELS):
        assert g.getUpdateIndex(lvl) == 63  # lastUpdateIndex starts at -1
    assert_same_matches(g, h, sc, f"{geom} {layout}")
    del keep
    g.close()
    h.close()


def test_host_array_entry_takes_the_same_path(capi, oracle_mod, traj):
    sc = traj
    g, h, refs = new_ctx(capi, "rect"), new_ctx(capi, "rect"), new_refs(oracle_mod, "rect")
    pts, offs = pack(sc.build_scans[:16])
    g.update_by_scans(sc.build_poses[:16], pts, offs)
    host_path(capi, h, sc.build_poses[:16], sc.build_scans[:16])
    ref_update(refs, sc.build_poses[:16], sc.build_scans[:16])
    check_all(capi, oracle_mod, g, h, refs, "host arrays")
    g.close()
    h.close()


# ---- 4: ragged CSR lengths and the shared scan ------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", list(GEOMS))
def test_ragged_lengths_and_the_shared_scan(capi, oracle_mod, traj, geom):
    sc = traj
    g, h, refs = new_ctx(capi, geom), new_ctx(capi, geom), new_refs(oracle_mod, geom)
    long_scan = np.concatenate([sc.build_scans[9], sc.build_scans[10]])[:1500]  # longer than the hint
    scans = [sc.build_scans[0], sc.build_scans[1][:700], np.zeros((0, 2), np.float32), sc.dense, sc.build_scans[3][:64],
             long_scan, sc.build_scans[4][:1], sc.build_scans[6]]
    poses = np.stack([sc.build_poses[i] for i in (0, 1, 2, 5, 3, 9, 4, 6)])
    assert len(scans[2]) == 0 and len(scans[3]) > 4096 and len(scans[5]) > 1081
    keep = device_update(g, poses, scans, max_beams=1081)
    host_path(capi, h, poses, scans)
    ref_update(refs, poses, scans)
    check_all(capi, oracle_mod, g, h, refs, f"{geom} ragged")
    # one scan at several poses (shared_n), hint 0 = unknown
    rng = np.random.default_rng(3)
    hyp = (sc.build_poses[20][None, :] + rng.normal(0, [0.05, 0.05, 0.02], (8, 3))).astype(np.float32)
    keep2 = device_update(g, hyp, shared=sc.build_scans[20])
    host_path(capi, h, hyp, [sc.build_scans[20]] * 8)
    ref_update(refs, hyp, [sc.build_scans[20]] * 8)
    check_all(capi, oracle_mod, g, h, refs, f"{geom} shared scan")
    assert_same_matches(g, h, sc, f"{geom} ragged")
    del keep, keep2
    g.close()
    h.close()


# ---- 5: edge poses ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", list(GEOMS))
def test_edge_poses(capi, oracle_mod, traj, geom):
    sc = traj
    sx, sy = GEOMS[geom]
    g, h, refs = new_ctx(capi, geom), new_ctx(capi, geom), new_refs(oracle_mod, geom)
    first = (sc.build_poses[:6], sc.build_scans[:6])
    keep = [device_update(g, *first, max_beams=1081)]
    host_path(capi, h, *first)
    ref_update(refs, *first)
    check_all(capi, oracle_mod, g, h, refs, "before the edge cases")
    scan = sc.build_scans[7]
    nan = np.float32(np.nan)

    def world(mx, my, th):  # the world pose of a level-0 map position
        return g.getWorldCoordsPose(0, np.float32([mx, my, th]))

    # reference-UB input, pinned to x86: (int)NaN = INT_MIN -> every beam dropped; all planes unchanged, counters advance
    before, idx = planes(g), [g.getUpdateIndex(l) for l in range(LEVELS)]
    nan_poses = np.float32([[nan, 0, 0], [0, nan, 0], [0.5, 0.5, nan], [nan, nan, nan]])
    keep.append(device_update(g, nan_poses, shared=scan))
    host_path(capi, h, nan_poses, [scan] * len(nan_poses))
    ref_update(refs, nan_poses, [scan] * len(nan_poses))
    check_all(capi, oracle_mod, g, h, refs, "NaN poses")
    for lvl, (a, b) in enumerate(zip(before, planes(g))):
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b)), ("a NaN pose changed a plane", lvl)
        assert g.getUpdateIndex(lvl) == idx[lvl] + len(nan_poses)

    begin_scan = np.concatenate([np.float32([[0, 0], [0.2, -0.3], [0.4, 0.4]]), scan[:300], np.float32([[0.1, 0.1]])])
    cases = [
        ("pose outside the map", np.float32([[100.0, 100.0, 0.3], [-1e6, 3.0, 0.0], [2.0, 1e6, 1.0]]), scan, None),
        # level 0 keeps the begin cell ((int)(sx - 0.6 + 0.5) = sx - 1), levels 1 and 2 do not ((sx - 0.6) / 2 + 0.5 >= sx / 2)
        ("begin cell outside the coarse levels only", np.stack([world(sx - 0.6, sy / 2, 3.0), world(sx / 2, sy - 0.6, -1.5)]), scan, None),
        ("beams that leave the map", np.stack([world(12.3, 15.7, 0.4), world(sx - 20.2, sy - 9.9, 2.0), world(3.0, sy / 2, 3.1)]), scan, None),
        ("beams that end in the begin cell", np.stack([sc.build_poses[8], world(0.2, 0.3, 0.0)]), begin_scan, None),
        ("origo off the robot's centre", sc.build_poses[10:13], scan, np.float32([3.5, -2.25])),
    ]
    for what, poses, pts, origo in cases:
        n = len(poses)
        keep.append(device_update(g, poses, shared=pts, origo=origo))
        host_path(capi, h, poses, [pts] * n, ZERO2 if origo is None else origo)
        ref_update(refs, poses, [pts] * n, ZERO2 if origo is None else origo)
        check_all(capi, oracle_mod, g, h, refs, what)
    assert_same_matches(g, h, sc, "after the edge cases")
    g.close()
    h.close()


# ---- 6: the key generation wraps inside one call ----------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", list(GEOMS))
def test_key_generation_wrap_inside_one_call(capi, oracle_mod, traj, geom):
    sc = traj
    g, h, refs = new_ctx(capi, geom), new_ctx(capi, geom), new_refs(oracle_mod, geom)
    first = (sc.build_poses[:4], sc.build_scans[:4])
    keep = [device_update(g, *first)]
    host_path(capi, h, *first)
    ref_update(refs, *first)
    for m in (g, h):
        m.synchronize()
        for lvl in range(LEVELS):
            capi._check(m._lib.hsm_debug_set_update_serial(m._h, lvl, 4093 - lvl), "set serial")  # wraps before scan 2, 3, 4 of the call
    nxt = (sc.build_poses[4:12], sc.build_scans[4:12])
    keep.append(device_update(g, *nxt))
    host_path(capi, h, *nxt)
    ref_update(refs, *nxt)
    check_all(capi, oracle_mod, g, h, refs, "across the wrap")
    nxt = (sc.build_poses[12:16], sc.build_scans[12:16])  # and the generations after it
    keep.append(device_update(g, *nxt))
    host_path(capi, h, *nxt)
    ref_update(refs, *nxt)
    check_all(capi, oracle_mod, g, h, refs, "after the wrap")
    g.close()
    h.close()


# ---- 7: the forms mixed on one context --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["quad", "plane"])
def test_device_side_updates_mix_with_the_host_forms(capi, oracle_mod, traj, layout):
    sc = traj
    g, refs = new_ctx(capi, "rect", layout), new_refs(oracle_mod, "rect")
    keep = device_update(g, sc.build_poses[:8], sc.build_scans[:8])
    ref_update(refs, sc.build_poses[:8], sc.build_scans[:8])
    g.synchronize()
    assert_same_as_refs(oracle_mod, g, refs, "device-side updates")
    host_path(capi, g, sc.build_poses[8:9], sc.build_scans[8:9])  # the keyed host form
    ref_update(refs, sc.build_poses[8:9], sc.build_scans[8:9])
    g.synchronize()
    assert_same_as_refs(oracle_mod, g, refs, "then a host update of a 1081-beam scan")
    host_path(capi, g, sc.build_poses[5:6], [sc.dense])  # the byte-map host form
    ref_update(refs, sc.build_poses[5:6], [sc.dense])
    g.synchronize()
    assert_same_as_refs(oracle_mod, g, refs, "then a dense host update")
    keep2 = device_update(g, sc.build_poses[9:12], sc.build_scans[9:12])
    ref_update(refs, sc.build_poses[9:12], sc.build_scans[9:12])
    g.synchronize()
    assert_same_as_refs(oracle_mod, g, refs, "and device-side updates again")
    for lvl in range(LEVELS):
        assert g.getUpdateIndex(lvl) == 8 + 1 + 1 + 3 - 1
    del keep, keep2
    g.close()


# ---- 8: match -> score -> select -> update, no host wait --------------------------------------------------------------------------
def test_closing_the_loop_on_one_stream(capi, oracle_mod, traj):
    import torch
    sc = traj
    a, b = new_ctx(capi, "square"), new_ctx(capi, "square")
    pts, offs = pack(sc.build_scans[:40])
    for m in (a, b):
        m.update_by_scans(sc.build_poses[:40], pts, offs)
        m.synchronize()
    B = 32
    scan = np.ascontiguousarray(sc.query_scans[50], np.float32)
    rng = np.random.default_rng(11)
    hyp = (sc.query_truth[50][None, :] + rng.normal(0, [0.08, 0.08, 0.03], (B, 3))).astype(np.float32)
    qpts, qoffs = pack(sc.query_scans[:B])
    s, s2 = torch.cuda.Stream(), torch.cuda.Stream()

    def match_score(m, stream):
        with torch.cuda.stream(stream):
            d = {"begin": dev(hyp), "pts": dev(scan), "pose": torch.zeros((B, 3), device="cuda:0"), "lh": torch.zeros(B, device="cuda:0"),
                 "idx": torch.zeros(1, dtype=torch.int32, device="cuda:0"), "best": torch.full((1, 3), -777.0, device="cuda:0")}
            m.match_score_batch_device(B, d["begin"].data_ptr(), d["pts"].data_ptr(), 0, len(scan), d["pose"].data_ptr(), 0, 0,
                                       d["lh"].data_ptr(), 0, 1, 0, B, d["idx"].data_ptr(), 0, d["best"].data_ptr(), stream.cuda_stream)
        return d

    def match_after(m, stream):
        with torch.cuda.stream(stream):
            d = {"begin": dev(sc.query_init[:B]), "pts": dev(qpts), "offs": dev(qoffs), "pose": torch.zeros((B, 3), device="cuda:0")}
            m.match_batch_device(B, d["begin"].data_ptr(), d["pts"].data_ptr(), d["offs"].data_ptr(), 1081, d["pose"].data_ptr(), 0,
                                 stream.cuda_stream)
        return d

    # B: the parent's way -- download the winner, wait, upload the scan again
    before_b = match_after(b, s2)
    s2.synchronize()
    db = match_score(b, s)
    s.synchronize()
    best_b = db["best"].cpu().numpy()[0]
    assert np.isfinite(best_b).all() and int(db["idx"].cpu()[0]) >= 0
    host_path(capi, b, best_b[None, :], [scan])
    after_b = match_after(b, s2)
    s2.synchronize()
    pose_before, pose_after = before_b["pose"].cpu().numpy(), after_b["pose"].cpu().numpy()
    assert (bits(pose_before) != bits(pose_after)).any(), "the update does not show in the matches: the check below would be blind"
    # A: the winner never leaves the device; the match on a second stream is queued right behind the update
    da = match_score(a, s)
    a.update_by_scans_device(1, da["best"].data_ptr(), da["pts"].data_ptr(), 0, len(scan), 1081, None, s.cuda_stream)
    after_a = match_after(a, s2)
    s2.synchronize()
    assert np.array_equal(bits(after_a["pose"].cpu().numpy()), bits(pose_after)), "a match queued behind the update did not see it"
    a.synchronize()
    assert np.array_equal(bits(da["best"].cpu().numpy()[0]), bits(best_b))
    assert_same_as_ctx(a, b, "closing the loop")
    a.close()
    b.close()


# ---- 9: the boxes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", list(GEOMS))
def test_boxes_after_a_call(capi, traj, geom):
    sc = traj
    g, h = new_ctx(capi, geom), new_ctx(capi, geom)
    for m in (g, h):
        for lvl in range(LEVELS):
            m.take_dirty_bbox(lvl)
    keep = [device_update(g, sc.build_poses[:63], sc.build_scans[:63], max_beams=1081)]
    host_path(capi, h, sc.build_poses[:63], sc.build_scans[:63])
    stamps = [g.download_level(l)[1] for l in range(LEVELS)]
    keep.append(device_update(g, sc.build_poses[63:], sc.build_scans[63:], max_beams=1081))  # the running boxes span calls
    host_path(capi, h, sc.build_poses[63:], sc.build_scans[63:])
    for lvl in range(LEVELS):
        last_g, last_h = g.last_update_bbox(lvl), h.last_update_bbox(lvl)
        dirty_g, dirty_h = g.take_dirty_bbox(lvl), h.take_dirty_bbox(lvl)
        ui = g.download_level(lvl)[1]
        if lvl == 0:
            assert np.array_equal(last_g, last_h), (last_g, last_h)
            assert np.array_equal(dirty_g, dirty_h), (dirty_g, dirty_h)
        for what, box, ref_box, changed in (("last", last_g, last_h, ui != stamps[lvl]), ("dirty", dirty_g, dirty_h, ui != -1)):
            ys, xs = np.nonzero(changed)
            assert len(xs) > 0
            assert box[0] <= xs.min() and box[1] <= ys.min() and box[2] >= xs.max() and box[3] >= ys.max(), (what, lvl, box)
            assert box[0] >= ref_box[0] and box[1] >= ref_box[1] and box[2] <= ref_box[2] and box[3] <= ref_box[3], (what, lvl, box, ref_box)
        assert np.array_equal(g.take_dirty_bbox(lvl), np.int32([0, 0, -1, -1]))  # taken: empty until the next update
    g.close()
    h.close()


# ---- 10: refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(capi, traj):
    import torch
    sc = traj
    g = new_ctx(capi, "square")
    keep = [device_update(g, sc.build_poses[:4], sc.build_scans[:4])]
    g.synchronize()
    before, idx = planes(g), g.getUpdateIndex(0)
    pts, offs = pack(sc.build_scans[4:6])
    d_p, d_pts, d_offs = dev(sc.build_poses[4:6]), dev(pts), dev(offs)
    s = torch.cuda.Stream()

    def refused(*args):
        with pytest.raises(capi.HsmError) as e:
            g.update_by_scans_device(*args)
        assert f"({HSM_ERR_INVALID})" in str(e.value), str(e.value)
        return str(e.value)

    refused(-1, d_p.data_ptr(), d_pts.data_ptr(), d_offs.data_ptr(), 0, 0, None, s.cuda_stream)
    refused(2, 0, d_pts.data_ptr(), d_offs.data_ptr(), 0, 0, None, s.cuda_stream)       # no poses
    refused(2, d_p.data_ptr(), d_pts.data_ptr(), 0, -1, 0, None, s.cuda_stream)         # shared_n < 0 without offsets
    refused(2, d_p.data_ptr(), 0, 0, 100, 0, None, s.cuda_stream)                       # a shared scan of 100 beams at NULL
    refused(2, d_p.data_ptr(), d_pts.data_ptr(), d_offs.data_ptr(), 0, -5, None, s.cuda_stream)
    with pytest.raises(capi.HsmError):
        g.update_by_scans(sc.build_poses[4:6], pts, np.int32([0, 50, 20]))              # offsets that decrease
    g.update_by_scans_device(0, 0, 0, 0, 0, 0, None, s.cuda_stream)                     # count == 0: accepted, nothing to do
    g.update_by_scans(np.zeros((0, 3), np.float32), np.zeros((0, 2), np.float32), np.int32([0]))
    # while `stream` is being captured
    x = torch.zeros(8, device="cuda:0")
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        x.add_(1.0)
        assert "captur" in refused(2, d_p.data_ptr(), d_pts.data_ptr(), d_offs.data_ptr(), 0, 1081, None, s.cuda_stream)
        x.add_(1.0)
    torch.cuda.synchronize()
    g.synchronize()
    assert g.getUpdateIndex(0) == idx
    for a, b in zip(before, planes(g)):
        assert all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in zip(a, b)), "a refused call changed the map"
    g.update_by_scans_device(2, d_p.data_ptr(), d_pts.data_ptr(), d_offs.data_ptr(), 0, 1081, None, s.cuda_stream)  # the capture has ended
    g.synchronize()
    assert g.getUpdateIndex(0) == idx + 2
    del keep
    g.close()
