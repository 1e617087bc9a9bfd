"""Every form of the map update on RESTORED levels: planes uploaded with hsm_upload_level whose stamps lie at or ahead of the
context's update counter (tests/stamp_cases.py), then integrated, against the CPU checkers bit for bit.

The reference's cell rules read the stored stamp: a cell whose stamp is at or past the scan's occupied mark stays as it is, a
cell whose stamp equals the scan's free mark takes no free update and, under an end, unsetFree in front of the occupied one
(map_update.h "stored stamps").  tests/test_stamp_reference.py pins, on the CPU, that every class of such cells is touched on
both levels of both geometries and that a rule which ignores the stamp misses every class.

Geometries (64, 64, 2) and (90, 24, 2), a fresh counter and one warmed by 5 updates, both layouts, both beam orders.  Forms:
hsm_update_by_scan keyed and byte-map (and with HSM_DENSE_BITS=0), hsm_update_by_scan_level, hsm_update_by_scans,
hsm_update_by_scans_device in one call and scan by scan, .._origos, .._gated with a gate that accepts some scans and rejects
others, hsm_slam_scans_device, hsm_retain_scan + hsm_update_by_ingested; the same-context and the fresh-context round trip.

After every call: hsm_download_level (both planes), hsm_download_prob, hsm_download_cells over the whole level,
hsm_update_index, hsm_occupancy_changes against the checker's grid, hsm_take_dirty_bbox around every changed cell; at the end
one hsm_match, pose and covariance bits.

On the kernels before the stamp-aware apply passes every test of this file fails (the round-trip test on its fresh-context
half; the same-context half holds on both): the frozen cells, the stored free marks (ended and only crossed), the stored occupied marks, the thawing cells and the clamp
cells all take the stamp-blind update."""
import numpy as np
import pytest

import stamp_cases as sc
from conftest import bits, oracle_kinds
from support import capi, dev, layout_of, pack, single_update

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max
PARAMS = [(g, U, layout, order) for g in sc.GEOMETRIES for U in sc.COUNTERS for layout in ("quad", "plane") for order in sc.ORDERS]
IDS = ["%s-U%d-%s-%s" % (sc.gid(g), U, layout, order) for g, U, layout, order in PARAMS]


class Restored:
    """a device context and the checkers, both warmed to counter U and restored from stamp_cases' planes"""

    def __init__(self, capi, oracle_mod, geom, U, layout, upload=True):
        self.capi, self.om, self.geom, self.U = capi, oracle_mod, geom, U
        self.g = capi.MapRepMultiMap(sc.RES, geom[0], geom[1], geom[2], layout=layout_of(capi, layout))
        self.g.setUpdateFactorFree(sc.FACTOR_FREE)
        self.g.setUpdateFactorOccupied(sc.FACTOR_OCC)
        self.refs = {kind: sc.new_checker(oracle_mod, kind, geom) for kind in oracle_kinds()}
        for _ in range(U // 3):
            single_update(capi, self.g, sc.sensor_pose(geom), sc.warm_scan())
            for o in self.refs.values():
                sc.checker_update(o, sc.sensor_pose(geom), sc.warm_scan())
        self.updates = U // 3
        if upload:
            for m in [self.g] + list(self.refs.values()):
                sc.upload(m, geom, U)
        self.grids = [np.full((geom[1] >> lvl, geom[0] >> lvl), 55, np.int8) for lvl in range(sc.LEVELS)]
        self.before = self.planes()
        for lvl in range(sc.LEVELS):
            self.g.take_dirty_bbox(lvl)

    def planes(self):
        return [self.g.download_level(lvl) for lvl in range(sc.LEVELS)]

    def check(self, applied, what, snaps=None):
        """the context after `applied` more updates against the checkers' present state (or `snaps`: {kind: planes per level})"""
        g = self.g
        self.updates += applied
        now = self.planes()
        for lvl, (lo_g, ui_g) in enumerate(now):
            sx, sy = sc.dims(self.geom, lvl)
            for kind, o in self.refs.items():
                lo_o, ui_o = snaps[kind][lvl] if snaps else o.download_level(lvl)
                w = (what, kind, "level", lvl)
                assert np.array_equal(ui_g, ui_o), w + ("stamps", int((ui_g != ui_o).sum()))
                assert np.array_equal(bits(lo_g), bits(lo_o)), w + ("log odds", int((bits(lo_g) != bits(lo_o)).sum()))
                _, prob = self.om.libm_expf(lo_o.reshape(-1), kind)
                assert np.array_equal(bits(g.download_prob(lvl)).reshape(-1), bits(prob)), w + ("probability",)
                if kind == "ho":
                    bb = g.occupancy_changes(lvl, self.grids[lvl])
                want = np.where(lo_o < 0, 0, np.where(lo_o > 0, 100, -1)).astype(np.int8)  # publishMap's thresholds
                if not snaps:
                    assert np.array_equal(want, o.occupancy_grid(lvl)), w
                assert np.array_equal(self.grids[lvl], want), w + ("occupancy changes", bb)
            cells = np.empty((sy, sx, 2), np.int32)
            self.capi._check(g._lib.hsm_download_cells(g._h, lvl, 0, 0, sx - 1, sy - 1, cells.ctypes.data, sx), "hsm_download_cells")
            assert np.array_equal(cells[:, :, 0].view(np.uint32), bits(lo_g)) and np.array_equal(cells[:, :, 1], ui_g), (what, lvl, "cells")
            assert g.getUpdateIndex(lvl) == self.updates - 1, (what, lvl, g.getUpdateIndex(lvl), self.updates)
            assert g.debug_marks_nonzero(lvl) == (0, 0), (what, lvl, "marks left behind")
            x0, y0, x1, y1 = (int(v) for v in g.take_dirty_bbox(lvl))
            changed = (bits(lo_g) != bits(self.before[lvl][0])) | (ui_g != self.before[lvl][1])
            ys, xs = np.nonzero(changed)
            if len(ys):
                assert x0 <= xs.min() and xs.max() <= x1 and y0 <= ys.min() and ys.max() <= y1, (what, lvl, "dirty box", (x0, y0, x1, y1))
        self.before = now

    def check_match(self, what):
        pose = sc.sensor_pose(self.geom) + np.float32([0.02, -0.015, 0.01])
        pts = np.ascontiguousarray(sc.short_scan()[::3])
        pg, cg = self.g.matchData(pose, pts)
        for kind, o in self.refs.items():
            po, co = o.match(pose, pts)
            assert np.array_equal(bits(pg), bits(po)) and np.array_equal(bits(cg), bits(co)), (what, kind, "match", pg, po)

    def close(self):
        self.g.close()
        for o in self.refs.values():
            o.close()


# ---- single scans --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom,U,layout,order", PARAMS, ids=IDS)
def test_single_scan_forms_on_restored_levels(capi, oracle_mod, monkeypatch, geom, U, layout, order):
    """hsm_update_by_scan: the keyed one-launch form (4095 beams), the byte-map form (4096) and the same scan with
    HSM_DENSE_BITS=0; two scans each, so the second meets the first one's stamps and the restored U+3 .. U+5"""
    pose = sc.sensor_pose(geom)
    for form in ("keyed", "dense", "dense, byte map off"):
        if form == "dense, byte map off":
            monkeypatch.setenv("HSM_DENSE_BITS", "0")
        r = Restored(capi, oracle_mod, geom, U, layout)
        monkeypatch.delenv("HSM_DENSE_BITS", raising=False)
        pts = sc.keyed_scan(order) if form == "keyed" else sc.dense_scan(order)
        assert (len(pts) < sc.DENSE_BEAMS) == (form == "keyed")
        for k in range(2):
            single_update(capi, r.g, pose, pts)
            for o in r.refs.values():
                sc.checker_update(o, pose, pts)
            r.check(1, (form, "scan", k))
        r.check_match(form)
        r.close()


@pytest.mark.parametrize("geom,U,layout,order", PARAMS, ids=IDS)
def test_update_by_scan_level_on_restored_levels(capi, oracle_mod, geom, U, layout, order):
    r = Restored(capi, oracle_mod, geom, U, layout)
    pose, pts = sc.sensor_pose(geom), sc.keyed_scan(order)
    for lvl in range(sc.LEVELS):
        r.g.update_by_scan_level(lvl, pose, pts * np.float32(1.0 / 2 ** lvl))
    for o in r.refs.values():
        sc.checker_update(o, pose, pts)
    r.check(1, "hsm_update_by_scan_level")
    r.check_match("hsm_update_by_scan_level")
    r.close()


def test_update_by_ingested_on_restored_levels(capi, oracle_mod):
    """hsm_retain_scan + hsm_update_by_ingested: a 720-beam fan converted on the device"""
    rng = np.random.default_rng(7401)
    ranges = rng.uniform(0.45, 1.5, 720).astype(np.float32)
    for geom, U, layout, _ in PARAMS[::2]:
        r = Restored(capi, oracle_mod, geom, U, layout)
        pts = r.g.ingest_laser_scan(ranges, -np.pi, 2 * np.pi / 720, 0.1, 30.0)
        assert len(pts) == 720
        a = np.ascontiguousarray(pts, np.float32)
        capi._check(r.g._lib.hsm_retain_scan(r.g._h, a.ctypes.data, a.shape[0], np.zeros(2, np.float32)), "hsm_retain_scan")
        r.g.update_by_ingested(sc.sensor_pose(geom))
        for o in r.refs.values():
            sc.checker_update(o, sc.sensor_pose(geom), a)
        r.check(1, ("hsm_update_by_ingested", sc.gid(geom), U, layout))
        r.close()


# ---- batches -------------------------------------------------------------------------------------------------------------------------
def checker_snaps(r, poses, scans, origos=None):
    """drive the checkers through the batch -> [after scan k: {kind: planes per level}]"""
    snaps = []
    for k, (pose, pts) in enumerate(zip(poses, scans)):
        for o in r.refs.values():
            o.build_map(pose[None, :], [pts], origo=np.zeros(2, np.float32) if origos is None else origos[k])
        snaps.append({kind: sc.snapshot(o) for kind, o in r.refs.items()})
    return snaps


@pytest.mark.parametrize("geom,U,layout,order", PARAMS, ids=IDS)
def test_batch_forms_on_restored_levels(capi, oracle_mod, geom, U, layout, order):
    """the batch of 8 through hsm_update_by_scans, hsm_update_by_scans_device (one call; scan by scan, checked after every scan)
    and hsm_update_by_scans_device_origos: the marks move per scan, the U+10 / U+11 cells thaw behind scan 3"""
    import torch
    poses, scans = sc.batch(geom, order)
    pts, offs = pack(scans)
    s = torch.cuda.current_stream()
    d_poses, d_pts, d_offs = dev(poses), dev(pts), dev(offs)
    n_max = max(len(x) for x in scans)

    r = Restored(capi, oracle_mod, geom, U, layout)
    snaps = checker_snaps(r, poses, scans)
    r.g.update_by_scans(poses, pts, offs)
    r.check(sc.BATCH, "hsm_update_by_scans")
    r.check_match("hsm_update_by_scans")
    r.close()

    r = Restored(capi, oracle_mod, geom, U, layout)
    r.g.update_by_scans_device(sc.BATCH, d_poses.data_ptr(), d_pts.data_ptr(), d_offs.data_ptr(), 0, n_max, None, s.cuda_stream)
    r.g.synchronize()
    r.check(sc.BATCH, "hsm_update_by_scans_device, one call", snaps=snaps[-1])
    r.close()

    r = Restored(capi, oracle_mod, geom, U, layout)
    keep = []
    for k in range(sc.BATCH):
        keep.append((dev(poses[k:k + 1]), dev(scans[k]), dev(np.int32([0, len(scans[k])]))))
        r.g.update_by_scans_device(1, keep[-1][0].data_ptr(), keep[-1][1].data_ptr(), keep[-1][2].data_ptr(), 0, n_max, None, s.cuda_stream)
        r.g.synchronize()
        r.check(1, ("hsm_update_by_scans_device, scan by scan", k), snaps=snaps[k])
    r.close()

    r = Restored(capi, oracle_mod, geom, U, layout)
    origos = np.float32([[0.2 * (k % 3) - 0.2, 0.15 * (k % 2)] for k in range(sc.BATCH)])
    checker_snaps(r, poses, scans, origos)
    d_origos = dev(origos)
    r.g.update_by_scans_device_origos(sc.BATCH, d_poses.data_ptr(), d_pts.data_ptr(), d_offs.data_ptr(), 0, n_max, d_origos.data_ptr(), s.cuda_stream)
    r.g.synchronize()
    r.check(sc.BATCH, "hsm_update_by_scans_device_origos")
    r.check_match("hsm_update_by_scans_device_origos")
    r.close()


@pytest.mark.parametrize("geom,U,layout,order", PARAMS, ids=IDS)
def test_gated_batch_on_restored_levels(capi, oracle_mod, geom, U, layout, order):
    """the marks advance by the APPLIED count: which scan thaws a cell depends on the gate"""
    import torch
    poses, scans = sc.batch(geom, order)
    pts, offs = pack(scans)
    r = Restored(capi, oracle_mod, geom, U, layout)
    ho = r.refs["ho"]
    last, flags = np.float32([FLT_MAX] * 3), []
    for k in range(sc.BATCH):
        go = ho.pose_difference_larger_than(poses[k], last, sc.GATE_MIN_DIST, sc.GATE_MIN_ANGLE)
        flags.append(int(go))
        if go:
            last = poses[k].copy()
            for o in r.refs.values():
                sc.checker_update(o, poses[k], scans[k])
    assert flags[0] == 1 and 0 in flags and sum(flags) > sc.M_THAW + 1, flags  # some rejected; the thaw stamps are passed
    s = torch.cuda.current_stream()
    d = [dev(poses), dev(pts), dev(offs), torch.full((sc.BATCH,), -7, dtype=torch.int32, device="cuda:0")]
    r.g.set_update_gate(sc.GATE_MIN_DIST, sc.GATE_MIN_ANGLE)
    r.g.update_by_scans_device_gated(sc.BATCH, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 0, max(len(x) for x in scans), None, 0,
                                     d[3].data_ptr(), s.cuda_stream)
    r.g.synchronize()
    assert d[3].cpu().numpy().tolist() == flags
    r.check(sum(flags), ("hsm_update_by_scans_device_gated", flags))
    r.check_match("hsm_update_by_scans_device_gated")
    r.close()


@pytest.mark.parametrize("geom,U,layout,order", PARAMS, ids=IDS)
def test_slam_scans_device_on_restored_levels(capi, oracle_mod, geom, U, layout, order):
    """a log of 8 scans through match, gate and update on the device against HectorSlamProcessor::update on the checkers"""
    import torch
    poses, scans = sc.batch(geom, order)
    scans = [np.ascontiguousarray(x[::2]) for x in scans]
    pts, offs = pack(scans)
    thr = (0.03, 0.02)
    deltas = np.concatenate([np.zeros((1, 3), np.float32), np.diff(poses, axis=0)]).astype(np.float32)
    r = Restored(capi, oracle_mod, geom, U, layout)
    want = {}
    for kind, o in r.refs.items():
        o.proc_set_thresholds(*thr)
        pose, last, out = poses[0].copy(), np.float32([FLT_MAX] * 3), []
        for k in range(sc.BATCH):
            o.proc_update(scans[k], (pose + deltas[k]).astype(np.float32), np.zeros(2, np.float32), False)
            pose, cov = o.proc_last_pose()
            go = o.pose_difference_larger_than(pose, last, *thr)
            if go:
                last = pose.copy()
            out.append((pose.copy(), cov.copy(), int(go)))
        want[kind] = out
    flags = [x[2] for x in want["ho"]]
    s = torch.cuda.current_stream()
    d = [dev(poses[0]), dev(deltas), dev(pts), dev(offs), torch.full((sc.BATCH, 3), -777.0, device="cuda:0"),
         torch.full((sc.BATCH, 9), -777.0, device="cuda:0"), torch.full((sc.BATCH,), -7, dtype=torch.int32, device="cuda:0")]
    r.g.set_update_gate(*thr)
    r.g.slam_scans_device(sc.BATCH, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), max(len(x) for x in scans), None, 0,
                          d[4].data_ptr(), d[5].data_ptr(), d[6].data_ptr(), s.cuda_stream)
    r.g.synchronize()
    got_pose, got_cov, got_flags = d[4].cpu().numpy(), d[5].cpu().numpy(), d[6].cpu().numpy().tolist()
    for kind, out in want.items():
        for k, (pose, cov, go) in enumerate(out):
            assert np.array_equal(bits(got_pose[k]), bits(pose)) and np.array_equal(bits(got_cov[k]), bits(cov)), (kind, k, got_pose[k], pose)
        assert got_flags == [x[2] for x in out], (kind, got_flags)
    assert sum(flags) >= 2, flags
    r.check(sum(flags), ("hsm_slam_scans_device", flags))
    r.close()


# ---- round trips ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ("quad", "plane"))
@pytest.mark.parametrize("geom", sc.GEOMETRIES, ids=sc.gid)
def test_round_trips_on_the_device(capi, oracle_mod, geom, layout):
    """W scans, download, upload into the SAME context, W more == 2 W scans; the same planes uploaded into a FRESH context are
    what the checker makes of them -- not the uninterrupted run (the restored stamps lie ahead of the fresh counter)"""
    poses, scans = sc.batch(geom)
    W = sc.BATCH // 2
    whole = Restored(capi, oracle_mod, geom, 0, layout, upload=False)
    for k in range(2 * W):
        single_update(capi, whole.g, poses[k], scans[k])
        for o in whole.refs.values():
            sc.checker_update(o, poses[k], scans[k])
    whole.check(2 * W, "2 W scans")
    half = Restored(capi, oracle_mod, geom, 0, layout, upload=False)
    for k in range(W):
        single_update(capi, half.g, poses[k], scans[k])
        for o in half.refs.values():
            sc.checker_update(o, poses[k], scans[k])
    half.check(W, "W scans")
    saved = half.planes()
    fresh = Restored(capi, oracle_mod, geom, 0, layout, upload=False)
    for r in (half, fresh):
        for m in [r.g] + list(r.refs.values()):
            for lvl, (lo, ui) in enumerate(saved):
                m.upload_level(lvl, lo, ui)
        for k in range(W, 2 * W):
            single_update(capi, r.g, poses[k], scans[k])
            for o in r.refs.values():
                sc.checker_update(o, poses[k], scans[k])
    half.check(W, "same-context restore")
    fresh.check(W, "fresh-context restore")
    for a, b in zip(whole.planes(), half.planes()):
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]), "the same-context restore is not exact"
    for a, b in zip(whole.planes(), fresh.planes()):
        assert int(((bits(a[0]) != bits(b[0])) | (a[1] != b[1])).sum()) >= 8, "the fresh-context restore froze nothing"
    for r in (whole, half, fresh):
        r.close()
