"""One origo per scan, on the device, in the update entries (hsm_update_by_scans_device_origos,
hsm_update_by_scans_device_gated_origos), on the MI355X.  The bar is BIT-EXACT against the CPU checkers ("hr": the unmodified
reference, "ho": the restatement), driven per scan and per level through update_by_scan_level(l, pose, pts * 2^-l,
origo * 2^-l): the log-odds / update-index / probability planes of every level, the counters, the decisions of the gate.

Inputs: tests/origo_cases.py -- a 512 x 512 (once 500 x 360) 3-level map, 24 scans of 1081 beams, origos within +-6 cells.
Every test first asserts that the reference's result depends on the origos on every level
(origo_cases.assert_the_reference_depends_on_the_origo) and that "ho" met no undefined read.

Nothing here provokes a device fault."""
import numpy as np
import pytest

from conftest import bits, oracle_kinds
import support
from support import capi, dev, new_context, stream_ptr
import origo_cases as oc

pytestmark = pytest.mark.gpu

LEVELS, N = oc.LEVELS, oc.N


@pytest.fixture(scope="module")
def traj():
    return oc.trajectory()


@pytest.fixture(scope="module", autouse=True)
def guard(oracle_mod):
    for kind in oracle_kinds():
        oc.assert_the_reference_depends_on_the_origo(kind)


def pack(scans):
    """support.pack, with an empty log padded to one row so that the device pointer is not null"""
    pts, offs = support.pack(scans)
    return (pts if offs[-1] else np.zeros((1, 2), np.float32)), offs


def new_ctx(capi, geom="square", layout="quad"):
    sx, sy = oc.GEOMS[geom]
    return new_context(capi, oc.RES, sx, sy, LEVELS, layout=layout)


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
        assert g.getUpdateIndex(lvl) == h.getUpdateIndex(lvl), (what, lvl)


def device_update(g, poses, origos, scans=None, shared=None, stream=None):
    """hsm_update_by_scans_device_origos on torch buffers -> the buffers, which must outlive the update"""
    import torch
    s = stream or torch.cuda.current_stream()
    with torch.cuda.stream(s):
        d_origos = None if origos is None else dev(np.asarray(origos, np.float32).reshape(-1, 2))
        if shared is None:
            pts, offs = pack(scans)
            keep = [dev(np.asarray(poses, np.float32).reshape(-1, 3)), dev(pts), dev(offs), d_origos]
            g.update_by_scans_device_origos(len(scans), keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), 0, 1081,
                                            0 if d_origos is None else d_origos.data_ptr(), s.cuda_stream)
        else:
            keep = [dev(np.asarray(poses, np.float32).reshape(-1, 3)), dev(np.asarray(shared, np.float32)), d_origos]
            g.update_by_scans_device_origos(len(poses), keep[0].data_ptr(), keep[1].data_ptr(), 0, len(shared), 1081,
                                            0 if d_origos is None else d_origos.data_ptr(), s.cuda_stream)
    return keep


# ---- 4: the ungated update ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["quad", "plane"])
@pytest.mark.parametrize("geom", list(oc.GEOMS))
def test_ungated_update_with_an_origo_per_scan(capi, oracle_mod, traj, geom, layout):
    sc = traj
    g, refs = new_ctx(capi, geom, layout), oc.new_refs(oracle_mod, geom)
    for o in refs.values():
        for k in range(N):
            oc.ref_update(o, sc.poses[k], sc.scans[k], sc.origos[k])
    keep = device_update(g, sc.poses, sc.origos, sc.scans)
    g.synchronize()
    assert_same_as_refs(oracle_mod, g, refs, (geom, layout))
    for lvl in range(LEVELS):
        assert g.getUpdateIndex(lvl) == N - 1  # lastUpdateIndex starts at -1
    del keep
    g.close()


@pytest.mark.parametrize("geom", list(oc.GEOMS))
def test_one_shared_scan_at_24_poses_and_24_origos(capi, oracle_mod, traj, geom):
    sc = traj
    g, refs = new_ctx(capi, geom), oc.new_refs(oracle_mod, geom)
    for o in refs.values():
        for k in range(N):
            oc.ref_update(o, sc.poses[k], sc.scans[3], sc.origos[k])
    keep = device_update(g, sc.poses, sc.origos, shared=sc.scans[3])
    g.synchronize()
    assert_same_as_refs(oracle_mod, g, refs, ("shared scan", geom))
    del keep
    g.close()


# ---- 5: no behaviour change ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("origo", [(3.25, -4.5), None], ids=["one pair", "null"])
def test_equal_origos_give_the_parent_entry_bit_for_bit(capi, traj, origo):
    sc = traj
    g, h = new_ctx(capi, "rect"), new_ctx(capi, "rect")
    for m in (g, h):
        for lvl in range(LEVELS):
            m.take_dirty_bbox(lvl)
    keep = device_update(g, sc.poses, None if origo is None else np.tile(np.float32(origo), (N, 1)), sc.scans)
    pts, offs = pack(sc.scans)
    d = [dev(sc.poses), dev(pts), dev(offs)]
    h.update_by_scans_device(N, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 0, 1081, None if origo is None else np.float32(origo),
                             stream_ptr())
    assert g.last_launch_config() == h.last_launch_config()
    for lvl in range(LEVELS):
        assert np.array_equal(g.last_update_bbox(lvl), h.last_update_bbox(lvl)), lvl
        assert np.array_equal(g.take_dirty_bbox(lvl), h.take_dirty_bbox(lvl)), lvl
    assert_same_as_ctx(g, h, origo)
    for lvl in range(LEVELS):
        assert g.debug_marks_nonzero(lvl) == (0, 0)
    if origo is not None:  # and the pair is not a no-op: the map differs from the one built at 0,0
        z = new_ctx(capi, "rect")
        keep.append(device_update(z, sc.poses, None, sc.scans))
        z.synchronize()
        assert all((bits(a[0]) != bits(b[0])).any() for a, b in zip(planes(g), planes(z)))
        z.close()
    del keep, d
    g.close()
    h.close()


# ---- 6: the gated update --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forced", [False, True], ids=["gate alone", "force mask"])
@pytest.mark.parametrize("thr", list(oc.THRESHOLDS))
def test_gated_update_with_an_origo_per_scan(capi, oracle_mod, traj, thr, forced):
    import torch
    sc, t = traj, oc.THRESHOLDS[thr]
    geom = "rect" if thr == "wide" else "square"
    g, refs = new_ctx(capi, geom), oc.new_refs(oracle_mod, geom)
    force = None
    if forced:  # two scans the reference's gate rejects by itself (forcing the first moves lastMapUpdatePose for what follows)
        rejected = np.nonzero(~oc.Gate(refs["ho"], t).walk(sc.poses))[0]
        force = np.zeros(N, np.uint8)
        force[rejected[[0, 3]]] = 1
    flags, gate = None, None
    for kind, o in refs.items():
        gate = oc.Gate(o, t)
        f = gate.walk(sc.poses, force)
        assert flags is None or np.array_equal(f, flags), "the two checkers disagree on a decision"
        flags = f
        for k in np.nonzero(flags)[0]:
            oc.ref_update(o, sc.poses[k], sc.scans[k], sc.origos[k])
    unforced = oc.Gate(refs["ho"], t).walk(sc.poses)
    oc.assert_gate_is_exercised(unforced, (thr, "the gate alone"))  # (forcing rejected scans leaves fewer rejected ones)
    if forced:
        assert flags[force.astype(bool)].all() and (flags != unforced).any() and (~flags).sum() >= 3, flags.astype(int)
    g.set_update_gate(*t)
    pts, offs = pack(sc.scans)
    d = [dev(sc.poses), dev(pts), dev(offs), dev(sc.origos), None if force is None else dev(force),
         torch.full((N,), -7, dtype=torch.int32, device="cuda:0")]
    g.update_by_scans_device_gated_origos(N, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), 0, 1081, d[3].data_ptr(),
                                          0 if force is None else d[4].data_ptr(), d[5].data_ptr(), stream_ptr())
    g.synchronize()
    assert np.array_equal(d[5].cpu().numpy(), flags.astype(np.int32)), (d[5].cpu().numpy(), flags.astype(int))
    pose, total = g.update_gate_state()
    assert np.array_equal(bits(pose), bits(gate.last)) and total == gate.count == int(flags.sum())
    assert_same_as_refs(oracle_mod, g, refs, (thr, forced))
    for lvl in range(LEVELS):
        assert g.getUpdateIndex(lvl) == int(flags.sum()) - 1
    del d
    g.close()


# ---- 8: a NaN and an infinite origo in mid-log ---------------------------------------------------------------------------------------
def test_nan_and_infinite_origo_in_mid_log(capi, oracle_mod, traj):
    """On this input "hr" and "ho" agree bit for bit and "ho" meets no undefined read (x86's truncating conversion makes the
    begin cell INT_MIN, which fails the map test of every beam; asserted below before anything is compared), so the device is
    held to the checkers -- and, independently, to the two properties: the scan changes no cell and counts as an update."""
    sc = traj
    origos = sc.origos.copy()
    origos[9] = [np.nan, 1.0]
    origos[14] = [np.inf, -2.0]
    refs = oc.new_refs(oracle_mod)
    for kind, o in refs.items():
        for k in range(N):
            before = oc.level_planes(o) if k in (9, 14) else None
            oc.ref_update(o, sc.poses[k], sc.scans[k], origos[k])
            if before is not None:
                assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(before, oc.level_planes(o))), (kind, k)
    assert refs["ho"].undefined_reads() == 0
    if "hr" in refs:
        for lvl in range(LEVELS):
            assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(refs["ho"].download_level(lvl), refs["hr"].download_level(lvl)))
    g = new_ctx(capi)
    keep = []
    for a, b in ((0, 9), (9, 10), (10, 14), (14, 15), (15, N)):
        before, idx = (planes(g), g.getUpdateIndex(0)) if b - a == 1 else (None, None)
        keep.append(device_update(g, sc.poses[a:b], origos[a:b], sc.scans[a:b]))
        g.synchronize()
        if before is not None:
            for lvl, (x, y) in enumerate(zip(before, planes(g))):
                assert all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in zip(x, y)), ("the scan changed a plane", a, lvl)
                assert g.getUpdateIndex(lvl) == idx + 1, "the scan must still count as an update"
    assert_same_as_refs(oracle_mod, g, refs, "NaN / infinite origo")  # the neighbouring scans included
    for lvl in range(LEVELS):
        assert g.getUpdateIndex(lvl) == N - 1
    del keep
    g.close()
