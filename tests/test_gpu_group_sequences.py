"""The device group (hsm_group_*, csrc/group.hip) held to one context across call sequences: tests/group_cases.py's sequences of
hsm_group_match_batch_device calls, each on ONE group from creation to close, so that what the group keeps between calls -- the
device-side exchanges shaped for a row count, the per-replica result blocks, the all-gather blocks of the replicas that are not
the root, the gather mode -- meets a gathered row count that changes, a covariance array that comes and goes, a root that moves,
an empty root shard in the first call, one shared scan, a mode that changes, scans without beams.  Then the SLAM side of the
group on a rectangular off-centre map, and the refusals.

No tolerance anywhere: every comparison is on bit patterns.  Expected values do not come from a group:
  * poses: the CPU reference's match_many ("hr" where oracle/_ref is present, else "ho"), asked where it is defined (a scan
    with beams), and ONE context's hsm_match_batch_device on the same scans;
  * covariances: that context's.
Every output array, pose and covariance, is filled with NaN before each call: a row that was never written shows.  After a
direct gather (and an RCCL all-gather of equal shards) the blocks that the replicas other than the root keep are read back
from their raw device pointers and held to the same rows.

Three replicas on [0, 1 % ndev, 2 % ndev]; RCCL runs over distinct devices (one replica on a one-GPU machine).  Every sequence
is a valid use of the API: nothing here provokes the exchange's bounded wait."""
import types

import numpy as np
import pytest

import group_cases as gc
from conftest import bits, make_oracle, oracle_kinds
from support import capi, dev, device_to_host, pack, same, stream_ptr, upload_planes

pytestmark = pytest.mark.gpu

KIND = oracle_kinds()[-1]  # "hr" (reference-compiled) where available
NO_SCAN = np.zeros((0, 2), np.float32)
FACTORS = (0.4, 0.9)


def gather_const(capi, mode):
    return {gc.DIRECT: capi.GATHER_DIRECT, gc.PEER: capi.GATHER_PEER, gc.RCCL: capi.GATHER_RCCL}[mode]


def group_devices(mode):
    import torch
    ndev = torch.cuda.device_count()
    return list(range(ndev)) if mode == gc.RCCL else [0, 1 % ndev, 2 % ndev]


def differing(got, want):
    """rows of two [n, cols] arrays whose bits differ"""
    assert got.shape == want.shape and got.ndim == 2, (got.shape, want.shape)
    return np.flatnonzero((bits(got) != bits(want)).any(1)).tolist()


# ---- expected values: one context and the CPU reference, once per call of a sequence -------------------------------------------------
@pytest.fixture(scope="module")
def world(capi, oracle_mod):
    """the scene, the built map's planes, and want(name, k) -> (poses [total, 3], covariances [total, 9], rows the reference
    defines) of call k of a sequence; computed once, shared by the tests, never changed"""
    import torch
    sc = gc.make_scene()
    one = capi.MapRepMultiMap(sc.resolution, sc.map_size, sc.map_size, sc.levels)
    one.setUpdateFactorFree(FACTORS[0])
    one.setUpdateFactorOccupied(FACTORS[1])
    one.build_map(sc.build_poses, sc.build_scans)
    one.synchronize()
    assert one.parity() == capi.PARITY_AUTO
    o = make_oracle(oracle_mod, KIND, sc)
    planes = [one.download_level(lvl) for lvl in range(sc.levels)]
    for lvl in range(sc.levels):
        lo, ui = o.download_level(lvl)
        assert same(planes[lvl][0], lo) and np.array_equal(planes[lvl][1], ui), lvl
    made = {}

    def want(name, k):
        if (name, k) in made:
            return made[(name, k)]
        init, scans = gc.call_batch(sc, name, k)
        total = len(init)
        shared = gc.SEQUENCES[name]["form"] == "shared"
        pose = torch.full((max(total, 1), 3), float("nan"), dtype=torch.float32, device="cuda:0")
        cov = torch.full((max(total, 1), 9), float("nan"), dtype=torch.float32, device="cuda:0")
        defined = np.zeros(total, bool)
        if total:
            if shared:
                scans = [scans] * total
            pts, offs = pack(scans)
            d_init, d_pts, d_offs = dev(init), dev(pts if len(pts) else np.zeros((1, 2), np.float32)), dev(offs)
            torch.cuda.synchronize()
            if shared:
                one.match_batch_device(total, d_init.data_ptr(), d_pts.data_ptr(), 0, len(scans[0]), pose.data_ptr(), cov.data_ptr(),
                                       stream_ptr())
            else:
                one.match_batch_device(total, d_init.data_ptr(), d_pts.data_ptr(), d_offs.data_ptr(), 0, pose.data_ptr(), cov.data_ptr(),
                                       stream_ptr())
            torch.cuda.synchronize()
            defined = np.array([len(s) > 0 for s in scans])
        pose, cov = pose.cpu().numpy()[:total], cov.cpu().numpy()[:total]
        if defined.any():
            rows = np.flatnonzero(defined)
            r_pts, r_offs = pack([scans[i] for i in rows])
            ref = o.match_many(init[rows], r_pts, r_offs)
            assert not np.isnan(pose[rows]).any() and not np.isnan(cov[rows]).any(), (name, k, "the single context left rows unwritten")
            bad = differing(pose[rows], ref)
            assert not bad, (name, k, f"the single context differs from the reference ({KIND}) in rows", rows[bad].tolist())
        made[(name, k)] = (pose, cov, defined)
        return made[(name, k)]

    yield types.SimpleNamespace(sc=sc, planes=planes, want=want)
    one.close()
    o.close()


def new_group(capi, w, devices):
    """a group on `devices` with the update factors set and the built map in every member"""
    grp = capi.MapRepGroup(w.sc.resolution, w.sc.map_size, w.sc.map_size, w.sc.levels, devices)
    try:
        grp.set_update_factors(*FACTORS)
        for r in range(grp.size()):
            upload_planes(grp.member(r), w.planes)
        grp.synchronize()
    except Exception:
        grp.close()
        raise
    return grp


class Shards:
    """one call's shards on the replicas' devices, and NaN-filled result arrays on the root's; kept until the call has been waited for"""

    def __init__(self, sc, name, k, call, devices):
        import torch
        init, scans = gc.call_batch(sc, name, k)
        self.shared = gc.SEQUENCES[name]["form"] == "shared"
        self.counts, self.root = call.counts, call.root
        self.total = len(init)
        first = gc.first_rows(call.counts)
        assert first[-1] == self.total and self.total <= gc.MAX_ROWS
        self.keep, self.begin, self.pts, self.offs = [], [], [], []
        for r, n in enumerate(call.counts):
            d = torch.device("cuda", devices[r])
            b, e = first[r], first[r + 1]
            p, of = (np.asarray(scans, np.float32), None) if self.shared else pack(scans[b:e])
            t_begin = torch.from_numpy(np.ascontiguousarray(init[b:e])).to(d) if n else None
            t_pts = torch.from_numpy(np.ascontiguousarray(p if len(p) else np.zeros((1, 2), np.float32))).to(d) if n else None
            t_offs = None if self.shared else torch.from_numpy(of).to(d)
            self.keep += [t_begin, t_pts, t_offs]
            self.begin.append(t_begin.data_ptr() if n else 0)
            self.pts.append(t_pts.data_ptr() if n else 0)
            self.offs.append(t_offs.data_ptr() if t_offs is not None else 0)
        self.shared_n = len(scans) if self.shared else 0
        rdev = torch.device("cuda", devices[call.root])
        self.pose = torch.full((max(self.total, 1), 3), float("nan"), dtype=torch.float32, device=rdev)
        self.cov = torch.full((max(self.total, 1), 9), float("nan"), dtype=torch.float32, device=rdev)
        torch.cuda.synchronize()

    def run(self, grp, want_cov=True, **over):
        a = dict(counts=self.counts, begin=self.begin, pts=self.pts, root=self.root)
        a.update(over)
        grp.match_batch_device(a["counts"], a["begin"], a["pts"], None if self.shared else self.offs, self.shared_n, a["root"],
                               self.pose.data_ptr(), self.cov.data_ptr() if want_cov else 0)

    def host(self):
        return self.pose.cpu().numpy(), self.cov.cpu().numpy()


def check_call(grp, sh, call, want, what, read_gathered):
    """the root's arrays are the expected rows [0, total) -- a covariance array that was not passed stays NaN, like every row of
    an all-zero call --, and so is every other replica's gathered block where the gather leaves one"""
    pose_w, cov_w, _ = want
    pose, cov = sh.host()
    total = sh.total
    assert np.isnan(pose[total:]).all() and np.isnan(cov[total:]).all(), what
    bad = differing(pose[:total], pose_w)
    assert not bad, (what, "pose rows", bad, pose[:total][bad], pose_w[bad])
    if call.want_cov:
        bad = differing(cov[:total], cov_w)
        assert not bad, (what, "covariance rows", bad)
    else:
        assert np.isnan(cov).all(), (what, "the covariance array was not passed")
    n_blocks = 0
    if read_gathered and total:
        for r in range(grp.size()):
            if r == call.root:
                continue
            bad = differing(device_to_host(grp.gathered(r), (total, 3)), pose_w)
            assert not bad, (what, f"replica {r}'s gathered pose rows", bad)
            if call.want_cov:
                bad = differing(device_to_host(grp.gathered(r, want_cov=True), (total, 9)), cov_w)
                assert not bad, (what, f"replica {r}'s gathered covariance rows", bad)
            n_blocks += 1
    return n_blocks


# ---- the sequences -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,name", [(m, n) for m in (gc.DIRECT, gc.PEER, gc.RCCL) for n in gc.SEQUENCES_OF[m]])
def test_sequence_on_one_group(capi, world, mode, name):
    """every call of the sequence on one group: synchronize() is OK, the root's rows [0, total) are the expected bits, and so
    are the gathered blocks of the other replicas after a direct gather or an all-gather of equal shards"""
    devices = group_devices(mode)
    grp = new_group(capi, world, devices)
    try:
        grp.set_gather(gather_const(capi, mode))
        now = mode
        rows = blocks = 0
        calls = gc.SEQUENCES[name]["calls"]
        for k, call in enumerate(calls):
            if call.mode is not None and mode != gc.RCCL:
                grp.set_gather(gather_const(capi, call.mode))
                now = call.mode
            assert grp.gather_mode()[0] == now, (name, k, grp.gather_mode())
            there = gc.reshard(call, len(devices))
            sh = Shards(world.sc, name, k, there, devices)
            sh.run(grp, there.want_cov)
            grp.synchronize()
            equal = there.counts[0] > 0 and len(set(there.counts)) == 1
            blocks += check_call(grp, sh, there, world.want(name, k), (name, mode, "call", k, there),
                                 read_gathered=now == gc.DIRECT or (now == gc.RCCL and equal))
            rows += sh.total
        print(f"\ngroup sequence | {name} | {mode} | {len(calls)} calls | {rows} pose rows, covariance rows and {blocks} gathered blocks matched")
    finally:
        grp.close()


# ---- the SLAM side -------------------------------------------------------------------------------------------------------------------
def state(g):
    """per level (log odds, stamps, update index)"""
    return [g.download_level(lvl) + (g.getUpdateIndex(lvl),) for lvl in range(g.getMapLevels())]


def same_state(a, b):
    return all(same(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2] == y[2] for x, y in zip(a, b))


def assert_replicas_are(grp, ref, what):
    for r in range(grp.size()):
        for lvl, (x, y) in enumerate(zip(state(grp.member(r)), ref)):
            w = (what, "replica", r, "level", lvl)
            assert same(x[0], y[0]), w + ("log odds", int((bits(x[0]) != bits(y[0])).sum()))
            assert np.array_equal(x[1], y[1]), w + ("stamps", int((x[1] != y[1]).sum()))
            assert x[2] == y[2], w + ("update index", x[2], y[2])


def test_slam_side_on_a_rectangular_off_centre_map(capi, oracle_mod):
    """process_scan steps, one without an update, one with a scan of no beams; a device-resident writer on replica 1 that the
    group does not replay, repaired by sync_maps with its dirty boxes; more steps.  One context runs alongside throughout, the
    CPU reference through the steps it defines"""
    import torch
    _, poses, scans = gc.slam_scene()
    sx, sy, levels, start = gc.SLAM_SX, gc.SLAM_SY, gc.SLAM_LEVELS, gc.SLAM_START
    ndev = torch.cuda.device_count()
    origo = np.float32([0.2, -0.1]) * np.float32(1.0 / gc.RES)
    grp = capi.MapRepGroup(gc.RES, sx, sy, levels, [0, 1 % ndev, 2 % ndev], startCoords=start)
    one = capi.MapRepMultiMap(gc.RES, sx, sy, levels, startCoords=start)
    o = oracle_mod.Oracle(KIND, gc.RES, sx, sy, levels, start)
    try:
        grp.set_update_factors(*FACTORS)
        one.setUpdateFactorFree(FACTORS[0])
        one.setUpdateFactorOccupied(FACTORS[1])
        o.set_update_factor_free(FACTORS[0])
        o.set_update_factor_occupied(FACTORS[1])
        assert grp.member(2).level_info(levels - 1)[:2] == (sx >> (levels - 1), sy >> (levels - 1))

        def step(t, hint, scan, update=True):
            pg, cg = grp.process_scan(hint, scan, origo, update)
            p1, c1 = one.matchData(hint, scan, None, origo)
            assert same(pg, p1) and same(cg, c1), ("step", t, pg, p1)
            if update:
                one.updateByScan(scan, p1, origo)
            return pg

        # 1. ten steps: every replica's planes are the single context's and the reference's
        hint = poses[0].copy()
        for t in range(gc.SLAM_FIRST):
            pg = step(t, hint, scans[t])
            po, _ = o.match(hint, scans[t], origo)
            assert same(pg, po), ("step", t, "the reference", KIND, pg, po)
            o.update_by_scan(po, scans[t], origo)
            o.on_map_updated()
            hint = pg + (poses[t + 1] - poses[t])
        grp.synchronize()
        ref = state(one)
        assert_replicas_are(grp, ref, "after the first steps")
        for lvl in range(levels):
            lo, ui = o.download_level(lvl)
            assert same(ref[lvl][0], lo) and np.array_equal(ref[lvl][1], ui), ("the reference", KIND, lvl)
        # 2. a match without an update: the pose, and nothing else
        t = gc.SLAM_FIRST
        pg = step(t, hint, scans[t], update=False)
        po, _ = o.match(hint, scans[t], origo)
        assert same(pg, po), ("no update", "the reference", KIND, pg, po)
        grp.synchronize()
        assert_replicas_are(grp, ref, "after a process_scan without an update")
        # 3. a scan of no beams, with an update
        pg = step(t + 1, hint, NO_SCAN)
        grp.synchronize()
        ref = state(one)
        assert_replicas_are(grp, ref, "after the empty scan")
        # 4. a device-resident writer on replica 1 alone; sync_maps with its dirty boxes, then without boxes
        m1 = grp.member(1)
        for lvl in range(levels):
            m1.take_dirty_bbox(lvl)
        k0 = t + 2
        w_scans = scans[k0:k0 + gc.SLAM_DEVICE]
        pts, offs = pack(w_scans)
        d1 = [torch.from_numpy(a).to(torch.device("cuda", 1 % ndev)) for a in (np.ascontiguousarray(poses[k0:k0 + gc.SLAM_DEVICE]), pts, offs)]
        d0 = [dev(poses[k0:k0 + gc.SLAM_DEVICE]), dev(pts), dev(offs)]
        torch.cuda.synchronize()
        most = max(len(s) for s in w_scans)
        m1.update_by_scans_device(gc.SLAM_DEVICE, d1[0].data_ptr(), d1[1].data_ptr(), d1[2].data_ptr(), 0, most, None, 0)
        one.update_by_scans_device(gc.SLAM_DEVICE, d0[0].data_ptr(), d0[1].data_ptr(), d0[2].data_ptr(), 0, most, None, 0)
        grp.synchronize()
        one.synchronize()
        assert same_state(state(grp.member(0)), ref) and same_state(state(grp.member(2)), ref)
        assert not same_state(state(m1), ref), "the writer changed nothing: the step would pass vacuously"
        boxes = np.stack([m1.take_dirty_bbox(lvl) for lvl in range(levels)])
        assert all(b[2] >= b[0] and b[3] >= b[1] for b in boxes), boxes
        grp.sync_maps(1, boxes)
        grp.synchronize()
        ref = state(one)
        assert_replicas_are(grp, ref, "after sync_maps with boxes")
        grp.sync_maps(1)
        grp.synchronize()
        assert_replicas_are(grp, ref, "after sync_maps without boxes")
        # 5. five more steps
        k1 = k0 + gc.SLAM_DEVICE
        hint = poses[k1].copy()
        for t in range(k1, k1 + gc.SLAM_LAST):
            pg = step(t, hint, scans[t])
            hint = pg + (poses[t + 1] - poses[t])
        grp.synchronize()
        assert_replicas_are(grp, state(one), "at the end")
    finally:
        grp.close()
        one.close()
        o.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_the_group_usable(capi, world):
    """host-side checks only: each bad call raises HsmError and writes nothing; the valid call straight after it gives the
    expected bits"""
    name, k = "totals", 0
    call = gc.SEQUENCES[name]["calls"][k]
    devices = group_devices(gc.DIRECT)
    grp = new_group(capi, world, devices)
    try:
        sh = Shards(world.sc, name, k, call, devices)
        neg = tuple(-1 if r == 1 else n for r, n in enumerate(call.counts))
        no_begin = [0 if r == 1 else p for r, p in enumerate(sh.begin)]
        no_pts = [0 if r == 0 else p for r, p in enumerate(sh.pts)]
        bad_calls = [("root -1", lambda: sh.run(grp, root=-1)), ("root = size", lambda: sh.run(grp, root=grp.size())),
                     ("a negative count", lambda: sh.run(grp, counts=neg)), ("NULL begin", lambda: sh.run(grp, begin=no_begin)),
                     ("NULL points", lambda: sh.run(grp, pts=no_pts)), ("sync_maps(from_=3)", lambda: grp.sync_maps(3))]
        for what, bad in bad_calls:
            with pytest.raises(capi.HsmError):
                bad()
            grp.synchronize()
            pose, cov = sh.host()
            assert np.isnan(pose).all() and np.isnan(cov).all(), (what, "a refused call wrote rows")
            ok = Shards(world.sc, name, k, call, devices)
            ok.run(grp)
            grp.synchronize()
            check_call(grp, ok, call, world.want(name, k), ("after", what), read_gathered=True)
        assert grp.gather_mode()[0] == gc.DIRECT
    finally:
        grp.close()
