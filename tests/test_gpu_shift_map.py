"""The window moved under the robot on the device (hsm_shift_map, hsm_map_start) against the reference, bit for bit.

The reference has no move.  A moved context must be indistinguishable from a checker created with the new start coordinates into
which the moved cells were loaded (shift_cases.moved_checker; the CPU pin tests/test_shift_reference.py shows that both checkers
agree on every case and that the cells move by whole cells).  The maps and moves are tests/shift_cases.py's: 64 x 64 x 2,
90 x 24 x 2 and 96 x 40 x 3 in the centred frame and in the frame of inexact scale and unequal translations, and (333, 90, 6)
with level widths 333, 166, 83, 41, 20, 10; the latter and the sensitive frame on 96 x 40 x 3 in the plane layout too.  Moves of
0, +-1, 3 / -2 coarsest cells, one that leaves a single cell of the coarsest level, one that clears every level.

Library default mode (the reference's summation order); every comparison is on uint32 views against oracle_kinds()[-1].
"""
import numpy as np
import pytest

import cast_cases
import frame_cases as fc
import shift_cases as sc
from conftest import bits, oracle_kinds
from support import capi, dev, new_context, same, stream_ptr

pytestmark = pytest.mark.gpu
KIND = oracle_kinds()[-1]
F = np.float32
HSM_ERR_INVALID = -1
CASES = pytest.mark.parametrize("name", sc.SHIFT_NAMES)
MAPS = pytest.mark.parametrize("m,layout", sc.MAP_LAYOUTS, ids=sc.MAP_LAYOUT_IDS)
DEEP_QUAD = (sc.MAPS[-1], "quad")
# the counters-carried variant builds its map from three scans of this many beams (+ 0, 1, 2).  Searched on the CPU among 60, 100,
# 150, 190, 197: with 150 and more the reference's estimate goes to NaN on (333, 90, 6) moved by (3, -2) -- a case it does not
# define (shift_cases.Guarded would fail it)
BUILD_BEAMS = 100


def new_ctx(capi, m, layout, start=None):
    """a cleared context in the map's frame (or at `start`) with the update factors of the cases"""
    return new_context(capi, m.resolution, m.geom[0], m.geom[1], m.geom[2], m.start if start is None else start, layout, fc.FACTORS)


def load(g, planes):
    for lvl, (lo, st) in enumerate(planes):
        g.upload_level(lvl, lo, st)
    for lvl in range(len(planes)):
        g.take_dirty_bbox(lvl)
    return g


def old_checker(oracle_mod, m, planes):
    """a checker of its own in the OLD frame that holds `planes` (the caller may change it), guarded like the moved one"""
    def make(kind):
        o = oracle_mod.Oracle(kind, m.resolution, m.geom[0], m.geom[1], m.geom[2], m.start)
        o.set_update_factor_free(fc.FACTORS[0])
        o.set_update_factor_occupied(fc.FACTORS[1])
        for lvl, (lo, st) in enumerate(planes):
            o.upload_level(lvl, lo, st)
        return o
    return sc.Guarded(oracle_mod, KIND, make)


def guarded(oracle_mod, m, name, planes=None, empty_updates=0):
    """the checker of the moved map, behind the restatement's count of undefined reads (shift_cases.Guarded)"""
    return sc.Guarded(oracle_mod, KIND, lambda kind: sc.moved_checker(oracle_mod, kind, m, name, planes, empty_updates))


def levels_of(x, n):
    return [x.download_level(lvl) for lvl in range(n)]


def assert_planes(what, got, want):
    for lvl, ((lo, st), (rlo, rst)) in enumerate(zip(got, want)):
        assert np.array_equal(st, rst), (what, lvl, "stamps", int((st != rst).sum()))
        assert same(lo, rlo), (what, lvl, "log-odds", int((bits(lo) != bits(rlo)).sum()))


def shift(g, m, name):
    kx, ky = sc.shift_of(m.geom, name)
    start = g.start_for_shift(kx, ky)
    return start, g.shift_map(start)


def whole(m, lvl):
    sx, sy = m.dims(lvl)
    return [0, 0, sx - 1, sy - 1]


# ---- 1. the moved context is the checker created at the new start ------------------------------------------------------------------
@CASES
@MAPS
def test_geometry_planes_matches_and_casts_after_a_move(capi, oracle_mod, m, layout, name):
    import torch
    planes = sc.old_planes(oracle_mod, m)
    g = load(new_ctx(capi, m, layout), planes)
    assert same(g.map_start(), np.asarray(m.start, F))
    want_start, refusal, d0, _ = sc.case_plan(m, name)
    start, got_d = shift(g, m, name)
    assert same(start, want_start) and same(g.map_start(), want_start), (start, want_start, g.map_start())
    assert got_d == d0, (got_d, d0)
    o = guarded(oracle_mod, m, name)
    rng = np.random.default_rng(2103)
    for lvl in range(m.levels):
        got, want = g.level_info(lvl), o.level_info(lvl)
        assert got[:2] == want[:2] and same(got[2:], want[2:]), (lvl, got, want)
        sx, sy = m.dims(lvl)
        for p in np.concatenate([rng.uniform([-2, -2, -3], [sx + 2, sy + 2, 3], (8, 3)), [[0, 0, 0], [sx - 1, sy - 1, 1]]]).astype(F):
            w = g.getWorldCoordsPose(lvl, p)
            assert same(w, o.world_coords_pose(lvl, p)), (lvl, p)
            assert same(g.getMapCoordsPose(lvl, w), o.map_coords_pose(lvl, w)), (lvl, w)
    assert_planes("moved", levels_of(g, m.levels), levels_of(o, m.levels))
    for lvl in range(m.levels):
        lo, _ = o.download_level(lvl)
        _, prob = oracle_mod.libm_expf(lo.reshape(-1), KIND)
        assert same(g.download_prob(lvl).reshape(-1), prob), (lvl, "probabilities")
        assert np.array_equal(g.occupancy_grid(lvl), o.occupancy_grid(lvl)), (lvl, "occupancy grid")
        if name != "zero":
            assert list(g.last_update_bbox(lvl))[2] < list(g.last_update_bbox(lvl))[0], (lvl, "last update box")
    # one match, and a batch of 65 (the texel plane in the quad layout)
    w0, pts = sc.case_scan(oracle_mod, m)
    pose, cov = g.matchData(w0, pts)
    rp, rc = o.match(w0, pts)
    assert same(pose, rp) and same(cov, rc), ("match", pose, rp)
    starts = sc.batch_starts(oracle_mod, m, name)
    d_in, d_pts = dev(starts), dev(pts)
    d_pose, d_cov = torch.zeros((65, 3), device="cuda:0"), torch.zeros((65, 9), device="cuda:0")
    g.match_batch_device(65, d_in.data_ptr(), d_pts.data_ptr(), 0, len(pts), d_pose.data_ptr(), d_cov.data_ptr(),
                         stream_ptr())
    torch.cuda.synchronize()
    want = [o.match(s, pts) for s in starts]
    assert same(d_pose.cpu().numpy(), np.stack([p for p, _ in want])), "batch poses"
    assert same(d_cov.cpu().numpy(), np.stack([c for _, c in want])), "batch covariances"
    # casts on level 0: 5 poses x 65 beams on the moved grid
    grid, meta = o.occupancy_grid(0), cast_cases.metadata(o, 0)
    poses, angles = np.asarray(m.truth(oracle_mod)[:5], F), cast_cases.beam_table(65)
    rmax = 0.45 * min(m.geom[0], m.geom[1]) * m.resolution
    rd, rh = cast_cases.expected_cast(KIND, grid, meta, poses, angles, rmax)
    d, h = g.cast_scans(0, poses, angles, rmax)
    assert same(d, rd), "cast ranges"
    has = rd >= 0
    assert same(h[has], rh[has]), "cast hit points"
    g.close()
    o.close()


# ---- 2. an update after the move --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ("stamps_restored", "stamps_cleared", "counters_carried"))
@CASES
@MAPS
def test_update_after_a_move(capi, oracle_mod, m, layout, name, variant):
    """(a) the map's stamps as they are (on the deep map they are ahead of a fresh context's counter: the restored-stamps form),
    (b) all -1, (c) the context is built by three real updates and keeps its counters over the move; the checker's are advanced
    by as many empty updates before its upload (tests/test_shift_reference.py)"""
    w0, pts = sc.case_scan(oracle_mod, m)
    n_before = 0
    if variant == "counters_carried":
        g, a = new_ctx(capi, m, layout), old_checker(oracle_mod, m, [])
        n_before = 3
        for k in range(n_before):
            g.matchData(w0, pts[: BUILD_BEAMS + k])
            a.match(w0, pts[: BUILD_BEAMS + k])
            g.updateByScan(pts[: BUILD_BEAMS + k], w0)
            a.update_by_scan(w0, pts[: BUILD_BEAMS + k])
        planes = levels_of(a, m.levels)
        a.close()
        assert_planes("built", levels_of(g, m.levels), planes)
    else:
        planes = sc.old_planes(oracle_mod, m)
        if variant == "stamps_cleared":
            planes = [(lo, np.full_like(st, -1)) for lo, st in planes]
        g = load(new_ctx(capi, m, layout), planes)
    counters = [g.getUpdateIndex(lvl) for lvl in range(m.levels)]
    shift(g, m, name)
    assert [g.getUpdateIndex(lvl) for lvl in range(m.levels)] == counters   # the counters stay
    o = guarded(oracle_mod, m, name, planes, empty_updates=n_before)
    assert_planes("moved", levels_of(g, m.levels), levels_of(o, m.levels))
    p, _ = g.matchData(w0, pts)
    rp, _ = o.match(w0, pts)
    assert same(p, rp)
    g.updateByScan(pts, rp)
    o.update_by_scan(rp, pts)
    assert_planes("updated", levels_of(g, m.levels), levels_of(o, m.levels))
    for lvl in range(m.levels):
        assert g.debug_marks_nonzero(lvl) == (0, 0), lvl
    g.close()
    o.close()


def test_dense_update_after_a_move_finds_no_stale_mark_or_key(capi, oracle_mod):
    """(333, 90, 6): a keyed update before the move leaves keys in the key planes; the 6000-beam scan of the deep case (the
    byte-map form: 4096 beams and more) after it gives the checker's planes, and both mark planes are zero again"""
    m, layout = DEEP_QUAD
    c = m.case()
    assert len(c.dense) >= 4096
    planes = sc.old_planes(oracle_mod, m)
    g, a = load(new_ctx(capi, m, layout), planes), old_checker(oracle_mod, m, planes)
    w0, pts = sc.case_scan(oracle_mod, m)
    g.matchData(w0, pts)
    a.match(w0, pts)
    g.updateByScan(pts, w0)
    a.update_by_scan(w0, pts)
    before = levels_of(a, m.levels)
    a.close()
    shift(g, m, "x1")
    o = guarded(oracle_mod, m, "x1", before, empty_updates=1)
    g.matchData(c.dense_pose, c.dense)
    o.match(c.dense_pose, c.dense)
    g.updateByScan(c.dense, c.dense_pose)
    o.update_by_scan(c.dense_pose, c.dense)
    assert_planes("dense update", levels_of(g, m.levels), levels_of(o, m.levels))
    for lvl in range(m.levels):
        assert g.debug_marks_nonzero(lvl) == (0, 0), lvl
    g.close()
    o.close()


# ---- 3. what a mirror and a publisher see ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_side", (False, True), ids=("host_box", "device_box"))
@MAPS
def test_publish_state_after_a_move(capi, oracle_mod, m, layout, device_side):
    """the dirty box and the publish box are the whole level once, afterwards only the next update's box; the exported grid is
    the checker's.  device_side: through hsm_occupancy_changes_device and its box on the device"""
    import torch
    planes = sc.old_planes(oracle_mod, m)
    g = load(new_ctx(capi, m, layout), planes)
    grids = [torch.full((m.dims(lvl)[1], m.dims(lvl)[0]), 55, dtype=torch.int8, device="cuda:0") for lvl in range(m.levels)]
    d_box = torch.zeros(4, dtype=torch.int32, device="cuda:0")

    def export(lvl):
        if device_side:
            g.occupancy_changes_device(lvl, grids[lvl].data_ptr(), d_box.data_ptr(), stream_ptr())
            g.synchronize()
            torch.cuda.synchronize()
            return [int(v) for v in d_box.cpu()], grids[lvl].cpu().numpy()
        host = grids[lvl].cpu().numpy().copy()
        bb = g.occupancy_changes(lvl, host)
        grids[lvl].copy_(torch.from_numpy(host))
        return [int(v) for v in bb], host

    for lvl in range(m.levels):
        export(lvl)
        assert export(lvl)[0][2] < export(lvl)[0][0], lvl
    shift(g, m, "x1")
    o = guarded(oracle_mod, m, "x1")
    for lvl in range(m.levels):
        assert [int(v) for v in g.take_dirty_bbox(lvl)] == whole(m, lvl), lvl
        assert g.take_dirty_bbox(lvl)[2] < 0, lvl
        bb, grid = export(lvl)
        assert bb == whole(m, lvl), (lvl, bb)
        assert np.array_equal(grid, o.occupancy_grid(lvl)), lvl
        bb, _ = export(lvl)
        assert bb[2] < bb[0], (lvl, bb)
    w0, pts = sc.case_scan(oracle_mod, m)
    g.matchData(w0, pts)
    o.match(w0, pts)
    g.updateByScan(pts, w0)
    o.update_by_scan(w0, pts)
    for lvl in range(m.levels):
        box = [int(v) for v in g.take_dirty_bbox(lvl)]
        bb, grid = export(lvl)
        assert bb == box, (lvl, bb, box)
        if lvl == 0:
            assert box[2] >= box[0] and box != whole(m, lvl), (lvl, box)   # an update's box, not the level
        assert np.array_equal(grid, o.occupancy_grid(lvl)), lvl
    g.close()
    o.close()


# ---- 4. moves in sequence, and the queue ------------------------------------------------------------------------------------------------
# (kx >= 0: a step against the first move's direction would bring back columns that the first move dropped -- cleared by then)
@pytest.mark.parametrize("k", ((1, 0), (0, -1), (3, -2)), ids=lambda k: "k%d_%d" % k)
@MAPS
def test_two_moves_equal_one_and_a_round_trip_clears_what_left(capi, oracle_mod, m, layout, k):
    planes = sc.old_planes(oracle_mod, m)
    top = m.levels - 1
    # (kx, ky), then on to the start of (kx + 1, ky): the offsets are derived from the start, never accumulated
    direct = sc.start_for_shift(m.start, m.geom, k[0] + 1, k[1])
    g1, g2 = load(new_ctx(capi, m, layout), planes), load(new_ctx(capi, m, layout), planes)
    assert g1.shift_map(sc.start_for_shift(m.start, m.geom, *k)) == (k[0] << top, k[1] << top)
    assert g1.shift_map(direct) == (1 << top, 0)
    assert g2.shift_map(direct) == ((k[0] + 1) << top, k[1] << top)
    assert same(g1.map_start(), direct) and same(g2.map_start(), direct)
    want = sc.shifted_levels(planes, ((k[0] + 1) << top, k[1] << top))
    assert_planes("two moves", levels_of(g1, m.levels), want)
    assert_planes("one move", levels_of(g2, m.levels), want)
    for lvl in range(m.levels):
        assert g1.level_info(lvl) == g2.level_info(lvl)
        p = np.array([1.5, -0.25, 0.3], F)
        assert same(g1.getWorldCoordsPose(lvl, p), g2.getWorldCoordsPose(lvl, p)) and same(g1.getMapCoordsPose(lvl, p), g2.getMapCoordsPose(lvl, p))
        assert same(g1.download_prob(lvl), g2.download_prob(lvl)), lvl
    # there and back: exactly the cells that left the window in between are cleared
    assert g2.shift_map(np.asarray(m.start, F)) == (-((k[0] + 1) << top), -(k[1] << top))
    assert same(g2.map_start(), np.asarray(m.start, F))
    back = sc.shifted_levels(want, (-((k[0] + 1) << top), -(k[1] << top)))
    assert_planes("round trip", levels_of(g2, m.levels), back)
    for lvl, ((lo, _), (blo, _)) in enumerate(zip(planes, back)):
        kept = blo != 0
        assert same(blo[kept], lo[kept]) and kept.sum() < lo.size, lvl   # what is left is what it was; something left the window
    g1.close()
    g2.close()


@MAPS
def test_an_update_queued_right_before_the_move_is_in_the_moved_planes(capi, oracle_mod, m, layout):
    planes = sc.old_planes(oracle_mod, m)
    g, a = load(new_ctx(capi, m, layout), planes), old_checker(oracle_mod, m, planes)
    w0, pts = sc.case_scan(oracle_mod, m)
    g.matchData(w0, pts)
    a.match(w0, pts)
    g.updateByScan(pts, w0)   # queued: returns before its kernels have run
    shift(g, m, "x-1_y1")
    a.update_by_scan(w0, pts)
    _, _, d0, _ = sc.case_plan(m, "x-1_y1")
    assert_planes("update, then move", levels_of(g, m.levels), sc.shifted_levels(levels_of(a, m.levels), d0))
    g.close()
    a.close()


# ---- 5. refusals and the zero move ------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_untouched(capi, oracle_mod):
    import torch
    m, layout = sc.MAP_LAYOUTS[5]   # 96 x 40 x 3, sensitive frame
    assert m.geom == (96, 40, 3)
    lib = capi.load_library()
    planes = sc.old_planes(oracle_mod, m)
    g = load(new_ctx(capi, m, layout), planes)
    start = g.map_start()

    def untouched(what):
        assert same(g.map_start(), start), what
        assert_planes(what, levels_of(g, m.levels), planes)
        for lvl in range(m.levels):
            assert g.take_dirty_bbox(lvl)[2] < 0, (what, lvl)
            assert g.level_info(lvl) == ref_info[lvl], (what, lvl)

    ref_info = [g.level_info(lvl) for lvl in range(m.levels)]
    d = np.full(2, 7, np.int32)
    s64 = start.astype(np.float64)
    for new, text in (((s64 + [1 / 96, 0]).astype(F), "multiple"),          # one level-0 cell on a 3-level map
                      ((s64 + [0, 6 / 40]).astype(F), "multiple"),
                      ((s64 + [4.5 / 96, 0]).astype(F), "1/64"),            # half a cell off
                      ((s64 + [0, (4 + 1 / 32) / 40]).astype(F), "1/64"),
                      (np.array([np.nan, start[1]], F), "finite"),
                      (np.array([start[0], np.inf], F), "finite")):
        rc = lib.hsm_shift_map(g._h, float(new[0]), float(new[1]), d.ctypes.data)
        msg = lib.hsm_last_error().decode()
        assert rc == HSM_ERR_INVALID and text in msg and "hsm_shift_map" in msg, (new, rc, msg)
        assert list(d) == [7, 7]
        untouched(msg)
    # a capture in progress on a stream the context has matched on
    w0, pts = sc.case_scan(oracle_mod, m)
    starts = np.repeat(w0[None], 4, 0).astype(F)
    t = [dev(starts), dev(pts), torch.zeros((4, 3), device="cuda:0")]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    launch = lambda: g.match_batch_device(4, t[0].data_ptr(), t[1].data_ptr(), 0, len(pts), t[2].data_ptr(), 0, s.cuda_stream)
    launch()
    s.synchronize()
    ok = g.start_for_shift(1, 0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        launch()
        rc = lib.hsm_shift_map(g._h, float(ok[0]), float(ok[1]), d.ctypes.data)
        msg = lib.hsm_last_error().decode()
    assert rc == HSM_ERR_INVALID and "captured" in msg, (rc, msg)
    torch.cuda.synchronize()
    assert list(d) == [7, 7]
    untouched("capture")
    assert g.shift_map(ok) == (4, 0)   # the capture over, the move goes through
    assert_planes("after the capture", levels_of(g, m.levels), sc.shifted_levels(planes, (4, 0)))
    g.close()


@MAPS
def test_a_zero_move_queues_nothing_and_changes_nothing(capi, oracle_mod, m, layout):
    planes = sc.old_planes(oracle_mod, m)
    g = load(new_ctx(capi, m, layout), planes)
    info = [g.level_info(lvl) for lvl in range(m.levels)]
    assert g.shift_map(g.map_start()) == (0, 0)
    assert g.shift_map(g.start_for_shift(0, 0)) == (0, 0)
    assert same(g.map_start(), np.asarray(m.start, F))
    for lvl in range(m.levels):
        assert g.take_dirty_bbox(lvl)[2] < 0, lvl   # no level was marked changed
        assert g.level_info(lvl) == info[lvl]
    assert_planes("zero move", levels_of(g, m.levels), planes)
    g.close()
