"""The device-resident entries on a context whose window has moved (hsm_shift_map), against the reference, bit for bit.

The cases are tests/moved_entry_cases.py's, pinned on the CPU by tests/test_moved_entries_reference.py: three maps (64 x 64 x 2,
96 x 40 x 3 in the sensitive frame, (333, 90, 6); the latter two in both layouts), the moves x1 and x3_y-2 (one_left for the
readers, and x4_y-1 on the deep map, where the reference loses track under x3_y-2), a trajectory of 4 + 4 scans around the move.  The reference has no move: the checker of everything after one is
created at the new start and loaded with the moved cells, its counters advanced by one empty update per scan applied so far.

  1. device-side updates outstanding at the move (the merge_device_boxes branch of hsm_shift_map), also with an origo per scan
  2. gated calls outstanding at the move (the fold_gate_counters branch), and with the fold done before the move
  3. hsm_slam_scans_device, its _origos form and hsm_slam_ranges_tf_device across a move queued without a wait
  4. the map readers on a moved map, every level
  5. hsm_copy_map / hsm_copy_map_boxes and moves on the one staging patch; again in a child with HSM_COPY_STAGE=1
  6. group members moved together, and one moved alone

Library default mode; every comparison is on uint32 views against oracle_kinds()[-1].  No tolerance anywhere.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import frame_cases as fc
import moved_entry_cases as mc
import shift_cases as sc
import test_gpu_copy_map as tcopy
import test_gpu_score_batch as tsb
import test_gpu_shift_map as tshift
import test_gpu_window as tw
import window_cases
from conftest import bits, oracle_kinds
from support import capi, dev, pack, same, stream_ptr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIND = oracle_kinds()[-1]
F = np.float32
HSM_ERR_INVALID = -1
EMPTY = [0, 0, -1, -1]
MAPS = pytest.mark.parametrize("m,layout", mc.MAP_LAYOUTS, ids=mc.MAP_LAYOUT_IDS)
MOVES = pytest.mark.parametrize("name", mc.MOVES)
DEEP_BOTH = [(mc.DEEP, "quad"), (mc.DEEP, "plane")]
LOOP_MAPS = [(mc.M64, "quad"), (mc.M96, "quad")] + DEEP_BOTH


def moved_cases(map_layouts):
    """every map and layout under its moves (moved_entry_cases.moves_of: the deep map has a third)"""
    cases = [(m, layout, name) for m, layout in map_layouts for name in mc.moves_of(m)]
    return pytest.mark.parametrize("m,layout,name", cases, ids=["%s-%s-%s" % (m.id, layout, name) for m, layout, name in cases])

new_ctx, load, levels_of, assert_planes, whole = tshift.new_ctx, tshift.load, tshift.levels_of, tshift.assert_planes, tshift.whole


def box(b):
    b = [int(v) for v in b]
    return EMPTY if b[2] < b[0] or b[3] < b[1] else b


def moved_start(m, name):
    return mc.case_plan(m, name)[0]


def posed_update(g, poses, scans, origos=None, gated=False):
    """hsm_update_by_scans_device (_origos, _gated) on torch buffers -> the buffers, which must outlive the update"""
    import torch
    pts, offs = pack(scans)
    keep = [dev(np.asarray(poses, F).reshape(-1, 3)), dev(pts), dev(offs), None if origos is None else dev(np.asarray(origos, F)),
            torch.full((len(scans),), -7, dtype=torch.int32, device="cuda:0")]
    if gated:
        g.update_by_scans_device_gated(len(scans), keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), 0, mc.MAX_BEAMS, None, 0,
                                       keep[4].data_ptr(), stream_ptr())
    elif origos is None:
        g.update_by_scans_device(len(scans), keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), 0, mc.MAX_BEAMS, None, stream_ptr())
    else:
        g.update_by_scans_device_origos(len(scans), keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), 0, mc.MAX_BEAMS,
                                        keep[3].data_ptr(), stream_ptr())
    return keep


def export_device(g, lvl, grid, d_box):
    import torch
    g.occupancy_changes_device(lvl, grid.data_ptr(), d_box.data_ptr(), stream_ptr())
    g.synchronize()
    torch.cuda.synchronize()
    return box(d_box.cpu())


# ---- 1. device-side updates outstanding at the move --------------------------------------------------------------------------------
def check_updates_outstanding(capi, oracle_mod, m, layout, name, origos):
    import torch
    t = mc.trajectory(oracle_mod, m)
    r = mc.posed_case(oracle_mod, KIND, m, name, False, origos)
    S = mc.SPLIT
    g = load(new_ctx(capi, m, layout), sc.old_planes(oracle_mod, m))
    grids = [torch.full((m.dims(lvl)[1], m.dims(lvl)[0]), 55, dtype=torch.int8, device="cuda:0") for lvl in range(m.levels)]
    d_box = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    for lvl in range(m.levels):
        export_device(g, lvl, grids[lvl], d_box)   # the first export is the whole level: out of the way
    keep = posed_update(g, r["poses"][:S], t.scans[:S], t.origos[:S] if origos else None)
    start = moved_start(m, name)
    g.shift_map(start)   # no host look since the update: its boxes are still on the device, in old coordinates
    assert_planes("moved", levels_of(g, m.levels), r["moved"])
    for lvl in range(m.levels):
        assert g.getUpdateIndex(lvl) == S - 1, (lvl, g.getUpdateIndex(lvl))
        assert box(g.last_update_bbox(lvl)) == EMPTY, (lvl, g.last_update_bbox(lvl))
        assert box(g.take_dirty_bbox(lvl)) == whole(m, lvl), lvl
        assert box(g.take_dirty_bbox(lvl)) == EMPTY, lvl
        assert export_device(g, lvl, grids[lvl], d_box) == whole(m, lvl), lvl
        assert export_device(g, lvl, grids[lvl], d_box) == EMPTY, lvl
    # a second context created at the new start with the moved planes: what the boxes of the next call have to be
    h = load(new_ctx(capi, m, layout, start=start), r["moved"])
    h_grids = [x.clone() for x in grids]
    for lvl in range(m.levels):
        export_device(h, lvl, h_grids[lvl], d_box)
    keep2 = [posed_update(x, r["poses"][S:], t.scans[S:], t.origos[S:] if origos else None) for x in (g, h)]
    assert_planes("updated", levels_of(g, m.levels), r["end"])
    for lvl in range(m.levels):
        assert g.debug_marks_nonzero(lvl) == (0, 0), lvl
        assert g.getUpdateIndex(lvl) == r["index"], lvl
        dirty, want = box(g.take_dirty_bbox(lvl)), box(h.take_dirty_bbox(lvl))
        assert dirty == want, (lvl, "dirty box", dirty, want)
        got, want = export_device(g, lvl, grids[lvl], d_box), export_device(h, lvl, h_grids[lvl], d_box)
        assert got == want, (lvl, "exported box", got, want)
        if lvl == 0:
            assert dirty != whole(m, 0) and dirty[2] >= dirty[0], dirty
            cb = r["box_new"][0]   # the box holds every cell the update changed
            assert dirty[0] <= cb[0] and dirty[1] <= cb[1] and dirty[2] >= cb[2] and dirty[3] >= cb[3], (dirty, cb)
    del keep, keep2
    g.close()
    h.close()


@moved_cases(mc.MAP_LAYOUTS)
def test_device_updates_outstanding_at_the_move(capi, oracle_mod, m, layout, name):
    check_updates_outstanding(capi, oracle_mod, m, layout, name, False)


@MOVES
def test_device_updates_with_origos_outstanding_at_the_move(capi, oracle_mod, name):
    check_updates_outstanding(capi, oracle_mod, mc.M96, "quad", name, True)


# ---- 2. gated calls outstanding at the move -----------------------------------------------------------------------------------------
def check_gated(capi, oracle_mod, m, layout, name, folded):
    t = mc.trajectory(oracle_mod, m)
    r = mc.posed_case(oracle_mod, KIND, m, name, True)
    S = mc.SPLIT
    g = load(new_ctx(capi, m, layout), sc.old_planes(oracle_mod, m))
    g.set_update_gate(*t.thresholds)
    k1 = posed_update(g, r["poses"][:S], t.scans[:S], gated=True)
    if folded:
        _, total = g.update_gate_state()
        assert total == int(r["flags"][:S].sum())
    g.shift_map(moved_start(m, name))
    k2 = posed_update(g, r["poses"][S:], t.scans[S:], gated=True)
    g.synchronize()
    applied = np.concatenate([k1[4].cpu().numpy(), k2[4].cpu().numpy()])
    assert np.array_equal(applied, r["flags"].astype(np.int32)), (applied, r["flags"].astype(int))
    pose, total = g.update_gate_state()
    assert same(pose, r["gate_last"]) and total == r["gate_count"], (pose, r["gate_last"], total, r["gate_count"])
    for lvl in range(m.levels):
        assert g.getUpdateIndex(lvl) == r["index"], (lvl, g.getUpdateIndex(lvl), r["index"])
        assert g.debug_marks_nonzero(lvl) == (0, 0), lvl
    assert_planes("gated", levels_of(g, m.levels), r["end"])
    del k1, k2
    g.close()


@moved_cases(mc.MAP_LAYOUTS)
def test_gated_calls_outstanding_at_the_move(capi, oracle_mod, m, layout, name):
    check_gated(capi, oracle_mod, m, layout, name, False)


@pytest.mark.parametrize("m", mc.MAPS, ids=[m.id for m in mc.MAPS])
def test_gated_calls_folded_before_the_move(capi, oracle_mod, m):
    """hsm_update_gate_state between the call and the move: the fold has happened when the move looks"""
    check_gated(capi, oracle_mod, m, "quad", "x1", True)


# ---- 3. the scan loop across a move -----------------------------------------------------------------------------------------------------
def check_loop(g, m, name, r, t, call):
    """call(k0, n, d): queues scans k0 .. k0 + n - 1 on d's buffers; the move is queued between the two calls with no wait"""
    import torch
    N, S = mc.N_SCANS, mc.SPLIT
    s = torch.cuda.Stream()
    g.set_update_gate(*t.thresholds)
    with torch.cuda.stream(s):
        d = {"start": dev(t.world[0]), "deltas": dev(t.deltas), "pose": torch.full((N, 3), -777.0, device="cuda:0"),
             "cov": torch.full((N, 9), -777.0, device="cuda:0"), "applied": torch.full((N,), -7, dtype=torch.int32, device="cuda:0")}
        call(0, S, d, s.cuda_stream)
        g.shift_map(moved_start(m, name))
        call(S, N - S, d, s.cuda_stream)
    s.synchronize()
    poses, covs, applied = d["pose"].cpu().numpy(), d["cov"].cpu().numpy(), d["applied"].cpu().numpy()
    assert np.array_equal(applied, r["flags"].astype(np.int32)), (applied, r["flags"].astype(int))
    assert same(poses, r["poses"]), (np.nonzero((bits(poses) != bits(r["poses"])).any(axis=1))[0], poses, r["poses"])
    assert same(covs, r["covs"]), np.nonzero((bits(covs) != bits(r["covs"])).any(axis=1))[0]
    g.synchronize()
    assert_planes("loop", levels_of(g, m.levels), r["ends"][-1])
    assert same(g.map_start(), moved_start(m, name))
    pose, total = g.update_gate_state()
    assert same(pose, r["gate_last"]) and total == r["gate_count"]
    for lvl in range(m.levels):
        assert g.getUpdateIndex(lvl) == r["gate_count"] - 1 and g.debug_marks_nonzero(lvl) == (0, 0), lvl


@moved_cases(LOOP_MAPS)
def test_slam_scans_device_across_a_move(capi, oracle_mod, m, layout, name):
    t = mc.trajectory(oracle_mod, m)
    r = mc.run_case(oracle_mod, KIND, m, name)
    g = load(new_ctx(capi, m, layout), sc.old_planes(oracle_mod, m))
    pts, offs = pack(t.scans)
    d_pts, d_offs = dev(pts), dev(offs)

    def call(k0, n, d, s):
        g.slam_scans_device(n, d["start"].data_ptr() if k0 == 0 else d["pose"][k0 - 1].data_ptr(), d["deltas"][k0:].data_ptr(),
                            d_pts.data_ptr(), d_offs[k0:].data_ptr(), mc.MAX_BEAMS, None, 0, d["pose"][k0:].data_ptr(),
                            d["cov"][k0:].data_ptr(), d["applied"][k0:].data_ptr(), s)
    check_loop(g, m, name, r, t, call)
    g.close()


@MOVES
def test_slam_scans_device_origos_across_a_move(capi, oracle_mod, name):
    m = mc.M96
    t = mc.trajectory(oracle_mod, m)
    r = mc.run_case(oracle_mod, KIND, m, name, True)
    g = load(new_ctx(capi, m, "quad"), sc.old_planes(oracle_mod, m))
    pts, offs = pack(t.scans)
    d_pts, d_offs, d_og = dev(pts), dev(offs), dev(t.origos)

    def call(k0, n, d, s):
        g.slam_scans_device_origos(n, d["start"].data_ptr() if k0 == 0 else d["pose"][k0 - 1].data_ptr(), d["deltas"][k0:].data_ptr(),
                                   d_pts.data_ptr(), d_offs[k0:].data_ptr(), mc.MAX_BEAMS, d_og[k0:].data_ptr(), 0,
                                   d["pose"][k0:].data_ptr(), d["cov"][k0:].data_ptr(), d["applied"][k0:].data_ptr(), s)
    check_loop(g, m, name, r, t, call)
    g.close()


@MOVES
def test_slam_ranges_tf_device_across_a_move(capi, oracle_mod, name):
    """the raw log of 96 x 40 x 3 (a tilted, moving mount: moved_entry_cases.raw_log) through the node's tf conversion and the
    loop in one call per half; the beams each scan keeps, and everything check_loop holds, against the composed loop on the
    checker's own containers"""
    import torch
    m = mc.M96
    raw, t = mc.raw_log(oracle_mod, m), mc.raw_trajectory(oracle_mod, KIND, m)
    r = mc.run_case(oracle_mod, KIND, m, name, mc.RAW)
    g = load(new_ctx(capi, m, "quad"), sc.old_planes(oracle_mod, m))
    n = mc.MAX_BEAMS
    d_ranges, d_rows = dev(raw["ranges"]), dev(raw["rows"])
    counts = torch.full((mc.N_SCANS,), -7, dtype=torch.int32, device="cuda:0")
    nbytes = g.slam_ranges_tf_workspace(mc.SPLIT, n)
    assert nbytes > 0
    ws = [torch.zeros((nbytes,), dtype=torch.uint8, device="cuda:0") for _ in range(2)]   # one per call: neither waits for the other

    def call(k0, cnt, d, s):
        g.slam_ranges_tf_device(cnt, d["start"].data_ptr() if k0 == 0 else d["pose"][k0 - 1].data_ptr(), d["deltas"][k0:].data_ptr(),
                                d_ranges[k0:].data_ptr(), n, raw["a0"], raw["inc"], *raw["lim"], d_rows[k0:].data_ptr(), False,
                                *raw["gates"], g.getScaleToMap(), 0, d["pose"][k0:].data_ptr(), d["cov"][k0:].data_ptr(),
                                d["applied"][k0:].data_ptr(), counts[k0:].data_ptr(), ws[k0 // mc.SPLIT].data_ptr(), nbytes, s)
    check_loop(g, m, name, r, t, call)
    assert np.array_equal(counts.cpu().numpy(), np.array([len(c) for c in t.scans], np.int32)), "beams kept"
    g.close()


# ---- 4. readers on a moved map -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.READER_MOVES)
@MAPS
def test_readers_on_a_moved_map(capi, oracle_mod, monkeypatch, m, layout, name):
    lib = capi.load_library()
    q, want = mc.reader_inputs(oracle_mod, m, name), mc.expected_readers(oracle_mod, KIND, m, name)
    lens = [len(s) for s in q["scans"]]
    pts, offs = pack(q["scans"])
    wposes = window_cases.window_poses(q["centre"], q["step"], mc.WINDOW_HALF)
    for form in tw.FORMS:
        tw.forced(monkeypatch, form)
        g = load(new_ctx(capi, m, layout), sc.old_planes(oracle_mod, m))
        g.shift_map(moved_start(m, name))
        d_poses = tw.written_poses(g, q["centre"], q["step"], mc.WINDOW_HALF)
        assert same(d_poses.cpu().numpy(), wposes), (form, "window poses")
        for lvl in range(m.levels):
            for n in mc.WINDOW_LENS:
                what = f"{form} level {lvl} {n} beams"
                got = tw.score_window(g, lvl, q["centre"], q["step"], mc.WINDOW_HALF, q["pts"][:n])
                assert lib.hsm_last_launch_kernel(g._h) == tw.KERNEL[form], what
                tw.assert_same_scores(what, got, want["window"][lvl][n], n)
            if form != "lane":
                continue
            tsb.assert_scores(f"score batch level {lvl}", tsb.score(g, lvl, q["poses"], pts, offs), want["score"][lvl], lens)
            st = q["states"][lvl]
            assert tw.same_bits(g.likelihood_states(lvl, st, q["pts"]), want["states"][lvl][0]), (lvl, "likelihood states")
            assert tw.same_bits(g.residual_states(lvl, st, q["pts"]), want["states"][lvl][1]), (lvl, "residual states")
            for a, b in zip(g.covariance_for_poses(lvl, st, q["pts"]), want["cov"][lvl]):
                assert tw.same_bits(a, b), (lvl, "covariance for poses")
            dist, hit = g.ray_distances(lvl, *q["rays"][lvl])
            assert same(dist, want["rays"][lvl][0]) and tw.same_bits(hit, want["rays"][lvl][1]), (lvl, "ray distances")
        if form == "lane":
            check_reloc(capi, g, q, want)
            check_ranges(capi, g, q, want)
        g.close()


def check_reloc(capi, g, q, want):
    import torch
    lvl, step, ref = want["reloc_level"], want["reloc_step"], want["reloc"]
    one, four = (tw.RelocBuffers(capi, q["centre"], q["pts"], step, mc.RELOC_HALF, mc.RELOC_K) for _ in range(2))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    one.one_call(g, lvl, s.cuda_stream)
    four.four_calls(g, lvl, s.cuda_stream)
    s.synchronize()
    r1, r4 = one.host(), four.host()
    kidx = four.kidx.cpu().numpy()
    r4["best_index"] = kidx[[int(r4["best_index"][0])]]
    for key in r1:
        assert tw.same_bits(r1[key], r4[key]), ("relocalize against its four calls", key)
    assert tw.same_bits(four.scores.cpu().numpy(), ref["scores"]), "window scores of the search level"
    assert np.array_equal(kidx, ref["index"]), (kidx, ref["index"])   # (a tied coarse level: the reference pin's indices)
    assert tw.same_bits(r1["cand"], ref["cand"]) and tw.same_bits(r1["cov"], ref["cov"]) and tw.same_bits(r1["lh0"], ref["lh0"])
    assert r1["best_index"][0] == ref["best_index"] and tw.same_bits(r1["best_pose"], ref["best_pose"])


def check_ranges(capi, g, q, want):
    import torch
    a0, inc, rmin, rmax = q["laser"]
    B, n = q["ranges"].shape
    ws_bytes = capi.match_batch_ranges_workspace(B, n)
    d = [dev(q["starts"]), dev(q["ranges"]), torch.full((B, 3), -777.0, device="cuda:0"), torch.full((B, 9), -777.0, device="cuda:0"),
         torch.full((B,), -7, dtype=torch.int32, device="cuda:0"), torch.zeros(max(ws_bytes // 4, 1), dtype=torch.int32, device="cuda:0")]
    g.match_batch_ranges_device(B, d[0].data_ptr(), d[1].data_ptr(), n, a0, inc, rmin, rmax, g.getScaleToMap(), d[2].data_ptr(),
                                d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(), ws_bytes, stream_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(d[4].cpu().numpy(), want["counts"]), "counts"
    assert same(d[2].cpu().numpy(), np.stack([p for p, _ in want["ranges_match"]])), "poses of the raw batch"
    assert same(d[3].cpu().numpy(), np.stack([c for _, c in want["ranges_match"]])), "covariances of the raw batch"
    cont = g.ingest_laser_scan(q["ranges"][0], a0, inc, rmin, rmax)
    assert same(cont, want["conts"][0]), "ingested container"
    pose, cov = g.match_ingested(q["starts"][0])
    assert same(pose, want["ranges_match"][0][0]) and same(cov, want["ranges_match"][0][1]), "match_ingested"


# ---- 5. copies and moves on one staging patch ---------------------------------------------------------------------------------------------
def filled(capi, oracle_mod, m, layout, seed, start=None):
    """a context with planes of its own on every level: the map's (seed None) or tests/test_gpu_copy_map.random_planes"""
    g = new_ctx(capi, m, layout, start=start)
    rng = np.random.default_rng(seed)
    planes = sc.old_planes(oracle_mod, m) if seed is None else [tcopy.random_planes(rng, *m.dims(lvl)) for lvl in range(m.levels)]
    return load(g, planes), planes


@MAPS
def test_copies_between_a_moved_and_an_unmoved_context(capi, oracle_mod, m, layout):
    lib = capi.load_library()
    src, p_src = filled(capi, oracle_mod, m, layout, None)
    dst, p_dst = filled(capi, oracle_mod, m, layout, 7)
    name = "x3_y-2"
    _, _, d0, _ = mc.case_plan(m, name)
    src.shift_map(moved_start(m, name))
    boxes = np.int32([[0, 0, min(9, m.dims(lvl)[0] - 1), min(9, m.dims(lvl)[1] - 1)] for lvl in range(m.levels)])
    before, start = tcopy.state(dst), dst.map_start()
    for lvl in range(m.levels):
        dst.take_dirty_bbox(lvl)
    for rc in (lib.hsm_copy_map(dst._h, src._h), lib.hsm_copy_map_boxes(dst._h, src._h, boxes.ctypes.data)):
        msg = lib.hsm_last_error().decode()
        assert rc == HSM_ERR_INVALID and "differ" in msg, (rc, msg)
    tcopy.assert_same_state(tcopy.state(dst), before, "refused")
    assert same(dst.map_start(), start)
    for lvl in range(m.levels):
        assert box(dst.take_dirty_bbox(lvl)) == EMPTY, lvl
    # both at the same start: accepted again.  First the boxes (in the new coordinates), then the whole map
    dst.shift_map(src.map_start())
    moved_dst, moved_src = sc.shifted_levels(p_dst, d0), sc.shifted_levels(p_src, d0)
    dst.copy_map_from(src, boxes)
    for lvl, (x0, y0, x1, y1) in enumerate(boxes.tolist()):
        inside = np.zeros(m.dims(lvl)[::-1], bool)
        inside[y0:y1 + 1, x0:x1 + 1] = True
        lo, st = dst.download_level(lvl)
        assert same(lo, np.where(inside, moved_src[lvl][0], moved_dst[lvl][0])), (lvl, "box copy, log-odds")
        assert np.array_equal(st, np.where(inside, moved_src[lvl][1], moved_dst[lvl][1])), (lvl, "box copy, stamps")
    dst.copy_map_from(src)
    tcopy.assert_same_state(tcopy.state(dst), tcopy.state(src), "whole copy")
    assert_planes("whole copy", levels_of(dst, m.levels), moved_src)
    for lvl in range(m.levels):
        _, prob = oracle_mod.libm_expf(moved_src[lvl][0].reshape(-1), KIND)
        assert same(dst.download_prob(lvl).reshape(-1), prob), (lvl, "probabilities")
    starts, (_, pts) = sc.batch_starts(oracle_mod, m, name, 8), sc.case_scan(oracle_mod, m)
    o = tshift.guarded(oracle_mod, m, name)
    ref = [o.match(w, pts) for w in starts]
    o.close()
    for g in (dst, src):
        pose, cov = g.match_batch(starts, pts)
        assert same(pose, np.stack([p for p, _ in ref])) and same(cov, np.stack([c for _, c in ref])), "a batch of matches"
    src.close()
    dst.close()


@MAPS
def test_move_copy_move_queued_and_a_patch_that_grows(capi, oracle_mod, m, layout):
    src, p_src = filled(capi, oracle_mod, m, layout, 5)
    first, second = moved_start(m, "x1"), moved_start(m, "x3_y-2")
    dst, _ = filled(capi, oracle_mod, m, layout, 7, start=first)
    top = m.levels - 1
    src.shift_map(first)        # nothing is synchronised between these three
    dst.copy_map_from(src)
    src.shift_map(second)
    assert_planes("dst: the state after the first move", levels_of(dst, m.levels), sc.shifted_levels(p_src, (1 << top, 0)))
    assert_planes("src: both moves", levels_of(src, m.levels), sc.shifted_levels(sc.shifted_levels(p_src, (1 << top, 0)), (2 << top, -2 << top)))
    assert same(dst.map_start(), first) and same(src.map_start(), second)
    # a small box copy (a patch of a few cells), then a move of dst that needs a patch of nearly the whole pyramid
    a, p_a = filled(capi, oracle_mod, m, layout, 8, start=first)
    b, p_b = filled(capi, oracle_mod, m, layout, 10, start=first)
    boxes = np.int32([[1, 0, min(3, m.dims(lvl)[0] - 1), min(1, m.dims(lvl)[1] - 1)] for lvl in range(m.levels)])
    a.copy_map_from(b, boxes)
    a.shift_map(np.asarray(m.start, F))
    model = []
    for lvl, (x0, y0, x1, y1) in enumerate(boxes.tolist()):
        inside = np.zeros(m.dims(lvl)[::-1], bool)
        inside[y0:y1 + 1, x0:x1 + 1] = True
        model.append((np.where(inside, p_b[lvl][0], p_a[lvl][0]), np.where(inside, p_b[lvl][1], p_a[lvl][1])))
    assert_planes("box copy, then a move", levels_of(a, m.levels), sc.shifted_levels(model, (-(1 << top), 0)))
    for g in (src, dst, a, b):
        g.close()


def test_staged_route_gives_the_same_bits():
    """the tests of this section again with HSM_COPY_STAGE=1, in a fresh child: every copy goes through the staging patch the
    move uses"""
    if os.environ.get("HSM_COPY_STAGE") == "1":
        pytest.fail("the child run must not select this test")
    env = dict(os.environ, HSM_COPY_STAGE="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__),
                        "-k", "copies_between or move_copy_move"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "%d passed" % (2 * len(mc.MAP_LAYOUTS)) in r.stdout, r.stdout[-2000:]


# ---- 6. group members ------------------------------------------------------------------------------------------------------------------------
def test_group_members_moved_together_and_one_alone(capi, oracle_mod):
    """built like tests/test_gpu_copy_map.py's group: two members on device 0"""
    m, name = mc.M64, "x1"
    t = mc.trajectory(oracle_mod, m)
    r = mc.posed_case(oracle_mod, KIND, m, name, False)
    S = mc.SPLIT
    grp = capi.MapRepGroup(m.resolution, m.geom[0], m.geom[1], m.geom[2], [0, 0], startCoords=m.start)
    grp.set_update_factors(*fc.FACTORS)
    members = [grp.member(0), grp.member(1)]
    keep = [posed_update(load(g, sc.old_planes(oracle_mod, m)), r["poses"][:S], t.scans[:S]) for g in members]   # the first half
    start = moved_start(m, name)
    members[0].shift_map(start)   # one member alone: the group refuses to synchronise, and nothing changes
    before = [tcopy.state(g) for g in members]
    with pytest.raises(capi.HsmError):
        grp.sync_maps(0)
    grp.synchronize()
    for g, b in zip(members, before):
        tcopy.assert_same_state(tcopy.state(g), b, "refused sync")
    members[1].shift_map(start)
    keep.append(posed_update(members[0], r["poses"][S:], t.scans[S:]))
    grp.sync_maps(0)
    grp.synchronize()
    tcopy.assert_same_state(tcopy.state(members[1]), tcopy.state(members[0]), "replicas")
    assert_planes("replica", levels_of(members[1], m.levels), r["end"])
    assert members[1].getUpdateIndex(0) == r["index"]
    del keep
    grp.close()
