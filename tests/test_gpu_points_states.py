"""hsm_occupied_points_device / hsm_occupied_points / hsm_align_map on the MI355X on every map state the suite has, bit for bit:
no tolerance, and no case skipped or chosen at run time.  The cases are tests/points_state_cases.py's, pinned on the CPU by
tests/test_points_states_reference.py.

  a. shapes   the eight frames on 90 x 24 x 2 and 96 x 40 x 3 and the three deep pyramids down to 10 x 2, 2 x 10 and 2 x 2 cells:
              every level, box, thinning and cap, the device entry and the host entry against the numpy model, and the model's
              transform against the context's own getWorldCoordsPose times getScaleToMap
  b. moved    the same after hsm_shift_map; and on a caller's stream, behind torch work that keeps the stream busy, an
              extraction, the move and a second extraction with no host wait in between: old cells in the old frame, shifted
              cells in the new one
  c. reset    a context that held a map (and one that had moved besides) after hsm_reset: nothing extracted, an alignment from
              it returns the guess, one onto it equals the public calls; rebuilt by six updates, it extracts the checker's cells
              in the frame it had at the reset
  d. align    hsm_align_map with src_level 0 and 1, on the search levels of entry_geometry_cases.reloc_levels, and with a src
              that has moved: the public calls, the reference chain on the extracted points, and neither context changes
  e. order    device-side updates queued on both contexts around two alignments, against a twin pair that waits after every
              step; the writers hsm_reset, hsm_upload_level, hsm_copy_map and hsm_merge_map queued directly behind an extraction
              on a busy caller's stream; and src after dst is closed.
              After an alignment src takes its next update without waiting on anything: hsm_align_map reads src on dst's
              stream, marks that stream pending in src's list (occupied_points_launch), waits for it on the host under src's
              lock and clears the mark again (window.hip: reader.mark->pending = false), so order_after_foreign_match finds nothing to
              record an event for.  The extraction on a caller's stream leaves its mark set, and the next writer waits for it.

Durations on the MI355X: the suite without this file 185 s, this file 4.4 s (69 ids, the longest 0.2 s).
"""
import numpy as np
import pytest

import entry_geometry_cases as egc
import merge_cases
import moved_entry_cases as mec
import points_cases as pc
import points_state_cases as psc
import test_gpu_shift_map as tshift
from conftest import bits, oracle_kinds
from support import capi, new_context, single_update
from test_gpu_align_map import assert_align_equals, public_chain, same_bits, state
from test_gpu_moved_entries import posed_update
from test_gpu_occupied_points import DeviceRun, assert_model, extract

pytestmark = pytest.mark.gpu
KIND = oracle_kinds()[-1]
F = np.float32
load, levels_of, assert_planes = tshift.load, tshift.levels_of, tshift.assert_planes


def new_ctx(capi, m, layout, start=None):
    return new_context(capi, m.resolution, m.geom[0], m.geom[1], m.geom[2], m.start if start is None else start, layout)


def assert_device_frame(g, lo, geom, lvl):
    """the third statement of the points: the model's transform is the context's own"""
    affine, scale = psc.frame_of(geom, lvl)
    assert bits(F(g.getScaleToMap())) == bits(scale)
    cells = psc.probe_cells(lo)
    host = np.stack([g.getWorldCoordsPose(lvl, F([x, y, 0]))[:2] * scale for x, y in cells]).astype(F)
    assert np.array_equal(bits(pc.cell_points(cells, affine, scale)), bits(host)), (lvl, "getWorldCoordsPose times getScaleToMap")


def assert_levels(capi, g, planes, geom, what):
    """every level, box, thinning and cap of the case file: the device entry and the host entry give the model's counts and bits"""
    runs = 0
    for lvl, (lo, _) in enumerate(planes):
        assert_device_frame(g, lo, geom, lvl)
        affine, scale = psc.frame_of(geom, lvl)
        for name, box, every, cap in psc.level_runs(lo):
            got = extract(capi, g, lvl, box, every, cap)
            assert_model(f"{what} level {lvl} {name} every {every} cap {cap}", got, lo, box, every, cap, affine, scale)
            pts, count = g.occupied_points(lvl, box, every, cap)
            assert np.array_equal(count, got[1]) and np.array_equal(bits(pts), bits(got[0])), (what, "host entry", lvl, name, every, cap)
            runs += 1
    assert runs >= len(planes) * 3 * len(psc.EVERY)


@pytest.fixture(scope="module")
def contexts(capi, oracle_mod):
    """get(m, layout, move=None) -> one context per map, layout and move, uploaded (and moved) once; the tests that share them
    leave them as they are"""
    made = {}

    def get(m, layout, move=None):
        key = (m.id, layout, move)
        if key not in made:
            g = load(new_ctx(capi, m, layout), psc.planes(oracle_mod, m))
            if move:
                mv = psc.moved_case(oracle_mod, m, move)
                assert g.shift_map(mv["start"]) == mv["d0"]
            made[key] = g
        return made[key]
    yield get
    for g in made.values():
        g.close()


@pytest.fixture(scope="module")
def busy(capi):
    """busy(stream) queues some ten milliseconds of torch work on the stream -> an event behind it.  While the event has not
    completed nothing queued behind it on that stream has started"""
    import torch
    a = torch.rand((4096, 4096), device="cuda:0")
    b = torch.empty_like(a)
    torch.mm(a, a, out=b)   # (the first product loads its kernel)
    torch.cuda.synchronize()

    def queue(stream):
        with torch.cuda.stream(stream):
            for _ in range(24):
                torch.mm(a, a, out=b)
            ev = torch.cuda.Event()
            ev.record(stream)
        return ev
    return queue


# ---- a. shapes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,layout", psc.MAP_LAYOUTS, ids=psc.MAP_LAYOUT_IDS)
def test_points_on_every_frame_and_level(capi, oracle_mod, contexts, m, layout):
    assert_levels(capi, contexts(m, layout), psc.planes(oracle_mod, m), psc.geometry(m), f"{m.id} {layout}")


# ---- b. moved -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,layout,name", psc.MOVED_CASES, ids=psc.MOVED_IDS)
def test_points_on_a_moved_map(capi, oracle_mod, contexts, m, layout, name):
    mv = psc.moved_case(oracle_mod, m, name)
    g = contexts(m, layout, name)
    assert np.array_equal(bits(g.map_start()), bits(mv["start"]))
    assert_levels(capi, g, mv["planes"], mv["geom"], f"{m.id} {layout} moved by {name}")
    if (m.id, name) in psc.NOTHING_SURVIVES:
        for lvl in range(m.levels):
            assert extract(capi, g, lvl, None, 1, 5)[1].tolist() == [0, 0], lvl


@pytest.mark.parametrize("m,layout,name", psc.STREAM_CASES, ids=["%s-%s-%s" % (m.id, layout, name) for m, layout, name in psc.STREAM_CASES])
def test_extraction_move_extraction_on_a_busy_caller_stream(capi, oracle_mod, busy, m, layout, name):
    import torch
    old, mv = psc.planes(oracle_mod, m), psc.moved_case(oracle_mod, m, name)
    g = load(new_ctx(capi, m, layout), old)
    s = torch.cuda.Stream()
    caps = [len(pc.kept_cells(lo, None, 1)) + 3 for lo, _ in old]
    first = [DeviceRun(capi, g, lvl, None, 1, caps[lvl]) for lvl in range(m.levels)]
    second = [DeviceRun(capi, g, lvl, None, 1, caps[lvl]) for lvl in range(m.levels)]
    torch.cuda.synchronize()
    ev = busy(s)
    for run in first:
        run.launch(s.cuda_stream)
    assert not ev.query(), "the stream has drained already: the extraction may have run before the move was queued"
    assert g.shift_map(mv["start"]) == mv["d0"]   # no host wait: the move orders itself behind the extraction
    for run in second:
        run.launch(s.cuda_stream)
    s.synchronize()
    for lvl in range(m.levels):
        assert_model(f"level {lvl} in front of the move", first[lvl].result(), old[lvl][0], None, 1, caps[lvl], *psc.frame_of(psc.geometry(m), lvl))
        assert_model(f"level {lvl} behind the move", second[lvl].result(), mv["planes"][lvl][0], None, 1, caps[lvl], *psc.frame_of(mv["geom"], lvl))
    a, b = first[0].result()[0], second[0].result()[0]
    assert len(a) > len(b) >= 1 and not np.array_equal(bits(a[:len(b)]), bits(b)), "the move changes the points"
    assert_planes("after the move", levels_of(g, m.levels), mv["planes"])
    g.close()


# ---- c. reset -------------------------------------------------------------------------------------------------------------------------
RESET_MOVE = "x3_y-2"


def align_args(oracle_mod, c):
    return (c.src_level, None, c.every, psc.MAX_POINTS, c.search_level, psc.align_guess(oracle_mod, c), psc.align_step(oracle_mod, c),
            egc.RELOC_HALF, egc.RELOC_K)


@pytest.mark.parametrize("move", (None, RESET_MOVE), ids=("plain", "moved"))
def test_points_and_alignment_across_a_reset(capi, oracle_mod, contexts, move):
    m = mec.M96
    old = psc.planes(oracle_mod, m)
    start = psc.moved_case(oracle_mod, m, move)["start"] if move else np.asarray(m.start, F)
    geom = psc.geometry(m, start if move else None)
    g = load(new_ctx(capi, m, "quad"), old)
    if move:
        g.shift_map(start)
    assert extract(capi, g, 0, None, 1, 2000)[1][0] > 100
    g.reset()
    assert np.array_equal(bits(g.map_start()), bits(start)), "a reset keeps the window where it is"
    for lvl in range(m.levels):
        for every in psc.EVERY:
            pts, count = extract(capi, g, lvl, None, every, 50)   # (its result() holds that no float was written)
            assert count.tolist() == [0, 0] and len(pts) == 0, (lvl, every, count)
            assert g.occupied_points(lvl, None, every, 50)[1].tolist() == [0, 0]
    # as src: the guess comes back; as dst: the public calls
    c = next(x for x in psc.ALIGN_CASES if x.m is m and x.src_level == 0 and not x.moved)
    full = contexts(m, "quad")
    args = align_args(oracle_mod, c)
    t, cov, lh, counts, index = full.align_map_from(g, *args)
    assert same_bits(t, args[5]) and np.isnan(lh) and index == -1 and counts.tolist() == [0, 0] and not cov.any()
    pts, want = public_chain(capi, g, full, *args)
    assert len(pts) == psc.align_points(oracle_mod, c)[1][0] > psc.MIN_POINTS
    assert_align_equals(f"onto a reset context ({move})", g.align_map_from(full, *args), want)
    # rebuilt: six posed scans into the context and into a checker that went through the same reset
    o = mec.moved(oracle_mod, KIND, m, move) if move else mec.old_checker(oracle_mod, KIND, m)
    for x in {id(o.guard): o.guard, id(o.o): o.o}.values():
        x.reset()
    t6 = mec.trajectory(oracle_mod, m)
    for k in range(6):
        single_update(capi, g, t6.world[k], t6.scans[k])
        o.build_map(t6.world[k:k + 1], [t6.scans[k]])
    for lvl in range(m.levels):
        lo, _ = o.download_level(lvl)
        cells, want_pts = psc.checker_points(o, lvl, m.resolution)
        assert len(cells) >= 1 and (lvl > 0 or len(cells) > 20), (lvl, len(cells))
        assert_device_frame(g, lo, geom, lvl)
        got = extract(capi, g, lvl, None, 1, len(cells) + 3)
        assert got[1].tolist() == [len(cells)] * 2 and np.array_equal(bits(got[0]), bits(want_pts)), (lvl, "the checker's cells")
        assert_model(f"rebuilt ({move}) level {lvl}", got, lo, None, 1, len(cells) + 3, *psc.frame_of(geom, lvl))
    o.close()
    g.close()


# ---- d. alignment ---------------------------------------------------------------------------------------------------------------------
ALIGN_RUNS = [(c, "quad") for c in psc.ALIGN_CASES] + [(c, "plane") for c in psc.ALIGN_CASES if c.m.planes_too]


@pytest.mark.parametrize("c,layout", ALIGN_RUNS, ids=["%s-%s" % (c.id, layout) for c, layout in ALIGN_RUNS])
def test_align_on_every_state_equals_the_public_calls_and_the_reference_chain(capi, oracle_mod, c, layout):
    m = c.m
    src_planes, src_geom = psc.align_src(oracle_mod, c)
    dst, src = load(new_ctx(capi, m, layout), psc.planes(oracle_mod, m)), load(new_ctx(capi, m, layout), psc.planes(oracle_mod, m))
    if c.moved:   # after the planes went in; the world does not move with the window
        src.shift_map(psc.moved_case(oracle_mod, m, c.moved)["start"])
    grids = {id(g): [np.full(m.dims(lvl)[::-1], 55, np.int8) for lvl in range(m.levels)] for g in (dst, src)}
    was = {id(g): state(g, grids[id(g)]) for g in (dst, src)}
    args = align_args(oracle_mod, c)
    pts, want = public_chain(capi, dst, src, *args)
    model_pts, model_count = psc.align_points(oracle_mod, c)
    assert tuple(want["counts"].tolist()) == model_count and np.array_equal(bits(pts), bits(model_pts)), "the points are the model's"
    assert psc.MIN_POINTS < len(pts) <= psc.MAX_POINTS and want["index"] >= 0
    got = dst.align_map_from(src, *args)
    assert_align_equals(f"{c.id} {layout}", got, want)
    ref = psc.align_reference(oracle_mod, KIND, c, pts)   # on the points the device wrote
    assert ref is not None, "the reference does not define this case"
    assert got[4] == ref["best_index"] and same_bits(got[0], ref["best_pose"]), (got[0], ref["best_pose"], got[4], ref["best_index"])
    assert bits(got[2]) == bits(ref["best_score"]) and same_bits(got[1], ref["cov"][ref["best"]])
    for g in (dst, src):
        planes, index, dirty, pub = state(g, grids[id(g)])
        for lvl in range(m.levels):
            assert np.array_equal(bits(planes[lvl][0]), bits(was[id(g)][0][lvl][0])) and np.array_equal(planes[lvl][1], was[id(g)][0][lvl][1])
            assert dirty[lvl][2] < dirty[lvl][0] and pub[lvl][2] < pub[lvl][0], (lvl, dirty[lvl], pub[lvl])
        assert index == was[id(g)][1]
    assert_planes("src", levels_of(src, m.levels), src_planes)
    dst.close()
    src.close()


# ---- e. ordering across contexts ------------------------------------------------------------------------------------------------------
def test_updates_queued_around_two_alignments_equal_a_pair_that_waits(capi, oracle_mod):
    import torch
    m = mec.M96
    old = psc.planes(oracle_mod, m)
    t = mec.trajectory(oracle_mod, m)
    c = next(x for x in psc.ALIGN_CASES if x.m is m and x.src_level == 0 and not x.moved)
    args = align_args(oracle_mod, c)
    pairs = {wait: (load(new_ctx(capi, m, "quad"), old), load(new_ctx(capi, m, "quad"), old)) for wait in (False, True)}
    results, keep = {}, []
    torch.cuda.synchronize()
    for wait, (dst, src) in pairs.items():
        def settle():
            if wait:
                src.synchronize()
                dst.synchronize()
                torch.cuda.synchronize()
        out = []
        keep.append(posed_update(src, t.world[0:2], t.scans[0:2]))
        settle()
        keep.append(posed_update(dst, t.world[2:4], t.scans[2:4]))
        settle()
        out.append(dst.align_map_from(src, *args))
        settle()
        keep.append(posed_update(src, t.world[4:6], t.scans[4:6]))   # at once: the alignment left nothing for src's writer to wait for
        keep.append(posed_update(dst, t.world[6:8], t.scans[6:8]))
        settle()
        out.append(dst.align_map_from(src, *args))
        settle()
        results[wait] = out
    for k in range(2):
        a, b = results[False][k], results[True][k]
        print("alignment", k, "pose", a[0].tolist(), "likelihood", float(a[2]), "counts", a[3].tolist(), "index", a[4])
        assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and same_bits(a[2], b[2]) and np.array_equal(a[3], b[3]) and a[4] == b[4], k
        assert a[4] >= 0 and a[3][0] > psc.MIN_POINTS
    for who in (0, 1):
        assert_planes("dst" if who == 0 else "src", levels_of(pairs[False][who], m.levels), levels_of(pairs[True][who], m.levels))
        assert [pairs[False][who].getUpdateIndex(lvl) for lvl in range(m.levels)] == [pairs[True][who].getUpdateIndex(lvl) for lvl in range(m.levels)] == [3] * m.levels
    assert not np.array_equal(bits(levels_of(pairs[False][1], 1)[0][0]), bits(old[0][0])), "the updates change src"
    # dst goes: src still takes an update and answers
    (dst, src), (tdst, tsrc) = pairs[False], pairs[True]
    dst.close()
    for g in (src, tsrc):
        single_update(capi, g, t.world[7], t.scans[7])
    tsrc.synchronize()
    geom = psc.geometry(m)
    for lvl in range(m.levels):
        lo = tsrc.download_level(lvl)[0]
        kept = len(pc.kept_cells(lo, None, 1))
        assert_model(f"src with dst closed, level {lvl}", extract(capi, src, lvl, None, 1, kept + 3), lo, None, 1, kept + 3, *psc.frame_of(geom, lvl))
    del keep
    for g in (src, tdst, tsrc):
        g.close()


WRITERS = ("reset", "upload_level", "copy_map", "merge_map")


@pytest.mark.parametrize("writer", WRITERS)
def test_a_writer_queued_behind_an_extraction_on_a_busy_caller_stream(capi, oracle_mod, busy, writer):
    import torch
    m = mec.M96
    geom = psc.geometry(m)
    old = psc.planes(oracle_mod, m)
    other_lo = merge_cases.synthetic_planes(geom, 4100)
    other = [(lo, np.full(lo.shape, -1, np.int32)) for lo in other_lo]
    g, h = load(new_ctx(capi, m, "quad"), old), load(new_ctx(capi, m, "quad"), other)
    s = torch.cuda.Stream()
    caps = [len(pc.kept_cells(lo, None, 1)) + 3 for lo, _ in old]
    runs = [DeviceRun(capi, g, lvl, None, 1, caps[lvl]) for lvl in range(m.levels)]
    h.synchronize()
    torch.cuda.synchronize()
    ev = busy(s)
    for run in runs:
        run.launch(s.cuda_stream)
    assert not ev.query(), "the stream has drained already: the extraction may have run before the writer was queued"
    if writer == "reset":
        g.reset()
    elif writer == "upload_level":
        for lvl, (lo, st) in enumerate(other):
            g.upload_level(lvl, lo, st)
    elif writer == "copy_map":
        g.copy_map_from(h)
    else:
        capi.merge_map(g, h, np.zeros(3, F))
    s.synchronize()
    for lvl in range(m.levels):
        assert_model(f"level {lvl} in front of {writer}", runs[lvl].result(), old[lvl][0], None, 1, caps[lvl], *psc.frame_of(geom, lvl))
    g.synchronize()
    now = levels_of(g, m.levels)
    if writer == "reset":
        want = [np.zeros_like(lo) for lo, _ in old]
    elif writer == "merge_map":
        want = [lo for lo, _ in merge_cases.merge_pyramid([lo for lo, _ in old], other_lo, geom, geom, np.zeros(3, F))]
    else:
        want = other_lo
    for lvl in range(m.levels):
        assert np.array_equal(bits(now[lvl][0]), bits(want[lvl])), (writer, lvl, "the writer ran")
        assert not np.array_equal(pc.kept_cells(want[lvl], None, 1), pc.kept_cells(old[lvl][0], None, 1)), (writer, lvl, "the writer changes the point set")
    g.close()
    h.close()
