"""hsm_map_extents* / hsm_map_image* / hsm_map_tiles* and hsm_score_windows_batch_device / hsm_select_topk_groups_device /
hsm_relocalize_batch* on the MI355X on every map and map state the suite has, bit for bit and byte for byte: no tolerance, and no
case skipped or chosen at run time.  The cases are tests/late_entry_cases.py's, pinned on the CPU by
tests/test_late_entries_reference.py.

  1. images    every map of entry_geometry_cases.MAPS, every level, quad layout (and plane where the map has it): extents (device,
               host, half open, twice), the image of six crops and of the extents box, tiles of every size of the case around
               image_cases.poses and the level's sensitive poses; every device output guarded and started at pads 67, 66, 64.
               The level's metadata: image_cases.metadata, the device's map_metadata and the checker's cast_cases.metadata agree.
               On one frame map and one deep map the image is also the reference node's published grid
  2. states    the same after hsm_shift_map, after hsm_reset of a used context (blank, then uploaded again), after hsm_copy_map and
               after hsm_merge_map, each with an extents call on every level in front
  3. batches   one CSR batch of five windows per map, every level, both forced forms, five window sizes (W = 105, 81, 1, 63,
               65): every window against the reference in every checker kind and against hsm_score_window_device; the shared
               scan against the batch of copies
  4. chains    batches of three relocalisations per map and search level: the reference composition per row, the grouped top-K's
               rows against tests/topk_rule.py, one hsm_relocalize_device call per row, the host form; the same on moved maps and
               after a reset.  Library default mode.

Where this file says less than the issue's wording, and why (tests/test_late_entries_reference.py asserts each):
  * the window around the infinite angle is held to the single call alone: the reference reads its grid at a NaN coordinate there;
  * on the frame maps moved by one_left no OCCUPIED cell survives, but the surviving corner is free space, which is known: the
    extents are that corner and the image holds 255 there, as the models of shift_cases.shifted_levels say -- not the empty box;
  * newer_entry_cases.merge_case("frames", "theta_0.3") has a dst whose every cell is known, so its hull starts at (0, 0) whatever
    the accumulators held: it runs as it stands and again with an unknown margin on dst, where a zeroed accumulator shows.

Nothing here provokes a device fault.

Durations on the MI355X: the suite without this file 190 s, this file 8.0 s (151 ids, the longest 0.2 s).
"""
import numpy as np
import pytest

import entry_geometry_cases as egc
import image_cases as ic
import late_entry_cases as lec
import moved_entry_cases as mec
import points_state_cases as psc
import test_gpu_shift_map as tshift
from conftest import bits, oracle_kinds
from support import capi, new_context, pack, same, single_update
from test_gpu_map_image import device_extents, device_image, device_tiles
from test_gpu_relocalize_batch import FORMS, KERNEL, BatchBuffers, assert_same_outputs, score_windows_batch, single_calls
from test_gpu_window import SENTINEL, forced, score_window

pytestmark = pytest.mark.gpu
KIND = oracle_kinds()[-1]
F = np.float32
load, new_ctx = tshift.load, tshift.new_ctx


def logodds_of(planes):
    return [lo for lo, _ in planes]


def minus_ones(levels):
    return [(lo, np.full(lo.shape, -1, np.int32)) for lo in levels]


def geometry_ctx(capi, geom, layout):
    return new_context(capi, geom[0], geom[1], geom[2], geom[3], geom[4], layout)


def use_accumulators(g, levels):
    for lvl in range(levels):
        device_extents(g, lvl)


# ---- 1 and 2: the image entries -----------------------------------------------------------------------------------------------------
def assert_images(g, levels, geom, what):
    """every image entry on every level of `g`, which holds the log-odds `levels` on the geometry `geom`, against the models"""
    for lvl, lo in enumerate(levels):
        sy, sx = lo.shape
        c = lec.image_level(geom, lvl, sx, sy)
        assert same(F(g.map_metadata(lvl)), F(c["meta"])), (what, lvl, "metadata", g.map_metadata(lvl), c["meta"])
        want = ic.extents_model(lo)
        assert device_extents(g, lvl) == want, (what, lvl, "extents")
        assert device_extents(g, lvl) == want, (what, lvl, "extents, a second call")
        assert tuple(int(v) for v in g.map_extents(lvl)) == want, (what, lvl, "host extents")
        half_open = g.map_extents(lvl, half_open=True)
        if want == ic.EMPTY:
            assert half_open is None, (what, lvl)
        else:
            assert tuple(int(v) for v in half_open) == (want[0], want[1], want[2] + 1, want[3] + 1), (what, lvl, "half open")
        for name, crop in c["crops"] + [("the extents box", want)]:
            model = ic.image_model(lo, crop)
            assert np.array_equal(g.map_image(lvl, crop), model), (what, lvl, name, "host image")
            for pad in lec.PADS:
                assert np.array_equal(device_image(g, lvl, crop, model.shape, pad), model), (what, lvl, name, pad)
        for tw, th in c["sizes"]:
            tiles, boxes = ic.tiles_model(lo, c["meta"], c["poses"], tw, th)
            host_tiles, host_boxes = g.map_tiles(lvl, c["poses"], tw, th)
            assert np.array_equal(host_boxes, boxes), (what, lvl, (tw, th), "host boxes", np.nonzero((host_boxes != boxes).any(1))[0])
            assert np.array_equal(host_tiles, tiles), (what, lvl, (tw, th), "host tiles")
            for pad in lec.PADS:
                got, got_boxes = device_tiles(g, lvl, c["poses"], tw, th, pad)
                assert np.array_equal(got_boxes, boxes), (what, lvl, (tw, th), pad, np.nonzero((got_boxes != boxes).any(1))[0])
                assert np.array_equal(got, tiles), (what, lvl, (tw, th), pad, np.nonzero((got != tiles).any((1, 2)))[0])


def assert_node(g, oracle_mod, levels, what):
    """the image is the reference node's published grid, the half-open extents HectorMapTools::getMapExtends of it"""
    byte_of = np.full(256, 77, np.uint8)
    byte_of[[255, 0, 100]] = [127, 255, 0]  # (-1 as a byte, 0, 100)
    for lvl, lo in enumerate(levels):
        grid = ic.node_published(oracle_mod, lo)
        assert np.array_equal(g.map_image(lvl), byte_of[grid.view(np.uint8)][::-1]), (what, lvl)
        assert np.array_equal(g.occupancy_grid(lvl), grid), (what, lvl)
        found, top_left, bottom_right = ic.extents_loop_map_tools(grid)
        assert found and tuple(int(v) for v in g.map_extents(lvl, half_open=True)) == top_left + bottom_right, (what, lvl)


@pytest.mark.parametrize("m,layout", lec.MAP_LAYOUTS, ids=lec.MAP_LAYOUT_IDS)
def test_images_on_every_level_of_every_map(capi, oracle_mod, m, layout):
    g = m.upload(oracle_mod, new_ctx(capi, m, layout))
    levels = logodds_of(lec.planes(oracle_mod, m))
    o = m.checker(oracle_mod, KIND)
    for lvl in range(m.levels):
        assert same(F(g.map_metadata(lvl)), F(lec.checker_metadata(o, lvl))), (m.id, lvl, "the checker's metadata")
        assert same(g.download_level(lvl)[0], levels[lvl]), (m.id, lvl)
    assert_images(g, levels, lec.geometry(m), f"{m.id} {layout}")
    if m in lec.NODE_MAPS:
        assert_node(g, oracle_mod, levels, m.id)
    g.close()


@pytest.mark.parametrize("m,layout,name", lec.MOVED_CASES, ids=lec.MOVED_IDS)
def test_images_on_a_moved_map(capi, oracle_mod, m, layout, name):
    mv = psc.moved_case(oracle_mod, m, name)
    g = load(new_ctx(capi, m, layout), lec.planes(oracle_mod, m))
    use_accumulators(g, m.levels)
    assert g.shift_map(mv["start"]) == mv["d0"]
    levels = logodds_of(mv["planes"])
    assert_images(g, levels, mv["geom"], f"{m.id} {layout} moved by {name}")
    if (m.id, name) in psc.NOTHING_SURVIVES:   # no occupied cell is left: no black byte on any level
        for lvl in range(m.levels):
            assert (g.map_image(lvl) != 0).all(), lvl
    g.close()


@pytest.mark.parametrize("m,layout", lec.RESET_LAYOUTS, ids=["%s-%s" % (m.id, layout) for m, layout in lec.RESET_LAYOUTS])
def test_images_across_a_reset(capi, oracle_mod, m, layout):
    old = lec.planes(oracle_mod, m)
    geom = lec.geometry(m)
    g = load(new_ctx(capi, m, layout), old)
    t = mec.trajectory(oracle_mod, m)
    for k in range(2):
        single_update(capi, g, t.world[k], t.scans[k])
    use_accumulators(g, m.levels)
    g.reset()
    blank = [np.zeros_like(lo) for lo, _ in old]
    for lvl in range(m.levels):
        assert device_extents(g, lvl) == ic.EMPTY, lvl
        assert (g.map_image(lvl) == 127).all() and (g.map_tiles(lvl, np.zeros((1, 3), F), 1, 1)[0] == 127).all(), lvl
    assert_images(g, blank, geom, f"{m.id} {layout} blank")
    load(g, old)
    fresh = load(new_ctx(capi, m, layout), old)
    assert_images(g, logodds_of(old), geom, f"{m.id} {layout} uploaded again")
    for lvl in range(m.levels):
        sx, sy = m.dims(lvl)
        assert device_extents(g, lvl) == device_extents(fresh, lvl), lvl
        assert np.array_equal(device_image(g, lvl, None, (sy, sx)), device_image(fresh, lvl, None, (sy, sx))), lvl
    g.close()
    fresh.close()


@pytest.mark.parametrize("layout", ("quad", "plane"))
def test_images_after_a_whole_copy(capi, oracle_mod, layout):
    m, c = lec.COPY_MAP, lec.copy_case(oracle_mod)
    dst = load(new_ctx(capi, m, layout), lec.planes(oracle_mod, m))
    src = load(new_ctx(capi, m, layout), minus_ones(c["src"]))
    for g in (dst, src):
        use_accumulators(g, m.levels)
    dst.copy_map_from(src)
    assert_images(dst, c["src"], c["geom"], f"copy {layout}: dst")
    assert_images(src, c["src"], c["geom"], f"copy {layout}: src")
    dst.close()
    src.close()


@pytest.mark.parametrize("layout", ("quad", "plane"))
@pytest.mark.parametrize("name", ("committed", "margin"))
def test_images_after_a_merge(capi, name, layout):
    c = lec.merge_cases_of_this_file()[name]
    dst = load(geometry_ctx(capi, c["gd"], layout), minus_ones(c["dst"]))
    src = load(geometry_ctx(capi, c["gs"], layout), minus_ones(c["src"]))
    for g, geom in ((dst, c["gd"]), (src, c["gs"])):
        use_accumulators(g, geom[3])
    capi.merge_map(dst, src, c["t"])
    merged = [lo for lo, _ in c["model"]]
    for lvl, lo in enumerate(merged):
        assert same(dst.download_level(lvl)[0], lo), (name, lvl, "the merged plane")
    assert_images(dst, merged, c["gd"], f"merge {name} {layout}: dst")
    assert_images(src, c["src"], c["gs"], f"merge {name} {layout}: src")
    dst.close()
    src.close()


# ---- 3: batched window scores -------------------------------------------------------------------------------------------------------
def assert_batch_scores(g, lib, capi, oracle_mod, m, lvl, half, form, what, expected_of):
    """one batched launch against one hsm_score_window_device call per window and against the reference's rows"""
    centres, scans, step = lec.batch_case(oracle_mod, m)
    pts, offs = pack(scans)
    got = score_windows_batch(g, lvl, centres, step, half, pts, offs)
    if form is not None:
        assert lib.hsm_last_launch_kernel(g._h) == KERNEL[form], what
    assert lib.hsm_last_launch_parity(g._h) == capi.PARITY_EXACT, what
    assert not (got[0] == SENTINEL).any() and not (got[1] == SENTINEL).any(), f"{what}: rows never written"
    for b in range(len(centres)):
        one = score_window(g, lvl, centres[b], step, half, scans[b])
        assert same(got[0][b], one[0]) and same(got[1][b], one[1]), (what, b, "the single call")
    empty = bits(got[0][lec.EMPTY_ROW])
    print(what, "the empty scan's likelihood bits", hex(int(empty[0])))
    assert (empty == lec.EMPTY_NAN).all() and (bits(got[1][lec.EMPTY_ROW]) == 0).all(), (what, "the empty scan's row")
    for kind in oracle_kinds():
        want = expected_of(kind)
        for b, w in enumerate(want):
            if w is None:   # the infinite angle: the reference does not define it
                continue
            assert same(got[1][b], w[1]), (what, kind, b, "residuals")
            if b != lec.EMPTY_ROW:
                assert same(got[0][b], w[0]), (what, kind, b, "likelihoods")
    return got


BATCH_RUNS = [(m, layout, form) for m, layout in lec.MAP_LAYOUTS for form in FORMS]


@pytest.mark.parametrize("m,layout,form", BATCH_RUNS, ids=["%s-%s-%s" % (m.id, layout, form) for m, layout, form in BATCH_RUNS])
def test_batched_window_scores_on_every_level(capi, oracle_mod, monkeypatch, m, layout, form):
    forced(monkeypatch, form)
    g = m.upload(oracle_mod, new_ctx(capi, m, layout))
    lib = capi.load_library()
    for lvl in range(m.levels):
        for half in lec.BATCH_HALVES:
            assert_batch_scores(g, lib, capi, oracle_mod, m, lvl, half, form, f"{m.id} {layout} {form} level {lvl} window {half}",
                                lambda kind: lec.expected_batch(oracle_mod, m, lvl, half, kind))
    # one shared scan is a CSR batch of copies of it
    centres, scans, step = lec.batch_case(oracle_mod, m)
    lvl, half = lec.shared_level(m), lec.BATCH_HALVES[0]
    shared = score_windows_batch(g, lvl, centres, step, half, scans[0], None, len(scans[0]))
    copies = score_windows_batch(g, lvl, centres, step, half, *pack([scans[0]] * len(centres)))
    assert lib.hsm_last_launch_kernel(g._h) == KERNEL[form]
    assert same(shared[0], copies[0]) and same(shared[1], copies[1]) and not (shared[1] == SENTINEL).any(), (m.id, "shared scan")
    g.close()


# ---- 4: the batched relocalisation --------------------------------------------------------------------------------------------------
HOST_KEYS = (("cand", "cand_pose"), ("cov", "cand_cov"), ("lh0", "cand_likelihood"), ("cand_index", "cand_index"),
             ("best_pose", "best_pose"), ("best_score", "best_score"), ("best_index", "best_index"))


def assert_reloc_batch(capi, oracle_mod, g, m, lvl, rows, what, host_form=False):
    """one hsm_relocalize_batch_device call against the reference's rows, the top-K rule and one single call per row"""
    import torch
    centres, scans, step = lec.reloc_rows(oracle_mod, m, lvl)
    half, k = egc.RELOC_HALF, egc.RELOC_K
    s = torch.cuda.Stream()
    b = BatchBuffers(capi, centres, scans, step, half, k)
    torch.cuda.synchronize()
    b.call(g, lvl, s.cuda_stream)
    s.synchronize()
    got = b.host()
    for key in got:
        assert not (got[key] == (SENTINEL if got[key].dtype == np.float32 else 99)).any(), (what, key, "never written")
    assert np.array_equal(got["cand_index"], lec.topk_of(rows)), (what, "the grouped top-K inside the chain", got["cand_index"])
    if (m.id, lvl) in lec.TIED:
        assert got["cand_index"].tolist() == [list(range(k))] * lec.RELOC_ROWS, (what, got["cand_index"])
    assert_same_outputs(got, lec.stacked(rows), what + ": the reference")
    assert_same_outputs(got, single_calls(capi, g, lvl, centres, scans, step, half, k, s.cuda_stream), what + ": single calls")
    if host_form:
        pts, offs = pack(scans)
        h = g.relocalize_batch(lvl, centres, step, half, k, pts, offs)
        for key, hk in HOST_KEYS:
            assert same(h[hk], got[key]) if got[key].dtype == np.float32 else np.array_equal(h[hk], got[key]), (what, "host form", key)
    return got


@pytest.mark.parametrize("m,lvl", lec.RELOC_CASES, ids=lec.RELOC_IDS)
def test_relocalize_batch_on_every_map(capi, oracle_mod, m, lvl):
    g = m.upload(oracle_mod, new_ctx(capi, m, "quad"))
    g.synchronize()
    rows = lec.expected_reloc_batch(oracle_mod, m, lvl, KIND)
    assert rows[0] is egc.expected_reloc(oracle_mod, m, lvl, KIND)
    assert_reloc_batch(capi, oracle_mod, g, m, lvl, rows, f"{m.id} search level {lvl}", host_form=lvl == egc.reloc_levels(m)[0])
    g.close()


MOVED_RUNS = [(m, name) for m in lec.RELOC_MOVED_MAPS for name in mec.READER_MOVES]


@pytest.mark.parametrize("m,name", MOVED_RUNS, ids=["%s-%s" % (m.id, name) for m, name in MOVED_RUNS])
def test_batched_scores_and_relocalisation_on_a_moved_map(capi, oracle_mod, monkeypatch, m, name):
    forced(monkeypatch, "wave")
    mv = psc.moved_case(oracle_mod, m, name)
    g = load(new_ctx(capi, m, "quad"), lec.planes(oracle_mod, m))
    assert g.shift_map(mv["start"]) == mv["d0"]
    g.synchronize()
    lib = capi.load_library()
    for lvl in range(m.levels):
        for half in lec.BATCH_HALVES:
            assert_batch_scores(g, lib, capi, oracle_mod, m, lvl, half, "wave", f"{m.id} moved by {name} level {lvl} window {half}",
                                lambda kind: lec.expected_batch(oracle_mod, m, lvl, half, kind, tag=("moved", name),
                                                                o=mec.reader_checker(oracle_mod, kind, m, name)))
    ran = 0
    for lvl in egc.reloc_levels(m):
        if (m.id, name, lvl) in lec.MOVED_DROPPED:
            continue
        rows = lec.expected_reloc_moved(oracle_mod, m, name, lvl, KIND)
        assert rows is not None, (m.id, name, lvl, "the reference does not define this case, and it is not named as dropped")
        assert_reloc_batch(capi, oracle_mod, g, m, lvl, rows, f"{m.id} moved by {name} search level {lvl}")
        ran += 1
    assert ran >= 1
    g.close()


def test_batched_entries_across_a_reset(capi, oracle_mod, monkeypatch):
    forced(monkeypatch, None)
    m = lec.RESET_MAP
    old = lec.planes(oracle_mod, m)
    g = load(new_ctx(capi, m, "quad"), old)
    t = mec.trajectory(oracle_mod, m)
    for k in range(2):
        single_update(capi, g, t.world[k], t.scans[k])
    use_accumulators(g, m.levels)
    g.reset()
    load(g, old)
    fresh = load(new_ctx(capi, m, "quad"), old)
    lib = capi.load_library()
    for lvl in range(m.levels):
        half = lec.BATCH_HALVES[lvl % len(lec.BATCH_HALVES)]
        a, b = (assert_batch_scores(x, lib, capi, oracle_mod, m, lvl, half, None, f"{m.id} {who} level {lvl} window {half}",
                                    lambda kind: lec.expected_batch(oracle_mod, m, lvl, half, kind))
                for x, who in ((g, "after the reset"), (fresh, "fresh")))
        assert same(a[0], b[0]) and same(a[1], b[1]), lvl
    lvl = egc.reloc_levels(m)[0]
    rows = lec.expected_reloc_batch(oracle_mod, m, lvl, KIND)
    a, b = (assert_reloc_batch(capi, oracle_mod, x, m, lvl, rows, f"{m.id} {who}") for x, who in ((g, "after the reset"), (fresh, "fresh")))
    assert_same_outputs(a, b, "a reset context against a fresh one")
    g.close()
    fresh.close()
