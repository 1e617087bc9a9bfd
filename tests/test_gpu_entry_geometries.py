"""The cast, window and copy entries against the reference on off-centre maps, odd cell sizes, rectangular levels and deep
pyramids (cases: tests/entry_geometry_cases.py, pinned on the CPU by tests/test_entry_geometries_reference.py).

Library default mode; every comparison is on uint32 views against the checker oracle_kinds()[-1] (the reference headers where
they are built; the pin shows both checkers agree on every case).  No tolerance anywhere.  Outputs are prefilled with a
sentinel (NaN for hit points), the kernel forms are forced through HSM_CAST_FORM / HSM_WINDOW_FORM and asked which one ran.

"frames": the eight frames of frame_cases.FRAMES on 64 x 64 x 2, 90 x 24 x 2 and 96 x 40 x 3; "deep": (333, 90, 6), (90, 333, 6)
and (256, 256, 8) of deep_cases, every level down to 10 x 2, 2 x 10 and 2 x 2 cells.  What runs where:

  hsm_cast_scans_device      frames and deep, every level, both forms, fans of 1 / 63 / 64 / 65 / 200 beams, five range maxima;
                             quad layout, and the plane layout on frame (0.03, (0.3, 0.7)) and on (333, 90, 6)
  hsm_cast_scans             once per map and layout of the above (level 0, 200 beams)
  hsm_ray_distances_device,
  hsm_ray_distances          frames and deep, every level, 500 mixed rays on the level's own metadata; layouts as above
  hsm_score_window_device    frames and deep, every level, both forms, both layouts, windows (3, 2, 1) and (40, 0, 0), scans of
                             1 / 65 / 200 beams; against the checker and against hsm_score_batch_device
  hsm_score_window           once per map and layout (level 0)
  hsm_window_poses_device    frames and deep, both windows (the far frame's 80 m centre with steps of 12.5 and 17.5 mm)
  hsm_select_topk_device,
  hsm_relocalize_device      frames: search level = the coarsest; deep: the coarsest (every window score ties: the K first
                             indices) and level 2; against the four separate calls and reference_relocalize
  hsm_relocalize             once per map
  hsm_copy_map               (333, 90, 6) and (96, 40, 3) in frame (0.03, (0.3, 0.7)), both layouts, direct and staged route
  hsm_copy_map_boxes         (333, 90, 6): the hand-made boxes on every level (widths 333, 166, 83, 41, 20, 10) and one with an odd
                             x0 and an odd width, both layouts, direct and staged route
  refusals of both           contexts that differ in the start x alone, the start y alone, the resolution alone
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import deep_cases
import entry_geometry_cases as eg
import frame_cases as fc
import test_gpu_cast_scans as tcast
import test_gpu_copy_map as tcopy
import test_gpu_window as tw
import topk_rule
import window_cases
from conftest import bits, oracle_kinds
from support import capi, dev, new_context, same, single_update, stream_ptr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HSM_ERR_INVALID = -1
KIND = oracle_kinds()[-1]
SENTINEL = tcast.SENTINEL
QUAD = [(m, "quad") for m in eg.MAPS]
SOME_PLANE = QUAD + [(m, "plane") for m in eg.MAPS if m.planes_too]
BOTH = QUAD + [(m, "plane") for m in eg.MAPS]


def ids(cases):
    return [f"{m.id}-{layout}" for m, layout in cases]


def new_ctx(capi, oracle_mod, m, layout="quad", upload=True, frame=None):
    """a context in the library's default mode on the map's geometry (or in another frame), with the map"""
    res, start = (m.resolution, m.start) if frame is None else frame
    g = new_context(capi, res, m.geom[0], m.geom[1], m.geom[2], start, layout, fc.FACTORS)
    if upload:
        m.upload(oracle_mod, g)
    g.synchronize()
    return g


# ---- casts and rays -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,layout", SOME_PLANE, ids=ids(SOME_PLANE))
def test_casts_and_rays_on_every_level(capi, oracle_mod, monkeypatch, m, layout):
    import torch
    lib = capi.load_library()
    for form in sorted(tcast.FORMS):
        monkeypatch.setenv("HSM_CAST_FORM", form)
        g = new_ctx(capi, oracle_mod, m, layout)
        for lvl in range(m.levels):
            c, want = eg.level_case(oracle_mod, m, lvl), eg.expected(oracle_mod, m, lvl, KIND)
            for name in eg.RANGES:
                rd, rh, rmax = want["cast"][name]
                for n in eg.FANS:
                    what = f"{form}, level {lvl}, range_max {name}, {n} beams"
                    got = tcast.cast_device(g, lvl, c["poses"], c["angles"][:n], rmax)
                    assert lib.hsm_last_launch_kernel(g._h) == tcast.FORMS[form], what
                    tcast.assert_rays(what, got, (rd[:, :n], rh[:, :n]))
            if form != "lane":
                continue
            assert g.map_metadata(lvl) == c["meta"], (lvl, g.map_metadata(lvl), c["meta"])
            d_b, d_e = dev(c["begin"]), dev(c["end"])
            dist = torch.full((eg.N_RAYS,), SENTINEL, dtype=torch.float32, device="cuda:0")
            hit = torch.full((eg.N_RAYS, 2), float("nan"), dtype=torch.float32, device="cuda:0")
            g.ray_distances_device(lvl, eg.N_RAYS, d_b.data_ptr(), d_e.data_ptr(), dist.data_ptr(), hit.data_ptr(),
                                   origin_xy=c["meta"][:2], resolution=c["meta"][2], stream=stream_ptr())
            got = dist.cpu().numpy(), hit.cpu().numpy()
            assert lib.hsm_last_launch_kernel(g._h) == b"ray_distance_kernel"
            tcast.assert_rays(f"level {lvl}, device rays", got, want["rays"])
            tcast.assert_rays(f"level {lvl}, host rays", g.ray_distances(lvl, c["begin"], c["end"]), want["rays"])
        if form == "lane":  # the host form, once per map and layout
            c, (rd, rh, rmax) = eg.level_case(oracle_mod, m, 0), eg.expected(oracle_mod, m, 0, KIND)["cast"]["short_side"]
            tcast.assert_rays("host cast", g.cast_scans(0, c["poses"], c["angles"], rmax), (rd, rh))
        g.close()


# ---- window scores --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,layout", BOTH, ids=ids(BOTH))
def test_window_scores_and_poses_on_every_level(capi, oracle_mod, monkeypatch, m, layout):
    lib = capi.load_library()
    centre, pts = m.scan(oracle_mod)
    step = eg.window_step(m)
    for form in tw.FORMS:
        tw.forced(monkeypatch, form)
        g = new_ctx(capi, oracle_mod, m, layout)
        for half in eg.WINDOWS:
            d_poses = tw.written_poses(g, centre, step, half)
            assert same(d_poses.cpu().numpy(), window_cases.window_poses(centre, step, half)), (form, half, "window poses")
            for lvl in range(m.levels):
                for n in eg.SCAN_LENS:
                    what = f"{form} level {lvl} window {half} {n} beams"
                    got = tw.score_window(g, lvl, centre, step, half, pts[:n])
                    assert lib.hsm_last_launch_kernel(g._h) == tw.KERNEL[form], what
                    assert lib.hsm_last_launch_parity(g._h) == capi.PARITY_EXACT, what
                    tw.assert_same_scores(what, got, eg.expected_window(oracle_mod, m, lvl, half, n, KIND), n)
                    tw.assert_same_scores(what + " (batched score)", got, tw.score_batch(g, lvl, d_poses, pts[:n]), n)
        if form == "lane":  # the host form
            lh, res = g.score_window(0, centre, step, (3, 2, 1), pts)
            want = eg.expected_window(oracle_mod, m, 0, (3, 2, 1), 200, KIND)
            assert same(lh, want[0]) and same(res, want[1])
        g.close()


# ---- relocalisation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", eg.MAPS, ids=eg.MAP_IDS)
def test_relocalize_equals_the_four_calls_and_the_reference(capi, oracle_mod, m):
    import torch
    g = new_ctx(capi, oracle_mod, m)
    centre, scan = m.scan(oracle_mod)
    half, k = eg.RELOC_HALF, eg.RELOC_K
    s = torch.cuda.Stream()
    for at, lvl in enumerate(eg.reloc_levels(m)):
        step = eg.reloc_step(oracle_mod, m, lvl)
        ref = eg.expected_reloc(oracle_mod, m, lvl, KIND)
        one, four = (tw.RelocBuffers(capi, centre, scan, step, half, k) for _ in range(2))
        torch.cuda.synchronize()
        one.one_call(g, lvl, s.cuda_stream)
        four.four_calls(g, lvl, s.cuda_stream)
        s.synchronize()
        r1, r4 = one.host(), four.host()
        kidx = four.kidx.cpu().numpy()
        place = int(r4["best_index"][0])
        assert 0 <= place < k, (lvl, place)
        r4["best_index"] = kidx[[place]]  # the fourth call names the place among the k; the one call the window index behind it
        for key in r1:
            assert not (r1[key] == (99 if key == "best_index" else SENTINEL)).any(), (lvl, key)
            assert tw.same_bits(r1[key], r4[key]), (lvl, key)
        assert same(four.scores.cpu().numpy(), ref["scores"]), (lvl, "window scores")
        assert np.array_equal(kidx, ref["index"]) and same(four.kscore.cpu().numpy(), ref["top"]), (lvl, kidx, ref["index"])
        if eg.tied_places(ref) >= k:  # a tied coarse level: the index alone decides
            assert np.array_equal(kidx, topk_rule.topk(ref["scores"], k)[0]) and kidx.tolist() == list(range(k)), (lvl, kidx)
        assert same(four.start.cpu().numpy(), ref["start"]), (lvl, "starts")
        assert same(r1["cand"], ref["cand"]) and same(r1["cov"], ref["cov"]) and same(r1["lh0"], ref["lh0"]), (lvl, "candidates")
        assert r1["best_index"][0] == ref["best_index"] and bits(r1["best_score"])[0] == bits(ref["best_score"]), lvl
        assert same(r1["best_pose"], ref["best_pose"]), (lvl, r1["best_pose"], ref["best_pose"])
        if at == 0:  # the host form, once per map
            h = g.relocalize(lvl, centre, step, half, k, scan)
            assert tw.same_bits(h["cand_pose"], r1["cand"]) and tw.same_bits(h["cand_cov"], r1["cov"])
            assert tw.same_bits(h["cand_likelihood"], r1["lh0"]) and tw.same_bits(h["best_pose"], r1["best_pose"])
            assert bits(h["best_score"]) == bits(r1["best_score"])[0] and h["best_index"] == r1["best_index"][0]
    g.close()


# ---- copies ---------------------------------------------------------------------------------------------------------------------------
N_SRC, N_MORE = 3, 2
COPY_MAPS = [eg.map_of(None, eg.COPY_DEEP), eg.map_of(*eg.COPY_FRAME)]


def update_log(oracle_mod, m):
    """(world poses, scans) of five updates: the deep case's first build scans, or frame_cases.trajectory on the frame"""
    if m.kind == "deep":
        c = m.case()
        return c.build_poses[:N_SRC + N_MORE + 1], c.build_scans[:N_SRC + N_MORE + 1]
    _, world, scans = fc.trajectory(oracle_mod, m.frame, m.geom, N_SRC + N_MORE + 1, 300)
    return world, scans


def updated_checkers(oracle_mod, m, n):
    """per kind a checker of its own: the empty deep map, or the frame's room, and the first n updates of the log"""
    poses, scans = update_log(oracle_mod, m)
    out = {}
    for kind in oracle_kinds():
        o = deep_cases.new_oracle(oracle_mod, kind, m.geom) if m.kind == "deep" else fc.new_oracle(oracle_mod, kind, m.frame, m.geom, fc.FACTORS)
        o.build_map(np.asarray(poses[:n], np.float32), scans[:n])
        out[kind] = o
    return out


@pytest.mark.parametrize("layout", ("quad", "plane"))
@pytest.mark.parametrize("m", COPY_MAPS, ids=[m.id for m in COPY_MAPS])
def test_whole_copy_is_the_source_and_stays_it(capi, oracle_mod, m, layout):
    poses, scans = update_log(oracle_mod, m)
    frame_map = m.kind == "frame"
    src, dst = new_ctx(capi, oracle_mod, m, layout, upload=frame_map), new_ctx(capi, oracle_mod, m, layout, upload=False)
    for k in range(N_SRC):
        single_update(capi, src, poses[k], scans[k])
    single_update(capi, dst, poses[-1], scans[-1])   # other contents, another counter
    assert dst.getUpdateIndex(0) != src.getUpdateIndex(0)
    dst.copy_map_from(src)
    s_dst = at_copy = tcopy.state(dst)
    tcopy.assert_same_state(s_dst, tcopy.state(src), "copy")
    tcopy.assert_state_is_checkers(oracle_mod, s_dst, updated_checkers(oracle_mod, m, N_SRC), N_SRC, "copy")
    for g in (src, dst):
        for k in range(N_SRC, N_SRC + N_MORE):
            single_update(capi, g, poses[k], scans[k])
    s_dst, s_src = tcopy.state(dst), tcopy.state(src)
    tcopy.assert_same_state(s_dst, s_src, "copy + 2 updates")
    after = updated_checkers(oracle_mod, m, N_SRC + N_MORE)
    tcopy.assert_state_is_checkers(oracle_mod, s_dst, after, N_SRC + N_MORE, "copy + 2 updates, the copy")
    tcopy.assert_state_is_checkers(oracle_mod, s_src, after, N_SRC + N_MORE, "copy + 2 updates, the source")
    assert not same(s_dst[0][0], at_copy[0][0])  # the two updates do change the map
    src.close()
    dst.close()


@pytest.mark.parametrize("layout", ("quad", "plane"))
def test_box_copies_on_odd_widths_leave_the_rest_alone(capi, oracle_mod, layout):
    m = eg.map_of(None, eg.COPY_DEEP)
    L = m.levels
    src, dst, exp = (new_ctx(capi, oracle_mod, m, layout, upload=(k == 0)) for k in range(3))
    tiny = np.float32([[3.0, 0.2], [0.1, 3.0], [-3.0, 0.3]])
    for _ in range(2):  # src's counters move; an upload leaves them where they are
        single_update(capi, src, m.case().build_poses[0], tiny)
    m.upload(oracle_mod, src)
    s_src = tcopy.state(src)
    prior = [eg.prior_planes(m.geom, lvl) for lvl in range(L)]
    for lvl in range(L):
        assert not same(s_src[lvl][0], prior[lvl][0]) and s_src[lvl][3] == 1
    for names, boxes in eg.copy_rounds(m.geom):
        for lvl in range(L):
            dst.upload_level(lvl, *prior[lvl])
            dst.take_dirty_bbox(lvl)
        dst.copy_map_from(src, boxes)
        for lvl, (x0, y0, x1, y1) in enumerate(boxes.tolist()):
            what = (layout, "level", lvl, names[lvl], (x0, y0, x1, y1))
            sx, sy = m.dims(lvl)
            inside = np.zeros((sy, sx), bool)
            if x1 >= x0 and y1 >= y0:
                inside[y0:y1 + 1, x0:x1 + 1] = True
            want_lo, want_ui = np.where(inside, s_src[lvl][0], prior[lvl][0]), np.where(inside, s_src[lvl][1], prior[lvl][1])
            lo, ui = dst.download_level(lvl)
            assert same(lo, want_lo) and np.array_equal(ui, want_ui), what + ("planes", int((bits(lo) != bits(want_lo)).sum()))
            _, p = oracle_mod.libm_expf(want_lo.reshape(-1), KIND)
            assert same(dst.download_prob(lvl).reshape(-1), p), what + ("probabilities",)
            assert dst.getUpdateIndex(lvl) == 1, what + ("counter",)
            assert dst.take_dirty_bbox(lvl).tolist() == ([x0, y0, x1, y1] if inside.any() else [0, 0, -1, -1]), what + ("dirty box",)
            if inside.any() and sx > 2 and sy > 2:  # the samples around the box's edges: the quad layout's texels
                exp.upload_level(lvl, want_lo, want_ui)
                seam = tcopy.seam_points(sx, sy, (x0, y0, x1, y1))
                assert same(dst.eval_beams(lvl, tcopy.ZERO3, seam), exp.eval_beams(lvl, tcopy.ZERO3, seam)), what + ("samples",)
        dst.copy_map_from(exp, np.int32([[0, 0, -1, -1]] * L))  # exp's counters back: the next round's copy must set them again
        assert dst.getUpdateIndex(0) == -1
    for g in (src, dst, exp):
        g.close()


def test_staged_route_gives_the_same_bits():
    """the whole copies and the box copies again with HSM_COPY_STAGE=1, in a fresh child: every copy goes through the staging patch"""
    if os.environ.get("HSM_COPY_STAGE") == "1":
        pytest.fail("the child run must not select this test")
    env = dict(os.environ, HSM_COPY_STAGE="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__),
                        "-k", "whole_copy or box_copies"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "6 passed" in r.stdout, r.stdout[-2000:]


REFUSAL_BASE = (0.03, (0.3, 0.7))
REFUSALS = {"the start x alone": (0.03, (0.4, 0.7)), "the start y alone": (0.03, (0.3, 0.6)), "the resolution alone": (0.06, (0.3, 0.7))}


@pytest.mark.parametrize("layout", ("quad", "plane"))
def test_copies_between_different_frames_are_refused(capi, oracle_mod, layout):
    assert REFUSAL_BASE == eg.SENSITIVE_FRAME
    m = eg.map_of(eg.SENSITIVE_FRAME, (64, 64, 2))
    dst = new_ctx(capi, oracle_mod, m, layout)
    twin = new_ctx(capi, oracle_mod, m, layout, upload=False)
    lib = dst._lib
    boxes = np.int32([[0, 0, 9, 9]] * m.levels)
    before = tcopy.state(dst)
    for name, frame in REFUSALS.items():
        other = new_ctx(capi, oracle_mod, m, layout, upload=False, frame=frame)
        assert [other.level_info(l)[:2] for l in range(m.levels)] == [dst.level_info(l)[:2] for l in range(m.levels)]
        for rc in (lib.hsm_copy_map(dst._h, other._h), lib.hsm_copy_map_boxes(dst._h, other._h, boxes.ctypes.data),
                   lib.hsm_copy_map(other._h, dst._h), lib.hsm_copy_map_boxes(other._h, dst._h, boxes.ctypes.data)):
            msg = lib.hsm_last_error().decode()
            assert rc == HSM_ERR_INVALID and "differ" in msg, (name, rc, msg)
        tcopy.assert_same_state(tcopy.state(dst), before, name)
        assert not np.asarray(tcopy.state(other)[0][0]).any(), (name, "the refused copy wrote into the other context")
        other.close()
    twin.copy_map_from(dst)  # the same frame: accepted
    tcopy.assert_same_state(tcopy.state(twin), before, "the same frame")
    dst.close()
    twin.close()
