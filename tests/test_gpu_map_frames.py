"""Every entry point against the reference on off-centre maps and odd cell sizes (cases: tests/frame_cases.py, pinned on the
CPU by tests/test_frame_reference.py).
(The cast, window and copy entries came after this file: tests/test_gpu_entry_geometries.py holds them to the same frames.)

The map frame -- start coordinates and resolution -- reaches the device in a dozen places: mapTworld / worldTmap once per
matcher form, the scorer, the per-level transforms of the device-side updates, the host update, the tile sort, the cell
length of the covariance probe, set_map_transformation itself and the group's replicas.  Everywhere else in the suite the
frame is (0.5, 0.5) at 0.05, 0.1 or 0.125, where x and y translations are equal whole numbers of cells and worldTmap is
exactly (cell length, -offset): swapped offsets, another level's offset or a rebuilt inverse would not show.  Here the same
cells are seen through eight frames (frame_cases.FRAMES) on two-level maps of 64 x 64 and 90 x 24 and a three-level 96 x 40.

Library default mode (the reference's summation order): every comparison is on uint32 views, against the checker
oracle_kinds()[-1] (the reference headers where they are built; the pin shows both checkers agree on every case).  The
opt-in fast forms are held to the float64 sums of tests/gn_f64.py with its own bound, on two frames of small world
coordinates: that bound works in map coordinates, the frame enters through the start pose only.  The form tables are those of the map-edge test.

The update forms are one test each, so that a slip in update_prep_kernel's per-level transforms shows in the device forms'
ids and leaves the host forms' green.
"""
import numpy as np
import pytest

import frame_cases as fc
import gn_f64
from conftest import bits, oracle_kinds
from support import capi, dev, new_context, pack, same
from test_gpu_border_sampling import BATCH_FORMS, BATCH_PARAMS, WPS, check_one_step

pytestmark = pytest.mark.gpu
FRAMES = pytest.mark.parametrize("frame", fc.FRAMES, ids=fc.fid)
GEOMS = pytest.mark.parametrize("geom", fc.GEOMETRIES, ids=fc.gid)
LAYOUTS = pytest.mark.parametrize("layout", ["quad", "plane"])
KIND = oracle_kinds()[-1]
F = np.float32
ZERO2 = np.zeros(2, F)
_REF = {}


def new_ctx(capi, frame, geom, layout="quad", upload=True, **kw):
    """a context in the library's default mode, in the frame, that holds the case's map"""
    g = new_context(capi, frame[0], geom[0], geom[1], geom[2], frame[1], layout, fc.FACTORS, **kw)
    if upload:
        fc.upload(g, geom)
    g.synchronize()
    return g


def ref(oracle_mod, frame, geom, key, op):
    """op(checker) once per frame, geometry and key, shared by the tests; the shared checker's map is never changed"""
    k = (frame, geom, key)
    if k not in _REF:
        o = fc.checker(oracle_mod, KIND, frame, geom)
        _REF[k] = op(o)
        assert o.undefined_reads() <= 0, (k, "the case has no reference result")
    return _REF[k]


# ---- geometry -------------------------------------------------------------------------------------------------------------------
@GEOMS
@FRAMES
def test_level_geometry_and_pose_conversions(capi, oracle_mod, frame, geom):
    """level_info, getScaleToMap, getMapCoordsPose and getWorldCoordsPose of every level on 40 poses each way (the far frame's
    80 m poses among them): the checker's bits and the numpy statement's"""
    g = new_ctx(capi, frame, geom, upload=False)
    o = fc.checker(oracle_mod, KIND, frame, geom)
    lv = fc.frame_numpy(frame, geom)
    assert g.getMapLevels() == geom[2] and same(g.getScaleToMap(), o.scale_to_map()) and same(g.getScaleToMap(), lv[0]["scale"])
    for lvl in range(geom[2]):
        got, want = g.level_info(lvl), o.level_info(lvl)
        assert got[:2] == want[:2] and same(got[2:], want[2:]), (lvl, got, want)
        mp, world = fc.geometry_poses(oracle_mod, frame, geom, lvl)
        for p in mp:
            w = g.getWorldCoordsPose(lvl, p)
            assert same(w, o.world_coords_pose(lvl, p)) and same(w, fc.world_coords_numpy(lv[lvl], p)), (lvl, p, w)
        for w in world:
            p = g.getMapCoordsPose(lvl, w)
            assert same(p, o.map_coords_pose(lvl, w)) and same(p, fc.map_coords_numpy(lv[lvl], w)), (lvl, w, p)
    g.close()


# ---- probes at a world pose -------------------------------------------------------------------------------------------------------
PROBE_SIZES = (1, 65, 300, 1081)


@LAYOUTS
@GEOMS
@FRAMES
def test_probes_at_a_world_pose(capi, oracle_mod, frame, geom, layout):
    """per-beam terms, H and dTr, likelihood, residual and the sigma-point covariance (the one reader of cell_length) at the
    map pose of each case's start pose, on every level; hsm_score_batch_device from the world poses themselves"""
    g = new_ctx(capi, frame, geom, layout)
    cases = fc.pairs(oracle_mod, frame, geom, PROBE_SIZES)
    for lvl in range(geom[2]):
        up = F(2.0 ** lvl)  # the probes take level-0 end points and scale them by 2^-level themselves (exact)
        for tag, w, pts in cases:
            lp = fc.level_pts(pts, lvl)
            pm = g.getMapCoordsPose(lvl, w)
            want = ref(oracle_mod, frame, geom, ("probes", lvl, tag), lambda o: (
                o.map_coords_pose(lvl, w), o.hessian_derivs(lvl, o.map_coords_pose(lvl, w), lp),
                o.likelihood_states(lvl, o.map_coords_pose(lvl, w)[None], lp), o.residual_states(lvl, o.map_coords_pose(lvl, w)[None], lp),
                o.covariance_for_poses(lvl, o.map_coords_pose(lvl, w)[None], lp)))
            assert same(pm, want[0]), (lvl, tag, pm, want[0])
            s, c = (v[0] for v in oracle_mod.libm_sincosf(pm[2:3], KIND))
            co = fc.bc.transform(pm, lp, (s, c))
            beams = ref(oracle_mod, frame, geom, ("interp", lvl, tag), lambda o: o.interp(lvl, co))
            got = g.eval_beams(lvl, pm, lp)
            assert same(got[:, :3], beams), (lvl, tag, "beams")
            Hg, dg = g.hessian_derivs(lvl, pm, lp)
            assert same(Hg, want[1][0]) and same(dg, want[1][1]), (lvl, tag, Hg, want[1][0])
            assert same(g.likelihood_states(lvl, pm[None], lp * up), want[2]), (lvl, tag)
            assert same(g.residual_states(lvl, pm[None], lp * up), want[3]), (lvl, tag)
            for a, b, what in zip(g.covariance_for_poses(lvl, pm[None], lp * up), want[4], ("cov map", "cov world", "likelihoods")):
                assert same(a, b), (lvl, tag, what, a, b)
        poses = np.stack([w for _, w, _ in cases])
        pts_all, offs = pack([p for _, _, p in cases])
        lh, rs = g.score_batch(lvl, poses, pts_all, offs)
        for j, (tag, w, pts) in enumerate(cases):
            want = _REF[(frame, geom, ("probes", lvl, tag))]
            assert same(lh[j], want[2][0]) and same(rs[j], want[3][0]), (lvl, tag, "score", lh[j], want[2][0])
    g.close()


# ---- single scans -----------------------------------------------------------------------------------------------------------------
def check_single(g, oracle_mod, frame, geom, tag, w, pts, expect_kernel=None, levels=True):
    def cfg_ok():
        cfg = g.last_launch_config()
        assert cfg["parity_effective"] == "exact" and cfg["kernel"], (tag, cfg)
        if expect_kernel:
            assert cfg["kernel"] == expect_kernel, (tag, cfg)
    pg, cg = g.matchData(w, pts)
    cfg_ok()
    po, co = ref(oracle_mod, frame, geom, ("match", tag), lambda o: o.match(w, pts))
    assert same(pg, po) and same(cg, co), (fc.fid(frame), fc.gid(geom), tag, pg, po)
    assert not same(pg, w), (tag, "the match did not move")
    if not levels:
        return
    for lvl in range(geom[2]):
        lp = fc.level_pts(pts, lvl)
        for it in range(4):
            pg, cg = g.match_level(lvl, w, lp, it)
            cfg_ok()
            po, co = ref(oracle_mod, frame, geom, ("match_level", tag, lvl, it), lambda o: o.match_level(lvl, w, lp, it))
            assert same(pg, po) and same(cg, co), (fc.fid(frame), fc.gid(geom), tag, lvl, it, pg, po)


@pytest.mark.parametrize("wps", WPS)
@LAYOUTS
@GEOMS
@FRAMES
def test_single_scan_matchers_for_every_team_width(capi, oracle_mod, frame, geom, layout, wps):
    """matchData and match_level at 0 .. 3 iterations on every level: every scan size at the library's own width, four of
    them at the forced widths"""
    g = new_ctx(capi, frame, geom, layout, waves_per_scan=wps)
    sizes = fc.SCAN_SIZES if wps == 0 else (1, 65, 300, 1081)
    for tag, w, pts in fc.pairs(oracle_mod, frame, geom, sizes):
        check_single(g, oracle_mod, frame, geom, tag, w, pts)
    g.close()


@LAYOUTS
@GEOMS
@FRAMES
def test_dense_and_speculative_single_scan_forms(capi, oracle_mod, frame, geom, layout, monkeypatch):
    """gn_match_exact_dense_kernel and gn_match_spec_kernel (HSM_EXACT_DENSE_MIN lowered to 1920 beams) on the 1920-beam
    scan, gn_match_spec1_kernel on 560 .. 1920 beams"""
    monkeypatch.setenv("HSM_EXACT_DENSE_MIN", "1920")
    lit = new_ctx(capi, frame, geom, layout)
    monkeypatch.setenv("HSM_EXACT_SPEC", "1")
    spec = new_ctx(capi, frame, geom, layout)
    monkeypatch.delenv("HSM_EXACT_SPEC")
    monkeypatch.delenv("HSM_EXACT_DENSE_MIN")
    monkeypatch.setenv("HSM_EXACT_SPEC1", "1")
    spec1 = new_ctx(capi, frame, geom, layout)
    for tag, w, pts in fc.pairs(oracle_mod, frame, geom, (1920,)):
        check_single(lit, oracle_mod, frame, geom, tag, w, pts, "gn_match_exact_dense_kernel")
        check_single(spec, oracle_mod, frame, geom, tag, w, pts, "gn_match_spec_kernel")
    for tag, w, pts in fc.pairs(oracle_mod, frame, geom, (560, 720, 1081, 1300, 1920)):
        check_single(spec1, oracle_mod, frame, geom, tag, w, pts, "gn_match_spec1_kernel")
    for ctx in (lit, spec, spec1):
        ctx.close()


# ---- batches ----------------------------------------------------------------------------------------------------------------------
def batch_case(oracle_mod, frame, geom, cap, count):
    """count ragged scans (the cap-beam scan, shortened by 0 .. 4 beams) from a cloud of starts -> (starts, [scans])"""
    starts, pts = fc.batch(oracle_mod, frame, geom, count, cap)
    return starts, [np.ascontiguousarray(pts[: cap - (j % 5)]) for j in range(count)]


@pytest.mark.parametrize("form", BATCH_PARAMS)
@GEOMS
@FRAMES
def test_batches_in_every_exact_form(capi, oracle_mod, frame, geom, form, monkeypatch):
    """16 .. 64 ragged scans through the texel-cache exact form (chain wavefront and rotating owner; 5, 9, 13 and 17 cached
    rows; a streamed tail), the one-wavefront-per-scan form, the plane layout and the form a small batch picks by itself: in
    map order (sorted by tile key), and shuffled with the tile sort FORCED -- HSM_ORDER_MORTON and HSM_BATCH_ORDER_MIN lowered
    to 16: the default HSM_ORDER_AUTO sorts batches of 1024 scans and more only, so at 64 scans it would never run; then
    level 0 alone through the schedule hook"""
    rows_form, _, chain = form.partition("/")
    cached = rows_form in BATCH_FORMS
    cap, rows = BATCH_FORMS.get(rows_form, (1081, 17))
    rotating = chain == "rotating-owner"
    count = 16 + 4 * BATCH_PARAMS.index(form)  # 16 .. 64
    monkeypatch.setenv("HSM_EXACT_CHAIN_WAVE", "0" if rotating else "1")
    monkeypatch.setenv("HSM_EXACT_CACHED", "0" if form == "one-wave-per-scan" else "1")
    monkeypatch.setenv("HSM_BATCH_ORDER_MIN", "16")
    g = new_ctx(capi, frame, geom, "plane" if form == "plane-layout" else "quad", **({} if form == "auto" else {"waves_per_scan": 1}))

    def check_cfg():
        cfg = g.last_launch_config()
        assert cfg["parity_effective"] == "exact", cfg
        if cached:
            assert cfg["texel_cache"] and cfg["block"] == (256 if rotating else 320) and cfg["beams_per_lane"] == rows, cfg
            assert ("chain wavefront" in cfg["kernel"]) == (not rotating) and cfg["kernel"].startswith("gn_match_exact_cached_kernel"), cfg
        elif form != "auto":
            assert not cfg["texel_cache"], cfg

    assert 16 <= count <= 64
    starts, scans = batch_case(oracle_mod, frame, geom, cap, count)
    want = ref(oracle_mod, frame, geom, ("batch", cap, count), lambda o: [o.match(starts[j], scans[j]) for j in range(count)])
    keys = fc.tile_keys(geom, np.stack([fc.checker(oracle_mod, KIND, frame, geom).map_coords_pose(0, w) for w in starts])[:, :2])
    orders = {"map order": np.argsort(keys, kind="stable"), "shuffled": np.random.default_rng(count).permutation(count)}
    for name, order in orders.items():
        g.set_batch_order(capi.ORDER_MORTON if name == "shuffled" else capi.ORDER_GIVEN)
        pts, offs = pack([scans[j] for j in order])
        pb, cb = g.match_batch(starts[order], pts, offs)
        check_cfg()
        if name == "shuffled" and cached:  # (the forms without a texel cache keep the caller's order)
            assert g.last_launch_sorted(), (form, "the tile sort did not run")
        for slot, j in enumerate(order):
            assert same(pb[slot], want[j][0]) and same(cb[slot], want[j][1]), (form, name, slot, j, pb[slot], want[j][0])
    g.set_batch_order(capi.ORDER_GIVEN)
    pts, offs = pack(scans)
    for gn_steps in (1, 4):
        g.debug_set_schedule(0, gn_steps)
        pb, cb = g.match_batch(starts, pts, offs)
        check_cfg()
        lv = ref(oracle_mod, frame, geom, ("batch level", cap, count, gn_steps), lambda o: [
            o.match_level(0, starts[j], scans[j], gn_steps - 1) for j in range(count)])
        for j in range(count):
            assert same(pb[j], lv[j][0]) and same(cb[j], lv[j][1]), (form, "level 0, steps", gn_steps, j, pb[j], lv[j][0])
    g.debug_set_schedule(-1)
    g.close()


def test_tile_sort_follows_the_checkers_map_coordinates(capi, oracle_mod):
    """hsm_debug_batch_order on the 90 x 24 map of the (0.03, (0.3, 0.7)) frame, where swapping the two translations changes
    most tile keys (pinned on the CPU): the permutation orders the scans by the keys of the checker's map_coords_pose"""
    import torch
    world, back, swapped = fc.order_case(oracle_mod)
    o = fc.checker(oracle_mod, KIND, fc.ORDER_FRAME, fc.ORDER_GEOM)
    assert all(same(o.map_coords_pose(0, w), b) for w, b in zip(world, back))
    keys = fc.tile_keys(fc.ORDER_GEOM, back[:, :2])
    g = new_ctx(capi, fc.ORDER_FRAME, fc.ORDER_GEOM, upload=False)
    g.set_batch_order(capi.ORDER_MORTON)
    d_b, d_p = dev(world), torch.full((len(world),), -1, dtype=torch.int32, device="cuda:0")
    s = torch.cuda.Stream()
    g.debug_batch_order(len(world), d_b.data_ptr(), d_p.data_ptr(), s.cuda_stream)
    s.synchronize()
    perm = d_p.cpu().numpy()
    assert np.array_equal(np.sort(perm), np.arange(len(world))), perm
    assert (np.diff(keys[perm]) >= 0).all(), (perm, keys[perm])
    assert not (np.diff(fc.tile_keys(fc.ORDER_GEOM, swapped[:, :2])[perm]) >= 0).all()  # the case tells the two apart
    g.close()


# ---- score and select ---------------------------------------------------------------------------------------------------------------
@GEOMS
@FRAMES
def test_score_and_select_over_64_hypotheses(capi, oracle_mod, frame, geom):
    """hsm_score_batch_device on every level and hsm_match_score_batch_device with one group of 64: the scores, the matched
    poses, the winner's index and pose"""
    g = new_ctx(capi, frame, geom)
    starts, pts = fc.batch(oracle_mod, frame, geom, 64, 300)
    for lvl in range(geom[2]):
        want = ref(oracle_mod, frame, geom, ("score64", lvl), lambda o: [
            (o.likelihood_states(lvl, o.map_coords_pose(lvl, w)[None], fc.level_pts(pts, lvl))[0],
             o.residual_states(lvl, o.map_coords_pose(lvl, w)[None], fc.level_pts(pts, lvl))[0]) for w in starts])
        lh, rs = g.score_batch(lvl, starts, pts, None)
        for j in range(64):
            assert same(lh[j], want[j][0]) and same(rs[j], want[j][1]), (lvl, j, lh[j], want[j][0])

    def chain(o):
        poses = [o.match(w, pts) for w in starts]
        scores = [o.likelihood_states(0, o.map_coords_pose(0, p)[None], pts)[0] for p, _ in poses]
        return poses, np.array(scores, F)
    poses, scores = ref(oracle_mod, frame, geom, ("chain64",), chain)
    r = g.match_score_batch(starts, pts, None, score_level=0, group_size=64)
    for j in range(64):
        assert same(r["pose"][j], poses[j][0]) and same(r["cov"][j], poses[j][1]), (j, r["pose"][j], poses[j][0])
    assert same(r["likelihood"], scores)
    best = int(np.argmax(scores))  # (the first of equal maxima, as the selection rule has it)
    assert np.isfinite(scores).all() and int(r["best_index"][0]) == best and same(r["best_score"][0], scores[best])
    assert same(r["best_pose"][0], poses[best][0])
    g.close()


# ---- updates ------------------------------------------------------------------------------------------------------------------------
TRAJ_BEAMS = [300, 63, 1920, 1, 560, 65]
ORIGO = np.array([0.25, -0.5], F)


def planes(g, geom):
    return [g.download_level(lvl) + (g.download_prob(lvl),) for lvl in range(geom[2])]


def assert_planes(oracle_mod, g, geom, snap, what):
    for lvl, (lo_g, ui_g, prob_g) in enumerate(planes(g, geom)):
        lo_o, ui_o = snap[lvl]
        assert np.array_equal(ui_g, ui_o), (what, lvl, "stamps", int((ui_g != ui_o).sum()))
        assert np.array_equal(bits(lo_g), bits(lo_o)), (what, lvl, "log odds", int((bits(lo_g) != bits(lo_o)).sum()))
        _, prob = oracle_mod.libm_expf(lo_o.reshape(-1), KIND)
        assert np.array_equal(bits(prob_g).reshape(-1), bits(prob)), (what, lvl, "probability")
        assert g.debug_marks_nonzero(lvl) == (0, 0), (what, lvl)


def update_reference(oracle_mod, frame, geom, origo):
    """a checker of its own over the six-step trajectory -> its planes after every update"""
    def run(_):
        u = fc.new_oracle(oracle_mod, KIND, frame, geom, fc.FACTORS)
        _, world, scans = fc.trajectory(oracle_mod, frame, geom, fc.N_TRAJ, TRAJ_BEAMS)
        snaps = []
        for k in range(fc.N_TRAJ):
            u.build_map(world[k][None], [scans[k]], origo)
            snaps.append([u.download_level(lvl) for lvl in range(geom[2])])
        assert u.undefined_reads() <= 0
        changed = int((bits(snaps[-1][0][0]) != bits(fc.map_planes(geom)[0][0])).sum())
        assert changed >= 100, ("the trajectory hardly touches the map", changed)
        return snaps
    return ref(oracle_mod, frame, geom, ("updates", tuple(float(v) for v in origo)), run)


def device_update(g, world, scans, form, origo=None):
    """the whole trajectory in ONE call of a device-side form; returns the buffers, which must outlive the update"""
    import torch
    s = torch.cuda.current_stream()
    n = len(scans)
    pts, offs = pack(scans)
    keep = [dev(world), dev(pts), dev(offs)]
    mb = max(len(x) for x in scans)
    if form == "device":
        g.update_by_scans_device(n, keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), 0, mb, origo, s.cuda_stream)
    elif form == "origos":
        keep.append(dev(np.repeat(np.asarray(ZERO2 if origo is None else origo, F)[None], n, 0)))
        g.update_by_scans_device_origos(n, keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), 0, mb, keep[3].data_ptr(), s.cuda_stream)
    else:  # gated, every scan forced
        keep += [dev(np.ones(n, np.uint8)), torch.full((n,), -7, dtype=torch.int32, device="cuda:0")]
        g.update_by_scans_device_gated(n, keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), 0, mb, origo, keep[3].data_ptr(),
                                       keep[4].data_ptr(), s.cuda_stream)
        g.synchronize()
        assert keep[4].cpu().numpy().tolist() == [1] * n, "a forced scan was not integrated"
    g.synchronize()
    return keep


UPDATE_FORMS = ["hsm_update_by_scan", "hsm_update_by_scan/byte-map", "hsm_update_by_scans", "device", "device/byte-map", "origos", "gated"]
HOST_FORMS = UPDATE_FORMS[:3]  # these reach the map through the host's transform (map_update.hip), the others through update_prep_kernel


@pytest.mark.parametrize("form", UPDATE_FORMS)
@GEOMS
@FRAMES
def test_every_update_form_over_a_six_step_trajectory(capi, oracle_mod, frame, geom, form, monkeypatch):
    """one form per test: hsm_update_by_scan scan by scan in both layouts (the keyed form; "/byte-map": HSM_MERGED_MARK_MAX
    lowered to 256 beams, the threshold from which a scan takes the byte-map form -- the library reports no update form, so
    that it was taken is not asserted), hsm_update_by_scans, hsm_update_by_scans_device, its origo-per-scan and gated forms
    in one call each; with a zero and a non-zero origo: log-odds, stamps and probability planes of every level.  The first
    three forms take the host's transform, the others update_prep_kernel's per-level copies: the three-level geometry tells
    a level's own transform from another's"""
    _, world, scans = fc.trajectory(oracle_mod, frame, geom, fc.N_TRAJ, TRAJ_BEAMS)
    if form.endswith("/byte-map"):
        monkeypatch.setenv("HSM_MERGED_MARK_MAX", "256")
    kind = form.partition("/")[0]
    for origo in (ZERO2, ORIGO):
        snaps = update_reference(oracle_mod, frame, geom, origo)
        what = (fc.fid(frame), fc.gid(geom), form, "origo", origo.tolist())
        if kind == "hsm_update_by_scan":
            ctxs = [new_ctx(capi, frame, geom, "quad"), new_ctx(capi, frame, geom, "plane")]
            for k in range(fc.N_TRAJ):
                for i, g in enumerate(ctxs):
                    a = scans[k]
                    capi._check(g._lib.hsm_retain_scan(g._h, a.ctypes.data, a.shape[0], origo), "hsm_retain_scan")
                    g.updateByScan(a, world[k], origo)
                    g.synchronize()
                    assert_planes(oracle_mod, g, geom, snaps[k], what + ("context", i, "update", k))
        else:
            ctxs = [new_ctx(capi, frame, geom)]
            if kind == "hsm_update_by_scans":
                pts, offs = pack(scans)
                ctxs[0].update_by_scans(world, pts, offs, origo)
                ctxs[0].synchronize()
            else:
                keep = device_update(ctxs[0], world, scans, kind, origo)
                del keep
            assert_planes(oracle_mod, ctxs[0], geom, snaps[-1], what)
        for g in ctxs:
            g.close()


# ---- the loop -----------------------------------------------------------------------------------------------------------------------
@GEOMS
@FRAMES
def test_slam_loop_over_a_12_scan_log(capi, oracle_mod, frame, geom):
    """hsm_slam_scans_device: match, gate (thresholds of 1.5 cells in metres and 0.1 rad: the pin shows the reference both
    integrates and rejects at least three scans), update -- every pose, covariance and decision, and all maps afterwards"""
    import torch
    world, deltas, scans = fc.slam_log(oracle_mod, frame, geom)

    def run(_):
        s = fc.new_oracle(oracle_mod, KIND, frame, geom, fc.FACTORS)
        poses, covs, flags = fc.reference_loop(s, frame, world, deltas, scans)
        assert s.undefined_reads() <= 0
        return poses, covs, flags, [s.download_level(lvl) for lvl in range(geom[2])]
    rp, rc, rf, snap = ref(oracle_mod, frame, geom, ("loop",), run)
    assert rf.sum() >= 3 and (~rf).sum() >= 3
    g = new_ctx(capi, frame, geom)
    g.set_update_gate(*fc.thresholds(frame))
    n = fc.N_LOG
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        pts, offs = pack(scans)
        d = {"start": dev(world[0]), "deltas": dev(deltas), "pts": dev(pts), "offs": dev(offs),
             "pose": torch.full((n, 3), -777.0, device="cuda:0"), "cov": torch.full((n, 9), -777.0, device="cuda:0"),
             "applied": torch.full((n,), -7, dtype=torch.int32, device="cuda:0")}
        g.slam_scans_device(n, d["start"].data_ptr(), d["deltas"].data_ptr(), d["pts"].data_ptr(), d["offs"].data_ptr(), fc.LOG_BEAMS, None,
                            0, d["pose"].data_ptr(), d["cov"].data_ptr(), d["applied"].data_ptr(), s.cuda_stream)
    s.synchronize()
    poses, covs, applied = d["pose"].cpu().numpy(), d["cov"].cpu().numpy(), d["applied"].cpu().numpy()
    assert np.array_equal(applied, rf.astype(np.int32)), (applied, rf.astype(int))
    assert same(poses, rp), np.nonzero((bits(poses) != bits(rp)).any(axis=1))[0]
    assert same(covs, rc), np.nonzero((bits(covs) != bits(rc)).any(axis=1))[0]
    g.synchronize()
    assert_planes(oracle_mod, g, geom, snap, (fc.fid(frame), fc.gid(geom), "loop"))
    del d
    g.close()


@GEOMS
@FRAMES
def test_slam_ranges_tf_loop_over_a_12_scan_log(capi, oracle_mod, frame, geom):
    """hsm_slam_ranges_tf_device: the same trajectory as raw ranges from a laser on a mount that moves from scan to scan, with
    hsm_scale_to_map() of the frame -- the beams each scan keeps, every pose, covariance and decision, and all maps afterwards,
    against the checker's projectLaser + rosPointCloudToDataContainer and its HectorSlamProcessor::update per scan"""
    import torch
    raw = fc.raw_log(oracle_mod, frame, geom)
    world, deltas, ranges, rows, a0, inc, lim, gates = raw

    def run(o):
        conts, origos = fc.convert_log(o, raw)
        s = fc.new_oracle(oracle_mod, KIND, frame, geom, fc.FACTORS)
        poses, covs, flags = fc.reference_loop(s, frame, world, deltas, conts, origos)
        assert s.undefined_reads() <= 0
        return poses, covs, flags, [s.download_level(lvl) for lvl in range(geom[2])], np.array([len(c) for c in conts], np.int32), origos
    rp, rc, rf, snap, counts, origos = ref(oracle_mod, frame, geom, ("tf loop",), run)
    assert rf.sum() >= 3 and (~rf).sum() >= 3 and (counts >= fc.LOG_BEAMS // 2).all() and (counts < fc.LOG_BEAMS).all()
    assert len({tuple(bits(o)) for o in origos}) == fc.N_LOG
    g = new_ctx(capi, frame, geom)
    g.set_update_gate(*fc.thresholds(frame))
    n = fc.N_LOG
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        nbytes = g.slam_ranges_tf_workspace(n, fc.LOG_BEAMS)
        assert nbytes > 0
        d = {"start": dev(world[0]), "deltas": dev(deltas), "ranges": dev(ranges), "T": dev(rows),
             "ws": torch.zeros((nbytes,), dtype=torch.uint8, device="cuda:0"),
             "pose": torch.full((n, 3), -777.0, device="cuda:0"), "cov": torch.full((n, 9), -777.0, device="cuda:0"),
             "applied": torch.full((n,), -7, dtype=torch.int32, device="cuda:0"), "counts": torch.full((n,), -7, dtype=torch.int32, device="cuda:0")}
        g.slam_ranges_tf_device(n, d["start"].data_ptr(), d["deltas"].data_ptr(), d["ranges"].data_ptr(), fc.LOG_BEAMS, a0, inc, lim[0], lim[1],
                                lim[2], d["T"].data_ptr(), False, gates[0], gates[1], gates[2], gates[3], g.getScaleToMap(), 0,
                                d["pose"].data_ptr(), d["cov"].data_ptr(), d["applied"].data_ptr(), d["counts"].data_ptr(), d["ws"].data_ptr(),
                                nbytes, s.cuda_stream)
    s.synchronize()
    poses, covs, applied = d["pose"].cpu().numpy(), d["cov"].cpu().numpy(), d["applied"].cpu().numpy()
    assert np.array_equal(d["counts"].cpu().numpy(), counts)
    assert np.array_equal(applied, rf.astype(np.int32)), (applied, rf.astype(int))
    assert same(poses, rp), np.nonzero((bits(poses) != bits(rp)).any(axis=1))[0]
    assert same(covs, rc), np.nonzero((bits(covs) != bits(rc)).any(axis=1))[0]
    g.synchronize()
    assert_planes(oracle_mod, g, geom, snap, (fc.fid(frame), fc.gid(geom), "tf loop"))
    del d
    g.close()


# ---- ingestion, occupancy export, the group -------------------------------------------------------------------------------------------
def test_ingestion_with_the_inexact_scale(capi, oracle_mod):
    """raw ranges through hsm_ingest_laser_scan with hsm_scale_to_map() of the 0.03 frame (33.333336: the one inexact scale),
    then matched: the end points and the pose"""
    frame, geom = fc.FRAMES[1], fc.GEOMETRIES[0]
    g = new_ctx(capi, frame, geom)
    o = fc.checker(oracle_mod, KIND, frame, geom)
    scale = g.getScaleToMap()
    assert same(scale, F(33.333336)) and same(scale, o.scale_to_map())
    _, w, pts = fc.pairs(oracle_mod, frame, geom, (300,))[0]
    rng = np.random.default_rng(8800)
    n = 360
    a0, inc = -2.3, 4.6 / (n - 1)
    ranges = (rng.uniform(0.3, 0.9, n)).astype(F)   # 10 .. 30 cells
    ranges[::37] = np.inf
    ranges[5::41] = 0.01
    want = o.laser_scan_to_container(ranges, a0, inc, 0.05, 2.0, o.scale_to_map())
    got = g.ingest_laser_scan(ranges, a0, inc, 0.05, 2.0)
    assert 300 <= len(want) < n and same(got, want)
    pg, cg = g.match_ingested(w)
    po, co = o.match(w, want)
    assert same(pg, po) and same(cg, co), (pg, po)
    g.close()


@pytest.mark.parametrize("frame", [fc.FRAMES[1], fc.FRAMES[3]], ids=fc.fid)
def test_occupancy_changes_after_an_update(capi, oracle_mod, frame):
    """hsm_occupancy_changes after one update on two off-centre frames: the grid equals the checker's on every level and the
    box holds every cell that changed"""
    geom = fc.GEOMETRIES[2]
    g = new_ctx(capi, frame, geom)
    u = fc.new_oracle(oracle_mod, KIND, frame, geom, fc.FACTORS)
    _, world, scans = fc.trajectory(oracle_mod, frame, geom, 2, [300, 560])
    grids = [np.full(fc.dims(geom, lvl)[::-1], 7, np.int8) for lvl in range(geom[2])]
    for lvl in range(geom[2]):
        g.occupancy_changes(lvl, grids[lvl])
        assert np.array_equal(grids[lvl], u.occupancy_grid(lvl)), (lvl, "first export")
    for k in range(2):
        before = [u.occupancy_grid(lvl).copy() for lvl in range(geom[2])]
        u.build_map(world[k][None], [scans[k]])
        a = scans[k]
        capi._check(g._lib.hsm_retain_scan(g._h, a.ctypes.data, a.shape[0], ZERO2), "hsm_retain_scan")
        g.updateByScan(a, world[k])
        for lvl in range(geom[2]):
            box = [int(v) for v in g.occupancy_changes(lvl, grids[lvl])]
            want = u.occupancy_grid(lvl)
            assert np.array_equal(grids[lvl], want), (lvl, k, int((grids[lvl] != want).sum()))
            ys, xs = np.nonzero(want != before[lvl])
            if len(xs):
                assert box[0] <= xs.min() and xs.max() <= box[2] and box[1] <= ys.min() and ys.max() <= box[3], (lvl, k, box)
    g.close()


def test_group_replicas_take_the_frame(capi, oracle_mod):
    """MapRepGroup(.., [0, 0], startCoords=..) on the (0.03, (0.3, 0.7)) frame: both replicas' geometry, and the batched match
    equal to one context's and to the checker's"""
    frame, geom = fc.FRAMES[1], fc.GEOMETRIES[1]
    grp = capi.MapRepGroup(frame[0], geom[0], geom[1], geom[2], [0, 0], startCoords=frame[1])
    o = fc.checker(oracle_mod, KIND, frame, geom)
    assert grp.size() == 2
    _, world = fc.geometry_poses(oracle_mod, frame, geom, 0)
    for i in range(2):
        m = grp.member(i)
        fc.upload(m, geom)
        m.synchronize()
        for lvl in range(geom[2]):
            assert same(m.level_info(lvl)[2:], o.level_info(lvl)[2:])
            assert all(same(m.getMapCoordsPose(lvl, w), o.map_coords_pose(lvl, w)) for w in world)
    starts, pts = fc.batch(oracle_mod, frame, geom, 32, 300)
    g = new_ctx(capi, frame, geom)
    pg, cg = grp.match_batch(starts, pts, None)
    ph, ch = g.match_batch(starts, pts, None)
    assert same(pg, ph) and same(cg, ch)
    for j in range(32):
        po, co = ref(oracle_mod, frame, geom, ("group", j), lambda o: o.match(starts[j], pts))
        assert same(pg[j], po) and same(cg[j], co), (j, pg[j], po)
    g.close()
    grp.close()


# ---- the opt-in tree-summation forms: one GN step against float64 -------------------------------------------------------------------
@LAYOUTS
@pytest.mark.parametrize("frame", [fc.FRAMES[1], fc.FRAMES[0]], ids=fc.fid)
def test_fast_forms_one_step_against_float64(capi, oracle_mod, frame, layout, monkeypatch):
    """HSM_PARITY_FAST on two frames (the inexact one and the node's default resolution): gn_match_cached_kernel (batches), the
    team form (1 .. 4 wavefronts) and gn_match_coop_kernel (HSM_COOP_MIN lowered) -- H of one step and the step itself within
    gn_f64's bound.  Not the far frame: check_step reads the step off the returned WORLD pose and allows two ulps of the map
    coordinate for that trip, and 80 m from the origin a world ulp is 3e-4 cell (the pin counts the poses that do not come
    back), forty times that allowance, for the reference as for the kernels"""
    geom = fc.GEOMETRIES[2]
    o = fc.checker(oracle_mod, "ho", frame, geom)
    cases = fc.pairs(oracle_mod, frame, geom, (300, 1081))
    fast = new_ctx(capi, frame, geom, layout, waves_per_scan=1, parity=capi.PARITY_FAST)
    for lvl in range(geom[2]):
        init = np.stack([w for _, w, _ in cases])
        pts, offs = pack([p for _, _, p in cases])
        fast.debug_set_schedule(lvl, 1)
        pb, cb = fast.match_batch(init, pts, offs)
        cfg = fast.last_launch_config()
        if layout == "quad":
            assert cfg["kernel"] == "gn_match_cached_kernel" and cfg["texel_cache"] and cfg["parity_effective"] == "fast", cfg
        else:
            assert cfg["parity_effective"] == "fast" and cfg["waves_per_scan"] == 1, cfg
        for j, (tag, w, p) in enumerate(cases):
            lp = fc.level_pts(p, lvl)
            check_one_step(fast, o, "ho", lvl, w, lp, pb[j], cb[j], gn_f64.depth_team(len(lp), 1), f"cached L{lvl} {tag}")
        fast.debug_set_schedule(-1)
    fast.close()
    for W in (1, 2, 4):
        g = new_ctx(capi, frame, geom, layout, waves_per_scan=W, parity=capi.PARITY_FAST)
        for lvl in range(geom[2]):
            for tag, w, p in cases:
                lp = fc.level_pts(p, lvl)
                pose, cov = g.match_level(lvl, w, lp, 0)
                cfg = g.last_launch_config()
                assert cfg["kernel"] == "gn_match_kernel" and cfg["waves_per_scan"] == W and cfg["parity_effective"] == "fast", cfg
                check_one_step(g, o, "ho", lvl, w, lp, pose, cov, gn_f64.depth_team(len(lp), W), f"team W={W} L{lvl} {tag}")
        g.close()
    monkeypatch.setenv("HSM_COOP_MIN", "1024")
    g = new_ctx(capi, frame, geom, layout, parity=capi.PARITY_FAST)
    for lvl in range(geom[2]):
        for tag, w, p in fc.pairs(oracle_mod, frame, geom, (1081, 1920)):
            lp = fc.level_pts(p, lvl)
            pose, cov = g.match_level(lvl, w, lp, 0)
            K = gn_f64.coop_workgroups(len(lp))
            cfg = g.last_launch_config()
            assert cfg["kernel"] == "gn_match_coop_kernel" and cfg["grid"] == K and cfg["block"] == 256, cfg
            check_one_step(g, o, "ho", lvl, w, lp, pose, cov, gn_f64.depth_coop(len(lp), K), f"coop L{lvl} {tag}")
    assert g.debug_coop_fallbacks() == 0
    g.close()
    assert o.undefined_reads() == 0
