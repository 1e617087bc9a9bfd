"""Every sampler kernel against the reference on the map's edge cells (cases: tests/border_cases.py, pinned on the CPU by
tests/test_border_reference.py).

All matcher, scorer and probe kernels share one beam loop -- rotate, add the estimate, bounds-test on the bit patterns, truncate
with a saturating convert, v_fract, gather four texels; out-of-map beams read an all-zero texel, the texel-cache forms re-gather
only where the effective offset changed (beam_sample.h cell_coord / sample_fetch, gn_match_exact.h locate).  Here that loop meets
coordinates exactly on 0, -0.0, subnormals, integers, dims - 2 and one ulp either side of it, and beams that cross the border
between two Gauss-Newton steps, on maps whose border cells all differ.  Library default mode (the reference's summation order):
every comparison is on uint32 views.  The opt-in fast forms are held to the float64 sums of tests/gn_f64.py with its bound.
"""
import numpy as np
import pytest

import border_cases as bc
import gn_f64
from conftest import bits
from support import capi, kind, new_context, pack, same

pytestmark = pytest.mark.gpu
GEOMS = pytest.mark.parametrize("geom", bc.GEOMETRIES, ids=bc.gid)
LAYOUTS = pytest.mark.parametrize("layout", ["quad", "plane"])
F = np.float32
_REF = {}


def new_ctx(capi, geom, layout="quad", **kw):
    """a context in the library's default mode that holds the case's map"""
    g = new_context(capi, bc.RES, geom[0], geom[1], geom[2], bc.START, layout, factors=None, **kw)
    bc.upload(g, geom)
    g.synchronize()
    return g


def ref(oracle_mod, kind, geom, key, op):
    """op(checker), computed once per checker, geometry and key and shared by the tests; guarded (border_cases.run_checked)"""
    k = (kind, geom, key)
    if k not in _REF:
        _REF[k] = bc.run_checked(oracle_mod, kind, geom, op)
    return _REF[k]


def eval_cases(geom, lvl):
    """(name, map-frame pose, end points of that level): the exact lists in both orders, the coordinates themselves from the
    +-0 poses, rotated poses over band points"""
    pm = bc.exact_map_pose(lvl)
    cases = []
    for n in (400, 1081):
        for order, pts in bc.in_orders(bc.level_list(geom, lvl, n)).items():
            cases.append((f"exact n{n} {order}", pm, pts))
    ex = bc.exact_coords(geom, lvl)
    for k, zp in enumerate(bc.ZERO_POSES):
        cases.append((f"zero pose {k}", zp, ex))
        cases.append((f"zero pose {k} reversed", zp, np.ascontiguousarray(ex[::-1])))
    for th in bc.THETAS:
        pmt = bc.exact_map_pose(lvl, th)
        cases.append((f"theta {th}", pmt, bc.level_list(geom, lvl, 720, pmt)))
    return cases


def check_beam_terms(g, oracle_mod, kind, geom, lvl, name, pm, pts):
    """hsm_eval_beams against interp of the transformed points plus the source's rotDeriv expression"""
    s, c = (v[0] for v in oracle_mod.libm_sincosf(pm[2:3], kind))
    co = bc.transform(pm, pts, (s, c))
    want = ref(oracle_mod, kind, geom, ("interp", lvl, name), lambda o: o.interp(lvl, co))
    got = g.eval_beams(lvl, pm, pts)
    bad = (bits(got[:, :3]) != bits(want)).any(1)
    assert not bad.any(), (bc.gid(geom), lvl, name, "beams", np.flatnonzero(bad)[:8], co[bad][:8], got[bad][:4], want[bad][:4])
    x, y = pts[:, 0], pts[:, 1]
    with np.errstate(over="ignore", invalid="ignore"):
        rot = ((-s * x - c * y) * want[:, 1] + (c * x - s * y) * want[:, 2]).astype(F)
    assert same(got[:, 3], rot), (bc.gid(geom), lvl, name, "rotDeriv")
    return int((want[:, 0] != 0).sum())


@LAYOUTS
@GEOMS
def test_one_evaluation_on_every_level(capi, oracle_mod, kind, geom, layout):
    """per-beam terms, H and dTr, likelihood, residual and the sigma-point covariance at the exact poses, at poses of +0 / -0
    components over end points of +0 / -0 / subnormals (the only way e + r is -0.0: what step_origin exists for), at rotated
    poses; hsm_score_batch_device from the world poses of the exact pose and of the map's corner"""
    g = new_ctx(capi, geom, layout)
    for lvl in range(geom[2]):
        up = F(2.0 ** lvl)  # the probes take level-0 end points and scale them by 2^-level themselves (exact)
        n_inside = {}
        for name, pm, pts in eval_cases(geom, lvl):
            n_inside[name] = check_beam_terms(g, oracle_mod, kind, geom, lvl, name, pm, pts)
            Hg, dg = g.hessian_derivs(lvl, pm, pts)
            Ho, do = ref(oracle_mod, kind, geom, ("H", lvl, name), lambda o: o.hessian_derivs(lvl, pm, pts))
            assert same(Hg, Ho) and same(dg, do), (lvl, name, Hg, Ho)
        assert n_inside["exact n400 built"] == 100 and n_inside["zero pose 1"] == 81 and n_inside["zero pose 2"] == 81
        states = np.concatenate([bc.exact_map_pose(lvl)[None], bc.ZERO_POSES, np.stack([bc.exact_map_pose(lvl, t) for t in bc.THETAS])])
        lists = [("exact n1081", bc.level_list(geom, lvl, 1081)), ("exact n400 reversed", bc.level_list(geom, lvl, 400)[::-1]),
                 ("coordinates", bc.exact_coords(geom, lvl))]
        for name, pts in lists:
            pts = np.ascontiguousarray(pts)
            lh, rs, cv = ref(oracle_mod, kind, geom, ("probes", lvl, name), lambda o: (
                o.likelihood_states(lvl, states, pts), o.residual_states(lvl, states, pts), o.covariance_for_poses(lvl, states, pts)))
            assert same(g.likelihood_states(lvl, states, pts * up), lh), (lvl, name)
            assert same(g.residual_states(lvl, states, pts * up), rs), (lvl, name)
            for a, b, what in zip(g.covariance_for_poses(lvl, states, pts * up), cv, ("cov map", "cov world", "likelihoods")):
                assert same(a, b), (lvl, name, what)
        # world poses: the exact pose (plain and rotated, over its own list) and the corner (map pose 0: end point == coordinate)
        world = [(bc.exact_world_pose(geom), bc.level_list(geom, lvl, 1081)), (bc.corner_world_pose(geom), bc.exact_coords(geom, lvl))]
        world += [(bc.exact_world_pose(geom, th), bc.level_list(geom, lvl, 560, bc.exact_map_pose(lvl, th))) for th in bc.THETAS[:3]]
        world.append((bc.exact_world_pose(geom), np.zeros((0, 2), F)))
        poses = np.stack([w for w, _ in world])
        pts, offs = pack([p * up for _, p in world])
        want = ref(oracle_mod, kind, geom, ("score", lvl), lambda o: [
            (o.likelihood_states(lvl, o.map_coords_pose(lvl, w)[None], p)[0], o.residual_states(lvl, o.map_coords_pose(lvl, w)[None], p)[0])
            for w, p in world])
        lh, rs = g.score_batch(lvl, poses, pts, offs)
        for j, (wl, wr) in enumerate(want):
            assert same(rs[j], wr) and (same(lh[j], wl) or (world[j][1].shape[0] == 0 and np.isnan(lh[j]) and np.isnan(wl))), (lvl, j)
    g.close()


def single_cases(geom):
    """(name, level or None for the whole pyramid, start world pose, end points, iteration counts)"""
    w0 = bc.exact_world_pose(geom)
    cases = []
    for lvl in range(geom[2]):
        for n in (400, 1081):
            for order, pts in bc.in_orders(bc.level_list(geom, lvl, n)).items():
                cases.append((f"L{lvl} n{n} {order}", lvl, w0, pts, (0, 1, 3, 7)))
    for n in bc.LIST_SIZES:
        for order, pts in bc.in_orders(bc.pyramid_list(geom, n)).items():
            cases.append((f"pyramid n{n} {order}", None, w0, pts, None))
    for th in bc.THETAS:
        cases.append((f"pyramid theta {th}", None, bc.exact_world_pose(geom, th), bc.pyramid_list(geom, 720, th), None))
    for seed in bc.CROSS_SEEDS:
        for n in (720, 1081):
            w, pts = bc.crossing_case(geom, seed, n)
            cases.append((f"crossing {seed} n{n}", 0, w, pts, tuple(range(bc.K_CROSS + 1))))
            cases.append((f"crossing {seed} n{n} pyramid", None, w, pts, None))
    return cases


def check_single(g, oracle_mod, kind, geom, case, expect_kernel=None):
    name, lvl, w, pts, its = case
    if lvl is None:
        pg, cg = g.matchData(w, pts)
        po, co = ref(oracle_mod, kind, geom, ("match", name), lambda o: o.match(w, pts))
        assert same(pg, po) and same(cg, co), (bc.gid(geom), name, pg, po)
        if expect_kernel:
            assert g.last_launch_config()["kernel"] == expect_kernel, (name, g.last_launch_config())
        return
    for it in its:
        pg, cg = g.match_level(lvl, w, pts, it)
        po, co = ref(oracle_mod, kind, geom, ("match_level", name, it), lambda o: o.match_level(lvl, w, pts, it))
        assert same(pg, po) and same(cg, co), (bc.gid(geom), name, it, pg, po)
        if expect_kernel:
            assert g.last_launch_config()["kernel"] == expect_kernel, (name, g.last_launch_config())


WPS = [0, 1, 2, 4, 8, 16]  # 0: the width the library picks (shared with tests/test_gpu_aged_maps.py, like the batch form tables)


@pytest.mark.parametrize("wps", WPS)
@LAYOUTS
@GEOMS
def test_single_scan_matchers_for_every_team_width(capi, oracle_mod, kind, geom, layout, wps):
    """match_level at 0, 1, 3 and 7 iterations on each level and matchData on the pyramid lists, the crossing cases step by
    step; the hook trace of every whole-pyramid case equal to the default team width's, record for record"""
    g = new_ctx(capi, geom, layout, waves_per_scan=wps)
    base = new_ctx(capi, geom, layout) if wps else g
    for case in single_cases(geom):
        check_single(g, oracle_mod, kind, geom, case)
        name, lvl, w, pts, _ = case
        if lvl is None and ("crossing" in name or "n1081" in name or "n300" in name):
            pose, cov, trace = g.match_trace(w, pts)
            po, co = ref(oracle_mod, kind, geom, ("match", name), lambda o: o.match(w, pts))
            assert trace.shape[0] == g.gn_iterations_per_match() and same(pose, po) and same(cov, co), name
            if base is not g:
                pb, cb, tb = base.match_trace(w, pts)
                assert same(trace, tb) and same(pose, pb) and same(cov, cb), name
    cov_in = np.arange(9, dtype=F)
    p, c = g.matchData(bc.exact_world_pose(geom), np.zeros((0, 2), F), cov_in)
    assert same(p, bc.exact_world_pose(geom)) and same(c, cov_in)
    g.close()
    if base is not g:
        base.close()


def dense_cases(geom):
    w0 = bc.exact_world_pose(geom)
    cases = []
    for n in (1920, 2561):
        for order, pts in bc.in_orders(bc.pyramid_list(geom, n)).items():
            cases.append((f"pyramid n{n} {order}", None, w0, pts, None))
        for order, pts in bc.in_orders(bc.level_list(geom, 0, n)).items():
            cases.append((f"L0 n{n} {order}", 0, w0, pts, (0, 3)))
    w, pts = bc.crossing_case(geom, bc.CROSS_SEEDS[0], 1920)
    cases.append(("crossing n1920", 0, w, pts, tuple(range(bc.K_CROSS + 1))))
    cases.append(("crossing n1920 pyramid", None, w, pts, None))
    return cases


@LAYOUTS
@GEOMS
def test_dense_and_speculative_single_scan_forms(capi, oracle_mod, kind, geom, layout, monkeypatch):
    """gn_match_exact_dense_kernel and gn_match_spec_kernel (HSM_EXACT_DENSE_MIN lowered to 1920 beams), gn_match_spec1_kernel
    (321 .. 2048 beams): the reference's bits, and the hook traces equal to the team form's"""
    monkeypatch.setenv("HSM_EXACT_DENSE_MIN", "1920")
    lit = new_ctx(capi, geom, layout)
    monkeypatch.setenv("HSM_EXACT_SPEC", "1")
    spec = new_ctx(capi, geom, layout)
    monkeypatch.delenv("HSM_EXACT_SPEC")
    monkeypatch.delenv("HSM_EXACT_DENSE_MIN")
    team = new_ctx(capi, geom, layout)
    monkeypatch.setenv("HSM_EXACT_SPEC1", "1")
    spec1 = new_ctx(capi, geom, layout)
    for case in dense_cases(geom):
        check_single(lit, oracle_mod, kind, geom, case, "gn_match_exact_dense_kernel")
        check_single(spec, oracle_mod, kind, geom, case, "gn_match_spec_kernel")
        name, lvl, w, pts, _ = case
        if lvl is None:
            tr = [ctx.match_trace(w, pts) for ctx in (team, lit, spec)]
            assert team.last_launch_config()["kernel"].startswith("gn_match_kernel"), team.last_launch_config()
            for other in tr[1:]:
                assert all(same(a, b) for a, b in zip(tr[0], other)), name
    for case in single_cases(geom):
        if 320 < case[3].shape[0] <= 2048 and ("n1081" in case[0] or "n720" in case[0] or "n560" in case[0] or "theta" in case[0]):
            check_single(spec1, oracle_mod, kind, geom, case, "gn_match_spec1_kernel")
            if case[1] is None:
                a, b = spec1.match_trace(case[2], case[3]), team.match_trace(case[2], case[3])
                assert all(same(x, y) for x, y in zip(a, b)), case[0]
    for ctx in (lit, spec, team, spec1):
        ctx.close()


BATCH_FORMS = {  # name: (beams of the longest scan, rows of the instantiation)
    "17rows": (1081, 17), "13rows": (720, 13), "9rows": (560, 9), "5rows": (300, 5), "tail": (1300, 17)}
BATCH_PARAMS = [f"{f}/{c}" for f in BATCH_FORMS for c in ("chain-wave", "rotating-owner")] + ["one-wave-per-scan", "plane-layout", "auto"]


def batch_scans(geom, cap):
    """a ragged batch: the pyramid list in both orders, an empty scan, the crossing cases, rotated starts, a short list"""
    w0 = bc.exact_world_pose(geom)
    scans = [(w0, pts) for pts in bc.in_orders(bc.pyramid_list(geom, cap)).values()]
    scans.append((w0, np.zeros((0, 2), F)))
    scans += [bc.crossing_case(geom, seed, cap) for seed in bc.CROSS_SEEDS]
    scans += [(bc.exact_world_pose(geom, th), bc.pyramid_list(geom, min(cap, 720), th)) for th in bc.THETAS[2:5]]
    scans.append((w0, bc.pyramid_list(geom, 300)[::-1]))
    return scans


@pytest.mark.parametrize("form", BATCH_PARAMS)
@GEOMS
def test_batches_in_every_exact_form(capi, oracle_mod, kind, geom, form, monkeypatch):
    """ragged CSR batches and a shared-scan batch of hypotheses around the exact pose through the texel-cache exact form (chain
    wavefront and rotating owner; 5, 9, 13 and 17 cached rows; a streamed tail), the one-wavefront-per-scan form, the plane
    layout and the form a small batch picks by itself; then one level at a time through the schedule hook: one step from the
    exact poses (every exact coordinate is hit), and the crossing cases over K_CROSS + 1 steps"""
    rows_form, _, chain = form.partition("/")
    cached = rows_form in BATCH_FORMS
    cap, rows = BATCH_FORMS.get(rows_form, (1081, 17))
    rotating = chain == "rotating-owner"
    monkeypatch.setenv("HSM_EXACT_CHAIN_WAVE", "0" if rotating else "1")
    monkeypatch.setenv("HSM_EXACT_CACHED", "0" if form == "one-wave-per-scan" else "1")
    g = new_ctx(capi, geom, "plane" if form == "plane-layout" else "quad", **({} if form == "auto" else {"waves_per_scan": 1}))

    def check_cfg():
        cfg = g.last_launch_config()
        assert cfg["parity_effective"] == "exact", cfg
        if cached:
            assert cfg["texel_cache"] and cfg["block"] == (256 if rotating else 320) and cfg["beams_per_lane"] == rows, cfg
            assert ("chain wavefront" in cfg["kernel"]) == (not rotating) and cfg["kernel"].startswith("gn_match_exact_cached_kernel"), cfg
        elif form != "auto":
            assert not cfg["texel_cache"], cfg

    scans = batch_scans(geom, cap)
    init = np.stack([w for w, _ in scans])
    pts, offs = pack([p for _, p in scans])
    pb, cb = g.match_batch(init, pts, offs)
    check_cfg()
    for j, (w, p) in enumerate(scans):
        po, co = ref(oracle_mod, kind, geom, ("batch", cap, j), lambda o: o.match(w, p, cov=np.zeros(9, F)))
        assert same(pb[j], po) and (p.shape[0] == 0 or same(cb[j], co)), (form, j, p.shape[0], pb[j], po)
    assert same(pb[2], init[2]) and not cb[2].any()  # the empty scan passes its start through
    # shared scan: nine hypotheses around the exact pose, the exact one among them
    hyp = np.repeat(bc.exact_world_pose(geom)[None], 9, 0)
    hyp[:, :2] += (np.arange(-4, 5, dtype=F) * F(bc.RES * 0.25))[:, None]
    hyp[:, 2] += np.arange(-4, 5, dtype=F) * F(0.004)
    shared = bc.pyramid_list(geom, cap)
    ph, ch = g.match_batch(hyp, shared, None)
    check_cfg()
    for k in range(9):
        po, co = ref(oracle_mod, kind, geom, ("hyp", cap, k), lambda o: o.match(hyp[k], shared))
        assert same(ph[k], po) and same(ch[k], co), (form, "hypothesis", k)
    # one level at a time
    for lvl in range(geom[2]):
        up = F(2.0 ** lvl)
        lv = [(bc.exact_world_pose(geom), p) for p in bc.in_orders(bc.level_list(geom, lvl, cap)).values()]
        lv.append((bc.exact_world_pose(geom), bc.level_list(geom, lvl, min(cap, 400))))
        lv += [(bc.exact_world_pose(geom, th), bc.level_list(geom, lvl, min(cap, 560), bc.exact_map_pose(lvl, th))) for th in bc.THETAS[:2]]
        steps = [1]
        if lvl == 0:
            lv += [bc.crossing_case(geom, seed, cap) for seed in bc.CROSS_SEEDS]
            steps.append(bc.K_CROSS + 1)
        init = np.stack([w for w, _ in lv])
        pts, offs = pack([p * up for _, p in lv])
        for gn_steps in steps:
            g.debug_set_schedule(lvl, gn_steps)
            pb, cb = g.match_batch(init, pts, offs)
            check_cfg()
            for j, (w, p) in enumerate(lv):
                po, co = ref(oracle_mod, kind, geom, ("sched", cap, lvl, gn_steps, j), lambda o: o.match_level(lvl, w, p, gn_steps - 1))
                assert same(pb[j], po) and same(cb[j], co), (form, "level", lvl, "steps", gn_steps, j, pb[j], po)
    g.debug_set_schedule(-1)
    g.close()


# ---- the opt-in tree-summation forms: same per-beam bits, sums within the float64 bound of tests/gn_f64.py ----------------------
def check_one_step(g, o, kind, lvl, w, pts, pose, cov, d, what):
    ev = gn_f64.Eval64(o, lvl, o.map_coords_pose(lvl, w), pts, kind)
    H = cov.reshape(3, 3).T
    gn_f64.check_H(H, ev, d, what)
    assert int(ev.nonzero().sum()) >= 50 and H[0, 0] != 0 and H[1, 1] != 0, what
    gn_f64.check_step(H, o.map_coords_pose(lvl, w), g.getMapCoordsPose(lvl, pose), ev, d, what)


@LAYOUTS
@GEOMS
def test_fast_forms_one_step_against_float64(capi, oracle_mod, geom, layout, monkeypatch):
    """HSM_PARITY_FAST: gn_match_cached_kernel (batches, one wavefront per scan), the team form (single scans, 1 .. 4 wavefronts)
    and gn_match_coop_kernel (HSM_COOP_MIN lowered): the per-beam terms are the reference's bits, H of one step and the step
    itself lie within the rounding bound of the form's addition depth.  These maps do not let Gauss-Newton settle: no pose bar"""
    kind = "ho"
    o = bc.checker(oracle_mod, kind, geom)
    fast = new_ctx(capi, geom, layout, waves_per_scan=1, parity=capi.PARITY_FAST)
    for lvl in range(geom[2]):
        for name, pm, pts in eval_cases(geom, lvl):
            check_beam_terms(fast, oracle_mod, kind, geom, lvl, name, pm, pts)
    w0 = bc.exact_world_pose(geom)
    for lvl in range(geom[2]):
        up = F(2.0 ** lvl)
        lv = [(w0, p) for n in (560, 1081) for p in bc.in_orders(bc.level_list(geom, lvl, n)).values()]
        lv += [(bc.exact_world_pose(geom, th), bc.level_list(geom, lvl, 720, bc.exact_map_pose(lvl, th))) for th in bc.THETAS[:3]]
        if lvl == 0:
            lv += [bc.crossing_case(geom, seed, 720) for seed in bc.CROSS_SEEDS]
        init = np.stack([w for w, _ in lv])
        pts, offs = pack([p * up for _, p in lv])
        fast.debug_set_schedule(lvl, 1)
        pb, cb = fast.match_batch(init, pts, offs)
        cfg = fast.last_launch_config()
        if layout == "quad":
            assert cfg["kernel"] == "gn_match_cached_kernel" and cfg["texel_cache"] and cfg["parity_effective"] == "fast", cfg
        else:
            assert cfg["parity_effective"] == "fast" and cfg["waves_per_scan"] == 1, cfg
        for j, (w, p) in enumerate(lv):
            check_one_step(fast, o, kind, lvl, w, p, pb[j], cb[j], gn_f64.depth_team(p.shape[0], 1), f"cached L{lvl} scan {j}")
        fast.debug_set_schedule(-1)
    fast.close()
    for W in (1, 2, 4):
        g = new_ctx(capi, geom, layout, waves_per_scan=W, parity=capi.PARITY_FAST)
        for lvl in range(geom[2]):
            for n in (400, 1081):
                for order, pts in bc.in_orders(bc.level_list(geom, lvl, n)).items():
                    pose, cov = g.match_level(lvl, w0, pts, 0)
                    cfg = g.last_launch_config()
                    assert cfg["kernel"] == "gn_match_kernel" and cfg["waves_per_scan"] == W and cfg["parity_effective"] == "fast", cfg
                    check_one_step(g, o, kind, lvl, w0, pts, pose, cov, gn_f64.depth_team(n, W), f"team W={W} L{lvl} n={n} {order}")
        g.close()
    monkeypatch.setenv("HSM_COOP_MIN", "1024")
    g = new_ctx(capi, geom, layout, parity=capi.PARITY_FAST)
    for lvl in range(geom[2]):
        for n in (1081, 1920):
            for order, pts in bc.in_orders(bc.level_list(geom, lvl, n)).items():
                pose, cov = g.match_level(lvl, w0, pts, 0)
                K = gn_f64.coop_workgroups(n)
                cfg = g.last_launch_config()
                assert cfg["kernel"] == "gn_match_coop_kernel" and cfg["grid"] == K and cfg["block"] == 256, cfg
                check_one_step(g, o, kind, lvl, w0, pts, pose, cov, gn_f64.depth_coop(n, K), f"coop L{lvl} n={n} {order}")
    assert g.debug_coop_fallbacks() == 0
    g.close()
    assert o.undefined_reads() == 0
