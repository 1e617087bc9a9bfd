"""Every matcher form against the reference on AGED maps and degenerate Gauss-Newton steps (cases: tests/aged_cases.py, pinned
on the CPU by tests/test_aged_reference.py).

The other GPU files hold the kernels to the reference on maps of young cells (log-odds within a few units of 0) and through
steps whose Hessian is regular or all zero.  Here the maps are what a long-lived map becomes -- free space far below -87
(probabilities subnormal or +0), walls at the 50.0 clamp (probability exactly 1.0f) -- and the steps are the ones between
"regular" and "NaN": one diagonal entry of H exactly 0 (step skipped), all of H +0 by underflow under a dTr of subnormals,
rotation steps beyond the +-0.2 clamp of either sign, final angles normalize_angle has to wrap, nearly singular H whose finite
step throws the pose off the map, and determinants that underflow (`tiny`: the solve goes non-finite).

Library default mode (the reference's summation order): every comparison is on uint32 views wherever the reference has a
result.  Where it has none (the restatement counted a read with a NaN coordinate: the reference headers crash there) the
kernels are compared with the restatement alone: the same components non-finite, every finite component bit-identical, the
call succeeds, and the matches that follow on the same context are bit-exact again.  The opt-in fast forms are held to the
float64 sums of tests/gn_f64.py with its bound and subnormal floor.  The form tables are those of the map-edge test.
"""
import numpy as np
import pytest

import aged_cases as ac
import gn_f64
from conftest import bits
from support import capi, kind, new_context, pack, same
from test_gpu_border_sampling import BATCH_FORMS, BATCH_PARAMS, WPS

pytestmark = pytest.mark.gpu
GEOMS = pytest.mark.parametrize("geom", ac.GEOMETRIES, ids=ac.gid)
LAYOUTS = pytest.mark.parametrize("layout", ["quad", "plane"])
DEFINED = pytest.mark.parametrize("family", ac.DEFINED)
FAMILIES = pytest.mark.parametrize("family", ac.FAMILIES)
F = np.float32
_REF = {}


def agrees(got, want):
    """bit-identical; where the checker's value has non-finite components: the same components non-finite, the finite ones
    bit-identical (NaN payloads and signs are pinned nowhere)"""
    got, want = np.asarray(got, F), np.asarray(want, F)
    fw = np.isfinite(want)
    if fw.all():
        return same(got, want)
    return np.array_equal(np.isfinite(got), fw) and np.array_equal(bits(got)[fw], bits(want)[fw])


def new_ctx(capi, family, geom, layout="quad", **kw):
    g = new_context(capi, ac.RES, geom[0], geom[1], geom[2], ac.START, layout, factors=None, **kw)
    ac.upload(g, family, geom)
    g.synchronize()
    return g


def ref(oracle_mod, kind, family, geom, key, op):
    """op(checker) once per checker, family, geometry and key.  The restatement runs first; if it counts an undefined read the
    reference has no result and the restatement's own is the yardstick -> (result, defined)"""
    k = (family, geom, key)
    if k not in _REF:
        ho = ac.checker(oracle_mod, "ho", family, geom)
        u0 = ho.undefined_reads()
        r = op(ho)
        _REF[k] = {"ho": r, "defined": ho.undefined_reads() == u0}
    e = _REF[k]
    if kind != "ho" and e["defined"]:
        if kind not in e:
            e[kind] = op(ac.checker(oracle_mod, kind, family, geom))
        return e[kind], True
    return e["ho"], e["defined"]


def level_pairs(family, geom, lvl, sizes=None, first_only=False):
    """(tag, pose index, start world pose, map pose of the level, end points of the level)"""
    out = []
    for j, (k, n, seed) in enumerate(ac.pairs(geom)):
        if (sizes is None or n in sizes) and not (first_only and j >= len(ac.SCAN_SIZES)):
            pts = ac.family_scan(family, geom, k, n, seed) * F(1.0 / 2 ** lvl)
            out.append((f"L{lvl} pose {k} n{n} seed {seed}", k, ac.world_pose(geom, k), ac.map_pose(geom, lvl, k), pts))
    return out


# ---- one evaluation -----------------------------------------------------------------------------------------------------------
@LAYOUTS
@DEFINED
@GEOMS
def test_one_evaluation_on_every_level(capi, oracle_mod, kind, geom, family, layout):
    """per-beam terms, H and dTr on every (pose, scan) pair; likelihood, residual, sigma-point covariance and
    hsm_score_batch_device on four of the scan lengths: bit-exact"""
    g = new_ctx(capi, family, geom, layout)
    for lvl in range(geom[2]):
        up = F(2.0 ** lvl)
        states = np.stack([ac.map_pose(geom, lvl, k) for k in range(4)])
        for tag, k, w, pm, pts in level_pairs(family, geom, lvl):
            s, c = (v[0] for v in oracle_mod.libm_sincosf(pm[2:3], kind))
            co = ac.bc.transform(pm, pts, (s, c))
            want, _ = ref(oracle_mod, kind, family, geom, ("interp", tag), lambda o: o.interp(lvl, co))
            got = g.eval_beams(lvl, pm, pts)
            assert same(got[:, :3], want), (family, tag, "beams")
            x, y = pts[:, 0], pts[:, 1]
            with np.errstate(under="ignore"):
                rot = ((-s * x - c * y) * want[:, 1] + (c * x - s * y) * want[:, 2]).astype(F)
            assert same(got[:, 3], rot), (family, tag, "rotDeriv")
            (Ho, do), _ = ref(oracle_mod, kind, family, geom, ("H", tag), lambda o: o.hessian_derivs(lvl, pm, pts))
            Hg, dg = g.hessian_derivs(lvl, pm, pts)
            assert same(Hg, Ho) and same(dg, do), (family, tag, Hg, Ho, dg, do)
            if family == "wall_x":
                assert Hg[1, 1] == 0 and Hg[0, 0] != 0, (tag, Hg)
            elif family == "wall_y":
                assert Hg[0, 0] == 0 and Hg[1, 1] != 0, (tag, Hg)
            elif family == "deep_free":
                assert not Hg.any() and dg.any(), (tag, Hg, dg)
        probe = level_pairs(family, geom, lvl, sizes=(3, 65, 300, 1081), first_only=True)
        for tag, k, w, pm, pts in probe:
            (lh, rs, cv), _ = ref(oracle_mod, kind, family, geom, ("probes", tag), lambda o: (
                o.likelihood_states(lvl, states, pts), o.residual_states(lvl, states, pts), o.covariance_for_poses(lvl, states, pts)))
            assert agrees(g.likelihood_states(lvl, states, pts * up), lh), (family, tag)
            assert agrees(g.residual_states(lvl, states, pts * up), rs), (family, tag)
            for a, b, what in zip(g.covariance_for_poses(lvl, states, pts * up), cv, ("cov map", "cov world", "likelihoods")):
                assert agrees(a, b), (family, tag, what)
        poses = np.stack([w for _, _, w, _, _ in probe])
        pts_all, offs = pack([p * up for _, _, _, _, p in probe])
        want, _ = ref(oracle_mod, kind, family, geom, ("score", lvl), lambda o: [
            (o.likelihood_states(lvl, o.map_coords_pose(lvl, w)[None], p)[0], o.residual_states(lvl, o.map_coords_pose(lvl, w)[None], p)[0])
            for _, _, w, _, p in probe])
        lh, rs = g.score_batch(lvl, poses, pts_all, offs)
        for j, (wl, wr) in enumerate(want):
            assert agrees(lh[j], wl) and agrees(rs[j], wr), (family, lvl, j)
    g.close()


# ---- the reference-order matchers -----------------------------------------------------------------------------------------------
def single_cases(family, geom, first_only=False, sizes=None):
    """(name, level or None for the whole pyramid, start world pose, end points, iteration counts)"""
    cases = []
    for lvl in range(geom[2]):
        for tag, k, w, pm, pts in level_pairs(family, geom, lvl, sizes, first_only):
            cases.append((tag, lvl, w, pts, (0, 1, 2, 3)))
            if lvl == 0:
                cases.append((tag + " pyramid", None, w, pts, None))
    if family in ac.SOLVE_FAMILIES and sizes is None:
        for name, w, pts in ac.solve_cases(family, geom):
            cases.append((f"solve {name}", 0, w, pts, tuple(range(ac.SOLVE_ITERS + 1))))
            cases.append((f"solve {name} pyramid", None, w, pts, None))
    return cases


def check_single(g, oracle_mod, kind, family, geom, case, expect_kernel=None):
    """-> how many of the case's results the reference does not define"""
    name, lvl, w, pts, its = case
    undefined = 0
    runs = [(None, lambda: g.matchData(w, pts), lambda o: o.match(w, pts))] if lvl is None else [
        (it, (lambda it=it: g.match_level(lvl, w, pts, it)), (lambda o, it=it: o.match_level(lvl, w, pts, it))) for it in its]
    for it, run, op in runs:
        pg, cg = run()  # raises unless the call returns success
        cfg = g.last_launch_config()
        assert cfg["parity_effective"] == "exact" and cfg["kernel"], (name, cfg)
        if expect_kernel:
            assert cfg["kernel"] == expect_kernel, (name, cfg)
        (po, co), defined = ref(oracle_mod, kind, family, geom, ("match", name, it), op)
        undefined += not defined
        assert agrees(pg, po) and agrees(cg, co), (family, ac.gid(geom), name, it, "defined" if defined else "undefined", pg, po, cg, co)
        if family in ("wall_x", "wall_y") and lvl is not None:
            assert same(pg, w), (family, name, it, "a skipped step must return the start pose", pg, w)
    return undefined


def ordinary_matches_still_exact(g, oracle_mod, kind, geom):
    """after the non-finite poses: the `mixed` planes into the SAME context, four ordinary matches bit-exact"""
    ac.upload(g, "mixed", geom)
    g.synchronize()
    for case in single_cases("mixed", geom, first_only=True, sizes=(65, 1081)):
        assert check_single(g, oracle_mod, kind, "mixed", geom, case) == 0


@pytest.mark.parametrize("wps", WPS)
@LAYOUTS
@FAMILIES
@GEOMS
def test_single_scan_matchers_for_every_team_width(capi, oracle_mod, kind, geom, family, layout, wps):
    """match_level at 0 .. 3 iterations on each level and matchData on every (pose, scan) pair (the library's own width: both
    pose sets; the forced widths: one), the solve cases of `mixed` and `saturated` step by step"""
    g = new_ctx(capi, family, geom, layout, waves_per_scan=wps)
    undefined = total = 0
    for case in single_cases(family, geom, first_only=wps != 0):
        undefined += check_single(g, oracle_mod, kind, family, geom, case)
        total += 1 if case[1] is None else len(case[4])
    if family == "tiny":
        assert undefined >= total // 2, (undefined, total)
        ordinary_matches_still_exact(g, oracle_mod, kind, geom)
    elif family in ("wall_x", "wall_y", "deep_free"):
        assert undefined == 0
    g.close()


@LAYOUTS
@FAMILIES
@GEOMS
def test_dense_and_speculative_single_scan_forms(capi, oracle_mod, kind, geom, family, layout, monkeypatch):
    """gn_match_exact_dense_kernel at its own threshold (scans tiled to 4096 beams) and lowered to 1920, gn_match_spec_kernel
    on the same scans, gn_match_spec1_kernel on 560 .. 1920 beams; the stitching pass of the speculative form had to re-run or
    shift segments on the deep_free and saturated scans"""
    dense_auto = new_ctx(capi, family, geom, layout)
    monkeypatch.setenv("HSM_EXACT_DENSE_MIN", "1920")
    lit = new_ctx(capi, family, geom, layout)
    monkeypatch.setenv("HSM_EXACT_SPEC", "1")
    spec = new_ctx(capi, family, geom, layout)
    monkeypatch.delenv("HSM_EXACT_SPEC")
    monkeypatch.delenv("HSM_EXACT_DENSE_MIN")
    monkeypatch.setenv("HSM_EXACT_SPEC1", "1")
    spec1 = new_ctx(capi, family, geom, layout)
    spec.debug_spec_stats(True)
    for case in single_cases(family, geom, sizes=(1920,)):
        check_single(lit, oracle_mod, kind, family, geom, case, "gn_match_exact_dense_kernel")
        check_single(spec, oracle_mod, kind, family, geom, case, "gn_match_spec_kernel")
    for name, lvl, w, pts, its in single_cases(family, geom, first_only=True, sizes=(300,)):
        big = (name + " tiled", lvl, w, ac.tile(pts, 4096), its)
        check_single(dense_auto, oracle_mod, kind, family, geom, big, "gn_match_exact_dense_kernel")
        check_single(spec, oracle_mod, kind, family, geom, big, "gn_match_spec_kernel")
    walked, exact, shifted, rerun = spec.debug_spec_stats(False)
    print(f"{family} {ac.gid(geom)} {layout}: stitching pass boundaries {walked}, candidate == carry {exact}, shifted {shifted}, re-run {rerun}")
    assert walked > 0
    if family in ("deep_free", "saturated"):
        assert rerun > 0 or exact < walked, (walked, exact, shifted, rerun)
    for case in single_cases(family, geom, first_only=True, sizes=(560, 720, 1081, 1300, 1920)):
        check_single(spec1, oracle_mod, kind, family, geom, case, "gn_match_spec1_kernel")
    if family == "tiny":
        for ctx in (lit, spec, spec1):
            ordinary_matches_still_exact(ctx, oracle_mod, kind, geom)
    for ctx in (dense_auto, lit, spec, spec1):
        ctx.close()


@pytest.mark.parametrize("form", BATCH_PARAMS)
@FAMILIES
@GEOMS
def test_batches_in_every_exact_form(capi, oracle_mod, kind, geom, family, form, monkeypatch):
    """ragged CSR batches of every (pose, scan) pair up to the form's length (and of the solve cases) through the texel-cache
    exact form (chain wavefront and rotating owner; 5, 9, 13 and 17 cached rows; a streamed tail), the one-wavefront-per-scan
    form, the plane layout and the form a small batch picks by itself; then one level at a time through the schedule hook, one
    and four GN steps"""
    rows_form, _, chain = form.partition("/")
    cached = rows_form in BATCH_FORMS
    cap, rows = BATCH_FORMS.get(rows_form, (1081, 17))
    rotating = chain == "rotating-owner"
    monkeypatch.setenv("HSM_EXACT_CHAIN_WAVE", "0" if rotating else "1")
    monkeypatch.setenv("HSM_EXACT_CACHED", "0" if form == "one-wave-per-scan" else "1")
    g = new_ctx(capi, family, geom, "plane" if form == "plane-layout" else "quad", **({} if form == "auto" else {"waves_per_scan": 1}))

    def check_cfg():
        cfg = g.last_launch_config()
        assert cfg["parity_effective"] == "exact", cfg
        if cached:
            assert cfg["texel_cache"] and cfg["block"] == (256 if rotating else 320) and cfg["beams_per_lane"] == rows, cfg
            assert ("chain wavefront" in cfg["kernel"]) == (not rotating) and cfg["kernel"].startswith("gn_match_exact_cached_kernel"), cfg
        elif form != "auto":
            assert not cfg["texel_cache"], cfg

    sizes = tuple(n for n in ac.SCAN_SIZES if n <= cap)
    scans = [(tag, w, pts) for tag, _, w, _, pts in level_pairs(family, geom, 0, sizes)]
    if family in ac.SOLVE_FAMILIES:
        scans += [(f"solve {name}", w, pts) for name, w, pts in ac.solve_cases(family, geom)]
    assert max(p.shape[0] for _, _, p in scans) == cap
    init = np.stack([w for _, w, _ in scans])
    pts, offs = pack([p for _, _, p in scans])
    pb, cb = g.match_batch(init, pts, offs)
    check_cfg()
    for j, (tag, w, p) in enumerate(scans):
        (po, co), defined = ref(oracle_mod, kind, family, geom, ("match", tag + " pyramid", None), lambda o: o.match(w, p))
        assert agrees(pb[j], po) and agrees(cb[j], co), (family, form, tag, "defined" if defined else "undefined", pb[j], po)
    for lvl in range(geom[2]):
        lv = [(tag, w, p) for tag, _, w, _, p in level_pairs(family, geom, lvl, sizes)]
        if lvl == 0 and family in ac.SOLVE_FAMILIES:
            lv += [(f"solve {name}", w, p) for name, w, p in ac.solve_cases(family, geom)]
        init = np.stack([w for _, w, _ in lv])
        pts, offs = pack([p * F(2.0 ** lvl) for _, _, p in lv])
        for gn_steps in (1, 4):
            g.debug_set_schedule(lvl, gn_steps)
            pb, cb = g.match_batch(init, pts, offs)
            check_cfg()
            for j, (tag, w, p) in enumerate(lv):
                (po, co), defined = ref(oracle_mod, kind, family, geom, ("match", tag, gn_steps - 1), lambda o: o.match_level(lvl, w, p, gn_steps - 1))
                assert agrees(pb[j], po) and agrees(cb[j], co), (family, form, tag, "steps", gn_steps, "defined" if defined else "undefined", pb[j], po)
                if family in ("wall_x", "wall_y"):
                    assert same(pb[j], w), (family, form, tag)
    g.debug_set_schedule(-1)
    if family == "tiny":
        ordinary_matches_still_exact(g, oracle_mod, kind, geom)
    g.close()


# ---- the opt-in tree-summation forms: one GN step against float64 ---------------------------------------------------------------
def check_one_step(g, o, family, lvl, w, pts, pose, cov, d, what, relaxed_prob=None):
    """H of one step within the bound (with its subnormal floor) of the form's addition depth.  Where the reference's test skips
    the step -- a diagonal entry whose every term is +-0 sums to 0 in any order -- the fast form must skip it too: the exactly
    zero entry, the start pose returned.  Elsewhere the step itself within its bound, where H is far enough from singular for
    that bound to be finite (scans of 63 beams and more)"""
    pm = o.map_coords_pose(lvl, w)
    ev = gn_f64.Eval64(o, lvl, pm, pts, "ho", relaxed_prob)  # relaxed_prob: the factors of the contracted per-beam arithmetic
    H = cov.reshape(3, 3).T
    gn_f64.check_H(H, ev, d, what)
    if ev.absH[0, 0] == 0 or ev.absH[1, 1] == 0:
        assert (H[0, 0] == 0 and ev.absH[0, 0] == 0) or (H[1, 1] == 0 and ev.absH[1, 1] == 0), (what, H)
        assert same(pose, w), (what, "the step must be skipped", pose, w)
        return "skipped"
    if family == "deep_free":  # H underflows to +0 in fp32 in every summation order: the products themselves are +0
        assert not H.any() and same(pose, w), (what, H, pose, w)
        return "skipped"
    if pts.shape[0] >= 63:
        gn_f64.check_step(H, pm, g.getMapCoordsPose(lvl, pose), ev, d, what)
        return "stepped"
    return "H only"


@LAYOUTS
@DEFINED
@GEOMS
def test_fast_forms_one_step_against_float64(capi, oracle_mod, geom, family, layout, monkeypatch):
    """HSM_PARITY_FAST: gn_match_cached_kernel (batches, one wavefront per scan), the team form (single scans, 1 .. 4 wavefronts)
    and gn_match_coop_kernel (HSM_COOP_MIN lowered, and a scan tiled to 4096 beams); HSM_PARITY_RELAXED: the cached kernel's
    contracted instantiation (quad layout), against the factors of gn_f64.relaxed_factors"""
    o = ac.checker(oracle_mod, "ho", family, geom)
    u0 = o.undefined_reads()
    seen = set()
    upto = tuple(n for n in ac.SCAN_SIZES if n <= 1081)  # the lengths these two forms are the library's choice for
    fast = new_ctx(capi, family, geom, layout, waves_per_scan=1, parity=capi.PARITY_FAST)
    for lvl in range(geom[2]):
        lv = level_pairs(family, geom, lvl, upto, first_only=True)
        init = np.stack([w for _, _, w, _, _ in lv])
        pts, offs = pack([p * F(2.0 ** lvl) for _, _, _, _, p in lv])
        fast.debug_set_schedule(lvl, 1)
        pb, cb = fast.match_batch(init, pts, offs)
        cfg = fast.last_launch_config()
        if layout == "quad":
            assert cfg["kernel"] == "gn_match_cached_kernel" and cfg["texel_cache"] and cfg["parity_effective"] == "fast", cfg
        else:
            assert cfg["parity_effective"] == "fast" and cfg["waves_per_scan"] == 1, cfg
        for j, (tag, _, w, _, p) in enumerate(lv):
            seen.add(check_one_step(fast, o, family, lvl, w, p, pb[j], cb[j], gn_f64.depth_team(p.shape[0], 1), f"cached {tag}"))
        fast.debug_set_schedule(-1)
    fast.close()
    if layout == "quad":
        rel = new_ctx(capi, family, geom, layout, waves_per_scan=1, parity=capi.PARITY_RELAXED)
        for lvl in range(geom[2]):
            prob = ac.prob_plane(oracle_mod, family, geom, lvl)
            lv = level_pairs(family, geom, lvl, upto, first_only=True)
            init = np.stack([w for _, _, w, _, _ in lv])
            pts, offs = pack([p * F(2.0 ** lvl) for _, _, _, _, p in lv])
            rel.debug_set_schedule(lvl, 1)
            pb, cb = rel.match_batch(init, pts, offs)
            cfg = rel.last_launch_config()
            assert cfg["kernel"] == "gn_match_cached_kernel" and cfg["texel_cache"] and cfg["parity_effective"] == "relaxed", cfg
            for j, (tag, _, w, _, p) in enumerate(lv):
                seen.add(check_one_step(rel, o, family, lvl, w, p, pb[j], cb[j], gn_f64.depth_team(p.shape[0], 1), f"relaxed {tag}", prob))
            rel.debug_set_schedule(-1)
        rel.close()
    for W in (1, 2, 4):
        g = new_ctx(capi, family, geom, layout, waves_per_scan=W, parity=capi.PARITY_FAST)
        for lvl in range(geom[2]):
            for tag, _, w, _, p in level_pairs(family, geom, lvl, upto, first_only=True):
                pose, cov = g.match_level(lvl, w, p, 0)
                cfg = g.last_launch_config()
                assert cfg["kernel"] == "gn_match_kernel" and cfg["waves_per_scan"] == W and cfg["parity_effective"] == "fast", cfg
                seen.add(check_one_step(g, o, family, lvl, w, p, pose, cov, gn_f64.depth_team(p.shape[0], W), f"team W={W} {tag}"))
        g.close()
    monkeypatch.setenv("HSM_COOP_MIN", "1024")
    g = new_ctx(capi, family, geom, layout, parity=capi.PARITY_FAST)
    for lvl in range(geom[2]):
        lv = level_pairs(family, geom, lvl, sizes=(1081, 1920))
        lv += [(tag + " tiled", k, w, pm, ac.tile(p, 4096)) for tag, k, w, pm, p in level_pairs(family, geom, lvl, sizes=(300,), first_only=True)]
        for tag, _, w, _, p in lv:
            pose, cov = g.match_level(lvl, w, p, 0)
            K = gn_f64.coop_workgroups(p.shape[0])
            cfg = g.last_launch_config()
            assert cfg["kernel"] == "gn_match_coop_kernel" and cfg["grid"] == K and cfg["block"] == 256, cfg
            seen.add(check_one_step(g, o, family, lvl, w, p, pose, cov, gn_f64.depth_coop(p.shape[0], K), f"coop {tag}"))
    assert g.debug_coop_fallbacks() == 0
    g.close()
    assert o.undefined_reads() == u0
    assert seen == ({"skipped"} if family in ("wall_x", "wall_y", "deep_free") else {"stepped", "H only"}), seen
