"""CPU pin of the aged-map cases (tests/aged_cases.py), no device: each family is what it says, the restatement equals the
reference headers bit for bit wherever the reference has a result, a numpy fp32 restatement of the per-beam products and of
the Gauss-Newton solve written in aged_cases equals both, and the solve cases go through the clamp, the wrap and the
ill-conditioned steps they were picked for (tests/test_gpu_aged_maps.py compares the kernels with these checkers).

A case is UNDEFINED when the restatement counts a map read with a NaN coordinate while running it (Oracle.undefined_reads):
the reference headers index their grid with (int)NaN there and crash.  The restatement always runs first; the
reference-compiled checker is never given such a case."""
import numpy as np
import pytest

import aged_cases as ac
import gn_f64
from conftest import bits
from support import same

GEOMS = pytest.mark.parametrize("geom", ac.GEOMETRIES, ids=ac.gid)
F = np.float32
MAX_UNDEFINED = 0.10   # of a family's cases, `tiny` excepted


def same_or_nan(a, b):
    """bit-identical where finite, non-finite in the same places (NaN payloads and signs are pinned nowhere in the suite)"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    fa, fb = np.isfinite(a), np.isfinite(b)
    return np.array_equal(fa, fb) and np.array_equal(bits(a)[fa], bits(b)[fb])


def entry_cases(family, geom):
    """every (name, op) the GPU tests compare: op(checker) -> tuple of arrays"""
    out = []
    for lvl in range(geom[2]):
        f = F(1.0 / 2 ** lvl)
        states = np.stack([ac.map_pose(geom, lvl, k) for k in range(4)])
        for k, n, seed in ac.pairs(geom):
            pm, w = ac.map_pose(geom, lvl, k), ac.world_pose(geom, k)
            pts = ac.family_scan(family, geom, k, n, seed) * f
            tag = f"L{lvl} pose {k} n{n} seed {seed}"
            out.append((f"H {tag}", lambda o, lvl=lvl, pm=pm, pts=pts: o.hessian_derivs(lvl, pm, pts)))
            out.append((f"likelihood {tag}", lambda o, lvl=lvl, pts=pts: (o.likelihood_states(lvl, states, pts),)))
            out.append((f"residual {tag}", lambda o, lvl=lvl, pts=pts: (o.residual_states(lvl, states, pts),)))
            out.append((f"covariance {tag}", lambda o, lvl=lvl, pts=pts: o.covariance_for_poses(lvl, states, pts)))
            for it in range(4):
                out.append((f"match_level it{it} {tag}", lambda o, lvl=lvl, w=w, pts=pts, it=it: o.match_level(lvl, w, pts, it)))
            if lvl == 0:
                out.append((f"match {tag}", lambda o, w=w, pts=pts: o.match(w, pts)))
    if family in ac.SOLVE_FAMILIES:
        for name, w, pts in ac.solve_cases(family, geom):
            for it in range(ac.SOLVE_ITERS + 1):
                out.append((f"solve {name} it{it}", lambda o, w=w, pts=pts, it=it: o.match_level(0, w, pts, it)))
            out.append((f"solve {name} match", lambda o, w=w, pts=pts: o.match(w, pts)))
    return out


@pytest.mark.parametrize("family", ac.FAMILIES)
@GEOMS
def test_restatement_equals_reference_wherever_it_is_defined(oracle_mod, geom, family):
    """interp at every beam's coordinate, hessian_derivs, the three probes, match_level(it = 0 .. 3) and match; the undefined
    share of the family stays under its cap (`tiny`: at least half of the matches must be undefined)"""
    ho = ac.checker(oracle_mod, "ho", family, geom)
    hr = ac.checker(oracle_mod, "hr", family, geom) if oracle_mod.available("hr") else None
    for lvl in range(geom[2]):
        for k, n, seed in ac.pairs(geom):
            pts = ac.family_scan(family, geom, k, n, seed) * F(1.0 / 2 ** lvl)
            pm = ac.map_pose(geom, lvl, k)
            s, c = (v[0] for v in oracle_mod.libm_sincosf(pm[2:3], "ho"))
            co = ac.bc.transform(pm, pts, (s, c))
            fac, _, _ = ac.beam_terms(oracle_mod, family, geom, lvl, pm, pts)
            a = ho.interp(lvl, co)
            assert same(a, fac[:, :3]), (family, lvl, n, "numpy restatement of the sampler")
            assert hr is None or same(a, hr.interp(lvl, co)), (family, lvl, n, "interp")
    cases = entry_cases(family, geom)
    undefined = matches = undefined_matches = 0
    for name, op in cases:
        u0 = ho.undefined_reads()
        a = op(ho)
        is_match = "match" in name
        matches += is_match
        if ho.undefined_reads() > u0:
            undefined += 1
            undefined_matches += is_match
            continue
        if hr is not None:  # (a step may end on a non-finite pose that nothing reads any more: defined, payloads unpinned)
            b = op(hr)
            assert all(same_or_nan(x, y) for x, y in zip(a, b)), (family, ac.gid(geom), name)
    share = undefined / len(cases)
    print(f"{family} {ac.gid(geom)}: {len(cases)} cases, undefined in the reference {undefined} ({100 * share:.1f} %), "
          f"of the {matches} matches {undefined_matches}")
    if family == "tiny":
        assert undefined_matches >= matches / 2
    else:
        assert share <= MAX_UNDEFINED, (family, share)


@pytest.mark.parametrize("family", ["wall_x", "wall_y"])
@GEOMS
def test_walls_give_one_exactly_zero_diagonal_entry(oracle_mod, geom, family):
    """on at least 90 % of the (pose, scan) pairs of every level: the diagonal entry along the wall exactly 0, the other one
    not, so the step is skipped and match_level returns the start pose bit for bit with H as the covariance"""
    o = ac.checker(oracle_mod, "ho", family, geom)
    u0 = o.undefined_reads()
    zero, other = ((1, 1), (0, 0)) if family == "wall_x" else ((0, 0), (1, 1))
    good = total = 0
    for lvl in range(geom[2]):
        for k, n, seed in ac.pairs(geom):
            pts = ac.family_scan(family, geom, k, n, seed) * F(1.0 / 2 ** lvl)
            H, d = o.hessian_derivs(lvl, ac.map_pose(geom, lvl, k), pts)
            total += 1
            if bits(H[zero]) in (0, 0x80000000) and H[other] != 0:
                good += 1
                assert d.any() and H[2, 2] != 0, (lvl, n)
                w = ac.world_pose(geom, k)
                for it in (0, 3):
                    pose, cov = o.match_level(lvl, w, pts, it)
                    assert same(pose, w) and same(cov.reshape(3, 3).T, H), (family, lvl, n, it, pose, w)
    print(f"{family} {ac.gid(geom)}: zero-diagonal cases {good} of {total}")
    assert good >= 0.9 * total
    assert o.undefined_reads() == u0


@GEOMS
def test_deep_free_and_saturated_reach_subnormal_terms(oracle_mod, geom):
    """deep_free: all nine H entries +0 by underflow while dTr is a non-zero sum of subnormal terms, every scan with at least
    one subnormal per-beam term; saturated: a subnormal term in every scan as well (a product of the
    bilinear blend wherever a beam touches a free cell), funVal = 1 - M exactly 0 on some beams, gradients of exactly +-1"""
    for family in ("deep_free", "saturated"):
        o = ac.checker(oracle_mod, "ho", family, geom)
        u0 = o.undefined_reads()
        zero_h = sub_scans = scans = fun_zero = unit_grad = 0
        for lvl in range(geom[2]):
            for k, n, seed in ac.pairs(geom):
                pm = ac.map_pose(geom, lvl, k)
                pts = ac.family_scan(family, geom, k, n, seed) * F(1.0 / 2 ** lvl)
                fac, prods, blend = ac.beam_terms(oracle_mod, family, geom, lvl, pm, pts)
                nsub = ac.n_subnormal(fac, prods, blend)
                scans += 1
                sub_scans += nsub > 0
                H, d = o.hessian_derivs(lvl, pm, pts)
                if family == "deep_free":
                    assert nsub > 0, (lvl, n)
                    assert not bits(H).any() and d.any() and ac.n_subnormal(d) + int((np.abs(d) < 1e-35).sum()) >= 3, (lvl, n, H, d)
                    zero_h += 1
                    # the float64 bound with its subnormal floor holds for the reference's own sequential sums, and means something
                    ev = gn_f64.Eval64(o, lvl, pm, pts, "ho")
                    gn_f64.check_H(H, ev, n, f"deep_free L{lvl} n{n}")
                    gn_f64.check_dtr(d, ev, n, f"deep_free L{lvl} n{n}")
                    assert (ev.bound(n)[1] < np.abs(ev.terms[:, 9:]).max(0)).all(), "the bound exceeds the largest term"
                else:
                    assert nsub > 0, (lvl, n)
                    inside = fac[:, 0] != 0
                    fun_zero += int((fac[inside, 4] == 0).sum())
                    unit_grad += int((np.abs(fac[:, 1:3]) == 1).sum())
        print(f"{family} {ac.gid(geom)}: scans with a subnormal per-beam term {sub_scans} of {scans}; all-zero H with non-zero dTr "
              f"{zero_h}; beams with funVal == 0: {fun_zero}; gradients of exactly +-1: {unit_grad}")
        if family == "saturated":
            assert fun_zero >= 20 and unit_grad >= 20
        assert o.undefined_reads() == u0


@pytest.mark.parametrize("family", ac.SOLVE_FAMILIES)
@GEOMS
def test_solve_cases_clamp_wrap_and_leave_the_map(oracle_mod, geom, family):
    """the committed picks are what the searches return; the numpy replay of the iteration (aged_cases.gn_step) equals the
    checker's match_level bit for bit on every solve case; the counts the cases are for"""
    assert ac.search(oracle_mod, family, geom) == ac.PICKS[(family, geom[0])]
    o = ac.checker(oracle_mod, "ho", family, geom)
    tot = {"clamp+": 0, "clamp-": 0, "wrap": 0, "ill": 0}
    for name, w, pts in ac.solve_cases(family, geom):
        u0 = o.undefined_reads()
        for it in range(ac.SOLVE_ITERS + 1):
            pose, cov, _ = ac.replay(o, 0, w, pts, it)
            po, co = o.match_level(0, w, pts, it)
            assert same(pose, po) and same(cov, co) and np.isfinite(po).all(), (family, name, it)
        assert o.undefined_reads() == u0, (family, name, "a solve case must be defined")
        c = ac.classify(o, geom, 0, w, pts, ac.SOLVE_ITERS)
        for key in tot:
            tot[key] += int(c[key])
    print(f"{family} {ac.gid(geom)}: GN steps clamped at +0.2: {tot['clamp+']}, at -0.2: {tot['clamp-']}; matches whose final "
          f"angle is wrapped: {tot['wrap']}; ill-conditioned finite matches that end off the map: {tot['ill']}")
    assert tot["clamp+"] >= 4 and tot["clamp-"] >= 4 and tot["wrap"] >= 4
    assert tot["ill"] >= len(ac.PICKS[(family, geom[0])]["ill"]) == ac.N_PICK  # (a short scan may qualify as well)


def test_enough_ill_conditioned_cases_over_all():
    assert sum(len(p["ill"]) for p in ac.PICKS.values()) >= 4
    assert set(ac.START_ANGLES) == {3.1415, -3.14159, 7.0, -100.0, 119.99}
    assert set(ac.SCAN_SIZES) == {1, 2, 3, 63, 64, 65, 300} | set(ac.bc.LIST_SIZES)


def test_tile_keeps_the_pattern_of_H(oracle_mod):
    """repeating a short list (the dense and cooperative forms need 4096 beams) keeps which entries of H are zero"""
    geom = ac.GEOMETRIES[0]
    for family in ("wall_x", "deep_free", "mixed"):
        o = ac.checker(oracle_mod, "ho", family, geom)
        pts = ac.family_scan(family, geom, 0, 300, 6)
        big = ac.tile(pts, 4096)
        assert big.shape[0] >= 4096 and same(big[:300], pts) and same(big[300:600], pts)
        Ha, _ = o.hessian_derivs(0, ac.map_pose(geom, 0, 0), pts)
        Hb, _ = o.hessian_derivs(0, ac.map_pose(geom, 0, 0), big)
        assert np.array_equal(Ha == 0, Hb == 0), family
