"""The float64 reference of one Gauss-Newton evaluation (tests/gn_f64.py) checked on the CPU, and the self-check that
makes its bound a bar: on every scan the GPU cases of test_gpu_parity.py use, dropping any one non-zero beam moves at
least one of the twelve sums beyond twice the bound the GPU test applies (margin > 1)."""
import numpy as np
import pytest

import gn_cases
import gn_f64
from conftest import make_oracle


def test_gamma_and_depths():
    assert gn_f64.gamma(0) == 0.0 and gn_f64.gamma(1) > gn_f64.U
    # team forms: per-lane beams + six butterfly levels + the sequential chain of the W wave partials
    assert gn_f64.depth_team(1081, 1) == 17 + 6 and gn_f64.depth_team(64, 1) == 1 + 6 and gn_f64.depth_team(1, 16) == 1 + 6 + 15
    assert gn_f64.depth_team(17 * 1024 + 65, 16) == 18 + 6 + 15
    assert gn_f64.coop_workgroups(4096) == 16 and gn_f64.coop_workgroups(16384) == 64 and gn_f64.coop_workgroups(20000) == 64
    assert gn_f64.depth_coop(20000, 64) == 2 + 15 and gn_f64.depth_eval(5000) == 5 + 21


def test_oracle_sequential_sums_lie_within_the_bound(oracle_mod, pyramid_scene):
    """the reference's own fp32 chains (d = n) against the float64 sums of the same per-beam factors"""
    sc = pyramid_scene
    o = make_oracle(oracle_mod, "ho", sc)
    worst = 0.0
    for q in range(len(sc.query_scans)):
        for lvl in range(sc.levels):
            pts = sc.query_scans[q] * np.float32(1.0 / 2 ** lvl)
            pm = o.map_coords_pose(lvl, sc.query_init[q])
            Ho, do = o.hessian_derivs(lvl, pm, pts)
            ev = gn_f64.Eval64(o, lvl, pm, pts, "ho")
            worst = max(worst, gn_f64.check_H(Ho, ev, pts.shape[0], f"q{q} L{lvl}"))
            gn_f64.check_dtr(do, ev, pts.shape[0], f"q{q} L{lvl}")
            # the float64 sums see what the fp32 chain sees: the oracle is within a few ulps of |H| of them
            assert np.abs(Ho - ev.H).max() <= 1e-5 * np.abs(ev.H).max()
    print(f"oracle chains: worst |H - H64| = {worst:.3f} of the d = n bound")


def test_sequential_bound_sees_a_lost_beam_on_the_random_map():
    """the helper's margin means what it says: on a random-map scan, the fp32 sum without beam i lies outside the bound
    of the sum with it, for every beam the margin calls significant"""
    w, p0, pts, ev = gn_cases.single_inputs(1, 127)
    pm = w.o.map_coords_pose(0, p0)
    d = gn_f64.depth_team(pts.shape[0], 1)
    m = ev.beam_margin(d)
    for i in np.nonzero(ev.nonzero())[0][:40]:
        assert m[i] > 1.0
        Hd, dd = w.o.hessian_derivs(0, pm, np.delete(pts, i, 0))
        bh, bd = ev.bound(d)
        assert (np.abs(Hd - ev.H) > bh).any() or (np.abs(dd - ev.dTr) > bd).any(), i


@pytest.mark.parametrize("case", gn_cases.BATCH_CASES, ids=[c["id"] for c in gn_cases.BATCH_CASES])
def test_batch_case_scans_see_every_beam(case):
    _, init, scans, evs = gn_cases.batch_inputs(case)
    assert [s.shape[0] for s in scans] == case["sizes"]
    worst = np.inf
    for j, (pts, ev_list) in enumerate(zip(scans, evs)):
        for ev in ev_list:
            mm = gn_f64.min_margin(ev, gn_cases.batch_depth(case, pts.shape[0]))
            assert mm > 1.0, (case["id"], j, mm)
            worst = min(worst, mm)
    kinds = np.concatenate([e.nonzero() for el in evs for e in el])
    print(f"{case['id']}: smallest single-beam margin {worst:.2f}x the bound, {int((~kinds).sum())} all-zero beams")


@pytest.mark.parametrize("W,n", gn_cases.SINGLE_CASES)
def test_single_scan_cases_see_every_beam(W, n):
    _, _, pts, ev = gn_cases.single_inputs(W, n)
    mm = gn_f64.min_margin(ev, gn_f64.depth_team(n, W))
    assert pts.shape[0] == n and mm > 1.0, mm
    print(f"team W={W} n={n}: margin {mm:.2f}")


@pytest.mark.parametrize("n", gn_cases.COOP_SIZES)
def test_coop_cases_see_every_beam(n):
    _, _, pts, ev = gn_cases.coop_inputs(n)
    mm = gn_f64.min_margin(ev, gn_f64.depth_coop(n, gn_f64.coop_workgroups(n)))
    assert pts.shape[0] == n and mm > 1.0, mm
    print(f"coop n={n}: margin {mm:.2f}")


def test_trace_and_eval_cases_see_every_beam():
    _, _, pts, ev = gn_cases.trace_inputs()
    assert gn_f64.min_margin(ev, gn_f64.depth_team(pts.shape[0], 16)) > 1.0
    for n, lvl in gn_cases.EVAL_CASES:
        _, _, pts, ev = gn_cases.eval_inputs(n, lvl)
        mm = gn_f64.min_margin(ev, gn_f64.depth_eval(n))
        assert mm > 1.0, (n, lvl, mm)


@pytest.mark.parametrize("world,W,n", gn_cases.RECT_SINGLE_CASES)
def test_rect_single_scan_cases_see_every_beam(world, W, n):
    w, _, pts, ev = gn_cases.single_inputs(W, n, world_name=world)
    assert w.size != w.size_y
    mm = gn_f64.min_margin(ev, gn_f64.depth_team(n, W))
    assert pts.shape[0] == n and mm > 1.0, mm
    print(f"team W={W} n={n} on {world}: margin {mm:.2f}")


@pytest.mark.parametrize("world,n", gn_cases.RECT_COOP_CASES)
def test_rect_coop_cases_see_every_beam(world, n):
    _, _, pts, ev = gn_cases.coop_inputs(n, world_name=world)
    mm = gn_f64.min_margin(ev, gn_f64.depth_coop(n, gn_f64.coop_workgroups(n)))
    assert pts.shape[0] == n and mm > 1.0, mm


@pytest.mark.parametrize("world,n,lvl", gn_cases.RECT_EVAL_CASES)
def test_rect_eval_cases_see_every_beam(world, n, lvl):
    _, _, pts, ev = gn_cases.eval_inputs(n, lvl, world_name=world)
    mm = gn_f64.min_margin(ev, gn_f64.depth_eval(n))
    assert pts.shape[0] == n and mm > 1.0, mm


def test_rect_worlds_are_rectangular_and_square_worlds_unchanged():
    """the rectangular worlds hold sx != sy on every level (the oracle's own geometry); a square World draws the random
    numbers it drew before size_y existed"""
    for name, (sx, sy) in (("wide", (640, 192)), ("tall", (192, 640)), ("bigwide", (8192, 1040))):
        w = gn_cases.world(name)
        for lvl in range(w.levels):
            assert w.o.level_info(lvl)[:2] == (sx >> lvl, sy >> lvl) and w.lv[lvl][0].shape == (sy >> lvl, sx >> lvl)
    w = gn_cases.World("ho", 64, 2, seed=5)
    rng = np.random.default_rng(5)
    for lvl in range(2):
        assert np.array_equal(w.lv[lvl][0], rng.uniform(-2.5, 2.5, (64 >> lvl, 64 >> lvl)).astype(np.float32))

@pytest.mark.parametrize("case", [c for c in gn_cases.BATCH_CASES if c["id"] in ("cached4x17-quad-L0", "cached4x9-plane-L2", "plain1x4x0-L0")],
                         ids=lambda c: c["id"])
def test_step_check_accepts_the_oracles_own_step(case):
    """check_step on the reference's own one-step match (match_level with max_iter = 0, sequential chains, d = n): the
    replayed fp32 solve and its allowances hold for the reference itself"""
    w, init, scans, evs = gn_cases.batch_inputs(case)
    lvl = case["level"]
    checked = 0
    for j, pts in enumerate(scans):
        n = pts.shape[0]
        if n < 3:
            continue
        po, co = w.o.match_level(lvl, init[j], pts, 0)
        H = co.reshape(3, 3).T
        gn_f64.check_H(H, evs[j][0], n, case["id"])
        checked += gn_f64.check_step(H, w.o.map_coords_pose(lvl, init[j]), w.o.map_coords_pose(lvl, po), evs[j][0], n, f"{case['id']} {j}")
    assert checked >= len(scans) // 2


def test_relaxed_model_is_the_reference_where_the_contraction_cannot_matter():
    """the relaxed model against the reference at theta = 0, where the rotation is exact in both forms and the endpoints
    agree: the same beams are non-zero, the factors differ by a few ulps at most, M stays in [0, 1]"""
    w = gn_cases.world("pyr")
    rng = np.random.default_rng(5)
    p0 = w.start_pose(0, rng, theta=0.0)
    pts = (rng.uniform(-100, 100, (2000, 2))).astype(np.float32)
    pm = w.o.map_coords_pose(0, p0)
    ref = gn_f64.Eval64(w.o, 0, pm, pts, "ho")
    rel = gn_f64.Eval64(w.o, 0, pm, pts, "ho", w.prob(0))
    assert np.array_equal(ref.nonzero(), rel.nonzero())
    assert np.abs(rel.fac[:, :3] - ref.fac[:, :3]).max() <= 8 * gn_f64.U
    assert (rel.fac[:, 0] >= 0).all() and (rel.fac[:, 0] <= 1).all()
