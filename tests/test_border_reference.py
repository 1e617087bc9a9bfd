"""CPU pin of the map-edge cases (tests/border_cases.py), no device: the conditions the cases promise hold, the restatement
equals the reference headers bit for bit on every one of them, and both equal a plain numpy fp32 restatement of
interpMapValueWithDerivatives written here -- so a slip in a checker cannot hide the same slip in a kernel
(tests/test_gpu_border_sampling.py compares the kernels with these checkers)."""
import numpy as np
import pytest

import border_cases as bc
from conftest import bits, oracle_kinds
from support import same

GEOMS = pytest.mark.parametrize("geom", bc.GEOMETRIES, ids=bc.gid)


def interp_numpy(oracle_mod, geom, lvl, coords):
    """OccGridMapUtil.h:287-347 in numpy fp32: the bounds test of MapDimensionProperties.h:65-68 (x < 0 or x > dims - 2: zeros),
    truncation by a cast to int, factors = coords - (float)index, four reads at index, + 1, + sizeX, + sizeX + 1 of the
    probability plane (getGridProbability of the log-odds: host expf), and the three expressions of :332-346"""
    f = np.float32
    lo = bc.map_planes(geom)[lvl][0]
    sy, sx = lo.shape
    prob = oracle_mod.libm_expf(lo.reshape(-1))[1]
    c = np.asarray(coords, f)
    out = np.zeros((c.shape[0], 3), f)
    for k in range(c.shape[0]):
        x, y = c[k]
        if x < f(0) or x > f(sx - 2) or y < f(0) or y > f(sy - 2):
            continue
        ix, iy = int(x), int(y)
        fx, fy = f(x - f(ix)), f(y - f(iy))
        index = iy * sx + ix
        i0, i1, i2, i3 = prob[index], prob[index + 1], prob[index + sx], prob[index + sx + 1]
        dx1, dx2, dy1, dy2 = f(i0 - i1), f(i2 - i3), f(i0 - i2), f(i1 - i3)
        xi, yi = f(f(1) - fx), f(f(1) - fy)
        out[k, 0] = f(f(f(f(i0 * xi) + f(i1 * fx)) * yi) + f(f(f(i2 * xi) + f(i3 * fx)) * fy))
        out[k, 1] = -f(f(dx1 * xi) + f(dx2 * fx))
        out[k, 2] = -f(f(dy1 * yi) + f(dy2 * fy))
    return out


def sample_coords(geom, lvl):
    """every coordinate set the GPU tests sample: the exact ones, what the exact lists really reach from the exact pose, band points"""
    ex = bc.exact_coords(geom, lvl)
    pm = bc.exact_map_pose(lvl)
    return np.concatenate([ex, bc.transform(pm, bc.end_points(ex, pm)), bc.band_coords(geom, lvl, 1600)])


@GEOMS
def test_the_cases_are_what_they_say(oracle_mod, geom):
    o = bc.checker(oracle_mod, "ho", geom)
    bc.check_exact_pose(o, geom)  # integer map poses on every level
    assert o.scale_to_map() == 8.0
    for lvl in range(geom[2]):
        lo = bc.map_planes(geom)[lvl][0]
        assert same(o.download_level(lvl)[0], lo)
        # border cells and corners differ from their neighbours
        assert (lo[0, :-1] != lo[0, 1:]).all() and (lo[-1, :-1] != lo[-1, 1:]).all() and (lo[:-1, 0] != lo[1:, 0]).all()
        assert (lo[0] != lo[1]).all() and (lo[-1] != lo[-2]).all() and (lo[:, 0] != lo[:, 1]).all() and (lo[:, -1] != lo[:, -2]).all()
        ex = bc.exact_coords(geom, lvl)
        assert ex.shape == (bc.N_EXACT, 2) and np.isfinite(ex).all()
        # of the 20 values of an axis nine are inside (0, -0.0, the positive subnormal, 1, lim, lim - 1 ulp, 0.5, lim - 0.5, lim / 2)
        assert bc.n_inside_exact(geom, lvl) == 81 and int(bc.inside(geom, lvl, ex).sum()) == 81
        assert int((interp_numpy(oracle_mod, geom, lvl, ex)[:, 0] != 0).sum()) == 81
        # from the exact pose every value but -0.0 and the two subnormals is reached bit for bit; those three become +0.0 (inside)
        hit = bc.reached(ex, bc.exact_map_pose(lvl))
        assert int(hit.sum()) == 17 * 17
        got = bc.transform(bc.exact_map_pose(lvl), bc.end_points(ex, bc.exact_map_pose(lvl)))
        assert int(bc.inside(geom, lvl, got).sum()) == 100
        # ... and the map-frame poses of ZERO_POSES take the coordinates themselves as end points: -0.0 + -0.0 stays -0.0
        for zp in bc.ZERO_POSES[1:3]:
            co = bc.transform(zp, ex)
            assert (bits(co[:, 0]) == 0x80000000).any() and (bits(co[:, 1]) == 0x80000000).any()
            assert (bits(co) == 1).any() and (bits(co) == 0x80000001).any()
            assert int(bc.inside(geom, lvl, co).sum()) == 81
    for n in bc.LIST_SIZES:
        assert bc.level_list(geom, 0, n).shape == (n, 2) and bc.pyramid_list(geom, n).shape == (n, 2)
    a, b = bc.pyramid_list(geom, 1081), bc.level_list(geom, 1, 400)
    assert same(a[1:800:2] * np.float32(0.5), b)  # aimed at level 1's edges, exactly


@pytest.mark.parametrize("n", bc.LIST_SIZES)
@pytest.mark.parametrize("seed", bc.CROSS_SEEDS)
@GEOMS
def test_crossing_cases_cross(oracle_mod, geom, seed, n):
    """every length the GPU tests run a crossing case at: the reference's own iteration moves at least 8 beams out of the map and
    8 into it between consecutive steps, and at least two leave it without leaving their cell"""
    o = bc.checker(oracle_mod, "ho", geom)
    w, pts = bc.crossing_case(geom, seed, n)
    assert pts.shape == (n, 2)
    n_out, n_in, n_same = bc.count_crossings(oracle_mod, o, geom, 0, w, pts)
    print(bc.gid(geom), seed, n, "in->out", n_out, "out->in", n_in, "in->out inside one cell", n_same)
    assert n_out >= bc.MIN_CROSSINGS and n_in >= bc.MIN_CROSSINGS and n_same >= 2
    assert o.undefined_reads() == 0


@pytest.mark.parametrize("kind", oracle_kinds())
@GEOMS
def test_numpy_restatement_equals_the_checkers(oracle_mod, geom, kind):
    o = bc.checker(oracle_mod, kind, geom)
    for lvl in range(geom[2]):
        c = sample_coords(geom, lvl)
        assert same(o.interp(lvl, c), interp_numpy(oracle_mod, geom, lvl, c)), (kind, lvl)


def entry_results(oracle_mod, o, geom):
    """every entry the GPU tests compare, on every case -> a list of (name, array)"""
    out = []
    for lvl in range(geom[2]):
        pm = bc.exact_map_pose(lvl)
        out.append((f"interp L{lvl}", o.interp(lvl, sample_coords(geom, lvl))))
        states = np.concatenate([pm[None], bc.ZERO_POSES, np.stack([bc.exact_map_pose(lvl, t) for t in bc.THETAS])])
        for n in (400, 1081):
            for order, pts in bc.in_orders(bc.level_list(geom, lvl, n)).items():
                H, d = o.hessian_derivs(lvl, pm, pts)
                out += [(f"H L{lvl} n{n} {order}", H), (f"dTr L{lvl} n{n} {order}", d)]
                for it in (0, 1, 3):
                    p, c = o.match_level(lvl, bc.exact_world_pose(geom), pts, it)
                    out += [(f"match_level L{lvl} n{n} {order} it{it}", p), (f"its cov L{lvl} n{n} {order} it{it}", c)]
                out.append((f"likelihood L{lvl} n{n} {order}", o.likelihood_states(lvl, states, pts)))
                out.append((f"residual L{lvl} n{n} {order}", o.residual_states(lvl, states, pts)))
                for k, a in enumerate(o.covariance_for_poses(lvl, states, pts)):
                    out.append((f"covariance_for_poses[{k}] L{lvl} n{n} {order}", a))
        ex = bc.exact_coords(geom, lvl)  # end point == coordinate from the zero poses
        for zp in bc.ZERO_POSES:
            H, d = o.hessian_derivs(lvl, zp, ex)
            out += [(f"H zero pose L{lvl}", H), (f"dTr zero pose L{lvl}", d)]
    for n in bc.LIST_SIZES:
        for order, pts in bc.in_orders(bc.pyramid_list(geom, n)).items():
            p, c = o.match(bc.exact_world_pose(geom), pts)
            out += [(f"match n{n} {order}", p), (f"match cov n{n} {order}", c)]
    for th in bc.THETAS:
        p, c = o.match(bc.exact_world_pose(geom, th), bc.pyramid_list(geom, 720, th))
        out += [(f"match theta {th}", p), (f"match cov theta {th}", c)]
    for seed in bc.CROSS_SEEDS:
        w, pts = bc.crossing_case(geom, seed, 1081)
        for it in (0, 1, bc.K_CROSS):
            out.append((f"crossing {seed} it{it}", np.concatenate(o.match_level(0, w, pts, it))))
        out.append((f"crossing {seed} match", np.concatenate(o.match(w, pts))))
    return out


@GEOMS
def test_restatement_equals_reference_on_every_case(oracle_mod, geom):
    if not oracle_mod.available("hr"):
        pytest.skip("oracle/_ref/libhector_ref.so not built (needs the reference's sources)")
    ho = bc.checker(oracle_mod, "ho", geom)
    a = entry_results(oracle_mod, ho, geom)
    assert ho.undefined_reads() == 0  # the guard: only then is the reference given the same inputs
    b = entry_results(oracle_mod, bc.checker(oracle_mod, "hr", geom), geom)
    assert len(a) == len(b) > 100
    for (name, x), (_, y) in zip(a, b):
        assert np.isfinite(x).all(), name
        assert same(x, y), (bc.gid(geom), name)
