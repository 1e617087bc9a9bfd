"""The cases of tests/cast_cases.py on the CPU: the restatement of getDist ("ho") and, where it is built, the unmodified
hector_map_tools ("hr") agree on every ray the GPU test casts, and the cases are what that test takes them for -- neither all
hits nor all misses on any level, every special family with both outcomes (or, by definition, none), the cap reached."""
import numpy as np
import pytest

import cast_cases
from conftest import bits, make_oracle, oracle_kinds


@pytest.fixture(scope="module")
def levels(oracle_mod, pyramid_scene):
    o = make_oracle(oracle_mod, "ho", pyramid_scene)
    return [(o.occupancy_grid(lvl), cast_cases.metadata(o, lvl)) for lvl in range(pyramid_scene.levels)]


def both(grid, meta, begin, end):
    d, h = cast_cases.expected_rays("ho", grid, meta, begin, end)
    for kind in oracle_kinds()[1:]:
        d2, h2 = cast_cases.expected_rays(kind, grid, meta, begin, end)
        has = d >= 0
        assert np.array_equal(bits(d), bits(d2)), kind
        assert np.array_equal(bits(h[has]), bits(h2[has])) and np.isnan(h2[~has]).all(), kind
    return d, h


def test_mixed_rays_on_every_level(levels):
    for lvl, (grid, meta) in enumerate(levels):
        d, h = both(grid, meta, *cast_cases.mixed_rays(grid, meta, 2000, 100 + lvl))
        has = d >= 0
        assert np.isnan(h[~has]).all() and np.isfinite(h[has]).all()
        if min(grid.shape) >= 16:
            assert 0.1 < has.mean() < 0.95, (lvl, has.mean())


def test_cast_cases_on_every_level(levels, pyramid_scene):
    angles = cast_cases.beam_table(1081)
    for lvl, (grid, meta) in enumerate(levels):
        res = np.float32(meta[2])
        poses, fam = cast_cases.poses(pyramid_scene, grid, meta, seed=lvl)
        for name, rmax in cast_cases.range_maxes(grid, meta).items():
            begin, end = cast_cases.cast_rays(poses, angles, rmax)
            d, _ = both(grid, meta, begin, end)
            d = d.reshape(cast_cases.B, -1)
            has = d >= 0
            assert (d[~has] == -res).all()
            if name in ("zero", "two_diagonals"):
                assert not has.any(), (lvl, name)   # begin == end: no step is walked; every end point outside the level
            if name != "8m":
                continue
            if min(grid.shape) >= 16:
                assert 0.1 < has.mean() < 0.95, (lvl, has.mean())
            for f in ("general", "wall", "edge"):
                assert has[fam[f]].any() and not has[fam[f]].all(), (lvl, f)
            assert (d[fam["wall"]][has[fam["wall"]]] == 0).all()  # step 0 is the occupied cell
            assert all(has[k].any() for k in range(fam["wall"].start, fam["wall"].stop)), lvl
            assert not has[fam["outside"]].any() and not has[fam["nonfinite"]].any(), lvl
            # the non-finite poses make non-finite rays -- which is why the rule, not the checker, answers for them
            e = end.reshape(cast_cases.B, -1, 2)[fam["nonfinite"]]
            b = begin.reshape(cast_cases.B, -1, 2)[fam["nonfinite"]]
            assert (~np.isfinite(e).all(-1) | ~np.isfinite(b).all(-1)).all()
        sub = cast_cases.range_maxes(grid, meta)["sub_cell"]
        d, _ = both(grid, meta, *cast_cases.cast_rays(poses, angles, sub))
        assert (d >= 0).any() and not (d >= 0).all(), lvl  # a third of a cell crosses into the next one for some beams only


def test_every_fan_length_is_a_prefix_of_the_table():
    full = cast_cases.beam_table(1081)
    for n in cast_cases.BEAMS:
        assert np.array_equal(bits(cast_cases.beam_table(n)), bits(full[:n]))


def test_the_cap_is_reached_on_the_long_map(oracle_mod):
    grid = cast_cases.cap_grid()
    o = oracle_mod.Oracle("ho", cast_cases.CAP_RES, cast_cases.CAP_SX, cast_cases.CAP_SY, 1)
    meta = cast_cases.metadata(o, 0)
    res = meta[2]
    far, near = cast_cases.cap_poses(meta)
    d_far, _ = both(grid, meta, *cast_cases.cast_rays(far, cast_cases.CAP_ANGLES, cast_cases.CAP_FAR_CELLS * res))
    d_near, h_near = both(grid, meta, *cast_cases.cast_rays(near, cast_cases.CAP_ANGLES, cast_cases.CAP_NEAR_CELLS * res))
    assert (d_far < 0).all()   # the wall is more than 5000 steps away: not seen, although every beam ends behind it
    assert (d_near > 0).all()  # 500 cells closer: seen
    wall_x = meta[0] + cast_cases.CAP_WALL * np.float32(res)
    assert np.allclose(h_near[:, 0], wall_x, atol=res)
    d_edge, _ = both(grid, meta, *cast_cases.cast_rays(cast_cases.cap_edge_poses(meta), cast_cases.CAP_ANGLES[:1],
                                                        cast_cases.CAP_EDGE_CELLS * res))
    assert d_edge[0] < 0 and d_edge[1] == np.float32(res) * np.float32(4999)
