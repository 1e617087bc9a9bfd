"""The numpy model of hsm_occupied_points* (tests/points_cases.py) against the rule written as a double loop, and the two workspace
functions as host arithmetic; no GPU.

The model is what tests/test_gpu_occupied_points.py holds the device to bit for bit, so it is itself held here to a restatement
that shares nothing with it: rank order, `every`, the max_points cap, box clamping, and cells that are NaN, +0, -0, negative,
infinite or denormal.  hsm_occupied_points_workspace and hsm_align_map_workspace are called from the built library without a
device.

At the parent commit the workspace tests fail: the entries do not exist.
"""
import numpy as np
import pytest

import points_cases as pc

F = np.float32


def _planes():
    yield "random_37x23", pc.random_plane(37, 23, 1)
    yield "random_64x5", pc.random_plane(64, 5, 2)
    yield "random_3x70", pc.random_plane(3, 70, 3)
    yield "zeros", np.zeros((9, 11), F)
    yield "all_occupied", np.full((8, 8), 2.5, F)
    special = np.zeros((2, 6), F)
    special[0] = F([np.nan, 0.0, -0.0, -1.0, 1e-45, np.inf])
    special[1] = F([-np.inf, 3.0, -1e-45, np.nan, 0.5, -0.0])
    yield "special", special


BOXES = [None, (0, 0, -1, -1), (2, 1, 2, 1), (0, 3, 100, 3), (-4, -2, 5, 6), (1, 1, 1000, 1000), (500, 0, 600, 4), (3, 2, 30, 20)]


@pytest.mark.parametrize("name,lo", list(_planes()), ids=[n for n, _ in _planes()])
def test_model_is_the_double_loop(name, lo):
    affine = pc.world_from_map((0.1, lo.shape[1], lo.shape[0], 1, (0.5, 0.5)), 0)
    seen = 0
    for box in BOXES:
        for every in (1, 2, 3, 7):
            total = pc.brute_force(lo, box, every, 10 ** 9)[1][1]
            for cap in sorted({0, 1, max(total - 1, 0), total, total + 5}):
                want_cells, want_counts = pc.brute_force(lo, box, every, cap)
                pts, counts = pc.occupied_points_model(lo, box, every, cap, affine, F(10.0))
                assert counts == want_counts, (box, every, cap)
                want = pc.cell_points(np.array(want_cells, np.int64).reshape(-1, 2), affine, F(10.0))
                assert np.array_equal(pts.view(np.uint32), want.view(np.uint32)), (box, every, cap)
                seen += counts[0]
    assert (seen > 0) == (name != "zeros")


def test_special_values_count_as_the_rule_says():
    lo = dict(_planes())["special"]
    cells = pc.kept_cells(lo, None, 1).tolist()
    assert cells == [[4, 0], [5, 0], [1, 1], [4, 1]]   # the denormal, +inf, 3.0, 0.5: NaN, +-0 and the negatives are not occupied


def test_thinning_is_by_rank_not_by_lattice():
    lo = np.zeros((12, 12), F)
    lo[:, 4] = 1.0   # a wall along y: a lattice of every second column would lose it
    cells = pc.kept_cells(lo, None, 2)
    assert len(cells) == 6 and (cells[:, 0] == 4).all() and cells[:, 1].tolist() == [0, 2, 4, 6, 8, 10]


def test_clamped_box():
    assert pc.clamp_box(None, 7, 5) == (0, 0, 6, 4)
    assert pc.clamp_box((-3, -3, 100, 100), 7, 5) == (0, 0, 6, 4)
    assert pc.clamp_box((2, 1, 2, 1), 7, 5) == (2, 1, 2, 1)
    for miss in ((7, 0, 9, 4), (0, 5, 6, 9), (-9, 0, -1, 4), (0, 0, -1, -1), (4, 2, 3, 2)):
        assert pc.clamp_box(miss, 7, 5) == pc.EMPTY, miss


def test_world_from_map_is_the_inverse_scaling():
    for geom in (pc.BIG_GEOM, (0.1, 70, 52, 3, (0.5, 0.5)), (0.1, 48, 44, 3, (0.4, 0.55))):
        for lvl in range(geom[3]):
            l00, l10, l01, l11, t0, t1 = pc.world_from_map(geom, lvl)
            cell = geom[0] * 2 ** lvl
            assert abs(l00 - cell) < 1e-6 and l00 == l11 and l10 == 0 and l01 == 0
            assert abs(t0 + geom[0] * geom[1] * geom[4][0]) < 1e-4 and abs(t1 + geom[0] * geom[2] * geom[4][1]) < 1e-4


# ---- the workspace functions: host arithmetic of the built library -------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from hector_slam_amd import build, capi
    build.build_native()
    return capi.load_library()


def test_occupied_points_workspace_is_host_arithmetic(lib):
    from hector_slam_amd import capi
    f = lib.hsm_occupied_points_workspace
    assert f(-1) == 0 and f(-2 ** 31) == 0
    sizes = [0, 1, capi.POINTS_TILE - 1, capi.POINTS_TILE, capi.POINTS_TILE + 1, 63000, 2048 * 2048, 8192 * 8192, 2 ** 28, 2 ** 31 - 1]
    got = [f(c) for c in sizes]
    assert all(b > 0 and b % 8 == 0 for b in got), got
    assert got == sorted(got) and got[-1] > got[0]
    for c, b in zip(sizes, got):   # one int per tile, one at least
        assert b >= 4 * max(-(-c // capi.POINTS_TILE), 1), (c, b)
    assert capi.MapRepMultiMap.occupied_points_workspace(63000) == f(63000)


def test_align_map_workspace_is_host_arithmetic(lib):
    from hector_slam_amd import capi
    f = lib.hsm_align_map_workspace
    ok = (63000, 1089, 8, 1100)
    base = f(*ok)
    assert base > 0 and base % 8 == 0
    for bad in ((-1, 1089, 8, 1100), (63000, 0, 8, 1100), (63000, -5, 8, 1100), (63000, 1089, 0, 1100), (63000, 1089, 65, 1100),
                (63000, 1089, 8, -1), (63000, 1089, 8, capi.MAX_ALIGN_POINTS + 1)):
        assert f(*bad) == 0, bad
    assert f(63000, 1089, 8, capi.MAX_ALIGN_POINTS) > base
    for axis, values in ((0, (0, 1, 63000, 2 ** 26, 2 ** 28)), (1, (1, 27, 1089, 35301, 10 ** 6)), (2, (1, 8, 64)),
                         (3, (0, 1, 1100, capi.MAX_ALIGN_POINTS))):
        got = []
        for v in values:
            a = list(ok)
            a[axis] = v
            got.append(f(*a))
        assert all(b > 0 and b % 8 == 0 for b in got) and got == sorted(got) and got[-1] > got[0], (axis, got)
    # it holds what the two steps need
    assert base >= lib.hsm_occupied_points_workspace(63000) + lib.hsm_relocalize_workspace(1089, 8) + 1100 * 8
    assert capi.MapRepMultiMap.align_map_workspace(*ok) == base
