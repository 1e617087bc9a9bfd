"""The host-array probes on their staging plans (hector_slam_amd/csrc/stage_layout.h: score_states_stage, pose_covariance_stage,
ray_distances_stage; probes.hip): every region of the block starts on a 256-byte boundary now, so this file holds each entry's
results to the oracle at the sizes where a misplaced region would show -- one element, odd sizes well inside one 256-byte line, and
sizes at which every region crosses a line -- in both texel layouts and both summation orders.  Each entry is called with a larger
and then a smaller size in turn, all entries through the one block, so a region read or written at a stale offset of the call
before would show as well.

Map: 64 x 64 cells, 2 levels, two updateByScan calls of a 90-beam synthetic scan; expected values from the oracle's restatement,
computed once for all four contexts.

Exact order: everything bit for bit.  Tree order (HSM_PARITY_FAST): the per-beam terms 1 - M are the same bits in both orders, only
the order of the n additions differs.  Any order of adding n fp32 terms is within (n - 1) * 2^-24 * sum|terms| of the true sum, the
terms are >= 0, so two orders differ by at most 2 * (n - 1) * 2^-24 * residual (RES_TOL); the likelihood 1 - residual / n adds the
division's and the subtraction's rounding in each order, 4 * 2^-24 (LH_TOL).  The covariance statistics on top of the seven
likelihoods have no order of their own: they are held, bit for bit, to the scalar fp32 restatement of tests/test_node_rows.py fed
with the device's own likelihoods, and the world-frame matrices to the map-frame ones scaled.  Ray distances have no sampler form:
bit for bit in every context.
"""
import ctypes as C

import numpy as np
import pytest

from support import layout_of, same
from test_node_rows import sigma_statistics_f32

pytestmark = pytest.mark.gpu

RES, SIZE, LEVELS = 0.05, 64, 2
SIZES = [(65, 129), (3, 7), (1, 1)]  # (batch, n), a larger size in front of a smaller one
RAY_SIZES = [65, 1]
SENTINEL = np.float32(-12345.5)
U = 2.0 ** -24


def RES_TOL(n, residual):
    return 2.0 * (n - 1) * U * np.abs(residual.astype(np.float64))


def LH_TOL(n, residual):
    return RES_TOL(n, residual) / n + 4.0 * U


def scan_and_poses():
    a = np.linspace(-np.pi, np.pi, 90, endpoint=False)
    r = 1.0 + 0.2 * np.sin(3.0 * a)  # a wavy room wall about 1 m away, well inside the 3.2 m map
    scan = (np.stack([np.cos(a), np.sin(a)], 1) * r[:, None] / RES).astype(np.float32)  # level-0 cells
    return scan, np.float32([[0.0, 0.0, 0.0], [0.1, -0.05, 0.1]])


@pytest.fixture(scope="module")
def want(oracle_mod):
    """the oracle's map, the inputs of every call and what each must return"""
    scan, poses = scan_and_poses()
    o = oracle_mod.Oracle("ho", RES, SIZE, SIZE, LEVELS)
    for p in poses:
        o.update_by_scan(p, scan)
    rng = np.random.default_rng(16)
    w = {"scan": scan, "poses": poses, "levels": [o.download_level(lvl) for lvl in range(LEVELS)], "states": {}, "rays": {}}
    for lvl in range(LEVELS):
        f = np.float32(1.0 / 2 ** lvl)
        centre = np.float32([SIZE / 2 ** (lvl + 1), SIZE / 2 ** (lvl + 1), 0.0])
        for batch, n in SIZES:
            states = (centre + rng.normal(0, [1.5 * f, 1.5 * f, 0.3], (batch, 3))).astype(np.float32)
            pts = np.resize(scan, (n, 2)).copy()
            w["states"][lvl, batch, n] = (states, pts, o.likelihood_states(lvl, states, pts * f), o.residual_states(lvl, states, pts * f),
                                          o.covariance_for_poses(lvl, states, pts * f))
        grid = o.occupancy_grid(lvl)
        for n in RAY_SIZES:
            begin = rng.uniform(-0.3, 0.3, (n, 2)).astype(np.float32)
            ang = rng.uniform(0, 2 * np.pi, n)
            length = rng.uniform(0.2, 1.5, n)  # some stop short of the wall (no hit), some reach it
            end = (begin + np.stack([np.cos(ang), np.sin(ang)], 1) * length[:, None]).astype(np.float32)
            w["rays"][lvl, n] = (begin, end, grid)
    return w


@pytest.mark.parametrize("parity", ["fast", "exact"])
@pytest.mark.parametrize("layout", ["quad", "plane"])
def test_probes_return_the_oracles_values_from_their_aligned_regions(oracle_mod, want, layout, parity):
    import torch
    assert torch.cuda.is_available(), "gpu-marked tests need a HIP device"
    from hector_slam_amd import capi
    exact = parity == "exact"
    g = capi.MapRepMultiMap(RES, SIZE, SIZE, LEVELS, layout=layout_of(capi, layout),
                            parity=capi.PARITY_EXACT if exact else capi.PARITY_FAST)
    for p in want["poses"]:
        g.updateByScan(want["scan"], p)
    for lvl in range(LEVELS):
        lo, ui = g.download_level(lvl)
        assert same(lo, want["levels"][lvl][0]) and np.array_equal(ui, want["levels"][lvl][1]), ("the maps differ", lvl)
    # hsm_ray_distances with its optional in/out array absent: the binding's array type takes no null
    raw = C.CDLL(capi.load_library()._name).hsm_ray_distances
    raw.restype, raw.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int] + [C.c_void_p] * 4
    seen_hit = seen_miss = False
    for lvl in range(LEVELS):
        cell = np.float32(g.level_info(lvl)[2])
        ox, oy, res = g.map_metadata(lvl)
        for (batch, n), n_rays in zip(SIZES, RAY_SIZES + [None]):
            states, pts, lh_o, res_o, (cm_o, cw_o, l7_o) = want["states"][lvl, batch, n]
            lh, rs = g.likelihood_states(lvl, states, pts), g.residual_states(lvl, states, pts)
            cm, cw, l7 = g.covariance_for_poses(lvl, states, pts)
            what = (layout, parity, lvl, batch, n)
            print(what, "max |dlh|", np.abs(lh - lh_o).max(), "max |dres|", np.abs(rs - res_o).max(), "max |dlh7|", np.abs(l7 - l7_o).max())
            if exact:
                assert same(lh, lh_o) and same(rs, res_o), what
                assert same(l7, l7_o) and same(cm, cm_o) and same(cw, cw_o), what
            else:
                assert (np.abs(rs.astype(np.float64) - res_o) <= RES_TOL(n, res_o)).all(), what
                assert (np.abs(lh.astype(np.float64) - lh_o) <= LH_TOL(n, res_o)).all(), what
                # the sigma points' residuals are not returned: n * (1 - likelihood) stands in for them, rounded up by the same 4 u
                assert (np.abs(l7.astype(np.float64) - l7_o) <= LH_TOL(n, n * (1.0 - l7_o) + 4.0 * n * U)).all(), what
                for i in range(batch):
                    assert same(cm[i], sigma_statistics_f32(states[i], l7[i])), (what, i)
                assert same(cw[:, 0], cm[:, 0] * (cell * cell)) and same(cw[:, 4], cm[:, 4] * (cell * cell)), what
                assert same(cw[:, 1], cm[:, 1] * (cell * cell)) and same(cw[:, 3], cw[:, 1]), what
                assert same(cw[:, 2], cm[:, 2] * cell) and same(cw[:, 6], cw[:, 2]), what
                assert same(cw[:, 5], cm[:, 5] * cell) and same(cw[:, 7], cw[:, 5]) and same(cw[:, 8], cm[:, 8]), what
            assert same(l7[:, 6], lh), what  # the seventh sigma point is the pose itself
            if n_rays is None:
                continue
            begin, end, grid = want["rays"][lvl, n_rays]
            rd, rh = oracle_mod.ray_distances("ho", grid, (ox, oy), res, begin, end)
            has = rd >= 0
            seen_hit, seen_miss = seen_hit or has.any(), seen_miss or (~has).any()
            for with_hit in (True, False):
                dist = np.full(n_rays, SENTINEL, np.float32)
                hit = np.full((n_rays, 2), SENTINEL, np.float32)
                rc = raw(g._h, lvl, ox, oy, res, n_rays, begin.ctypes.data, end.ctypes.data, dist.ctypes.data,
                         hit.ctypes.data if with_hit else None)
                assert rc == 0, (what, n_rays, with_hit, capi.load_library().hsm_last_error())
                assert same(dist, rd), (what, n_rays, with_hit)
                if with_hit:
                    assert same(hit[has], rh[has]) and same(hit[~has], np.full_like(hit[~has], SENTINEL)), (what, n_rays)
                else:
                    assert same(hit, np.full_like(hit, SENTINEL)), (what, n_rays)
    assert seen_hit and seen_miss, "the rays must include one that hits and one that does not"
    g.close()
