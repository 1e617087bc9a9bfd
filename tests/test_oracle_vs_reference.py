"""Pin the plain-C++ restatement (oracle/hector_oracle.cpp, "ho") against the reference's own
code (oracle/_ref/libhector_ref.so, "hr" = unmodified hector_slam_lib headers compiled through
the private Eigen/tf stand-in).  Every comparison is BIT-EXACT (integer/index work and fp32)."""
import os
import numpy as np
import pytest
from hypothesis import HealthCheck, given, seed, settings

import border_cases
import deep_cases
import rect_cases
from conftest import bits, make_oracle, oracle_kinds



@pytest.fixture(scope="module", autouse=True, params=["cpu", pytest.param("gpubox", marks=pytest.mark.gpu)])
def where(request):
    """every test of this module runs twice: in the CPU suite, and (gpu-marked, no device needed) in the GPU box's
    `-m gpu` run, so that the pin of the restatement to the reference shows up in the driver's own GPU-box log"""
    return request.param


@pytest.fixture(scope="module")
def pair(oracle_mod, pyramid_scene):
    if not oracle_mod.available("hr"):
        pytest.skip("oracle/_ref/libhector_ref.so not built (needs /root/reference)")
    ho = make_oracle(oracle_mod, "ho", pyramid_scene)
    hr = make_oracle(oracle_mod, "hr", pyramid_scene)
    return ho, hr


def test_level_geometry_and_transforms(pair, pyramid_scene):
    ho, hr = pair
    rng = np.random.default_rng(5)
    for lvl in range(pyramid_scene.levels):
        assert ho.level_info(lvl) == hr.level_info(lvl)
        for _ in range(50):
            w = rng.uniform(-12, 12, 3).astype(np.float32)
            m_o, m_r = ho.map_coords_pose(lvl, w), hr.map_coords_pose(lvl, w)
            assert np.array_equal(bits(m_o), bits(m_r))
            assert np.array_equal(bits(ho.world_coords_pose(lvl, m_o)), bits(hr.world_coords_pose(lvl, m_r)))


def test_map_built_by_update_by_scan_is_identical(pair, pyramid_scene):
    ho, hr = pair
    for lvl in range(pyramid_scene.levels):
        lo_o, ui_o = ho.download_level(lvl)
        lo_r, ui_r = hr.download_level(lvl)
        assert np.array_equal(bits(lo_o), bits(lo_r))
        assert np.array_equal(ui_o, ui_r)
        assert (lo_o > 0).sum() > 100 and (lo_o < 0).sum() > 1000  # the map is not trivial


def test_interp_with_derivatives(pair, pyramid_scene):
    ho, hr = pair
    rng = np.random.default_rng(6)
    for lvl in range(pyramid_scene.levels):
        s = pyramid_scene.map_size >> lvl
        c = rng.uniform(-3, s + 3, size=(4000, 2)).astype(np.float32)
        c[:8] = [[0, 0], [s - 2, s - 2], [s - 2, 0], [0, s - 2], [s - 1.999, 5], [-0.0, 3], [5, s - 2.0001], [s - 1, s - 1]]
        # ... and the shared edge values (border_cases.axis_values: +-0, subnormals, lim +- 1 ulp, 2^23 + 0.5, +-1e30 ...), all pairs
        v = border_cases.axis_values(s - 2)
        edge = np.stack([np.repeat(v, v.size), np.tile(v, v.size)], 1)
        c[8:8 + edge.shape[0]] = edge
        assert np.array_equal(bits(ho.interp(lvl, c)), bits(hr.interp(lvl, c)))
        assert int((ho.interp(lvl, edge)[:, 0] != 0).sum()) > 0  # (this scene's border cells are unknown, 0.5: the edge values sample them)


def test_hessian_derivs_and_match_level(pair, pyramid_scene):
    ho, hr = pair
    sc = pyramid_scene
    for q in range(6):
        for lvl in range(sc.levels):
            pts = sc.query_scans[q] * np.float32(1.0 / 2 ** lvl)
            pm = ho.map_coords_pose(lvl, sc.query_init[q])
            H_o, d_o = ho.hessian_derivs(lvl, pm, pts)
            H_r, d_r = hr.hessian_derivs(lvl, pm, pts)
            assert np.array_equal(bits(H_o), bits(H_r)) and np.array_equal(bits(d_o), bits(d_r))
            for it in (0, 3, 5):
                p_o, c_o = ho.match_level(lvl, sc.query_init[q], pts, it)
                p_r, c_r = hr.match_level(lvl, sc.query_init[q], pts, it)
                assert np.array_equal(bits(p_o), bits(p_r)) and np.array_equal(bits(c_o), bits(c_r))


def test_full_match_and_empty_scan(pair, pyramid_scene):
    ho, hr = pair
    sc = pyramid_scene
    for q in range(len(sc.query_scans)):
        p_o, c_o = ho.match(sc.query_init[q], sc.query_scans[q])
        p_r, c_r = hr.match(sc.query_init[q], sc.query_scans[q])
        assert np.array_equal(bits(p_o), bits(p_r)) and np.array_equal(bits(c_o), bits(c_r))
    cov_in = np.arange(9, dtype=np.float32)
    empty = np.zeros((0, 2), np.float32)
    for o in (ho, hr):  # ScanMatcher.h:68,189: pose passes through, cov untouched
        p, c = o.match(sc.query_init[0], empty, cov=cov_in)
        assert np.array_equal(bits(p), bits(sc.query_init[0])) and np.array_equal(c, cov_in)


def test_clamp_and_far_start(pair, pyramid_scene):
    """large initial errors: exercises the +-0.2 rad clamp and partially out-of-map scans"""
    ho, hr = pair
    sc = pyramid_scene
    rng = np.random.default_rng(7)
    for q in range(8):
        init = sc.query_truth[q] + np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-0.8, 0.8)], np.float32)
        p_o, c_o = ho.match(init, sc.query_scans[q])
        p_r, c_r = hr.match(init, sc.query_scans[q])
        assert np.array_equal(bits(p_o), bits(p_r)) and np.array_equal(bits(c_o), bits(c_r))
    far = np.array([11.5, 9.0, 0.3], np.float32)  # near the map border: most beams out of bounds
    assert np.array_equal(bits(ho.match(far, sc.query_scans[0])[0]), bits(hr.match(far, sc.query_scans[0])[0]))


def test_processor_trajectory_from_empty_map(oracle_mod, pyramid_scene):
    """a12: match -> threshold -> updateByScan -> onMapUpdated, incl. first-scan and stale-coarse quirks"""
    if not oracle_mod.available("hr"):
        pytest.skip("no reference build")
    sc = pyramid_scene
    o = [make_oracle(oracle_mod, k, sc, build=False) for k in ("ho", "hr")]
    for x in o:
        x.proc_set_thresholds(0.05, 0.02)
    hints = [sc.build_poses[0].copy(), sc.build_poses[0].copy()]
    origo = np.array([0.3, -0.1], np.float32) * np.float32(sc.scale_to_map)
    for t in range(10):
        mwm = t in (4,)  # one map_without_matching step: coarse levels reuse stale containers
        for k in range(2):
            o[k].proc_update(sc.build_scans[t], hints[k], origo=origo, map_without_matching=mwm)
        (p0, c0), (p1, c1) = o[0].proc_last_pose(), o[1].proc_last_pose()
        assert np.array_equal(bits(p0), bits(p1)), t
        if t > 0:
            assert np.array_equal(bits(c0), bits(c1)), t
        step = sc.build_poses[t + 1] - sc.build_poses[t]
        hints = [p0 + step, p1 + step]
    for lvl in range(sc.levels):
        a, b = o[0].download_level(lvl), o[1].download_level(lvl)
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])


def test_reset_and_factor_setters(oracle_mod, small_scene):
    if not oracle_mod.available("hr"):
        pytest.skip("no reference build")
    sc = small_scene
    o = [make_oracle(oracle_mod, k, sc, free=0.3, occ=0.8) for k in ("ho", "hr")]
    for x in o:
        x.reset()
        x.set_update_factor_free(0.45)
        x.set_update_factor_occupied(0.7)
        x.build_map(sc.build_poses[:5], sc.build_scans[:5])
    a, b = o[0].download_level(0), o[1].download_level(0)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])


def test_util_helpers(oracle_mod):
    if not oracle_mod.available("hr"):
        pytest.skip("no reference build")
    f_o, f_r = oracle_mod._load("ho"), oracle_mod._load("hr")
    rng = np.random.default_rng(8)
    for a in np.concatenate([rng.uniform(-50, 50, 500), [0.0, np.pi, -np.pi, 3.1415927, -3.1415927, 6.2831855]]):
        x, y = f_o["normalize_angle"](float(a)), f_r["normalize_angle"](float(a))
        assert np.float32(x).view(np.uint32) == np.float32(y).view(np.uint32)
    for _ in range(300):
        p1 = rng.uniform(-2, 2, 3).astype(np.float32)
        p2 = p1 + rng.uniform(-0.5, 0.5, 3).astype(np.float32) * np.array([1, 1, 8], np.float32)
        assert f_o["pose_difference_larger_than"](p1, p2, 0.4, 0.13) == f_r["pose_difference_larger_than"](p1, p2, 0.4, 0.13)
    fmax = np.full(3, np.finfo(np.float32).max, np.float32)
    assert f_o["pose_difference_larger_than"](np.zeros(3, np.float32), fmax, 0.4, 0.13) == 1


def test_randomised_geometries_restatement_equals_reference(oracle_mod):
    """odd square map sizes (rectangular maps: the two tests after this one), 1..4 levels, off-centre start coordinates,
    random update factors, rooms larger than the map (beams ending outside): restatement == reference, bit for bit.  (Poses
    that make H singular are avoided on purpose: the reference then casts a NaN coordinate to an index and segfaults.)"""
    if not oracle_mod.available("hr"):
        pytest.skip("oracle/_ref not built")
    from hector_slam_amd import synth
    rng = np.random.default_rng(20240924)
    for trial in range(6):
        size = int(rng.choice([96, 125, 250, 333, 512]))
        levels = int(rng.integers(1, 5))
        while (size >> (levels - 1)) < 8:
            levels -= 1
        res = float(rng.choice([0.05, 0.1, 0.2]))
        start = (float(rng.uniform(0.3, 0.7)), float(rng.uniform(0.3, 0.7)))
        free, occ = float(rng.uniform(0.3, 0.49)), float(rng.uniform(0.55, 0.95))
        ext = size * res
        # every other trial: a room LARGER than the map, so many beams end outside it (skipped by the update,
        # exact zeros in the matcher)
        grow = 1.15 if trial % 2 else 0.6
        world = synth.World.make(ext * grow, ext * grow * 0.75, n_boxes=4, seed=int(rng.integers(1 << 30)),
                                 keep_clear=0.5)
        s = float(np.float32(1.0) / np.float32(res))
        o = {k: oracle_mod.Oracle(k, res, size, size, levels, start) for k in ("ho", "hr")}
        for k in o:
            o[k].set_update_factor_free(free)
            o[k].set_update_factor_occupied(occ)
            o[k].proc_set_thresholds(0.02, 0.02)
        n_beams = int(rng.choice([181, 400, 1081]))
        poses = synth.loop_trajectory(world, 14, frac=0.25).astype(np.float32)
        poses[:, 0] += (0.5 - start[0]) * ext * 0.3  # so that the map origin offset (start coords) matters
        noise = np.random.default_rng(trial)
        hint = {k: poses[0].copy() for k in o}
        for t in range(14):
            pts = synth.make_scan(world, poses[t], n_beams, s, noise, range_max=min(30.0, ext))
            origo = rng.uniform(-2, 2, 2).astype(np.float32)
            last = {}
            for k in o:
                o[k].proc_update(pts, hint[k], origo=origo, map_without_matching=(t == 5))
                last[k] = o[k].proc_last_pose()
            assert np.array_equal(last["ho"][0].view(np.uint32), last["hr"][0].view(np.uint32)), (trial, t)
            assert np.array_equal(last["ho"][1].view(np.uint32), last["hr"][1].view(np.uint32)), (trial, t)
            step = poses[min(t + 1, 13)] - poses[t]
            for k in o:
                hint[k] = last[k][0] + step
        for lvl in range(levels):
            a, b = o["ho"].download_level(lvl), o["hr"].download_level(lvl)
            assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1]), (trial, lvl)
            assert np.array_equal(o["ho"].occupancy_grid(lvl), o["hr"].occupancy_grid(lvl))


def test_rectangular_geometries_restatement_equals_reference(oracle_mod):
    """the processor loop of the test above on the rectangular maps of tests/rect_cases.py (wide / tall, sx % 4 != 0, strips
    whose coarsest level is 6 cells across), each with its transpose: proc_update with a laser origin, one
    map_without_matching step, rooms larger than the map -- poses, covariances, every level and the occupancy grids
    bit-identical.  The restatement runs first on every step and must not read the map at a NaN coordinate (the reference
    would crash there), so every step of every geometry is compared."""
    if not oracle_mod.available("hr"):
        pytest.skip("oracle/_ref not built")
    import rect_cases
    from hector_slam_amd import synth
    for gi, (sx, sy, levels) in enumerate(rect_cases.SMALL):
        rng = np.random.default_rng([sx, sy, levels])
        res = rect_cases.RES
        start = (float(rng.uniform(0.35, 0.65)), float(rng.uniform(0.35, 0.65)))
        free, occ = float(rng.uniform(0.3, 0.49)), float(rng.uniform(0.55, 0.95))
        grow = 1.15 if gi % 2 else 0.8
        n_beams = (1081, 4096)[gi % 2]
        world, poses, scans = rect_cases.scene(sx, sy, 12, n_beams, seed=sx * 7 + sy, res=res, grow=grow)
        o = {k: oracle_mod.Oracle(k, res, sx, sy, levels, start) for k in ("ho", "hr")}
        for k in o:
            o[k].set_update_factor_free(free)
            o[k].set_update_factor_occupied(occ)
            o[k].proc_set_thresholds(0.02, 0.02)
        hint = {k: poses[0].copy() for k in o}
        for t in range(12):
            origo = rng.uniform(-2, 2, 2).astype(np.float32)
            last = {}
            for k in ("ho", "hr"):
                o[k].proc_update(scans[t], hint[k], origo=origo, map_without_matching=(t == 5))
                last[k] = o[k].proc_last_pose()
                assert o["ho"].undefined_reads() == 0, (sx, sy, t)
            assert np.array_equal(bits(last["ho"][0]), bits(last["hr"][0])), (sx, sy, t)
            assert np.array_equal(bits(last["ho"][1]), bits(last["hr"][1])), (sx, sy, t)
            step = poses[min(t + 1, 11)] - poses[t]
            for k in o:
                hint[k] = last[k][0] + step
        for lvl in range(levels):
            a, b = o["ho"].download_level(lvl), o["hr"].download_level(lvl)
            assert a[0].shape == (sy >> lvl, sx >> lvl)
            assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]), (sx, sy, lvl)
            assert np.array_equal(o["ho"].occupancy_grid(lvl), o["hr"].occupancy_grid(lvl))
        _, ui = o["ho"].download_level(0)
        assert (ui >= 0).sum() > 100, (sx, sy)  # the loop did map something


@pytest.mark.parametrize("geom", deep_cases.GEOMETRIES + [deep_cases.LARGE], ids=deep_cases.gid)
def test_deep_pyramids_restatement_equals_reference(oracle_mod, geom):
    """the cases of tests/deep_cases.py (6 to 8 levels, coarsest levels of 64 x 64 down to 2 x 2 cells, the 4096^2 map: the very
    scenes the GPU tests run, build counts included): the case is usable (deep_cases.check: no empty level, a regular H on the levels of 16 cells or more, no map read
    at a NaN coordinate -- the restatement goes first everywhere, the reference would crash there), and restatement == reference
    headers on the built map's planes, match, match_many, the per-level chain, and every level after each update of the SLAM loop
    the GPU test runs"""
    if not oracle_mod.available("hr"):
        pytest.skip("oracle/_ref not built")
    from hector_slam_amd import synth
    case = deep_cases.case(geom)
    deep_cases.check(oracle_mod, case)
    assert case.undefined_reads == 0
    L = case.levels
    ho, hr = (deep_cases.built_oracle(oracle_mod, k, case) for k in ("ho", "hr"))

    def same_maps(what):
        for lvl in range(L):
            a, b = ho.download_level(lvl), hr.download_level(lvl)
            assert a[0].shape == (geom[1] >> lvl, geom[0] >> lvl)
            assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]), (geom, what, lvl)
            assert np.array_equal(ho.occupancy_grid(lvl), hr.occupancy_grid(lvl)), (geom, what, lvl)
            assert ho.level_info(lvl) == hr.level_info(lvl)

    same_maps("built")
    pts, offs = synth.pack_scans(case.query_scans)
    pm = ho.match_many(case.query_init, pts, offs)
    assert ho.undefined_reads() == 0
    assert np.array_equal(bits(pm), bits(hr.match_many(case.query_init, pts, offs)))
    for q, (init, sc) in enumerate(zip(case.query_init, case.query_scans)):
        (po, co), (pr, cr) = ho.match(init, sc, case.origo), hr.match(init, sc, case.origo)
        assert np.array_equal(bits(po), bits(pr)) and np.array_equal(bits(co), bits(cr)), (geom, q)
        po, _ = ho.match(init, sc)
        assert np.array_equal(bits(po), bits(pm[q])), (geom, q)
        chain, _, _ = deep_cases.level_chain(ho, init, sc, L)
        for lvl, start, p, it in chain[:: 1 if q < 2 else L]:
            at = ho.map_coords_pose(lvl, start)
            assert np.array_equal(bits(at), bits(hr.map_coords_pose(lvl, start)))
            (Ho, do), (Hr, dr) = ho.hessian_derivs(lvl, at, p), hr.hessian_derivs(lvl, at, p)
            assert np.array_equal(bits(Ho), bits(Hr)) and np.array_equal(bits(do), bits(dr)), (geom, q, lvl)
            for j in (0, it):
                (a, ca), (b, cb) = ho.match_level(lvl, start, p, j), hr.match_level(lvl, start, p, j)
                assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(ca), bits(cb)), (geom, q, lvl, j)
    steps_o = deep_cases.slam_loop(ho, case)
    assert ho.undefined_reads() == 0
    for t, (hint, sc, og, p, c) in enumerate(steps_o):
        pr, cr = hr.match(hint, sc, og)
        assert np.array_equal(bits(p), bits(pr)) and np.array_equal(bits(c), bits(cr)), (geom, t)
        hr.update_by_scan(pr, sc, og)
        hr.on_map_updated()
    same_maps("after the loop")


@pytest.mark.skipif("hr" not in oracle_kinds(), reason="oracle/_ref not built")
@seed(rect_cases.RECT_SEED)
@settings(max_examples=20, deadline=None, database=None, suppress_health_check=list(HealthCheck))
@given(g=rect_cases.rect_geometry())
def test_rectangular_property_restatement_equals_reference(oracle_mod, g):
    """independent size_x / size_y (tests/rect_cases.py rect_geometry): the restatement equals the reference headers on every
    pose, covariance and map of a short SLAM loop.  The GPU test of tests/test_gpu_rect_maps.py draws the same examples."""
    rect_cases.run_loop(g, rect_cases.oracle_impl(oracle_mod, "ho"), rect_cases.oracle_impl(oracle_mod, "hr"))


def test_dense_fans_on_and_beyond_the_map_borders_restatement_equals_reference(oracle_mod):
    """the inputs of tests/test_gpu_dense_edges.py (>= 4096-beam fans ending on and 0.5 .. 6 cells outside the four borders,
    begin cells next to / off every border, widths 64 .. 512, heights with sy % 4 != 0): restatement == reference headers on
    every level after every update, and the fans do reach all four borders -- the CPU pin of what the GPU box then runs"""
    if not oracle_mod.available("hr"):
        pytest.skip("oracle/_ref not built")
    from edge_cases import GEOMETRIES, begin_cells, border_fan, world_pose_of_cell
    for sx, sy, levels, n in GEOMETRIES:
        res = 0.05
        o = [oracle_mod.Oracle(k, res, sx, sy, levels) for k in ("ho", "hr")]
        for x in o:
            x.set_update_factor_free(0.4)
            x.set_update_factor_occupied(0.9)
        rng = np.random.default_rng(sx * 1000 + sy)
        for k, (cx, cy) in enumerate(begin_cells(sx, sy)):
            th = float(rng.uniform(-np.pi, np.pi)) if k % 3 else 0.0
            pose = world_pose_of_cell(res, sx, sy, cx, cy, th)
            pts = border_fan(rng, sx, sy, cx, cy, th, n)
            og = np.zeros(2, np.float32) if k % 4 else np.array([0.3, -0.2], np.float32)
            for x in o:
                x.match(pose, pts, og)
                x.update_by_scan(pose, pts, og)
                x.on_map_updated()
            for lvl in range(levels):
                a, b = o[0].download_level(lvl), o[1].download_level(lvl)
                assert np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), (sx, sy, k, lvl)
        _, ui = o[0].download_level(0)
        assert (ui[0] >= 0).any() and (ui[-1] >= 0).any() and (ui[:, 0] >= 0).any() and (ui[:, -1] >= 0).any(), (sx, sy)


def test_reference_shim_is_thread_safe_about_stdout(oracle_mod, small_scene):
    """the bench's all-cores CPU leg drives the reference from many threads; the shim silences the reference's
    std::cout chatter process-wide (a per-call save/restore once left std::cout on a dead buffer: exit crash)"""
    if not oracle_mod.available("hr"):
        pytest.skip("oracle/_ref not built")
    import subprocess, sys, textwrap
    code = textwrap.dedent("""
        import sys, threading, numpy as np
        sys.path.insert(0, %r)
        from oracle import pyoracle
        pts = np.random.default_rng(0).uniform(-40, 40, (64, 2)).astype(np.float32)
        def work():
            o = pyoracle.Oracle("hr", 0.1, 128, 128, 2)
            for k in range(400):
                o.match(np.zeros(3, np.float32), pts)
                o.update_by_scan(np.zeros(3, np.float32), pts)
                o.on_map_updated()
        th = [threading.Thread(target=work) for _ in range(8)]
        [t.start() for t in th]
        [t.join() for t in th]
        print("done", flush=True)
    """ % os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "done" in r.stdout, (r.returncode, r.stderr[-500:])


def test_ray_distance_restatement_equals_hector_map_tools(oracle_mod):
    """f4: the restatement of DistanceMeasurementProvider::getDist ("ho") against the UNMODIFIED
    hector_map_tools/HectorMapTools.h:132-234 ("hr", compiled against the nav_msgs stand-in) -- 12k random rays on a
    6000 x 400 grid: rays inside and outside the map, zero-length and axis-aligned rays, and rays longer than the
    5000-step cap of bresenham2D (a wall beyond step 5000 must NOT be found)."""
    if not oracle_mod.available("hr"):
        pytest.skip("oracle/_ref/libhector_ref.so not built (needs /root/reference)")
    rng = np.random.default_rng(44)
    sx, sy, res = 6000, 400, 0.05
    grid = np.full((sy, sx), -1, np.int8)
    grid[rng.random((sy, sx)) < 0.002] = 100      # sparse obstacles
    grid[rng.random((sy, sx)) < 0.3] = 0
    grid[:, 5600:5603] = 100                      # a wall 5600 cells out: beyond the cap for rays starting at x < 600
    grid[:, 0:560] = np.where(grid[:, 0:560] == 100, 0, grid[:, 0:560])  # keep the start region free
    grid[180:220, 560:5590] = 0                   # ... and a free corridor to the wall
    ox, oy = -3.0, -7.5
    n = 12000
    begin = np.stack([rng.uniform(ox, ox + sx * res, n), rng.uniform(oy, oy + sy * res, n)], 1).astype(np.float32)
    ang = rng.uniform(0, 2 * np.pi, n)
    length = rng.uniform(0.0, 40.0, n)
    end = (begin + np.stack([np.cos(ang), np.sin(ang)], 1) * length[:, None]).astype(np.float32)
    end[:50] = begin[:50]
    begin[50:100] += 1000.0
    end[100:150] -= 1000.0
    end[150:200, 1] = begin[150:200, 1]
    end[200:250, 0] = begin[200:250, 0]
    # the capped ones: along the corridor from x < 560 cells to beyond the wall (> 5000 major steps away)
    begin[250:450] = np.stack([ox + rng.uniform(1, 550, 200) * res, oy + rng.uniform(182, 218, 200) * res], 1)
    end[250:450] = np.stack([np.full(200, ox + 5900 * res), begin[250:450, 1] + rng.uniform(-0.05, 0.05, 200)], 1)
    d_o, h_o = oracle_mod.ray_distances("ho", grid, (ox, oy), res, begin, end)
    d_r, h_r = oracle_mod.ray_distances("hr", grid, (ox, oy), res, begin, end)
    assert np.array_equal(bits(d_o), bits(d_r))
    has = d_r >= 0
    assert np.array_equal(bits(h_o[has]), bits(h_r[has]))
    assert np.isnan(h_o[~has]).all() and np.isnan(h_r[~has]).all()
    assert (d_r[250:450] < 0).all()               # the cap: the wall 5000+ steps away is not seen
    near = begin[250:450].copy()
    near[:, 0] += 100 * res * 5                   # the same rays started 500 cells closer do see it
    d2, _ = oracle_mod.ray_distances("hr", grid, (ox, oy), res, near[near[:, 0] > ox + 700 * res], end[250:450][near[:, 0] > ox + 700 * res])
    assert (d2 > 0).all() and d2.size > 20
    assert 0.1 < has.mean() < 0.95
