"""hsm_ray_distances_device / hsm_cast_scans_device / hsm_cast_scans on the MI355X, against DistanceMeasurementProvider::getDist
of the CPU checker on the cases of tests/cast_cases.py (held to the unmodified reference in test_cast_scans_reference.py).

Every comparison is on bits.  Ranges: the checker's float for every ray, -resolution where it finds no hit and for every ray
with a non-finite coordinate (the library's stated rule).  Hit points: prefilled with NaN, the checker's bits where there is a
hit, still NaN elsewhere.  Both launch shapes of the cast (a wavefront per beam, a lane per beam) are forced in turn through
HSM_CAST_FORM and asked which one ran."""
import numpy as np
import pytest

import cast_cases
from conftest import bits, make_oracle
from support import capi, dev, layout_of, stream_ptr
from test_gpu_score_batch import gpu_for, oracle_update

pytestmark = pytest.mark.gpu

HSM_ERR_INVALID = -1
SENTINEL = -777.0
FORMS = {"wave": b"cast_scans_wave_kernel", "lane": b"cast_scans_lane_kernel"}


@pytest.fixture(scope="module")
def scene_cases(oracle_mod, pyramid_scene):
    """per level: grid, metadata, the 37 poses, and per range_max the expected (ranges, hit) of the full 1081-beam table -- a
    shorter fan is the first n beams of the table, so its expectation is the first n columns"""
    sc = pyramid_scene
    o = make_oracle(oracle_mod, "ho", sc)
    angles = cast_cases.beam_table(1081)
    out = []
    for lvl in range(sc.levels):
        grid, meta = o.occupancy_grid(lvl), cast_cases.metadata(o, lvl)
        poses, fam = cast_cases.poses(sc, grid, meta, seed=lvl)
        want = {name: cast_cases.expected_cast("ho", grid, meta, poses, angles, r) + (r,)
                for name, r in cast_cases.range_maxes(grid, meta).items()}
        out.append(dict(grid=grid, meta=meta, poses=poses, fam=fam, want=want))
    return dict(o=o, angles=angles, levels=out)


def context(capi, monkeypatch, sc, o, form=None, layout="quad", **kw):
    if form is None:
        monkeypatch.delenv("HSM_CAST_FORM", raising=False)
    else:
        monkeypatch.setenv("HSM_CAST_FORM", form)
    return gpu_for(capi, sc, o, layout=layout_of(capi, layout), **kw)


def assert_rays(what, got, want):
    (d, h), (rd, rh) = got, want
    d, h, rd, rh = d.reshape(-1), h.reshape(-1, 2), rd.reshape(-1), rh.reshape(-1, 2)
    assert not (d == SENTINEL).any(), f"{what}: ranges never written"
    bad = bits(d) != bits(rd)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {d.size} ranges differ, first {np.flatnonzero(bad)[:5]}"
    has = rd >= 0
    assert np.array_equal(bits(h[has]), bits(rh[has])), f"{what}: hit points differ"
    assert np.isnan(h[~has]).all(), f"{what}: a ray without a hit wrote its hit point"


def cast_device(g, level, poses, angles, range_max, stream=None, want_hit=True):
    import torch
    B, n = len(poses), len(angles)
    s = stream or torch.cuda.current_stream()
    with torch.cuda.stream(s):
        d_p, d_a = dev(np.asarray(poses, np.float32)), dev(np.asarray(angles, np.float32))
        ranges = torch.full((B, n), SENTINEL, dtype=torch.float32, device="cuda:0")
        hit = torch.full((B, n, 2), float("nan"), dtype=torch.float32, device="cuda:0")
        g.cast_scans_device(level, B, d_p.data_ptr(), d_a.data_ptr(), n, range_max, ranges.data_ptr(),
                            hit.data_ptr() if want_hit else 0, s.cuda_stream)
        return ranges.cpu().numpy(), hit.cpu().numpy()


# ---- 1: arbitrary rays ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["quad", "plane"])
def test_device_ray_entry_equals_the_host_entry_and_the_checker(capi, monkeypatch, oracle_mod, pyramid_scene, scene_cases, layout):
    import torch
    sc = pyramid_scene
    g = context(capi, monkeypatch, sc, scene_cases["o"], layout=layout)
    for lvl, c in enumerate(scene_cases["levels"]):
        meta = c["meta"]
        assert g.map_metadata(lvl) == meta
        begin, end = cast_cases.mixed_rays(c["grid"], meta, 2000, 100 + lvl)
        want = cast_cases.expected_rays("ho", c["grid"], meta, begin, end)
        d_b, d_e = dev(begin), dev(end)
        dist = torch.full((2000,), SENTINEL, dtype=torch.float32, device="cuda:0")
        hit = torch.full((2000, 2), float("nan"), dtype=torch.float32, device="cuda:0")
        g.ray_distances_device(lvl, 2000, d_b.data_ptr(), d_e.data_ptr(), dist.data_ptr(), hit.data_ptr(),
                               stream=stream_ptr())
        got = dist.cpu().numpy(), hit.cpu().numpy()
        assert capi.load_library().hsm_last_launch_kernel(g._h) == b"ray_distance_kernel"
        assert_rays(f"level {lvl}, device entry", got, want)
        assert_rays(f"level {lvl}, host entry", g.ray_distances(lvl, begin, end), want)
        # without the hit array, and a ray of NaNs: without a hit by the rule
        begin[5], end[9, 1] = np.nan, np.inf
        dist.fill_(SENTINEL)
        d_b, d_e = dev(begin), dev(end)
        g.ray_distances_device(lvl, 2000, d_b.data_ptr(), d_e.data_ptr(), dist.data_ptr(), 0,
                               stream=stream_ptr())
        want2 = cast_cases.expected_rays("ho", c["grid"], meta, begin, end)[0]
        got2 = dist.cpu().numpy()
        assert np.array_equal(bits(got2), bits(want2)), (lvl, np.flatnonzero(bits(got2) != bits(want2))[:8])
        assert want2[5] == want2[9] == -np.float32(meta[2])
    g.close()


# ---- 2: whole fans from batches of poses, both launch shapes -------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["quad", "plane"])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_cast_scans_is_bit_identical_on_every_level(capi, monkeypatch, pyramid_scene, scene_cases, form, layout):
    sc = pyramid_scene
    g = context(capi, monkeypatch, sc, scene_cases["o"], form, layout)
    lib = capi.load_library()
    table = scene_cases["angles"]
    for lvl, c in enumerate(scene_cases["levels"]):
        res = np.float32(c["meta"][2])
        for name, (rd, rh, rmax) in c["want"].items():
            for n in cast_cases.BEAMS:
                what = f"{form}, level {lvl}, range_max {name}, {n} beams"
                want = rd[:, :n], rh[:, :n]
                got = cast_device(g, lvl, c["poses"], table[:n], rmax)
                assert lib.hsm_last_launch_kernel(g._h) == FORMS[form], what
                assert_rays(what, got, want)
                assert_rays(what + ", host entry", g.cast_scans(lvl, c["poses"], table[:n], rmax), want)
                if name in ("zero", "two_diagonals"):
                    assert (got[0] == -res).all(), what
        # the stated rule for the non-finite poses, and the ranges alone
        rd, _, rmax = c["want"]["8m"]
        only, untouched = cast_device(g, lvl, c["poses"], table, rmax, want_hit=False)
        assert np.array_equal(bits(only), bits(rd)) and np.isnan(untouched).all()
        assert (only[c["fam"]["nonfinite"]] == -res).all() and (only[c["fam"]["outside"]] == -res).all()
        on_wall = only[c["fam"]["wall"]]
        assert (on_wall[on_wall >= 0] == 0).all() and (on_wall >= 0).any(axis=1).all()  # step 0 is the occupied cell
    g.close()


def test_the_default_shape_follows_the_fan_length(capi, monkeypatch, pyramid_scene, scene_cases):
    """the measured rule (profiles/r18): a wavefront per beam below 32 beams, a lane per beam from there on -- also where a
    second or an eighteenth wavefront per pose is nearly empty (65, 1081 beams)"""
    g = context(capi, monkeypatch, pyramid_scene, scene_cases["o"])
    lib = capi.load_library()
    c = scene_cases["levels"][0]
    rd, rh, rmax = c["want"]["8m"]
    for n, form in ((1, "wave"), (31, "wave"), (32, "lane"), (63, "lane"), (64, "lane"), (65, "lane"), (1081, "lane")):
        assert_rays(f"default, {n} beams", cast_device(g, 0, c["poses"], scene_cases["angles"][:n], rmax), (rd[:, :n], rh[:, :n]))
        assert lib.hsm_last_launch_kernel(g._h) == FORMS[form], n
    g.close()


# ---- 3: the cap ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", sorted(FORMS))
def test_the_walk_stops_after_5000_steps(capi, monkeypatch, form):
    cc = cast_cases
    monkeypatch.setenv("HSM_CAST_FORM", form)
    g = capi.MapRepMultiMap(cc.CAP_RES, cc.CAP_SX, cc.CAP_SY, 1)
    g.upload_level(0, cc.cap_logodds(), None)
    meta = g.map_metadata(0)
    res = np.float32(meta[2])
    grid = cc.cap_grid()
    assert np.array_equal(g.occupancy_grid(0), grid)
    far, near = cc.cap_poses(meta)
    r_far, r_near, r_edge = cc.CAP_FAR_CELLS * meta[2], cc.CAP_NEAR_CELLS * meta[2], cc.CAP_EDGE_CELLS * meta[2]
    got_far = cast_device(g, 0, far, cc.CAP_ANGLES, r_far)
    got_near = cast_device(g, 0, near, cc.CAP_ANGLES, r_near)
    assert_rays("far", got_far, cc.expected_cast("ho", grid, meta, far, cc.CAP_ANGLES, r_far))
    assert_rays("near", got_near, cc.expected_cast("ho", grid, meta, near, cc.CAP_ANGLES, r_near))
    assert (got_far[0] == -res).all() and (got_near[0] > 0).all()
    edge = cast_device(g, 0, cc.cap_edge_poses(meta), cc.CAP_ANGLES[:1], r_edge)
    assert_rays("edge", edge, cc.expected_cast("ho", grid, meta, cc.cap_edge_poses(meta), cc.CAP_ANGLES[:1], r_edge))
    assert edge[0][0, 0] == -res and edge[0][1, 0] == res * np.float32(4999)
    g.close()


# ---- 4: ordering against map updates -------------------------------------------------------------------------------------------------
def test_casts_are_ordered_against_queued_updates(capi, monkeypatch, oracle_mod, pyramid_scene):
    """updates queued on the context, then a cast on a caller's stream with no host wait: the updated map's ranges; then another
    update behind the cast, which must not rewrite the map under it"""
    import torch
    from hector_slam_amd import synth
    sc = pyramid_scene
    o = make_oracle(oracle_mod, "ho", sc)
    g = context(capi, monkeypatch, sc, o, stamps=False)  # (log-odds only: see test_scores_are_ordered_against_queued_updates)
    rng = np.random.default_rng(8)
    sfac = float(np.float32(1.0) / np.float32(sc.resolution))
    dense = [synth.make_scan(sc.world, sc.build_poses[t], 16384, sfac, rng) for t in range(4)]  # long-running updates
    angles = cast_cases.beam_table(1081)
    meta = cast_cases.metadata(o, 0)
    poses, _ = cast_cases.poses(sc, o.occupancy_grid(0), meta, seed=0)
    before = cast_cases.expected_cast("ho", o.occupancy_grid(0), meta, poses, angles, 8.0)
    d_p, d_a = dev(poses), dev(angles)
    s = torch.cuda.Stream()
    outs = [(torch.full((cast_cases.B, 1081), SENTINEL, dtype=torch.float32, device="cuda:0"),
             torch.full((cast_cases.B, 1081, 2), float("nan"), dtype=torch.float32, device="cuda:0")) for _ in range(2)]
    torch.cuda.synchronize()
    for t in range(3):
        g.updateByScan(dense[t], sc.build_poses[t])  # queued, not waited for
        oracle_update(o, sc.build_poses[t], dense[t])
    g.cast_scans_device(0, cast_cases.B, d_p.data_ptr(), d_a.data_ptr(), 1081, 8.0, outs[0][0].data_ptr(), outs[0][1].data_ptr(),
                        s.cuda_stream)
    after = cast_cases.expected_cast("ho", o.occupancy_grid(0), meta, poses, angles, 8.0)
    g.updateByScan(dense[3], sc.build_poses[3])      # behind the cast
    oracle_update(o, sc.build_poses[3], dense[3])
    g.cast_scans_device(0, cast_cases.B, d_p.data_ptr(), d_a.data_ptr(), 1081, 8.0, outs[1][0].data_ptr(), outs[1][1].data_ptr(),
                        s.cuda_stream)
    last = cast_cases.expected_cast("ho", o.occupancy_grid(0), meta, poses, angles, 8.0)
    s.synchronize()
    g.synchronize()
    assert_rays("behind three updates", (outs[0][0].cpu().numpy(), outs[0][1].cpu().numpy()), after)
    assert_rays("behind the fourth", (outs[1][0].cpu().numpy(), outs[1][1].cpu().numpy()), last)
    assert not np.array_equal(bits(before[0]), bits(after[0]))  # the updates do change these ranges
    assert np.array_equal(bits(g.download_level(0)[0]), bits(o.download_level(0)[0]))  # and no update was disturbed
    g.close()


# ---- 5: graph capture ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", sorted(FORMS))
def test_a_captured_cast_replays_with_new_poses(capi, monkeypatch, pyramid_scene, scene_cases, form):
    import torch
    sc = pyramid_scene
    g = context(capi, monkeypatch, sc, scene_cases["o"], form)
    c = scene_cases["levels"][0]
    angles = scene_cases["angles"]
    rd, rh, rmax = c["want"]["8m"]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_p, d_a = dev(c["poses"]), dev(angles)
        ranges = torch.full((cast_cases.B, 1081), SENTINEL, dtype=torch.float32, device="cuda:0")
        hit = torch.full((cast_cases.B, 1081, 2), float("nan"), dtype=torch.float32, device="cuda:0")

    def launch():
        g.cast_scans_device(0, cast_cases.B, d_p.data_ptr(), d_a.data_ptr(), 1081, rmax, ranges.data_ptr(), hit.data_ptr(), s.cuda_stream)
    launch()  # eager first
    s.synchronize()
    assert_rays("eager", (ranges.cpu().numpy(), hit.cpu().numpy()), (rd, rh))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        launch()
    moved = np.roll(c["poses"], 5, axis=0).copy()
    moved[:20, :2] += np.float32(0.11)
    want = cast_cases.expected_cast("ho", c["grid"], c["meta"], moved, angles, rmax)
    with torch.cuda.stream(s):
        d_p.copy_(dev(moved))
        ranges.fill_(SENTINEL)
        hit.fill_(float("nan"))
        graph.replay()
    s.synchronize()
    assert_rays("replay", (ranges.cpu().numpy(), hit.cpu().numpy()), want)
    assert not np.array_equal(bits(want[0]), bits(rd))
    del graph
    g.close()


# ---- 6: refusals -----------------------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing(capi, monkeypatch, oracle_mod, small_scene):
    import torch
    sc = small_scene
    g = context(capi, monkeypatch, sc, make_oracle(oracle_mod, "ho", sc, build=False))
    lib = capi.load_library()
    buf = torch.full((64,), SENTINEL, dtype=torch.float32, device="cuda:0")
    p = buf.data_ptr()
    g.score_batch_device(0, 1, p, p, 0, 1, p + 128)  # some launch of this context: the name the refusals must leave alone
    torch.cuda.synchronize()
    buf.fill_(SENTINEL)
    name = lib.hsm_last_launch_kernel(g._h)
    assert name == b"score_batch_kernel"
    cast, rays, host = lib.hsm_cast_scans_device, lib.hsm_ray_distances_device, lib.hsm_cast_scans
    hb = np.full(64, SENTINEL, np.float32)
    hp = hb.ctypes.data
    nan, inf = float("nan"), float("inf")
    bad = {
        "cast: null context": lambda: cast(None, 0, 1, p, p, 1, 8.0, p, p, None),
        "cast: level -1": lambda: cast(g._h, -1, 1, p, p, 1, 8.0, p, p, None),
        "cast: level 1 of 1": lambda: cast(g._h, 1, 1, p, p, 1, 8.0, p, p, None),
        "cast: batch < 0": lambda: cast(g._h, 0, -1, p, p, 1, 8.0, p, p, None),
        "cast: n < 0": lambda: cast(g._h, 0, 1, p, p, -1, 8.0, p, p, None),
        "cast: null poses": lambda: cast(g._h, 0, 1, None, p, 1, 8.0, p, p, None),
        "cast: null angles": lambda: cast(g._h, 0, 1, p, None, 1, 8.0, p, p, None),
        "cast: null ranges": lambda: cast(g._h, 0, 1, p, p, 1, 8.0, None, p, None),
        "cast: range_max < 0": lambda: cast(g._h, 0, 1, p, p, 1, -1.0, p, p, None),
        "cast: range_max NaN": lambda: cast(g._h, 0, 1, p, p, 1, nan, p, p, None),
        "cast: range_max inf": lambda: cast(g._h, 0, 1, p, p, 1, inf, p, p, None),
        "host cast: null context": lambda: host(None, 0, 1, hp, hp, 1, 8.0, hp, hp),
        "host cast: level": lambda: host(g._h, 3, 1, hp, hp, 1, 8.0, hp, hp),
        "host cast: batch < 0": lambda: host(g._h, 0, -1, hp, hp, 1, 8.0, hp, hp),
        "host cast: n < 0": lambda: host(g._h, 0, 1, hp, hp, -1, 8.0, hp, hp),
        "host cast: null poses": lambda: host(g._h, 0, 1, None, hp, 1, 8.0, hp, hp),
        "host cast: null angles": lambda: host(g._h, 0, 1, hp, None, 1, 8.0, hp, hp),
        "host cast: null ranges": lambda: host(g._h, 0, 1, hp, hp, 1, 8.0, None, hp),
        "host cast: range_max": lambda: host(g._h, 0, 1, hp, hp, 1, -0.5, hp, hp),
        "rays: null context": lambda: rays(None, 0, 0.0, 0.0, 0.1, 1, p, p, p, p, None),
        "rays: level": lambda: rays(g._h, 2, 0.0, 0.0, 0.1, 1, p, p, p, p, None),
        "rays: n < 0": lambda: rays(g._h, 0, 0.0, 0.0, 0.1, -1, p, p, p, p, None),
        "rays: null begin": lambda: rays(g._h, 0, 0.0, 0.0, 0.1, 1, None, p, p, p, None),
        "rays: null end": lambda: rays(g._h, 0, 0.0, 0.0, 0.1, 1, p, None, p, p, None),
        "rays: null distances": lambda: rays(g._h, 0, 0.0, 0.0, 0.1, 1, p, p, None, p, None),
        "rays: resolution 0": lambda: rays(g._h, 0, 0.0, 0.0, 0.0, 1, p, p, p, p, None),
        "rays: resolution < 0": lambda: rays(g._h, 0, 0.0, 0.0, -0.1, 1, p, p, p, p, None),
        "rays: resolution NaN": lambda: rays(g._h, 0, 0.0, 0.0, nan, 1, p, p, p, p, None),
    }
    for what, call in bad.items():
        assert call() == HSM_ERR_INVALID, what
        assert lib.hsm_last_launch_kernel(g._h) == name, what
    # nothing to do: HSM_OK, nothing launched
    assert cast(g._h, 0, 0, None, None, 5, 8.0, None, None, None) == 0
    assert cast(g._h, 0, 5, None, None, 0, 8.0, None, None, None) == 0
    assert host(g._h, 0, 0, None, None, 5, 8.0, None, None) == 0
    assert rays(g._h, 0, 0.0, 0.0, 0.1, 0, None, None, None, None, None) == 0
    assert lib.hsm_last_launch_kernel(g._h) == name
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all() and (hb == SENTINEL).all()
    g.close()
