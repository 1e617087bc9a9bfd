"""CPU pin of the map-frame cases (tests/frame_cases.py), no device: the frames are what they say, every case is an ordinary
one the reference defines, and the restatement equals the reference headers bit for bit on every entry the GPU tests compare
(tests/test_gpu_map_frames.py) -- and both equal the numpy statement of the frame written in the case module, so a slip in
a checker's transform cannot hide the same slip in the product's."""
import numpy as np
import pytest

import frame_cases as fc
from conftest import bits, oracle_kinds
from support import same

FRAMES = pytest.mark.parametrize("frame", fc.FRAMES, ids=fc.fid)
GEOMS = pytest.mark.parametrize("geom", fc.GEOMETRIES, ids=fc.gid)
SQUARE = fc.GEOMETRIES[0]


def test_the_frames_are_what_they_say():
    """every frame but the control has at least one of the four facts (on the square map, where the geometry adds none), the
    control has none, and each fact is held by several frames"""
    counts = {}
    for frame in fc.FRAMES:
        facts = fc.frame_facts(frame, SQUARE)
        print(fc.fid(frame), [k for k, v in facts.items() if v])
        if frame == fc.CONTROL:
            assert not any(facts.values()), facts
        else:
            assert any(facts.values()), (frame, facts)
        for k, v in facts.items():
            counts[k] = counts.get(k, 0) + int(v)
    print("frames per fact:", counts)
    assert all(v >= 2 for v in counts.values()), counts
    # what the two exact frames are there for
    for frame in ((0.07, (1.0, 0.0)), (1.0, (0.7, 0.2))):
        facts = fc.frame_facts(frame, SQUARE)
        assert not facts["inverse is not the cell length"] and not facts["inverse translation is not -offset"], (frame, facts)
    lv = fc.frame_numpy((0.03, (0.3, 0.7)), (90, 24, 2))[0]
    assert lv["scale"] == np.float32(33.333336) and lv["m"][4] == np.float32(27.000004), lv
    assert fc.frame_numpy((1.0, (0.7, 0.2)), SQUARE)[0]["scale"] == 1.0


@pytest.mark.parametrize("kind", oracle_kinds())
@GEOMS
@FRAMES
def test_numpy_statement_equals_the_checkers(oracle_mod, frame, geom, kind):
    """level_info, map_coords_pose and world_coords_pose of every level, 40 poses each way"""
    o = fc.checker(oracle_mod, kind, frame, geom)
    lv = fc.frame_numpy(frame, geom)
    assert same(o.scale_to_map(), lv[0]["scale"])
    for lvl in range(geom[2]):
        sx, sy, cell, scale = o.level_info(lvl)
        assert (sx, sy) == fc.dims(geom, lvl) and same(cell, lv[lvl]["cell"]) and same(scale, lv[lvl]["scale"]), (lvl, cell, scale)
        mp, world = fc.geometry_poses(oracle_mod, frame, geom, lvl)
        for p in mp:
            assert same(o.world_coords_pose(lvl, p), fc.world_coords_numpy(lv[lvl], p)), (lvl, p)
        for w in world:
            assert same(o.map_coords_pose(lvl, w), fc.map_coords_numpy(lv[lvl], w)), (lvl, w)


@GEOMS
@FRAMES
def test_the_cases_are_ordinary_and_move(oracle_mod, frame, geom):
    """no case reads what the reference does not define; at least one start pose takes a first Gauss-Newton step that changes
    all three components; every full match moves its start pose; the recorded PICKS hold"""
    o = fc.checker(oracle_mod, "ho", frame, geom)
    u0 = o.undefined_reads()
    all_three = 0
    for tag, w, pts in fc.pairs(oracle_mod, frame, geom):
        p1, _ = o.match_level(0, w, pts, 0)
        all_three += int((bits(p1) != bits(w)).all())
        pm, _ = o.match(w, pts)
        assert np.isfinite(pm).all() and not same(pm, w), (tag, pm, w)
    print(fc.fid(frame), fc.gid(geom), "first steps that change x, y and theta:", all_three, "of", len(fc.SCAN_SIZES))
    assert all_three >= 1
    for n in fc.SCAN_SIZES:
        seed = fc.seed_of(frame, geom, n)
        assert fc.defined_and_moving(oracle_mod, frame, geom, n, seed), (n, seed)
    assert o.undefined_reads() == u0 == 0


def test_the_far_frame_does_not_round_trip(oracle_mod):
    """80 m from the world origin one fp32 ulp of a world coordinate is 3e-4 cell: world -> map -> world is not the identity"""
    lost = 0
    for geom in fc.GEOMETRIES:
        o = fc.checker(oracle_mod, "ho", fc.FAR, geom)
        _, world = fc.geometry_poses(oracle_mod, fc.FAR, geom, 0)
        assert (np.abs(world[:, 0]) > 75).all(), world[:3]
        lost += sum(not same(o.world_coords_pose(0, o.map_coords_pose(0, w)), w) for w in world)
    print("far-frame world poses that do not come back:", lost)
    assert lost >= 10


def test_swapping_the_translations_changes_the_tile_keys(oracle_mod):
    world, back, swapped = fc.order_case(oracle_mod)
    k, ks = fc.tile_keys(fc.ORDER_GEOM, back[:, :2]), fc.tile_keys(fc.ORDER_GEOM, swapped[:, :2])
    changed = int((k != ks).sum())
    print("tile keys:", np.unique(k).size, "distinct;", changed, "of", len(k), "change when t0 and t1 are swapped")
    assert np.unique(k).size >= 32 and changed >= 32
    assert not np.array_equal(np.argsort(k, kind="stable"), np.argsort(ks, kind="stable"))
    T = 1 << fc.tile_shift(fc.ORDER_GEOM)
    assert (np.abs(back[:, :2] / T - np.round(back[:, :2] / T)) * T > 5e-3).all()


@GEOMS
@FRAMES
def test_the_log_passes_and_fails_the_gate(oracle_mod, frame, geom):
    world, deltas, scans = fc.slam_log(oracle_mod, frame, geom)
    o = fc.new_oracle(oracle_mod, "ho", frame, geom, fc.FACTORS)
    poses, _, flags = fc.reference_loop(o, frame, world, deltas, scans)
    print(fc.fid(frame), fc.gid(geom), "integrated", int(flags.sum()), "rejected", int((~flags).sum()))
    assert flags.sum() >= 3 and (~flags).sum() >= 3, flags
    assert o.undefined_reads() == 0 and np.isfinite(poses).all()
    cells = np.abs(poses[-1, :2] - world[-1, :2]).max() / frame[0]
    assert cells < 1.0, ("the reference lost track", cells)
    # the same trajectory as raw ranges from a moving mount
    raw = fc.raw_log(oracle_mod, frame, geom)
    conts, origos = fc.convert_log(fc.checker(oracle_mod, "ho", frame, geom), raw)
    t = fc.new_oracle(oracle_mod, "ho", frame, geom, fc.FACTORS)
    poses, _, flags = fc.reference_loop(t, frame, raw[0], raw[1], conts, origos)
    print(fc.fid(frame), fc.gid(geom), "raw log: integrated", int(flags.sum()), "rejected", int((~flags).sum()), "beams kept", [len(c) for c in conts])
    assert flags.sum() >= 3 and (~flags).sum() >= 3, flags
    assert all(fc.LOG_BEAMS // 2 <= len(c) < fc.LOG_BEAMS for c in conts) and len({tuple(bits(o)) for o in origos}) == fc.N_LOG
    assert t.undefined_reads() == 0 and np.abs(poses[-1, :2] - raw[0][-1, :2]).max() / frame[0] < 1.0


def entry_results(oracle_mod, kind, frame, geom):
    """every entry the GPU tests compare -> a list of (name, array)"""
    o = fc.checker(oracle_mod, kind, frame, geom)
    out = []
    for tag, w, pts in fc.pairs(oracle_mod, frame, geom):
        out.append((f"match {tag}", np.concatenate(o.match(w, pts))))
        for lvl in range(geom[2]):
            lp = fc.level_pts(pts, lvl)
            pm = o.map_coords_pose(lvl, w)
            for it in range(4):
                out.append((f"match_level L{lvl} {tag} it{it}", np.concatenate(o.match_level(lvl, w, lp, it))))
            H, d = o.hessian_derivs(lvl, pm, lp)
            out += [(f"H L{lvl} {tag}", H), (f"dTr L{lvl} {tag}", d)]
            out.append((f"likelihood L{lvl} {tag}", o.likelihood_states(lvl, pm[None], lp)))
            for k, a in enumerate(o.covariance_for_poses(lvl, pm[None], lp)):
                out.append((f"covariance_for_poses[{k}] L{lvl} {tag}", a))
    starts, pts = fc.batch(oracle_mod, frame, geom, 16, 300)
    out += [(f"batch {j}", np.concatenate(o.match(starts[j], pts))) for j in range(len(starts))]
    # a short update sequence and the log, on checkers of their own
    u = fc.new_oracle(oracle_mod, kind, frame, geom, fc.FACTORS)
    _, world, scans = fc.trajectory(oracle_mod, frame, geom, fc.N_TRAJ, [300, 63, 1920, 1, 560, 65])
    for k in range(fc.N_TRAJ):
        u.build_map(world[k][None], [scans[k]])
        for lvl in range(geom[2]):
            lo, ui = u.download_level(lvl)
            out += [(f"update {k} L{lvl} log-odds", lo), (f"update {k} L{lvl} stamps", ui.astype(np.float32))]
    s = fc.new_oracle(oracle_mod, kind, frame, geom, fc.FACTORS)
    poses, covs, flags = fc.reference_loop(s, frame, *fc.slam_log(oracle_mod, frame, geom))
    out += [("loop poses", poses), ("loop covariances", covs), ("loop decisions", flags.astype(np.float32))]
    out += [(f"loop L{lvl} log-odds", s.download_level(lvl)[0]) for lvl in range(geom[2])]
    raw = fc.raw_log(oracle_mod, frame, geom)
    conts, origos = fc.convert_log(o, raw)
    t = fc.new_oracle(oracle_mod, kind, frame, geom, fc.FACTORS)
    poses, covs, flags = fc.reference_loop(t, frame, raw[0], raw[1], conts, origos)
    out += [("raw log origos", origos), ("raw log poses", poses), ("raw log covariances", covs), ("raw log decisions", flags.astype(np.float32))]
    out += [(f"raw log container {k}", c) for k, c in enumerate(conts)]
    out += [(f"raw log L{lvl} log-odds", t.download_level(lvl)[0]) for lvl in range(geom[2])]
    assert u.undefined_reads() <= 0 and s.undefined_reads() <= 0
    return out


@GEOMS
@FRAMES
def test_restatement_equals_reference_on_every_case(oracle_mod, frame, geom):
    if not oracle_mod.available("hr"):
        pytest.skip("oracle/_ref/libhector_ref.so not built (needs the reference's sources)")
    ho = fc.checker(oracle_mod, "ho", frame, geom)
    a = entry_results(oracle_mod, "ho", frame, geom)
    assert ho.undefined_reads() == 0  # the guard: only then is the reference given the same inputs
    b = entry_results(oracle_mod, "hr", frame, geom)
    assert len(a) == len(b) > 100
    for (name, x), (_, y) in zip(a, b):
        assert np.isfinite(x).all(), name
        assert same(x, y), (fc.fid(frame), fc.gid(geom), name)
