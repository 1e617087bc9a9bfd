"""Drop-in proof for the C++ boundary: tests/cpp/slam_driver.cpp drives the reference's
UNCHANGED HectorSlamProcessor.h like the ROS node does.  oracle/Makefile compiles that one source twice:

  oracle/_ref/slam_driver_ref    reference include tree only                       -> CPU reference
  oracle/_ref/slam_driver_mi355  same tree with slam_main/MapRepMultiMap.h replaced by
                                 include/hector_slam_lib/slam_main/MapRepMultiMap.h   -> MI355X drop-in

Both binaries are built in the build container (where /root/reference exists) and travel to the GPU
box with the snapshot.  CPU tests pin the driver against the oracle; the gpu test runs both binaries
on the same scenario and compares poses (1e-4 m / 1e-4 rad), covariances, the draw/debug hook
streams, locker usage and the host-mirror grids the map publisher would read.
"""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ang_diff, make_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SAN = ["san"] if os.environ.get("HSM_ORACLE_SAN") == "1" else []  # tools/sanitize_cpu.sh: the ASan/UBSan build
REF_BIN = os.path.join(ROOT, "oracle", "_ref", *_SAN, "slam_driver_ref")
GPU_BIN = os.path.join(ROOT, "oracle", "_ref", "slam_driver_mi355")
FACADE = os.path.join(ROOT, "include", "hector_slam_lib", "slam_main", "MapRepMultiMap.h")


def write_scenario(path, sc, steps, hooks, min_dist=0.05, min_ang=0.02, origo=(0.3, -0.1), mwm_at=(7,)):
    s = np.float32(sc.scale_to_map)
    with open(path, "wb") as f:
        f.write(struct.pack("<fiiffffii", sc.resolution, sc.map_size, sc.levels, 0.4, 0.9, min_dist, min_ang,
                            int(hooks), steps))
        for t in range(steps):
            if t == 0:
                hint, use_last = sc.build_poses[0], 0
            else:  # odometry delta on top of the last matched pose, like scanCallback's start estimate
                hint, use_last = sc.build_poses[t] - sc.build_poses[t - 1], 1
            pts = np.ascontiguousarray(sc.build_scans[t], np.float32)
            f.write(struct.pack("<fffii", *[float(v) for v in hint], use_last, 1 if t in mwm_at else 0))
            f.write(struct.pack("<ffi", float(origo[0] * s), float(origo[1] * s), pts.shape[0]))
            f.write(pts.tobytes())


def read_output(path, steps):
    buf = open(path, "rb").read()
    off = 0
    pc = np.frombuffer(buf, np.float32, steps * 12, off).reshape(steps, 12)
    off += steps * 48
    (nb,) = struct.unpack_from("<i", buf, off)
    off += 4
    batch = np.frombuffer(buf, np.float32, nb * 3, off).reshape(nb, 3)
    off += 12 * nb
    (nlog,) = struct.unpack_from("<i", buf, off)
    off += 4
    log = np.frombuffer(buf, np.float32, nlog, off)
    off += 4 * nlog
    locks, unlocks, scale, levels = struct.unpack_from("<iifi", buf, off)
    off += 16
    grids = []
    for _ in range(levels):
        sx, sy, cell, upd = struct.unpack_from("<iifi", buf, off)
        off += 16
        occ = np.frombuffer(buf, np.int8, sx * sy, off).reshape(sy, sx)
        off += sx * sy
        val = np.frombuffer(buf, np.float32, sx * sy, off).reshape(sy, sx)
        off += 4 * sx * sy
        grids.append(dict(sx=sx, sy=sy, cell=cell, update_index=upd, occ=occ, val=val))
    assert off == len(buf)
    return dict(pose=pc[:, :3], cov=pc[:, 3:], batch=batch, log=log, locks=locks, unlocks=unlocks, scale=scale, grids=grids)


def parse_log(log):
    calls, i = [], 0
    while i < len(log):
        tag, n = int(log[i]), int(log[i + 1])
        calls.append((tag, log[i + 2:i + 2 + n]))
        i += 2 + n
    return calls


def run(binary, scenario, out):
    r = subprocess.run([binary, scenario, out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


needs_ref = pytest.mark.skipif(not os.path.exists(REF_BIN), reason="oracle/_ref/slam_driver_ref not built")


def test_facade_is_source_only_forwarding():
    """the facade has no compute path of its own: it forwards to the C ABI and nothing else"""
    src = open(FACADE).read()
    for sym in ("hsm_create", "hsm_match", "hsm_match_trace", "hsm_update_by_scan", "hsm_download_cells",
                "hsm_set_update_factor_free", "hsm_set_update_factor_occupied", "hsm_reset", "hsm_destroy"):
        assert sym in src
    for forbidden in ("interpMapValueWithDerivatives", "getCompleteHessianDerivs", "ScanMatcher", "oracle"):
        assert forbidden not in src.replace("ScanMatcher.h", "").replace("ScanMatcher::", ""), forbidden
    assert "class MapRepMultiMap : public MapRepresentationInterface" in src


@needs_ref
def test_reference_driver_matches_oracle(tmp_path, oracle_mod, pyramid_scene):
    """pins the driver + scenario format: the reference binary == the oracle's HectorSlamProcessor loop"""
    sc, steps = pyramid_scene, 12
    scen, out = str(tmp_path / "s.bin"), str(tmp_path / "o.bin")
    write_scenario(scen, sc, steps, hooks=False)
    run(REF_BIN, scen, out)
    r = read_output(out, steps)
    o = make_oracle(oracle_mod, "ho", sc, build=False)
    o.proc_set_thresholds(0.05, 0.02)
    origo = np.array([0.3, -0.1], np.float32) * np.float32(sc.scale_to_map)
    last = np.zeros(3, np.float32)
    for t in range(steps):
        hint = sc.build_poses[0] if t == 0 else (sc.build_poses[t] - sc.build_poses[t - 1]) + last
        o.proc_update(sc.build_scans[t], hint.astype(np.float32), origo=origo, map_without_matching=(t == 7))
        last, cov = o.proc_last_pose()
        assert np.array_equal(last.view(np.uint32), r["pose"][t].view(np.uint32)), t
    for lvl in range(sc.levels):
        lo, _ = o.download_level(lvl)
        assert np.array_equal(lo.view(np.uint32), r["grids"][lvl]["val"].view(np.uint32))
    assert r["locks"] == r["unlocks"] > 0


@needs_ref
def test_hook_stream_of_reference_driver(tmp_path, pyramid_scene):
    sc, steps = pyramid_scene, 4
    scen, out = str(tmp_path / "s.bin"), str(tmp_path / "o.bin")
    write_scenario(scen, sc, steps, hooks=True, mwm_at=())
    run(REF_BIN, scen, out)
    calls = parse_log(read_output(out, steps)["log"])
    # per update: 3+3+5 addHessianMatrix, one debug send, one draw send
    assert sum(1 for t, _ in calls if t == 8) == steps * 11
    assert sum(1 for t, _ in calls if t == 6) == steps and sum(1 for t, _ in calls if t == 7) == steps


@needs_ref
def test_reference_driver_with_publisher_thread_is_unchanged(tmp_path, pyramid_scene):
    """the threaded mode of the driver does not disturb the reference run (publisher only reads under the mutex)"""
    sc, steps = pyramid_scene, 10
    scen0, scen2 = str(tmp_path / "s0.bin"), str(tmp_path / "s2.bin")
    write_scenario(scen0, sc, steps, hooks=0)
    write_scenario(scen2, sc, steps, hooks=2)
    run(REF_BIN, scen0, str(tmp_path / "o0.bin"))
    run(REF_BIN, scen2, str(tmp_path / "o2.bin"))
    a, b = read_output(str(tmp_path / "o0.bin"), steps), read_output(str(tmp_path / "o2.bin"), steps)
    assert np.array_equal(a["pose"].view(np.uint32), b["pose"].view(np.uint32))
    assert all(np.array_equal(x["val"].view(np.uint32), y["val"].view(np.uint32)) for x, y in zip(a["grids"], b["grids"]))
    assert b["locks"] == b["unlocks"] >= a["locks"] + 3


@pytest.mark.gpu
@pytest.mark.parametrize("hooks", [0, 1, 2], ids=["plain", "draw+debug hooks", "publisher thread"])
def test_dropin_matches_reference_node_loop(tmp_path, pyramid_scene, hooks):
    """hooks: 0 plain; 1 with DrawInterface/HectorDebugInfoInterface; 2 with a concurrent map-publisher THREAD that
    fetches getGridMap(0) and reads every cell under the (real) map mutex while the main thread matches and updates,
    like HectorMappingRos::publishMapLoop"""
    if not (os.path.exists(GPU_BIN) and os.path.exists(REF_BIN)):
        # the two drivers need the reference headers (/root/reference) at BUILD time; __graft_entry__.build()
        # makes them in the build container and they travel to the GPU box with the snapshot
        pytest.skip("oracle/_ref/slam_driver_{ref,mi355} not prebuilt (run __graft_entry__.build() where "
                    "/root/reference exists)")
    sc, steps = pyramid_scene, 25
    scen = str(tmp_path / "s.bin")
    write_scenario(scen, sc, steps, hooks=hooks)
    run(REF_BIN, scen, str(tmp_path / "ref.bin"))
    stdout = run(GPU_BIN, scen, str(tmp_path / "gpu.bin"))
    assert "MI355X resident" in stdout  # the facade's banner: proves which MapRepMultiMap was compiled in
    r, g = read_output(str(tmp_path / "ref.bin"), steps), read_output(str(tmp_path / "gpu.bin"), steps)
    dxy = np.abs(r["pose"][:, :2].astype(np.float64) - g["pose"][:, :2]).max()
    dth = ang_diff(r["pose"][:, 2], g["pose"][:, 2]).max()
    assert dxy <= 1e-4 and dth <= 1e-4, (dxy, dth)
    assert np.abs(r["cov"] - g["cov"]).max() <= 1e-3 * np.abs(r["cov"]).max()
    # the library default (round 5: the reference's summation order on the single-scan entry point too): not a bit differs
    # anywhere -- poses, covariances, the batched extension, every grid, every record the hooks saw
    exact_default = os.environ.get("HSM_PARITY", "auto") in ("auto", "exact")
    if exact_default:
        same = lambda a, b: np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))  # noqa: E731
        assert same(r["pose"], g["pose"]) and same(r["cov"], g["cov"]) and same(r["batch"], g["batch"])
        for a, b in zip(r["grids"], g["grids"]):
            assert same(a["val"], b["val"]) and np.array_equal(a["occ"], b["occ"])
    # the facade's batched extension (one launch) == the reference's per-scan matchData calls
    assert g["batch"].shape == r["batch"].shape == (8, 3)
    assert np.abs(r["batch"][:, :2].astype(np.float64) - g["batch"][:, :2]).max() <= 1e-4
    assert ang_diff(r["batch"][:, 2], g["batch"][:, 2]).max() <= 1e-4
    # lockers: the reference takes a level's locker around every update because the update writes the cells the
    # publisher reads; the facade's updates write device planes, and the locker is taken where the HOST mirror is
    # written -- once per (lazy) mirror refresh.  Balanced on both sides, and the level with the locker was refreshed at least once.
    assert g["locks"] == g["unlocks"] and r["locks"] == r["unlocks"]
    if hooks == 2:  # the publisher thread fetched the grid while the loop ran: at least one refresh under the locker
        assert g["locks"] >= 1  # (plain run: the driver reports the counts BEFORE it reads the grids, so none yet)
    assert g["scale"] == r["scale"] and len(g["grids"]) == len(r["grids"])
    for a, b in zip(r["grids"], g["grids"]):
        assert (a["sx"], a["sy"], a["cell"], a["update_index"]) == (b["sx"], b["sy"], b["cell"], b["update_index"])
        touched = (a["val"] != 0).sum()
        assert touched > 1000
        # poses differ in the last bits -> a handful of Bresenham end cells may flip
        assert (a["val"].view(np.uint32) != b["val"].view(np.uint32)).sum() <= 0.002 * touched
        assert (a["occ"] != b["occ"]).sum() <= 0.002 * touched
    ca, cb = parse_log(r["log"]), parse_log(g["log"])
    assert [t for t, _ in ca] == [t for t, _ in cb]  # identical hook call sequence
    if hooks == 1:
        assert len(ca) > 1000
        for (t, x), (_, y) in zip(ca, cb):
            if exact_default:
                assert np.array_equal(x, y), (t, x, y)
            elif t == 8:    # Hessians
                assert np.abs(x - y).max() <= 1e-3 * max(np.abs(x).max(), 1.0)
            elif t in (1, 2):  # drawn points / arrows, world frame
                assert np.abs(x[:2] - y[:2]).max() <= 2e-4
            else:
                assert np.array_equal(x, y)


@pytest.fixture(scope="module")
def deep_scene():
    """1081 beams, a 6-level pyramid 1024 / 512 / ... / 32 over a 40 m x 30 m room"""
    from hector_slam_amd import synth
    return synth.make_scene(n_beams=1081, map_size=1024, levels=6, resolution=0.05, n_build=40, n_query=4, room=(40.0, 30.0), seed=606)


@needs_ref
def test_reference_driver_six_levels_matches_oracle(tmp_path, oracle_mod, deep_scene):
    """the reference driver with numDepth = 6 on a 1024^2 map == the oracle's HectorSlamProcessor loop, which reads the map at
    no NaN coordinate on it: the CPU pin of the run below"""
    sc, steps = deep_scene, 12
    scen, out = str(tmp_path / "s.bin"), str(tmp_path / "o.bin")
    o = make_oracle(oracle_mod, "ho", sc, build=False)
    o.proc_set_thresholds(0.05, 0.02)
    origo = np.array([0.3, -0.1], np.float32) * np.float32(sc.scale_to_map)
    last, poses = np.zeros(3, np.float32), []
    for t in range(steps):
        hint = sc.build_poses[0] if t == 0 else (sc.build_poses[t] - sc.build_poses[t - 1]) + last
        o.proc_update(sc.build_scans[t], hint.astype(np.float32), origo=origo, map_without_matching=(t == 7))
        last, _ = o.proc_last_pose()
        poses.append(last)
    assert o.undefined_reads() == 0 and np.isfinite(poses).all()
    write_scenario(scen, sc, steps, hooks=False)
    run(REF_BIN, scen, out)
    r = read_output(out, steps)
    assert np.array_equal(np.stack(poses).view(np.uint32), r["pose"].view(np.uint32))
    assert len(r["grids"]) == 6 and (r["grids"][5]["sx"], r["grids"][5]["sy"]) == (32, 32)
    for lvl in range(6):
        lo, _ = o.download_level(lvl)
        assert np.array_equal(lo.view(np.uint32), r["grids"][lvl]["val"].view(np.uint32)) and (lo != 0).any(), lvl


@pytest.mark.gpu
def test_dropin_six_levels_on_a_1024_map(tmp_path, deep_scene):
    """numDepth = 6 through the facade, which forwards it untouched (only 3 had ever been run): poses, covariances, the batched
    extension, all six grids and every record the draw / debug hooks saw (20 Hessians per match) carry the reference's bits"""
    if not (os.path.exists(GPU_BIN) and os.path.exists(REF_BIN)):
        pytest.skip("oracle/_ref/slam_driver_{ref,mi355} not prebuilt (run __graft_entry__.build() where "
                    "/root/reference exists)")
    sc, steps = deep_scene, 12
    scen = str(tmp_path / "s.bin")
    write_scenario(scen, sc, steps, hooks=1)
    run(REF_BIN, scen, str(tmp_path / "ref.bin"))
    assert "MI355X resident" in run(GPU_BIN, scen, str(tmp_path / "gpu.bin"))
    r, g = read_output(str(tmp_path / "ref.bin"), steps), read_output(str(tmp_path / "gpu.bin"), steps)
    same = lambda a, b: np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))  # noqa: E731
    assert np.isfinite(r["pose"]).all()
    assert same(r["pose"], g["pose"]) and same(r["cov"], g["cov"]) and same(r["batch"], g["batch"])
    assert len(g["grids"]) == len(r["grids"]) == 6
    for a, b in zip(r["grids"], g["grids"]):
        assert (a["sx"], a["sy"], a["cell"], a["update_index"]) == (b["sx"], b["sy"], b["cell"], b["update_index"])
        assert same(a["val"], b["val"]) and np.array_equal(a["occ"], b["occ"]) and (a["val"] != 0).any()
    ca, cb = parse_log(r["log"]), parse_log(g["log"])
    assert [t for t, _ in ca] == [t for t, _ in cb]
    assert sum(1 for t, _ in ca if t == 8) == (steps - 1) * (3 * 5 + 5)  # (per match 3 on each coarse level, 5 on level 0; one step maps without matching)
    for (t, x), (_, y) in zip(ca, cb):
        assert np.array_equal(x, y), (t, x, y)


@pytest.mark.gpu
def test_dropin_dense_scans(tmp_path):
    """8192-beam scans through the C++ facade (the standalone driver runs on the system HIP runtime, not torch's): in the
    library default they take the exact-order dense matcher -- poses, the batched extension and every grid bit-identical; with
    HSM_PARITY=fast in the environment the multi-workgroup cooperative matcher, within 1e-4"""
    if not (os.path.exists(GPU_BIN) and os.path.exists(REF_BIN)):
        pytest.skip("oracle/_ref drivers not prebuilt")
    from hector_slam_amd import synth
    sc = synth.make_scene(n_beams=8192, map_size=512, levels=3, resolution=0.05, n_build=16, n_query=2,
                          room=(20.0, 15.0), seed=123)
    steps = 12
    scen = str(tmp_path / "s.bin")
    write_scenario(scen, sc, steps, hooks=0, mwm_at=())
    run(REF_BIN, scen, str(tmp_path / "ref.bin"))
    run(GPU_BIN, scen, str(tmp_path / "gpu.bin"))
    r, g = read_output(str(tmp_path / "ref.bin"), steps), read_output(str(tmp_path / "gpu.bin"), steps)
    assert np.abs(r["pose"][:, :2].astype(np.float64) - g["pose"][:, :2]).max() <= 1e-4
    assert ang_diff(r["pose"][:, 2], g["pose"][:, 2]).max() <= 1e-4
    assert np.abs(r["batch"].astype(np.float64) - g["batch"]).max() <= 1e-4
    exact_default = os.environ.get("HSM_PARITY", "auto") in ("auto", "exact")
    if exact_default:
        assert np.array_equal(r["pose"].view(np.uint32), g["pose"].view(np.uint32)) and np.array_equal(r["batch"].view(np.uint32), g["batch"].view(np.uint32))
    for a, b in zip(r["grids"], g["grids"]):
        touched = (a["val"] != 0).sum()
        assert touched > 1000 and (a["val"].view(np.uint32) != b["val"].view(np.uint32)).sum() <= (0 if exact_default else 0.002 * touched)


@pytest.mark.gpu
def test_facade_batch_of_hypotheses_of_one_scan(tmp_path, pyramid_scene):
    """BASELINE configs[2]'s use through the C++ facade: 4096 start estimates that all look at ONE scan (the same DataContainer
    4096 times in matchDataBatch) -- one launch, the start poses and results crossing PCIe once each in pinned memory, the scan
    copied once -- bit-identical to 4096 matchData calls of the reference; the call's time is recorded beside the reference's"""
    import json
    if not (os.path.exists(GPU_BIN) and os.path.exists(REF_BIN)):
        pytest.skip("oracle/_ref drivers not prebuilt")
    sc, steps, N = pyramid_scene, 12, 4096
    scen = str(tmp_path / "s.bin")
    write_scenario(scen, sc, steps, hooks=0)
    res = {}
    for name, binary in (("ref", REF_BIN), ("gpu", GPU_BIN)):
        env = dict(os.environ, SLAM_DRIVER_HYPOTHESES=str(N), SLAM_DRIVER_HYP_OUT=str(tmp_path / f"{name}_hyp.bin"),
                   SLAM_DRIVER_HYP_TIMING=str(tmp_path / f"{name}_hyp.json"))
        r = subprocess.run([binary, scen, str(tmp_path / f"{name}.bin")], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        res[name] = (np.fromfile(tmp_path / f"{name}_hyp.bin", np.float32).reshape(N, 3), json.load(open(tmp_path / f"{name}_hyp.json")))
    (pr, tr), (pg, tg) = res["ref"], res["gpu"]
    assert np.array_equal(pr.view(np.uint32), pg.view(np.uint32)), "facade batch of hypotheses differs from the reference's matchData calls"
    # (on a well-conditioned scene most starts within +-0.3 m / +-0.1 rad reach the SAME fixed point of the reference's iteration, bit
    # for bit; the others are the cases that tell a correct batch from a broadcast of hypothesis 0)
    assert len(np.unique(pr.view(np.uint32), axis=0)) > 8
    out = os.environ.get("HSM_FACADE_HYP_RECORD")
    rec = {"hypotheses": N, "beams": tg["beams"], "facade_matchDataBatch_us": tg["median_us_all_hypotheses"],
           "reference_matchData_calls_us": tr["median_us_all_hypotheses"], "bit_identical": True}
    print(json.dumps(rec))
    if out:
        json.dump(rec, open(out, "w"))
    assert tg["median_us_all_hypotheses"] < tr["median_us_all_hypotheses"]
