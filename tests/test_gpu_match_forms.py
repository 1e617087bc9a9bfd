"""The matcher form the library launches at every site of tests/golden/match_forms.json, on the device: kernel name, the five
hsm_last_launch_config values and hsm_last_launch_parity equal to what the library answered before csrc/match_plan.h existed
(recorded by tests/tools/record_match_forms.py; the sites and the helper that runs them are tests/match_form_sites.py, shared with
the recorder).  Exact comparison.  On a device whose compute-unit count is not the recorded one, the batches given in CUs are
rebuilt from the device's own count and their expected grids scaled by the same rule; the sites whose batch is a plain number
that sits elsewhere among that device's thresholds are left out -- on a 256-CU MI355X nothing is, and the test says so.

And staging: which form a single scan takes decides whether it is read from pinned host memory or from device memory
(MatchPlan::reads_scan_once); the pose does not depend on where the scan lies, bit for bit."""
import json
import os

import numpy as np
import pytest

import match_form_sites as mfs
from support import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "match_forms.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def answers(capi, golden):
    """every portable site run once, grouped by context (the large map is created once per context that needs it)"""
    r = mfs.Runner(capi)
    cu = r.compute_units()
    run = [s for s in golden["sites"] if mfs.portable(s, cu, golden["compute_units"])]
    got, r = mfs.run_all(capi, [{k: v for k, v in s.items() if k not in ("expect", "compute_units")} for s in run])
    return cu, got, r.contexts_created


def test_nothing_is_left_out_on_the_recorded_device(golden, answers):
    cu, got, created = answers
    if cu == golden["compute_units"]:
        assert len(got) == len(golden["sites"])
    assert got and all(n == 1 for n in created.values()), created  # one context per (map, layout, knobs)


@pytest.mark.parametrize("entry", ["batch", "single"])
def test_library_launches_the_recorded_form(golden, answers, entry):
    cu, got, _ = answers
    wrong, seen = [], 0
    for s in golden["sites"]:
        if s["entry"] != entry or s["id"] not in got:
            continue
        seen += 1
        e = dict(s["expect"], config=list(s["expect"]["config"]))
        e["config"][3] = mfs.scaled_grid(s, s["expect"], cu, golden["compute_units"])
        if got[s["id"]] != e:
            wrong.append((s["id"], got[s["id"]], e))
    assert seen > 50 and not wrong, (len(wrong), wrong[:5])


def staging_scene():
    from hector_slam_amd import synth
    return synth.make_scene(n_beams=360, map_size=256, levels=2, resolution=0.1, n_build=30, n_query=2, room=(20.0, 15.0), seed=977)


# one single-scan site per family that hsm_match can reach: (parity, beams, knobs, kernel)
STAGING = [("fast", 1081, {}, "gn_match_kernel"),
           ("auto", 1081, {}, "gn_match_kernel (exact order)"),
           ("auto", 1500, {"HSM_EXACT_DENSE_MIN": 1200}, "gn_match_exact_dense_kernel"),
           ("auto", 1500, {"HSM_EXACT_DENSE_MIN": 1200, "HSM_EXACT_SPEC": 1}, "gn_match_spec_kernel"),
           ("auto", 1081, {"HSM_EXACT_SPEC1": 1}, "gn_match_spec1_kernel"),
           ("fast", 1081, {"HSM_COOP_MIN": 1024}, "gn_match_coop_kernel")]


@pytest.mark.parametrize("parity,n_beams,env,kernel", STAGING, ids=[s[3] for s in STAGING])
def test_pose_does_not_depend_on_where_the_scan_is_staged(capi, monkeypatch, parity, n_beams, env, kernel):
    """hsm_match stages a host scan where the plan says (pinned host memory if the form reads it once); hsm_match_ingested runs the
    same form on the same endpoints from device memory (the ingested container).  Same kernel, same pose and covariance bits."""
    import math
    from hector_slam_amd import synth
    sc = staging_scene()
    for k in mfs.KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    g = capi.MapRepMultiMap(sc.resolution, sc.map_size, sc.map_size, sc.levels, device=0,
                            parity={"auto": capi.PARITY_AUTO, "fast": capi.PARITY_FAST}[parity])
    try:
        g.build_map(sc.build_poses, sc.build_scans)
        a0, inc = -math.pi, 2.0 * math.pi / n_beams
        ang = np.float32(a0) + np.float32(inc) * np.arange(n_beams, dtype=np.float32)
        ranges = np.clip(sc.world.raycast(sc.query_truth[0], ang), 0.45, 29.0).astype(np.float32)
        pts = g.ingest_laser_scan(ranges, a0, inc, 0.4, 30.0)  # the endpoints, as the device container holds them
        assert pts.shape == (n_beams, 2)
        pose_d, cov_d = g.match_ingested(sc.query_init[0])
        assert g.last_launch_config()["kernel"] == kernel, g.last_launch_config()
        pose, cov = g.matchData(sc.query_init[0], pts)
        assert g.last_launch_config()["kernel"] == kernel, g.last_launch_config()
        assert np.array_equal(pose.view(np.uint32), pose_d.view(np.uint32)) and np.array_equal(cov.view(np.uint32), cov_d.view(np.uint32))
        assert not np.array_equal(pose, np.asarray(sc.query_init[0], np.float32))  # (a match that moved, not two poses left where they began)
    finally:
        g.close()
