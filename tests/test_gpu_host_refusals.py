"""The refusals of the scan-log, update and raw-scan entries on the MI355X, held to what the library answered before those entries
were rewritten onto argument bundles, and those of the probes, test hooks and group entries to what it answered before they moved
out of the core translation unit, and those of the single-scan conversions (refusal_cases.INGEST) to what it answered before
raw-scan conversion moved to ingest.hip, and those of the batched match, score, covariance, select, window, relocalisation and
ray entries (refusal_cases.MATCHER) to what it answered before the matcher's front door was rewritten onto argument bundles: for every case of tests/refusal_cases.py the status code and the full hsm_last_error()
text equal tests/golden/host_refusals.json (tests/tools/record_host_refusals.py) -- which check wins where two apply, and the entry
each text names.  No case but one queues anything: the case that pins the text of a failing HIP status check converts an empty
scan (one launch of ingest_laser_scan_kernel with n = 0, which writes its count of 0, and the context's ingestion buffers stay
allocated).  The map is empty and stays so.
"""
import json
import os

import pytest

import refusal_cases as rc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "host_refusals.json")


def test_every_refusal_keeps_its_code_and_text():
    import torch
    assert torch.cuda.is_available(), "gpu-marked tests need a HIP device"
    from hector_slam_amd import capi
    capi.load_library()
    with open(GOLDEN) as f:
        want = json.load(f)["cases"]
    case_list = rc.cases()
    assert sorted(want) == sorted(name for name, _, _, _ in case_list), "the case list and the recording differ"
    runner = rc.Runner(capi)
    got = runner.run(case_list)
    assert runner.g.getUpdateIndex(0) == -1, "a refused call updated the map"
    runner.close()
    wrong = {name: (got[name], want[name]) for name in want if got[name] != want[name]}
    assert not wrong, wrong
