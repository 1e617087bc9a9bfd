"""Records tests/golden/host_refusals.json: for every case of tests/refusal_cases.py, the status code and the full
hsm_last_error() text the library answers with.

The file pins the refusals of the scan-log, update and raw-scan entries across their rewrite onto argument bundles, and those of the
probes, test hooks and group entries across their move out of the core translation unit, and those of the batched match, score,
covariance, window and ray entries across the matcher's rewrite onto bundles (tests/test_gpu_host_refusals.py replays
the cases against the library under test).  It is recorded on the device from the commit BEFORE such a change, all cases at once
-- the cases of an earlier recording come out again and must come out unchanged (`recorded_from` keeps the earlier revisions) --
and never regenerated from the code under test: to record it again, check that commit out (or build its library and name it in
HSM_LIB), copy tests/refusal_cases.py and this file into it and run

    python tests/tools/record_host_refusals.py [--out tests/golden/host_refusals.json]

A case the library accepts aborts the recording: every case of the list must refuse.  Nothing is queued; well under a second.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "host_refusals.json"))
    args = ap.parse_args()
    import refusal_cases as rc
    from hector_slam_amd import capi
    capi.load_library()
    case_list = rc.cases()
    runner = rc.Runner(capi)
    got = runner.run(case_list)
    runner.close()
    accepted = [name for name, _, _, _ in case_list if got[name]["code"] == 0]
    if accepted:
        sys.exit(f"accepted, not refused: {accepted}")
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    with open(args.out, "w") as f:
        f.write("{\n")
        f.write(f' "recorded_from": {json.dumps(commit or os.environ.get("HSM_RECORDED_FROM", ""))},\n "cases": {{\n')
        f.write(",\n".join(f"  {json.dumps(name)}: {json.dumps(got[name], sort_keys=True)}" for name, _, _, _ in case_list))
        f.write("\n }\n}\n")
    print(json.dumps({"cases": len(case_list), "codes": sorted({v["code"] for v in got.values()})}))


if __name__ == "__main__":
    main()
