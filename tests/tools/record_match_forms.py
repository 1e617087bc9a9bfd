"""Records tests/golden/match_forms.json: for every launch site of tests/match_form_sites.py, the matcher form the library picks
on this device -- kernel name, the five hsm_last_launch_config values, hsm_last_launch_parity.

The file is the behavioural pin of the host runtime's form selection (tests/test_match_plan.py compares csrc/match_plan.h with it
on the CPU, tests/test_gpu_match_forms.py the library on the device).  It was recorded ONCE, from the commit before match_plan.h
existed, and is never regenerated from the code under test: to record it again, check that commit out and run

    python tests/tools/record_match_forms.py [--out tests/golden/match_forms.json]

Public binding only (MapRepMultiMap, match_batch_device, matchData, last_launch_config, device_info); every launch is a few
milliseconds on an empty map.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "match_forms.json"))
    args = ap.parse_args()
    import match_form_sites as mfs
    from hector_slam_amd import capi
    capi.load_library()
    site_list = mfs.sites()
    t0 = time.time()
    got, runner = mfs.run_all(capi, site_list)
    cu = runner.compute_units()
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    rec = {"recorded_from": commit or os.environ.get("HSM_RECORDED_FROM", ""), "compute_units": cu,
           "sites": [dict(s, compute_units=cu, expect=got[s["id"]]) for s in site_list]}
    with open(args.out, "w") as f:
        f.write("{\n")
        f.write(f' "recorded_from": {json.dumps(rec["recorded_from"])},\n "compute_units": {cu},\n "sites": [\n')
        f.write(",\n".join("  " + json.dumps(s, sort_keys=True) for s in rec["sites"]))
        f.write("\n ]\n}\n")
    kernels = sorted({s["expect"]["kernel"] for s in rec["sites"]})
    print(json.dumps({"sites": len(site_list), "seconds": round(time.time() - t0, 1), "compute_units": cu, "kernels": kernels}))


if __name__ == "__main__":
    main()
