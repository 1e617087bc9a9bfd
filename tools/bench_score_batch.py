"""Time the device-resident weighting step: match + score (+ select over one group) on one stream, against the only route the
library had before hsm_score_batch_device -- match on the device, synchronise, download the poses, getMapCoordsPose per pose on
the host, hsm_likelihood_states, argmax on the host.

Workload: the benchmark's 2048^2 single-level map, 4096 hypotheses of one 1081-beam scan (shared) and 4096 distinct scans
(CSR), in the default mode and in HSM_PARITY_FAST.  Device events over a window of at least --seconds after warm-up; the old
route is host-synchronous, so it is timed with the host clock, twice, alternated with the new one (its two figures give the
run-to-run spread the new route is judged against).  Prints one JSON line per case.

  python tools/bench_score_batch.py [--seconds 1.0] [--profile-steps N]

--profile-steps N: no timing, N steps of every case and nothing else -- the run to put under `rocprofv3 --kernel-trace --stats`
for the score and select kernels' own times.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B = 4096
CHAIN_CYCLES_PER_ADD = 8.5  # reference-order chain, DESIGN.md 8 / profiles/r05


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--profile-steps", type=int, default=0)
    args = ap.parse_args()
    import torch
    from hector_slam_amd import capi
    from hsm_bench import common
    bp, bs, truth, init_l0, _, pts, offs = common.make_inputs(0, B)[:7]
    m = capi.MapRepMultiMap(common.RESOLUTION, common.MAP_SIZE, common.MAP_SIZE, 1)
    m.setUpdateFactorFree(0.4)
    m.setUpdateFactorOccupied(0.9)
    m.build_map(bp, bs)
    m.synchronize()
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    scan = np.ascontiguousarray(pts[offs[0]:offs[1]])
    d_init, d_scan, d_pts, d_offs = t(init_l0), t(scan), t(pts), t(offs.astype(np.int32))
    pose = torch.empty((B, 3), dtype=torch.float32, device=dev)
    lh = torch.empty(B, dtype=torch.float32, device=dev)
    idx = torch.empty(1, dtype=torch.int32, device=dev)
    best = torch.empty(1, dtype=torch.float32, device=dev)
    best_pose = torch.empty(3, dtype=torch.float32, device=dev)
    s = torch.cuda.Stream()
    n = scan.shape[0]
    clock_hz = m.device_info()["clock_khz"] * 1e3

    def new_route(shared, select=True):
        m.match_score_batch_device(B, d_init.data_ptr(), d_scan.data_ptr() if shared else d_pts.data_ptr(),
                                   0 if shared else d_offs.data_ptr(), n, pose.data_ptr(), 0, 0, lh.data_ptr(), 0,
                                   1 if select else 0, 0, B, idx.data_ptr(), best.data_ptr(), best_pose.data_ptr(), s.cuda_stream)

    def match_only(shared):
        m.match_batch_device(B, d_init.data_ptr(), d_scan.data_ptr() if shared else d_pts.data_ptr(),
                             0 if shared else d_offs.data_ptr(), n, pose.data_ptr(), 0, s.cuda_stream)

    def old_route():
        """shared scan only: the library before this entry had no way to score a CSR batch"""
        match_only(True)
        s.synchronize()
        p = pose.cpu().numpy()
        pm = np.stack([m.getMapCoordsPose(0, q) for q in p]).astype(np.float32)
        l = m.likelihood_states(0, pm, scan)
        return int(np.nanargmax(l)), l

    def device_window(fn, seconds):
        """mean microseconds per step over a window of at least `seconds`, by device events"""
        for _ in range(20):
            fn()
        s.synchronize()
        steps, total_ms = 0, 0.0
        chunk = 200
        while total_ms < seconds * 1e3:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(chunk):
                fn()
            e1.record(s)
            e1.synchronize()
            total_ms += e0.elapsed_time(e1)
            steps += chunk
        return total_ms * 1e3 / steps, steps

    def host_window(fn, seconds):
        for _ in range(3):
            fn()
        steps, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < seconds:
            fn()
            steps += 1
        return (time.perf_counter() - t0) * 1e6 / steps, steps

    for mode_name, mode in (("default", capi.PARITY_AUTO), ("fast", capi.PARITY_FAST)):
        m.set_parity(mode)
        if args.profile_steps:
            for shared in (True, False):
                for _ in range(args.profile_steps):
                    new_route(shared)
            s.synchronize()
            continue
        # the winner of the new route is the old route's (default mode: both sum in the reference's order)
        new_route(True)
        s.synchronize()
        old_idx, old_lh = old_route()
        same_bits = bool(np.array_equal(lh.cpu().numpy().view(np.uint32), old_lh.view(np.uint32)))
        same_winner = int(idx.item()) == int(np.flatnonzero(old_lh == np.nanmax(old_lh))[0])
        old_a, steps_old = host_window(old_route, args.seconds)
        new_us, steps = device_window(lambda: new_route(True), args.seconds)
        new_host_us, _ = host_window(lambda: (new_route(True), s.synchronize()), args.seconds)
        old_b, _ = host_window(old_route, args.seconds)
        match_us, _ = device_window(lambda: match_only(True), args.seconds)
        nosel_us, _ = device_window(lambda: new_route(True, select=False), args.seconds)
        chain_floor_us = n * CHAIN_CYCLES_PER_ADD / clock_hz * 1e6
        print(json.dumps({
            "case": "shared scan", "mode": mode_name, "hypotheses": B, "beams": n, "steps": steps,
            "match_score_select_us": round(new_us, 2), "match_score_us": round(nosel_us, 2), "match_only_us": round(match_us, 2),
            "score_us_by_difference": round(nosel_us - match_us, 2), "select_us_by_difference": round(new_us - nosel_us, 2),
            "match_score_select_host_sync_us": round(new_host_us, 2),
            "old_route_us": [round(old_a, 1), round(old_b, 1)], "old_route_steps": steps_old,
            "old_route_spread_us": round(abs(old_a - old_b), 1),
            "not_slower_than_old_route_plus_spread": bool(new_host_us <= min(old_a, old_b) + abs(old_a - old_b)),
            "likelihood_bits_equal_old_route": same_bits, "winner_equals_old_route": same_winner,
            "chain_floor_us_per_hypothesis": round(chain_floor_us, 2) if mode_name == "default" else None,
            "kernel": capi.load_library().hsm_last_launch_kernel(m._h).decode()}), flush=True)
        new_us, steps = device_window(lambda: new_route(False), args.seconds)
        match_us, _ = device_window(lambda: match_only(False), args.seconds)
        nosel_us, _ = device_window(lambda: new_route(False, select=False), args.seconds)
        print(json.dumps({
            "case": "4096 distinct scans (CSR)", "mode": mode_name, "hypotheses": B, "beams": n, "steps": steps,
            "match_score_select_us": round(new_us, 2), "match_score_us": round(nosel_us, 2), "match_only_us": round(match_us, 2),
            "score_us_by_difference": round(nosel_us - match_us, 2), "select_us_by_difference": round(new_us - nosel_us, 2),
            "old_route_us": None}), flush=True)
    m.close()


if __name__ == "__main__":
    main()
