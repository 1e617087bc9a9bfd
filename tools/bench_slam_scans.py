"""Time HectorSlamProcessor::update for a log of scans: 256 scans of 1081 beams on the 3-level 2048^2 pyramid, queued whole by one
hsm_slam_scans_device call (match, gate and update of every scan on the device, no host wait), against the per-scan host loop
(hsm_match + the gate on the host + hsm_update_by_scan where it lets the scan through: capi.HectorSlamProcessor.update).  Wall
time from the first call to the return of hsm_synchronize, per scan.  Both routes run the same log on two contexts, alternating,
`--reps` times each; every repetition starts from a reset gate (the first scan is integrated) on the map the repetitions before
built.  Run at the reference's thresholds (0.4, 0.13) and at (1.0, 0.3), where two scans in three are rejected: a rejected scan
costs the queued form its gate launch and two launches that return at once, and the host loop nothing.
Prints one JSON line per threshold pair: medians, all repetitions, how many scans were integrated, and whether the two routes
produced the same poses, decisions and maps.  Ends itself after --time-limit seconds.

  python tools/bench_slam_scans.py [--reps 5] [--profile-steps N]

--profile-steps N: no timing, N queued calls and nothing else -- the run to put under `rocprofv3 --kernel-trace --stats`.
"""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SCANS, BEAMS, MAP, LEVELS, RES = 256, 1081, 2048, 3, 0.05
THRESHOLDS = ((0.4, 0.13), (1.0, 0.3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--profile-steps", type=int, default=0)
    ap.add_argument("--time-limit", type=int, default=300)
    args = ap.parse_args()
    signal.alarm(args.time_limit)
    import torch
    from hector_slam_amd import capi, synth
    sc = synth.make_scene(n_beams=BEAMS, map_size=MAP, levels=LEVELS, resolution=RES, n_build=SCANS, n_query=4, room=(40.0, 30.0), seed=909)
    scans = [np.ascontiguousarray(s, np.float32) for s in sc.build_scans]
    poses = np.ascontiguousarray(sc.build_poses, np.float32)
    deltas = np.zeros((SCANS, 3), np.float32)
    deltas[1:] = poses[1:] - poses[:-1]
    pts, offs = synth.pack_scans(scans)
    fmax = np.finfo(np.float32).max

    def processor():
        p = capi.HectorSlamProcessor(RES, MAP, MAP, (0.5, 0.5), LEVELS)
        p.setUpdateFactorFree(0.4)
        p.setUpdateFactorOccupied(0.9)
        return p

    a, b = processor(), processor()
    dev = torch.device("cuda", 0)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    d_start, d_deltas, d_pts, d_offs = t(poses[0]), t(deltas), t(pts), t(offs.astype(np.int32))
    d_pose = torch.zeros((SCANS, 3), dtype=torch.float32, device=dev)
    d_applied = torch.zeros(SCANS, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream()
    s.synchronize()
    host_poses, host_applied = np.zeros((SCANS, 3), np.float32), np.zeros(SCANS, np.int32)

    def queued_route():
        a.mapRep.reset_update_gate()
        a.update_scans_device(SCANS, d_start.data_ptr(), d_deltas.data_ptr(), d_pts.data_ptr(), d_offs.data_ptr(), d_pose.data_ptr(), 0,
                              d_applied.data_ptr(), 0, BEAMS, None, s.cuda_stream)
        a.mapRep.synchronize()

    def host_route():
        b.lastMapUpdatePose = np.array([fmax, fmax, fmax], np.float32)
        pose = poses[0].copy()
        for k in range(SCANS):
            before = b.lastMapUpdatePose
            b.update(scans[k], (pose + deltas[k]).astype(np.float32))
            pose = b.getLastScanMatchPose()
            host_poses[k] = pose
            host_applied[k] = 0 if b.lastMapUpdatePose is before else 1
        b.mapRep.synchronize()

    def wall(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e6

    for thr in THRESHOLDS:
        for p in (a, b):
            p.setMapUpdateMinDistDiff(thr[0])
            p.setMapUpdateMinAngleDiff(thr[1])
        if args.profile_steps:
            for _ in range(args.profile_steps):
                queued_route()
            continue
        queued_route()  # warm-up: allocations, first launches
        host_route()
        qv, hv = [], []
        for _ in range(args.reps):
            qv.append(wall(queued_route) / SCANS)
            hv.append(wall(host_route) / SCANS)
        s.synchronize()
        same_poses = bool(np.array_equal(d_pose.cpu().numpy().view(np.uint32), host_poses.view(np.uint32)))
        same_flags = bool(np.array_equal(d_applied.cpu().numpy(), host_applied))
        same_maps = all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for lvl in range(LEVELS)
                        for x, y in zip(a.mapRep.download_level(lvl) + (a.mapRep.download_prob(lvl),),
                                        b.mapRep.download_level(lvl) + (b.mapRep.download_prob(lvl),)))
        print(json.dumps({"case": f"{SCANS} x {BEAMS}-beam scans, {LEVELS}-level {MAP}^2, thresholds {thr}", "reps": args.reps,
                          "scans_integrated": int(host_applied.sum()),
                          "queued_us_per_scan": [round(x, 2) for x in qv], "host_loop_us_per_scan": [round(x, 2) for x in hv],
                          "queued_median": round(float(np.median(qv)), 2), "host_loop_median": round(float(np.median(hv)), 2),
                          "poses_bit_identical": same_poses, "decisions_equal": same_flags, "maps_bit_identical": bool(same_maps),
                          "final_error_m": round(float(np.linalg.norm(host_poses[-1, :2] - poses[-1, :2])), 4)}), flush=True)
    a.mapRep.close()
    b.mapRep.close()


if __name__ == "__main__":
    main()
