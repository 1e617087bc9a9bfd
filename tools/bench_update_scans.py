"""Time the device-side map update: one hsm_update_by_scans_device call of 256 posed 1081-beam scans on the 3-level 2048^2
pyramid, against the only route the library had before it -- hsm_retain_scan + hsm_update_by_scan per scan, in a loop.  Wall
time from the call to the return of hsm_synchronize, per scan; the two routes alternate, `--reps` times each, on two contexts
that end with bit-identical maps (checked).  Also:
  * the same call with poses far outside the map: every box is empty, so the figure is what the 1 + 2 * 256 launches cost when
    the whole-level apply grids have nothing to do;
  * closing the loop (match + score + select over one group, then integrate the scan at the winner): winner stays on the
    device (hsm_match_score_batch_device -> hsm_update_by_scans_device, one hsm_synchronize) against download + host update.
Prints one JSON line per case.  Ends itself after --time-limit seconds.

  python tools/bench_update_scans.py [--reps 5] [--profile-steps N]

--profile-steps N: no timing, N device-side calls and nothing else -- the run to put under `rocprofv3 --kernel-trace --stats`.
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
HYP = 256


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
    pts, offs = synth.pack_scans(scans)
    zero2 = np.zeros(2, np.float32)

    def ctx():
        m = capi.MapRepMultiMap(RES, MAP, MAP, LEVELS)
        m.setUpdateFactorFree(0.4)
        m.setUpdateFactorOccupied(0.9)
        return m

    a, b = ctx(), ctx()
    dev = torch.device("cuda", 0)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    d_poses, d_pts, d_offs = t(sc.build_poses), t(pts), t(offs.astype(np.int32))
    far = np.tile(np.float32([[1e5, 1e5, 0.0]]), (SCANS, 1))
    d_far = t(far)
    s = torch.cuda.Stream()
    s.synchronize()

    def device_route(d_p=d_poses):
        a.update_by_scans_device(SCANS, d_p.data_ptr(), d_pts.data_ptr(), d_offs.data_ptr(), 0, BEAMS, None, s.cuda_stream)
        a.synchronize()

    def host_route():
        for p, sp in zip(sc.build_poses, scans):
            capi._check(b._lib.hsm_retain_scan(b._h, sp.ctypes.data, sp.shape[0], zero2), "hsm_retain_scan")
            b.updateByScan(sp, p)
        b.synchronize()

    def wall(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e6

    if args.profile_steps:
        for _ in range(args.profile_steps):
            device_route()
        a.close()
        b.close()
        return
    device_route()  # warm-up: allocations, first launches
    host_route()
    dv, hv, ev = [], [], []
    for _ in range(args.reps):
        dv.append(wall(device_route) / SCANS)
        hv.append(wall(host_route) / SCANS)
    same = all(np.array_equal(x.view(np.uint32), y.view(np.uint32))
               for lvl in range(LEVELS) for x, y in zip(a.download_level(lvl) + (a.download_prob(lvl),), b.download_level(lvl) + (b.download_prob(lvl),)))
    print(json.dumps({"case": f"{SCANS} x {BEAMS}-beam scans, {LEVELS}-level {MAP}^2", "reps": args.reps,
                      "device_entry_us_per_scan": [round(x, 2) for x in dv], "host_loop_us_per_scan": [round(x, 2) for x in hv],
                      "device_entry_median": round(float(np.median(dv)), 2), "host_loop_median": round(float(np.median(hv)), 2),
                      "maps_bit_identical": bool(same)}), flush=True)
    for _ in range(args.reps):
        ev.append(wall(lambda: device_route(d_far)) / SCANS)
    print(json.dumps({"case": "the same call, every pose outside the map (empty boxes: launches and whole-level apply grids only)",
                      "device_entry_us_per_scan": [round(x, 2) for x in ev], "device_entry_median": round(float(np.median(ev)), 2)}), flush=True)
    # closing the loop (the two maps hold the same cells; only the counters differ after the far poses)
    scan = scans[17]
    rng = np.random.default_rng(5)
    hyp = (sc.build_poses[17][None, :] + rng.normal(0, [0.08, 0.08, 0.03], (HYP, 3))).astype(np.float32)
    d_hyp, d_scan = t(hyp), t(scan)
    pose = torch.empty((HYP, 3), dtype=torch.float32, device=dev)
    lh = torch.empty(HYP, dtype=torch.float32, device=dev)
    idx = torch.empty(1, dtype=torch.int32, device=dev)
    best = torch.empty((1, 3), dtype=torch.float32, device=dev)
    s.synchronize()

    def match_score(m):
        m.match_score_batch_device(HYP, d_hyp.data_ptr(), d_scan.data_ptr(), 0, len(scan), pose.data_ptr(), 0, 0, lh.data_ptr(), 0,
                                   1, 0, HYP, idx.data_ptr(), 0, best.data_ptr(), s.cuda_stream)

    def loop_device():
        match_score(a)
        a.update_by_scans_device(1, best.data_ptr(), d_scan.data_ptr(), 0, len(scan), BEAMS, None, s.cuda_stream)
        a.synchronize()

    def loop_host():
        match_score(b)
        s.synchronize()
        p = best.cpu().numpy()[0]
        capi._check(b._lib.hsm_retain_scan(b._h, scan.ctypes.data, scan.shape[0], zero2), "hsm_retain_scan")
        b.updateByScan(scan, p)
        b.synchronize()

    for fn in (loop_device, loop_host):
        for _ in range(5):
            fn()
    ld, lh_ = [], []
    for _ in range(max(args.reps, 5) * 10):
        ld.append(wall(loop_device))
        lh_.append(wall(loop_host))
    print(json.dumps({"case": f"match + score + select over {HYP} hypotheses, then integrate at the winner", "steps": len(ld),
                      "winner_stays_on_device_us": round(float(np.median(ld)), 2), "download_and_host_update_us": round(float(np.median(lh_)), 2),
                      "p10_p90_device": [round(float(np.percentile(ld, 10)), 2), round(float(np.percentile(ld, 90)), 2)],
                      "p10_p90_host": [round(float(np.percentile(lh_, 10)), 2), round(float(np.percentile(lh_, 90)), 2)]}), flush=True)
    a.close()
    b.close()


if __name__ == "__main__":
    main()
