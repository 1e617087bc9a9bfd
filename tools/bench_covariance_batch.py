"""Time the batched sigma-point covariance entry (hsm_covariance_batch_device) against the routes the library had before it.

Workload: 4096 hypotheses x 1081 beams on the 3-level 2048^2 pyramid, covariance on level 0, in the default mode and in
HSM_PARITY_FAST.  Medians of --runs (30) runs; the device legs by device events around one launch, the host-synchronous legs of
the earlier routes by the host clock.  One JSON line per mode:

  a  the new entry, one shared scan                       b  the new entry, 4096 distinct scans (CSR)
  c  the earlier route on the shared scan: download the poses, hsm_map_coords_pose per pose, ONE hsm_covariance_for_poses call
  d  the earlier route on distinct scans: hsm_map_coords_pose and one hsm_covariance_for_poses call PER scan, on 256 of them,
     reported per scan (and times 4096 for the batch)
  e  hsm_score_batch_device alone on the same batch (shared scan; CSR as e_csr): the floor -- the new kernel takes seven scores'
     worth of samples

  python tools/bench_covariance_batch.py [--runs 30]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B = 4096
PER_SCAN_CALLS = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    args = ap.parse_args()
    import torch
    from hector_slam_amd import capi
    from hsm_bench import common
    bp, bs, truth, init_l0, _, pts, offs = common.make_inputs(0, B)[:7]
    m = capi.MapRepMultiMap(common.RESOLUTION, common.MAP_SIZE, common.MAP_SIZE, 3)
    m.setUpdateFactorFree(0.4)
    m.setUpdateFactorOccupied(0.9)
    m.build_map(bp, bs)
    m.synchronize()
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    scan = np.ascontiguousarray(pts[offs[0]:offs[1]])
    n = scan.shape[0]
    d_poses, d_scan, d_pts, d_offs = t(init_l0), t(scan), t(pts), t(offs.astype(np.int32))
    cw = torch.empty((B, 9), dtype=torch.float32, device=dev)
    cm = torch.empty((B, 9), dtype=torch.float32, device=dev)
    l7 = torch.empty((B, 7), dtype=torch.float32, device=dev)
    lh = torch.empty(B, dtype=torch.float32, device=dev)
    s = torch.cuda.Stream()

    def new_entry(shared):
        m.covariance_batch_device(0, B, d_poses.data_ptr(), d_scan.data_ptr() if shared else d_pts.data_ptr(),
                                  0 if shared else d_offs.data_ptr(), n if shared else 0, cw.data_ptr(), cm.data_ptr(), l7.data_ptr(),
                                  lh.data_ptr(), s.cuda_stream)

    def score_alone(shared):
        m.score_batch_device(0, B, d_poses.data_ptr(), d_scan.data_ptr() if shared else d_pts.data_ptr(),
                             0 if shared else d_offs.data_ptr(), n if shared else 0, lh.data_ptr(), 0, s.cuda_stream)

    def earlier_shared():
        p = d_poses.cpu().numpy()
        pm = np.stack([m.getMapCoordsPose(0, q) for q in p]).astype(np.float32)
        return m.covariance_for_poses(0, pm, scan)

    def earlier_per_scan():
        p = d_poses[:PER_SCAN_CALLS].cpu().numpy()
        out = []
        for k in range(PER_SCAN_CALLS):
            out.append(m.covariance_for_poses(0, m.getMapCoordsPose(0, p[k])[None], pts[offs[k]:offs[k + 1]]))
        return out

    def device_median_us(fn):
        for _ in range(5):
            fn()
        s.synchronize()
        times = []
        for _ in range(args.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            fn()
            e1.record(s)
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3)
        return float(np.median(times))

    def host_median_us(fn):
        fn()
        times = []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            fn()
            times.append((time.perf_counter() - t0) * 1e6)
        return float(np.median(times))

    for mode_name, mode in (("default", capi.PARITY_AUTO), ("fast", capi.PARITY_FAST)):
        m.set_parity(mode)
        # the new entry gives the earlier route's bits (both sum in the same order in either mode)
        new_entry(True)
        s.synchronize()
        old = earlier_shared()
        same = all(np.array_equal(a.cpu().numpy().view(np.uint32), b.view(np.uint32)) for a, b in zip((cm, cw, l7), old))
        a_us, b_us = device_median_us(lambda: new_entry(True)), device_median_us(lambda: new_entry(False))
        e_us, e_csr_us = device_median_us(lambda: score_alone(True)), device_median_us(lambda: score_alone(False))
        c_us = host_median_us(earlier_shared)
        d_us = host_median_us(earlier_per_scan) / PER_SCAN_CALLS
        print(json.dumps({
            "mode": mode_name, "hypotheses": B, "beams": n, "level": 0, "runs": args.runs,
            "a_new_shared_us": round(a_us, 1), "b_new_distinct_us": round(b_us, 1),
            "c_earlier_shared_wall_us": round(c_us, 1), "d_earlier_per_scan_wall_us": round(d_us, 1),
            "d_earlier_4096_scans_wall_us": round(d_us * B, 1),
            "e_score_alone_us": round(e_us, 1), "e_csr_score_alone_us": round(e_csr_us, 1),
            "a_over_e": round(a_us / e_us, 2), "b_over_e_csr": round(b_us / e_csr_us, 2),
            "a_below_c": bool(a_us < c_us), "b_below_d_batch": bool(b_us < d_us * B),
            "sharing_bought_something": bool(a_us <= 7 * e_us),
            "bits_equal_earlier_route": bool(same),
            "kernel": "covariance_batch_kernel"}), flush=True)
    m.close()


if __name__ == "__main__":
    main()
