"""Time the HOST side of one hsm_match_batch_device call: the argument checks, the plan, the ordering against map updates and the
launch itself, queue only -- the clock stops when the call returns, nothing waits for the kernel inside a timed interval.

Workload: the benchmark's 2048^2 single-level map, 4096 hypotheses of one 1081-beam scan (shared), on a stream of the caller's own
and on the null stream (both take the map reader's ordering: the context's stream is not handed out).  Every call is timed on its
own with the host clock; the stream is drained every --drain calls, outside the timed intervals, so that no call waits for a full
queue.  Prints one JSON line per stream: median, quartiles and the 5th / 95th percentile in microseconds.

To compare two builds of the library, run this once per build in one session (HSM_LIB=<the other library>), the other build
twice: its two medians give the run-to-run spread the first is judged against.

  python tools/bench_match_call.py [--calls 4000] [--drain 8]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B = 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=4000)
    ap.add_argument("--drain", type=int, default=8)
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
    scan = np.ascontiguousarray(pts[offs[0]:offs[1]])
    d_init = torch.from_numpy(np.ascontiguousarray(init_l0)).to(dev)
    d_scan = torch.from_numpy(scan).to(dev)
    pose = torch.empty((B, 3), dtype=torch.float32, device=dev)
    own = torch.cuda.Stream()
    lib = capi.load_library()
    fn = lib.hsm_match_batch_device
    now = time.perf_counter_ns
    for name, stream in (("caller's stream", own.cuda_stream), ("null stream", None)):
        a = (m._h, B, d_init.data_ptr(), d_scan.data_ptr(), None, scan.shape[0], pose.data_ptr(), None, stream)
        for _ in range(50):
            assert fn(*a) == 0
        torch.cuda.synchronize()
        m.synchronize()
        ns = np.empty(args.calls, np.int64)
        for i in range(args.calls):
            t0 = now()
            rc = fn(*a)
            ns[i] = now() - t0
            assert rc == 0
            if i % args.drain == args.drain - 1:
                torch.cuda.synchronize()
                m.synchronize()
        torch.cuda.synchronize()
        m.synchronize()
        q = np.percentile(ns / 1e3, [5, 25, 50, 75, 95])
        print(json.dumps({"entry": "hsm_match_batch_device", "stream": name, "hypotheses": B, "beams": int(scan.shape[0]),
                          "calls": args.calls, "library": os.environ.get("HSM_LIB", "in-tree"),
                          "host_call_us": {"p5": round(q[0], 2), "p25": round(q[1], 2), "median": round(q[2], 2),
                                           "p75": round(q[3], 2), "p95": round(q[4], 2)},
                          "kernel": lib.hsm_last_launch_kernel(m._h).decode()}), flush=True)
    m.close()


if __name__ == "__main__":
    main()
