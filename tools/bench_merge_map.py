"""Time one pyramid merged into another under a rigid transform (hsm_merge_map), at theta = 0, 0.3 and pi/2:
  * a 3-level 2048^2 pyramid into another of the same geometry
  * a 512^2 local map into an 8192^2 one (one level each)
Three legs per set-up:
  * hsm_merge_map          on the device (direct route: the kernel reads the source's planes)
  * hsm_copy_map           of the same destination pyramid into a twin: the bandwidth yardstick (it moves every cell once)
  * the host route, the only one there was before: hsm_download_level of both contexts for every level, the numpy model of
    tests/merge_cases.py, hsm_upload_level (wall time)
The device calls run on the destination's own stream, which the caller cannot record events on; so the device events sit on a
caller's stream around  [a one-scan hsm_score_batch_device on the destination] [the call] [the same score again], as in
tools/bench_copy_map.py.  The same bracket around a merge that misses the destination, which queues nothing, is timed as well and
reported next to the figures -- it is not subtracted.  The wall time of the call is how long the host needs to queue it.
After the timed repetitions one more merge per angle is held to the numpy model bit for bit (checked).  Medians of --reps;
prints one JSON line per set-up.  Ends itself after --time-limit seconds.

  python tools/bench_merge_map.py [--reps 30] [--setups 2048x3:2048,8192x1:512]
"""
import argparse
import json
import math
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BEAMS, RES = 1081, 0.05
THETAS = (("0", 0.0), ("0.3", 0.3), ("pi/2", math.pi / 2))


def stats(v):
    return {"median": round(float(np.median(v)), 2), "p10": round(float(np.percentile(v, 10)), 2), "p90": round(float(np.percentile(v, 90)), 2)}


def run(dst_size, levels, src_size, reps, warmup, host_reps):
    import torch
    import merge_cases as mc
    from hector_slam_amd import capi, synth
    zero2 = np.zeros(2, np.float32)
    gd, gs = (RES, dst_size, dst_size, levels, (0.5, 0.5)), (RES, src_size, src_size, levels, (0.5, 0.5))

    def ctx(geom, seed):
        m = capi.MapRepMultiMap(RES, geom[1], geom[2], levels)
        m.setUpdateFactorFree(0.4)
        m.setUpdateFactorOccupied(0.9)
        side = min(geom[1] * RES * 0.8, 40.0)
        sc = synth.make_scene(n_beams=BEAMS, map_size=geom[1], levels=levels, resolution=RES, n_build=8, n_query=1,
                              room=(side, side * 0.75), seed=seed)
        for k in range(8):
            scan = np.ascontiguousarray(sc.build_scans[k], np.float32)
            capi._check(m._lib.hsm_retain_scan(m._h, scan.ctypes.data, scan.shape[0], zero2), "hsm_retain_scan")
            m.updateByScan(scan, sc.build_poses[k])
        m.synchronize()
        return m

    dst, src = ctx(gd, 515), ctx(gs, 77)
    twin = capi.MapRepMultiMap(RES, dst_size, dst_size, levels)
    s = torch.cuda.Stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    d_pose = torch.zeros(3, device="cuda:0")
    d_pts = torch.ones((8, 2), device="cuda:0")
    d_out = torch.zeros(1, device="cuda:0")
    miss = np.float32([1e6, 1e6, 0.0])
    torch.cuda.synchronize()

    def bracket(m, fn):
        """-> (device time between the events, wall time of fn)"""
        score = lambda: m.score_batch_device(levels - 1, 1, d_pose.data_ptr(), d_pts.data_ptr(), 0, 8, d_out.data_ptr(), 0, s.cuda_stream)
        score()
        ev[0].record(s)
        t0 = time.perf_counter()
        fn()
        wall = (time.perf_counter() - t0) * 1e6
        score()
        ev[1].record(s)
        s.synchronize()
        m.synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e3, wall

    def transform(theta):  # src's centre a little off dst's, so that no row of cells lines up by accident
        return np.float32([0.37, -0.21, theta])

    def host_route(t):
        t0 = time.perf_counter()
        for lvl in range(levels):
            d_lo, _ = dst.download_level(lvl)
            s_lo, _ = src.download_level(lvl)
            dst.upload_level(lvl, mc.merge_model(d_lo, s_lo, gd, gs, lvl, t)[0])
        return (time.perf_counter() - t0) * 1e6

    t = {k: [] for k in ["bracket_gpu", "copy_gpu", "copy_enqueue"] + [f"merge_{n}_{x}" for n, _ in THETAS for x in ("gpu", "enqueue")]}
    for k in range(reps + warmup):
        for name, theta in THETAS:
            gpu, wall = bracket(dst, lambda: capi.merge_map(dst, src, transform(theta)))
            if k >= warmup:
                t[f"merge_{name}_gpu"].append(gpu)
                t[f"merge_{name}_enqueue"].append(wall)
        gpu, wall = bracket(twin, lambda: twin.copy_map_from(dst))
        if k >= warmup:
            t["copy_gpu"].append(gpu)
            t["copy_enqueue"].append(wall)
        gpu, _ = bracket(dst, lambda: capi.merge_map(dst, src, miss))
        if k >= warmup:
            t["bracket_gpu"].append(gpu)
    same = True
    src_lo = [src.download_level(lvl)[0] for lvl in range(levels)]
    for name, theta in THETAS:
        before = [dst.download_level(lvl)[0] for lvl in range(levels)]
        capi.merge_map(dst, src, transform(theta))
        for lvl in range(levels):
            want = mc.merge_model(before[lvl], src_lo[lvl], gd, gs, lvl, transform(theta))[0]
            same = same and bool(np.array_equal(dst.download_level(lvl)[0].view(np.uint32), want.view(np.uint32)))
    host = [host_route(transform(0.3)) for _ in range(host_reps)]
    boxes = {n: [capi.merge_map_box(dst, src, transform(th), lvl).tolist() for lvl in range(levels)] for n, th in THETAS}
    out = {"case": f"{levels}-level {src_size}^2 into {levels}-level {dst_size}^2", "reps": reps, "host_route_reps": host_reps,
           "dst_pyramid_cells": int(sum((dst_size >> l) ** 2 for l in range(levels))),
           "box_cells": {n: int(sum(max(b[2] - b[0] + 1, 0) * max(b[3] - b[1] + 1, 0) for b in bs)) for n, bs in boxes.items()},
           "bracket_alone_gpu_us": stats(t["bracket_gpu"])}
    for name, _ in THETAS:
        out[f"hsm_merge_map_theta_{name}_gpu_us"] = stats(t[f"merge_{name}_gpu"])
        out[f"hsm_merge_map_theta_{name}_enqueue_us"] = stats(t[f"merge_{name}_enqueue"])
    out["hsm_copy_map_gpu_us"] = stats(t["copy_gpu"])
    out["hsm_copy_map_enqueue_us"] = stats(t["copy_enqueue"])
    out["host_route_download_model_upload_wall_us"] = stats(host)
    out["merges_equal_the_model"] = same
    for m in (dst, src, twin):
        m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=0, help="repetitions of the host route (0: 5, 2 on maps above 4096^2)")
    ap.add_argument("--setups", default="2048x3:2048,8192x1:512", help="dst size x levels : src size")
    ap.add_argument("--time-limit", type=int, default=540)
    args = ap.parse_args()
    signal.alarm(args.time_limit)
    for spec in args.setups.split(","):
        d, src_size = spec.split(":")
        size, levels = (int(v) for v in d.split("x"))
        host_reps = args.host_reps or (5 if size <= 4096 else 2)
        print(json.dumps(run(size, levels, int(src_size), args.reps, args.warmup, host_reps)), flush=True)


if __name__ == "__main__":
    main()
