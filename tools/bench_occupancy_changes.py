"""Time the export of the published grid after ONE 1081-beam update, on a 3-level 2048^2 pyramid and on an 8192^2 map:
  * hsm_occupancy_grid             the whole level: convert, copy sx * sy bytes to the host, wait (wall time of the call)
  * hsm_occupancy_changes          the changed box only, into a host grid (wall time of the call)
  * hsm_occupancy_changes_device   the changed box only, into a device grid: device events around the call on the caller's
                                   stream (the time the GPU spends, the host waits for nothing) and the wall time of the enqueue
  * hsm_occupancy_grid_device      the whole level into a device grid (events)
Each repetition integrates one scan of a loop through the room (hsm_retain_scan + hsm_update_by_scan, synchronised, outside the
timed windows) on two contexts -- one consumed through the host form, one through the device form -- and then times the calls
in turn, so the forms alternate and see the same update.  After the last repetition the grids kept by both consumers must equal
the full export (checked).  Level 0 only: it is the level the node publishes.  Prints one JSON line per map.  Ends itself after
--time-limit seconds.

  python tools/bench_occupancy_changes.py [--reps 30] [--maps 2048x3,8192x1]
"""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BEAMS, RES = 1081, 0.05


def stats(v):
    return {"median": round(float(np.median(v)), 2), "p10": round(float(np.percentile(v, 10)), 2), "p90": round(float(np.percentile(v, 90)), 2)}


def run(map_size, levels, reps, warmup):
    import torch
    from hector_slam_amd import capi, synth
    sc = synth.make_scene(n_beams=BEAMS, map_size=map_size, levels=levels, resolution=RES, n_build=reps + warmup, n_query=1,
                          room=(40.0, 30.0), seed=515)
    zero2 = np.zeros(2, np.float32)

    def ctx():
        m = capi.MapRepMultiMap(RES, map_size, map_size, levels)
        m.setUpdateFactorFree(0.4)
        m.setUpdateFactorOccupied(0.9)
        return m

    host, devc = ctx(), ctx()
    host_grid = np.empty((map_size, map_size), np.int8)
    d_grid = torch.empty((map_size, map_size), dtype=torch.int8, device="cuda:0")
    d_full = torch.empty((map_size, map_size), dtype=torch.int8, device="cuda:0")
    d_box = torch.empty(4, dtype=torch.int32, device="cuda:0")
    s = torch.cuda.Stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    host.occupancy_changes(0, host_grid)  # the first export of a level is all of it: not what is timed
    devc.occupancy_changes_device(0, d_grid.data_ptr(), 0, s.cuda_stream)
    s.synchronize()

    def wall(fn):
        t0 = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t0) * 1e6, r

    def events(fn):
        ev[0].record(s)
        t0 = time.perf_counter()
        fn()
        enqueue = (time.perf_counter() - t0) * 1e6
        ev[1].record(s)
        s.synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e3, enqueue

    t = {k: [] for k in ("grid", "changes", "changes_device_gpu", "changes_device_enqueue", "grid_device_gpu")}
    box_cells = []
    for k in range(reps + warmup):
        scan, pose = np.ascontiguousarray(sc.build_scans[k], np.float32), sc.build_poses[k]
        for m in (host, devc):
            capi._check(m._lib.hsm_retain_scan(m._h, scan.ctypes.data, scan.shape[0], zero2), "hsm_retain_scan")
            m.updateByScan(scan, pose)
            m.synchronize()
        full_us, full = wall(lambda: host.occupancy_grid(0))
        changes_us, box = wall(lambda: host.occupancy_changes(0, host_grid))
        gpu_us, enqueue_us = events(lambda: devc.occupancy_changes_device(0, d_grid.data_ptr(), d_box.data_ptr(), s.cuda_stream))
        full_gpu_us, _ = events(lambda: devc.occupancy_grid_device(0, d_full.data_ptr(), s.cuda_stream))
        if k < warmup:
            continue
        t["grid"].append(full_us)
        t["changes"].append(changes_us)
        t["changes_device_gpu"].append(gpu_us)
        t["changes_device_enqueue"].append(enqueue_us)
        t["grid_device_gpu"].append(full_gpu_us)
        box_cells.append(int(max(box[2] - box[0] + 1, 0)) * int(max(box[3] - box[1] + 1, 0)))
    same = bool(np.array_equal(host_grid, full) and np.array_equal(d_grid.cpu().numpy(), full) and np.array_equal(d_full.cpu().numpy(), full))
    out = {"case": f"one {BEAMS}-beam update, then the export of level 0 of a {levels}-level {map_size}^2 map", "reps": reps,
           "level_cells": map_size * map_size, "box_cells_median": int(np.median(box_cells)),
           "hsm_occupancy_grid_wall_us": stats(t["grid"]), "hsm_occupancy_changes_wall_us": stats(t["changes"]),
           "hsm_occupancy_changes_device_gpu_us": stats(t["changes_device_gpu"]),
           "hsm_occupancy_changes_device_enqueue_wall_us": stats(t["changes_device_enqueue"]),
           "hsm_occupancy_grid_device_gpu_us": stats(t["grid_device_gpu"]), "grids_equal_the_full_export": same}
    host.close()
    devc.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--maps", default="2048x3,8192x1")
    ap.add_argument("--time-limit", type=int, default=300)
    args = ap.parse_args()
    signal.alarm(args.time_limit)
    for spec in args.maps.split(","):
        size, levels = (int(v) for v in spec.split("x"))
        print(json.dumps(run(size, levels, args.reps, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
