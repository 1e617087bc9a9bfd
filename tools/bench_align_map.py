"""Time the extraction of a level's occupied cells as a point set (hsm_occupied_points_device) and the alignment of one map to
another (hsm_align_map), on level 0 of
  * a 3-level 2048^2 pyramid
  * an 8192^2 map (one level)
each after eight 1081-beam scans of a synth scene, into which 23 straight walls of 30 m, 1 m apart, are then drawn on every level
(hsm_upload_level): the scans alone leave 3 651 occupied cells on level 0, too few for a point set of 16 000.  Per set-up:
  * hsm_occupied_points_device  device events on the caller's stream around the call: every = 1 without a cap that bites (both
                                passes read the whole plane)
  * hsm_occupancy_grid_device   of the same level, in the same run: the yardstick, the same plane read once
  * hsm_align_map               the whole synchronous call (wall time) for windows of 1 089 and 35 301 poses at about 1 000 and
                                about 16 000 points, dst a copy of src (hsm_copy_map)
  * the route before it         hsm_download_level + numpy (occupied cells, thinning, points) + hsm_relocalize, wall time
A call of hsm_align_map whose point count misses its target by more than 10 % ends the run with an error.
After the timed repetitions the extraction is held to the numpy model of tests/points_cases.py bit for bit, and hsm_align_map to
the route before it (checked).  Medians of --reps; prints one JSON line per set-up.  Ends itself after --time-limit seconds.

  python tools/bench_align_map.py [--reps 30] [--setups 2048x3,8192x1]
"""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BEAMS, RES = 1081, 0.05
WINDOWS = ((1089, (5, 5, 4)), (35301, (20, 20, 10)))
STEP = (0.05, 0.05, 0.01)
POINTS = (1000, 16000)
K = 8


def stats(v):
    return {"median": round(float(np.median(v)), 2), "p10": round(float(np.percentile(v, 10)), 2), "p90": round(float(np.percentile(v, 90)), 2)}


def run(size, levels, reps, warmup, host_reps):
    import torch
    import points_cases as pc
    from hector_slam_amd import capi, synth
    zero2 = np.zeros(2, np.float32)
    geom = (RES, size, size, levels, (0.5, 0.5))
    src = capi.MapRepMultiMap(RES, size, size, levels)
    src.setUpdateFactorFree(0.4)
    src.setUpdateFactorOccupied(0.9)
    side = min(size * RES * 0.8, 40.0)
    sc = synth.make_scene(n_beams=BEAMS, map_size=size, levels=levels, resolution=RES, n_build=8, n_query=1, room=(side, side * 0.75),
                          seed=515)
    for k in range(8):
        scan = np.ascontiguousarray(sc.build_scans[k], np.float32)
        capi._check(src._lib.hsm_retain_scan(src._h, scan.ctypes.data, scan.shape[0], zero2), "hsm_retain_scan")
        src.updateByScan(scan, sc.build_poses[k])
    src.synchronize()
    for lvl in range(levels):  # the walls: rows of occupied cells across the room, the same world lines on every level
        plane, stamps = src.download_level(lvl)
        scale_l = 1.0 / (RES * 2 ** lvl)
        half = (size >> lvl) / 2.0
        x0, x1 = int(half - 15.0 * scale_l), int(half + 15.0 * scale_l)
        for wall in range(-11, 12):
            plane[int(half + wall * scale_l), x0:x1] = 2.0
        src.upload_level(lvl, plane, stamps)
    dst = capi.MapRepMultiMap(RES, size, size, levels)
    dst.copy_map_from(src)
    dst.synchronize()
    lo = src.download_level(0)[0]
    occupied = len(pc.kept_cells(lo, None, 1))
    affine, scale = pc.world_from_map(geom, 0), pc.scale_to_map(geom)

    s = torch.cuda.Stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    cells = size * size
    d_pts = torch.zeros((occupied + 8, 2), dtype=torch.float32, device="cuda:0")
    d_cnt = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    ws_bytes = capi.MapRepMultiMap.occupied_points_workspace(cells)
    d_ws = torch.zeros(ws_bytes // 4, dtype=torch.int32, device="cuda:0")
    d_grid = torch.zeros(cells, dtype=torch.int8, device="cuda:0")
    torch.cuda.synchronize()

    def timed(fn):
        ev[0].record(s)
        fn()
        ev[1].record(s)
        s.synchronize()
        src.synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e3

    legs = {
        "hsm_occupied_points_device_gpu_us": lambda: src.occupied_points_device(0, None, 1, occupied + 8, d_pts.data_ptr(), d_cnt.data_ptr(),
                                                                                d_ws.data_ptr(), ws_bytes, s.cuda_stream),
        "hsm_occupancy_grid_device_gpu_us": lambda: src.occupancy_grid_device(0, d_grid.data_ptr(), s.cuda_stream),
    }
    t = {name: [] for name in legs}
    for k in range(reps + warmup):
        for name, fn in legs.items():
            us = timed(fn)
            if k >= warmup:
                t[name].append(us)
    legs["hsm_occupied_points_device_gpu_us"]()
    s.synchronize()
    want, want_counts = pc.occupied_points_model(lo, None, 1, occupied + 8, affine, scale)
    got = d_pts.cpu().numpy()[:occupied]
    same = tuple(d_cnt.cpu().numpy().tolist()) == want_counts and bool(np.array_equal(got.view(np.uint32), want.view(np.uint32)))

    out = {"case": f"level 0 of a {levels}-level {size}^2 pyramid", "reps": reps, "host_route_reps": host_reps, "cells": cells,
           "occupied_cells": occupied}
    for name in legs:
        out[name] = stats(t[name])
    out["extraction_over_yardstick"] = round(out["hsm_occupied_points_device_gpu_us"]["median"] / out["hsm_occupancy_grid_device_gpu_us"]["median"], 2)
    out["extraction_equals_the_model"] = same

    guess = np.float32([0.07, -0.04, 0.015])
    aligned = True
    for n_target in POINTS:
        every = max(1, occupied // n_target)
        cap = min(n_target, capi.MAX_ALIGN_POINTS)
        for W, half in WINDOWS:
            args = (0, None, every, cap, levels - 1, guess, STEP, half, K)
            wall, host = [], []
            for k in range(reps + warmup):
                t0 = time.perf_counter()
                r = dst.align_map_from(src, *args)
                if k >= warmup:
                    wall.append((time.perf_counter() - t0) * 1e6)
            for k in range(host_reps):
                t0 = time.perf_counter()
                plane = src.download_level(0)[0]
                pts = pc.cell_points(pc.kept_cells(plane, None, every)[:cap], affine, scale)
                h = dst.relocalize(levels - 1, guess, STEP, half, K, pts, want_cov=False)
                host.append((time.perf_counter() - t0) * 1e6)
            n = int(r[3][0])
            if abs(n - n_target) > 0.1 * n_target:
                raise SystemExit(f"{n} points where about {n_target} were to be timed: the map holds {occupied} occupied cells")
            aligned = aligned and r[4] == h["best_index"] and bool(np.array_equal(r[0].view(np.uint32), h["best_pose"].view(np.uint32)))
            out[f"hsm_align_map_W{W}_n{n}_wall_us"] = stats(wall)
            out[f"download_numpy_relocalize_W{W}_n{n}_wall_us"] = stats(host)
    out["align_equals_the_route_before_it"] = aligned
    src.close()
    dst.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=0, help="repetitions of the route before it (0: 5, 2 on maps above 4096^2)")
    ap.add_argument("--setups", default="2048x3,8192x1", help="size x levels")
    ap.add_argument("--time-limit", type=int, default=540)
    args = ap.parse_args()
    signal.alarm(args.time_limit)
    for spec in args.setups.split(","):
        size, levels = (int(v) for v in spec.split("x"))
        host_reps = args.host_reps or (5 if size <= 4096 else 2)
        print(json.dumps(run(size, levels, args.reps, args.warmup, host_reps)), flush=True)


if __name__ == "__main__":
    main()
