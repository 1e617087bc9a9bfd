"""Time the map window moving by 64 level-0 cells on both axes, on a 3-level 2048^2 pyramid and on an 8192^2 map:
  (a) hsm_shift_map                on the device, in place
  (b) the route there was before:  hsm_download_level, a numpy roll (with the cells that scroll in cleared) and hsm_upload_level
                                   for every level, into a second context created at the new start (wall time)
  and hsm_copy_map of the same pyramid into another context, next to them: it moves the same planes once, without the staging trip.
The move runs on the context's own stream, which the caller cannot record events on; so, as tools/bench_copy_map.py does, the
device events sit on a caller's stream around  [a one-scan hsm_score_batch_device] [the call] [the same score again].  The same
bracket around a zero move, which queues nothing, is reported next to the figures -- it is not subtracted.  The wall time of the
call is how long the host needs to queue it.  The window moves there and back in turn (the timed call is always a move by 64
cells on both axes); after the last repetition the planes must equal the numpy model's (checked).  Medians of --reps; prints one
JSON line per map.  Ends itself after --time-limit seconds.

  python tools/bench_shift_map.py [--reps 30] [--maps 2048x3,8192x1]
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

BEAMS, RES, CELLS = 1081, 0.05, 64


def stats(v):
    return {"median": round(float(np.median(v)), 2), "p10": round(float(np.percentile(v, 10)), 2), "p90": round(float(np.percentile(v, 90)), 2)}


def roll(lo, st, dx, dy):
    """the host's move of one level: new(y, x) = old(y - dy, x - dx), cleared where that cell does not exist"""
    out_lo, out_st = np.zeros_like(lo), np.full_like(st, -1)
    sy, sx = lo.shape
    x0, x1, y0, y1 = max(dx, 0), sx + min(dx, 0), max(dy, 0), sy + min(dy, 0)
    out_lo[y0:y1, x0:x1] = lo[y0 - dy:y1 - dy, x0 - dx:x1 - dx]
    out_st[y0:y1, x0:x1] = st[y0 - dy:y1 - dy, x0 - dx:x1 - dx]
    return out_lo, out_st


def run(map_size, levels, reps, warmup, host_reps):
    import torch
    from hector_slam_amd import capi, synth
    sc = synth.make_scene(n_beams=BEAMS, map_size=map_size, levels=levels, resolution=RES, n_build=8, n_query=1,
                          room=(40.0, 30.0), seed=515)
    zero2 = np.zeros(2, np.float32)

    def ctx(start=(0.5, 0.5)):
        m = capi.MapRepMultiMap(RES, map_size, map_size, levels, startCoords=start)
        m.setUpdateFactorFree(0.4)
        m.setUpdateFactorOccupied(0.9)
        return m

    g, other = ctx(), ctx()
    for k in range(8):
        scan = np.ascontiguousarray(sc.build_scans[k], np.float32)
        capi._check(g._lib.hsm_retain_scan(g._h, scan.ctypes.data, scan.shape[0], zero2), "hsm_retain_scan")
        g.updateByScan(scan, sc.build_poses[k])
    g.synchronize()
    before = [g.download_level(lvl) for lvl in range(levels)]
    k = CELLS >> (levels - 1)
    assert k << (levels - 1) == CELLS
    home, away = g.map_start(), g.start_for_shift(k, k)
    s = torch.cuda.Stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    d_pose, d_pts, d_out = torch.zeros(3, device="cuda:0"), torch.ones((8, 2), device="cuda:0"), torch.zeros(1, device="cuda:0")
    torch.cuda.synchronize()

    def bracket(m, fn):
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

    t = {key: [] for key in ("shift_gpu", "shift_enqueue", "copy_gpu", "copy_enqueue", "bracket_gpu")}
    moves = 0
    for i in range(reps + warmup):
        to = away if moves % 2 == 0 else home
        gpu, wall = bracket(g, lambda: g.shift_map(to))
        moves += 1
        other.shift_map(to)   # (a copy needs the same offsets on both sides; not timed)
        other.synchronize()
        cgpu, cwall = bracket(other, lambda: other.copy_map_from(g))
        bgpu, _ = bracket(g, lambda: g.shift_map(g.map_start()))
        if i >= warmup:
            t["shift_gpu"].append(gpu)
            t["shift_enqueue"].append(wall)
            t["copy_gpu"].append(cgpu)
            t["copy_enqueue"].append(cwall)
            t["bracket_gpu"].append(bgpu)
    # the model of what the planes hold now: every move there clears a border, every move back another
    want = before
    for i in range(moves):
        d = CELLS if i % 2 == 0 else -CELLS
        want = [roll(lo, st, d >> lvl, d >> lvl) for lvl, (lo, st) in enumerate(want)]
    same = True
    for lvl in range(levels):
        lo, st = g.download_level(lvl)
        same = same and bool(np.array_equal(lo.view(np.uint32), want[lvl][0].view(np.uint32)) and np.array_equal(st, want[lvl][1]))
    # (b) the route before: download, roll, upload into a context created at the other start
    cur, new = (away, home) if moves % 2 else (home, away)
    d = -CELLS if moves % 2 else CELLS
    dst = ctx((float(new[0]), float(new[1])))
    host = []
    for _ in range(host_reps):
        t0 = time.perf_counter()
        for lvl in range(levels):
            lo, st = g.download_level(lvl)
            dst.upload_level(lvl, *roll(lo, st, d >> lvl, d >> lvl))
        host.append((time.perf_counter() - t0) * 1e6)
    g.shift_map(new)
    for lvl in range(levels):
        (a, b), (c, e) = g.download_level(lvl), dst.download_level(lvl)
        same = same and bool(np.array_equal(a.view(np.uint32), c.view(np.uint32)) and np.array_equal(b, e) and
                             np.array_equal(g.download_prob(lvl).view(np.uint32), dst.download_prob(lvl).view(np.uint32)) and
                             g.level_info(lvl) == dst.level_info(lvl))
    out = {"case": f"{levels}-level {map_size}^2 pyramid moved by {CELLS} level-0 cells on both axes", "reps": reps, "host_route_reps": host_reps,
           "pyramid_cells": int(sum((map_size >> l) ** 2 for l in range(levels))),
           "bracket_alone_gpu_us": stats(t["bracket_gpu"]),
           "hsm_shift_map_gpu_us": stats(t["shift_gpu"]), "hsm_shift_map_enqueue_us": stats(t["shift_enqueue"]),
           "hsm_copy_map_gpu_us": stats(t["copy_gpu"]), "hsm_copy_map_enqueue_us": stats(t["copy_enqueue"]),
           "host_route_download_roll_upload_wall_us": stats(host),
           "moved_planes_equal_the_model_and_the_host_route": same}
    for m in (g, other, dst):
        m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=0, help="repetitions of the host route (0: --reps, 3 on maps above 4096^2)")
    ap.add_argument("--maps", default="2048x3,8192x1")
    ap.add_argument("--time-limit", type=int, default=540)
    args = ap.parse_args()
    signal.alarm(args.time_limit)
    for spec in args.maps.split(","):
        size, levels = (int(v) for v in spec.split("x"))
        host_reps = args.host_reps or (args.reps if size <= 4096 else min(args.reps, 3))
        print(json.dumps(run(size, levels, args.reps, args.warmup, host_reps)), flush=True)


if __name__ == "__main__":
    main()
