"""Time a pyramid going from one context into another, on a 3-level 2048^2 pyramid and on an 8192^2 map:
  * hsm_copy_map          the whole pyramid, on the device
  * hsm_copy_map_boxes    the cell boxes of ONE 1081-beam update (hsm_take_dirty_bbox of the source), on the device
    each on the direct route (the kernel reads the source's planes) and on the staged route (HSM_COPY_STAGE=1 at the
    destination's hsm_create: rows into the staging patch first, what a copy between two devices does)
  * the host route, the only one there was before: hsm_download_level + hsm_upload_level for every level (wall time)
The copies run on the destination's own stream, which the caller cannot record events on; so the device events sit on a
caller's stream around  [a one-scan hsm_score_batch_device on the destination] [the copy] [the same score again]:  the copy is
ordered behind the first (a writer waits for the matches on callers' streams) and the second behind the copy (a reader waits
for the writers).  The same bracket around a copy of empty boxes, which queues nothing, is timed as well and reported next to the
figures -- it is not subtracted.  The wall time of the call is how long the host needs to queue the copy.
Each repetition first integrates one scan of a loop through the room into the source (synchronised, outside the timed windows).
After the last repetition both destinations' planes must equal the source's (checked).  Medians of --reps; prints one JSON line
per map.  Ends itself after --time-limit seconds.

  python tools/bench_copy_map.py [--reps 30] [--maps 2048x3,8192x1]
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


def run(map_size, levels, reps, warmup, host_reps):
    import torch
    from hector_slam_amd import capi, synth
    sc = synth.make_scene(n_beams=BEAMS, map_size=map_size, levels=levels, resolution=RES, n_build=reps + warmup + 8, n_query=1,
                          room=(40.0, 30.0), seed=515)
    zero2 = np.zeros(2, np.float32)

    def ctx(staged=False):
        if staged:
            os.environ["HSM_COPY_STAGE"] = "1"
        try:
            m = capi.MapRepMultiMap(RES, map_size, map_size, levels)
        finally:
            os.environ.pop("HSM_COPY_STAGE", None)
        m.setUpdateFactorFree(0.4)
        m.setUpdateFactorOccupied(0.9)
        return m

    def integrate(m, k):
        scan = np.ascontiguousarray(sc.build_scans[k], np.float32)
        capi._check(m._lib.hsm_retain_scan(m._h, scan.ctypes.data, scan.shape[0], zero2), "hsm_retain_scan")
        m.updateByScan(scan, sc.build_poses[k])
        m.synchronize()

    src, dst = ctx(), {"direct": ctx(), "staged": ctx(True)}
    for k in range(8):
        integrate(src, k)
    s = torch.cuda.Stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    d_pose = torch.zeros(3, device="cuda:0")
    d_pts = torch.ones((8, 2), device="cuda:0")
    d_out = torch.zeros(1, device="cuda:0")
    empty = np.int32([[0, 0, -1, -1]] * levels)
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

    def host_route(m):
        t0 = time.perf_counter()
        for lvl in range(levels):
            lo, ui = src.download_level(lvl)
            m.upload_level(lvl, lo, ui)
        return (time.perf_counter() - t0) * 1e6

    t = {k: [] for k in ("bracket_gpu",) + tuple(f"{w}_{r}_{x}" for w in ("whole", "boxes") for r in dst for x in ("gpu", "enqueue"))}
    box_cells = []
    for k in range(reps + warmup):
        for r, m in dst.items():  # whole, and dst == src outside the boxes that follow
            gpu, wall = bracket(m, lambda: m.copy_map_from(src))
            if k >= warmup:
                t[f"whole_{r}_gpu"].append(gpu)
                t[f"whole_{r}_enqueue"].append(wall)
        for lvl in range(levels):
            src.take_dirty_bbox(lvl)
        integrate(src, 8 + k)
        boxes = np.stack([src.take_dirty_bbox(lvl) for lvl in range(levels)])
        for r, m in dst.items():
            gpu, wall = bracket(m, lambda: m.copy_map_from(src, boxes))
            if k >= warmup:
                t[f"boxes_{r}_gpu"].append(gpu)
                t[f"boxes_{r}_enqueue"].append(wall)
        gpu, _ = bracket(dst["direct"], lambda: dst["direct"].copy_map_from(src, empty))
        if k >= warmup:
            t["bracket_gpu"].append(gpu)
            box_cells.append(int(sum(max(b[2] - b[0] + 1, 0) * max(b[3] - b[1] + 1, 0) for b in boxes)))
    same = True
    for lvl in range(levels):
        lo, ui = src.download_level(lvl)
        p = src.download_prob(lvl)
        for m in dst.values():
            a, b = m.download_level(lvl)
            same = same and bool(np.array_equal(a.view(np.uint32), lo.view(np.uint32)) and np.array_equal(b, ui) and
                                 np.array_equal(m.download_prob(lvl).view(np.uint32), p.view(np.uint32)))
    host = [host_route(dst["direct"]) for _ in range(host_reps)]
    out = {"case": f"{levels}-level {map_size}^2 pyramid; boxes: one {BEAMS}-beam update", "reps": reps, "host_route_reps": host_reps,
           "pyramid_cells": int(sum((map_size >> l) ** 2 for l in range(levels))), "box_cells_median": int(np.median(box_cells)),
           "bracket_alone_gpu_us": stats(t["bracket_gpu"])}
    for key in sorted(k for k in t if k != "bracket_gpu"):
        out[f"hsm_copy_map{'_boxes' if key.startswith('boxes') else ''}_{key.split('_', 1)[1]}_us"] = stats(t[key])
    out["host_route_download_upload_wall_us"] = stats(host)
    out["destinations_equal_the_source"] = same
    for m in [src] + list(dst.values()):
        m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=0, help="repetitions of the host route (0: --reps, 5 on maps above 4096^2)")
    ap.add_argument("--maps", default="2048x3,8192x1")
    ap.add_argument("--time-limit", type=int, default=540)
    args = ap.parse_args()
    signal.alarm(args.time_limit)
    for spec in args.maps.split(","):
        size, levels = (int(v) for v in spec.split("x"))
        host_reps = args.host_reps or (args.reps if size <= 4096 else min(args.reps, 5))
        print(json.dumps(run(size, levels, args.reps, args.warmup, host_reps)), flush=True)


if __name__ == "__main__":
    main()
