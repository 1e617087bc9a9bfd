"""Time the map image entries after ONE 1081-beam update, on level 0 of a 3-level 2048^2 pyramid and of an 8192^2 map:
  * hsm_occupancy_grid_device   the whole level into a device grid: the YARDSTICK, the same plane read once, a byte a cell written
  * hsm_map_image_device        the full image (crop = NULL) into device memory; it moves the yardstick's bytes
  * hsm_map_extents_device      the hull of the known cells: the plane read once, 16 bytes written
  * hsm_map_tiles_device        4096 tiles of 64 x 64 at poses along the scene's trajectory
and the routes a user had before them:
  * grid_device + torch         hsm_occupancy_grid_device, then a torch lookup (-1 / 0 / 100 -> 127 / 255 / 0) and flip; for the tiles
                                a torch gather of the same 4096 windows out of that image
  * grid + numpy                hsm_occupancy_grid to the host, then the numpy lookup and flip, or the numpy hull (wall time)
Measuring bracket: two device events on the caller's stream around the call(s), the stream synchronised behind them -- the time
the GPU side takes, event records and the hand-over between the caller's stream and the context's included, for the yardstick and
the new entries alike; the host routes are wall time of the calls.  Every repetition integrates one scan (synchronised, outside
the timed windows) and then times the calls in turn, so the forms alternate and see the same map.  After the last repetition the
image, the box and the tiles must equal the old routes' (checked).  Medians of --reps with p10 / p90.  Prints one JSON line per map.
Ends itself after --time-limit seconds.

  python tools/bench_map_image.py [--reps 30] [--maps 2048x3,8192x1]
"""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BEAMS, RES, TILES, TILE = 1081, 0.05, 4096, 64


def stats(v):
    return {"median": round(float(np.median(v)), 2), "p10": round(float(np.percentile(v, 10)), 2), "p90": round(float(np.percentile(v, 90)), 2)}


def run(map_size, levels, reps, warmup):
    import torch
    from hector_slam_amd import capi, synth
    sc = synth.make_scene(n_beams=BEAMS, map_size=map_size, levels=levels, resolution=RES, n_build=reps + warmup, n_query=1,
                          room=(40.0, 30.0), seed=515)
    zero2 = np.zeros(2, np.float32)
    m = capi.MapRepMultiMap(RES, map_size, map_size, levels)
    m.setUpdateFactorFree(0.4)
    m.setUpdateFactorOccupied(0.9)
    s = torch.cuda.Stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    rng = np.random.default_rng(3)
    poses = sc.build_poses[rng.integers(0, len(sc.build_poses), TILES)].astype(np.float32)
    poses[:, :2] += rng.normal(0.0, 0.5, (TILES, 2)).astype(np.float32)  # matched poses scatter round the trajectory
    with torch.cuda.stream(s):
        d_grid = torch.empty((map_size, map_size), dtype=torch.int8, device="cuda:0")
        d_img = torch.empty((map_size, map_size), dtype=torch.uint8, device="cuda:0")
        d_box = torch.empty(4, dtype=torch.int32, device="cuda:0")
        d_poses = torch.from_numpy(poses).to("cuda:0")
        d_tiles = torch.empty((TILES, TILE, TILE), dtype=torch.uint8, device="cuda:0")
        d_boxes = torch.empty((TILES, 4), dtype=torch.int32, device="cuda:0")
        lut = torch.full((256,), 127, dtype=torch.uint8, device="cuda:0")
        lut[0], lut[100] = 255, 0
        ar = torch.arange(TILE, device="cuda:0")
    s.synchronize()

    def wall(fn):
        t0 = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t0) * 1e6, r

    def events(fn):
        with torch.cuda.stream(s):
            ev[0].record(s)
            r = fn()
            ev[1].record(s)
        s.synchronize()
        return ev[0].elapsed_time(ev[1]) * 1e3, r

    def torch_image():
        m.occupancy_grid_device(0, d_grid.data_ptr(), s.cuda_stream)
        return lut[d_grid.view(torch.uint8).long()].flip(0)

    def torch_tiles(boxes):
        """the same windows gathered out of the torch image (the boxes known: the old route computes them on the host)"""
        img = torch_image()
        rows = (map_size - 1 - boxes[:, 3]).long()[:, None] + ar[None, :]
        cols = boxes[:, 0].long()[:, None] + ar[None, :]
        return img[rows[:, :, None], cols[:, None, :]]

    def numpy_image():
        g = m.occupancy_grid(0)
        return np.where(g == 0, 255, np.where(g == 100, 0, 127)).astype(np.uint8)[::-1]

    def numpy_extents():
        ys, xs = np.nonzero(m.occupancy_grid(0) != -1)
        return (0, 0, -1, -1) if ys.size == 0 else (int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()))

    names = ("grid_device", "image_device", "extents_device", "tiles_device", "image_torch", "tiles_torch", "image_numpy_wall",
             "extents_numpy_wall")
    t = {k: [] for k in names}
    for k in range(reps + warmup):
        scan, pose = np.ascontiguousarray(sc.build_scans[k], np.float32), sc.build_poses[k]
        capi._check(m._lib.hsm_retain_scan(m._h, scan.ctypes.data, scan.shape[0], zero2), "hsm_retain_scan")
        m.updateByScan(scan, pose)
        m.synchronize()
        one = {
            "grid_device": events(lambda: m.occupancy_grid_device(0, d_grid.data_ptr(), s.cuda_stream))[0],
            "image_device": events(lambda: m.map_image_device(0, None, d_img.data_ptr(), s.cuda_stream))[0],
            "extents_device": events(lambda: m.map_extents_device(0, d_box.data_ptr(), s.cuda_stream))[0],
            "tiles_device": events(lambda: m.map_tiles_device(0, TILES, d_poses.data_ptr(), TILE, TILE, d_tiles.data_ptr(),
                                                              d_boxes.data_ptr(), s.cuda_stream))[0],
        }
        one["image_torch"], img_torch = events(torch_image)
        one["tiles_torch"], tiles_torch = events(lambda: torch_tiles(d_boxes))
        one["image_numpy_wall"], img_numpy = wall(numpy_image)
        one["extents_numpy_wall"], box_numpy = wall(numpy_extents)
        if k >= warmup:
            for name in names:
                t[name].append(one[name])
    same = bool(torch.equal(d_img, img_torch) and np.array_equal(d_img.cpu().numpy(), img_numpy)
                and tuple(d_box.cpu().numpy().tolist()) == box_numpy and torch.equal(d_tiles, tiles_torch))
    out = {"case": f"one {BEAMS}-beam update, then level 0 of a {levels}-level {map_size}^2 map", "reps": reps,
           "level_cells": map_size * map_size, "tiles": f"{TILES} of {TILE} x {TILE}", "known_box": list(box_numpy),
           "hsm_occupancy_grid_device_gpu_us": stats(t["grid_device"]), "hsm_map_image_device_gpu_us": stats(t["image_device"]),
           "hsm_map_extents_device_gpu_us": stats(t["extents_device"]), "hsm_map_tiles_device_gpu_us": stats(t["tiles_device"]),
           "grid_device_plus_torch_image_gpu_us": stats(t["image_torch"]), "grid_device_plus_torch_tiles_gpu_us": stats(t["tiles_torch"]),
           "grid_plus_numpy_image_wall_us": stats(t["image_numpy_wall"]), "grid_plus_numpy_extents_wall_us": stats(t["extents_numpy_wall"]),
           "image_over_yardstick": round(float(np.median(t["image_device"]) / np.median(t["grid_device"])), 2),
           "extents_over_yardstick": round(float(np.median(t["extents_device"]) / np.median(t["grid_device"])), 2),
           "results_equal_the_old_routes": same}
    m.close()
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
