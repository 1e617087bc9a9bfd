"""Time the expected-scan cast: 4096 pose hypotheses x 1081 beams (270 degrees, range_max 30 m) on the 3-level 2048^2 map of
the benchmark scene, level 0 and level 2, poses = the scene's trajectory +- the headline perturbation.

Per level, device events around each launch, after warm-up, --repeats times (median, min - max):
  * hsm_cast_scans_device, a wavefront per beam (HSM_CAST_FORM=wave)
  * hsm_cast_scans_device, a lane per beam      (HSM_CAST_FORM=lane)
  * the two-step path: the end points of every beam written to arrays by torch ops, then hsm_ray_distances_device (the fill, the
    ray kernel, and their sum)
  * hsm_ray_distances on the identical rays from host arrays (what a user could do before these entries), host clock, whole call
and the histogram of the walked steps per ray (it says how much the lanes of a lane-per-beam wavefront diverge).  Every device
form is timed twice: ranges only (no hit array, `*_us`) and with the hit points written as well (`*_with_hit_us`) --
hsm_ray_distances always stages and writes the hit points, so its kernel compares with the second.
Prints one JSON line per level.

  python tools/bench_cast_scans.py [--repeats 7] [--batch 4096] [--profile-steps N] [--skip-host] [--short-fans]
  python tools/bench_cast_scans.py --host-rays-only [--profile-steps N]

--host-rays-only: nothing but hsm_ray_distances from host arrays on the same rays (end points from the same torch ops), 1 + 5
calls per level, whole-call times, the hit fraction and a checksum of the distances.  It uses no entry younger than
hsm_ray_distances, so this file, copied into tools/ of a checkout of an earlier commit, times that commit's library in a process
like this tree's; with --profile-steps N it makes N calls per level and nothing else (the run for
`rocprofv3 --kernel-trace --stats`: that commit's ray_distance_kernel on its own).

--short-fans: instead, both shapes of the cast on level 0 for fans of 1 ... 128 beams (the first beams of the table) -- where the
rule that picks the shape by the fan's length (rays.hip) has its threshold.

--profile-steps N: no timing, N launches of every device form and nothing else -- the run to put under
`rocprofv3 --kernel-trace --stats` for the kernels' own times.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_BEAMS = 1081
RANGE_MAX = 30.0
LEVELS = 3


def beam_angles(n=N_BEAMS):
    """the node's table: angle += angle_increment in fp32, 270 degrees"""
    inc = np.float32(np.deg2rad(270.0) / (n - 1))
    t = np.empty(n, np.float32)
    a = np.float32(-np.deg2rad(135.0))
    for i in range(n):
        t[i] = a
        a = np.float32(a + inc)
    return t


def stats(us):
    us = sorted(us)
    return {"median": round(us[len(us) // 2], 1), "min": round(us[0], 1), "max": round(us[-1], 1)}


def end_points(torch, d_poses, d_angles, d_begin, d_end):
    B, n = d_poses.shape[0], d_angles.shape[0]
    a = d_poses[:, 2:3] + d_angles[None, :]
    d_begin.copy_(d_poses[:, None, :2].expand(B, n, 2))
    d_end[..., 0] = d_poses[:, 0:1] + RANGE_MAX * torch.cos(a)
    d_end[..., 1] = d_poses[:, 1:2] + RANGE_MAX * torch.sin(a)


def host_rays_only(args, capi, common, torch, bp, bs, poses, angles):
    m = capi.MapRepMultiMap(common.RESOLUTION, common.MAP_SIZE, common.MAP_SIZE, LEVELS)
    m.setUpdateFactorFree(0.4)
    m.setUpdateFactorOccupied(0.9)
    m.build_map(bp, bs)
    m.synchronize()
    dev = torch.device("cuda", 0)
    B = poses.shape[0]
    d_begin = torch.empty((B, N_BEAMS, 2), dtype=torch.float32, device=dev)
    d_end = torch.empty((B, N_BEAMS, 2), dtype=torch.float32, device=dev)
    end_points(torch, torch.from_numpy(poses).to(dev), torch.from_numpy(angles).to(dev), d_begin, d_end)
    hb, he = d_begin.cpu().numpy().reshape(-1, 2), d_end.cpu().numpy().reshape(-1, 2)
    for lvl in (0, 2):
        host = []
        for _ in range(args.profile_steps or 6):
            t0 = time.perf_counter()
            d, _ = m.ray_distances(lvl, hb, he)
            host.append((time.perf_counter() - t0) * 1e6)
        print(json.dumps({"host_rays_only": True, "level": lvl, "rays": B * N_BEAMS, "calls": len(host),
                          "hsm_ray_distances_host_arrays_whole_call_us": stats(host[1:] or host),
                          "hit_fraction": round(float((d >= 0).mean()), 4), "checksum": float(d.astype(np.float64).sum())}),
              flush=True)
    m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--profile-steps", type=int, default=0)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--short-fans", action="store_true")
    ap.add_argument("--host-rays-only", action="store_true")
    args = ap.parse_args()
    import torch
    from hector_slam_amd import capi
    from hsm_bench import common
    B = args.batch
    bp, bs, truth, init_l0 = common.make_inputs(0, B)[:4]
    poses = np.ascontiguousarray(init_l0[:B], np.float32)
    angles = beam_angles()
    if args.host_rays_only:
        return host_rays_only(args, capi, common, torch, bp, bs, poses, angles)
    maps = {}
    for form in ("wave", "lane"):
        os.environ["HSM_CAST_FORM"] = form
        m = capi.MapRepMultiMap(common.RESOLUTION, common.MAP_SIZE, common.MAP_SIZE, LEVELS)
        m.setUpdateFactorFree(0.4)
        m.setUpdateFactorOccupied(0.9)
        if maps:
            for lvl in range(LEVELS):
                m.upload_level(lvl, *maps["wave"].download_level(lvl))
        else:
            m.build_map(bp, bs)
        m.synchronize()
        maps[form] = m
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_poses = torch.from_numpy(poses).to(dev)
        d_angles = torch.from_numpy(angles).to(dev)
        ranges = {f: torch.empty((B, N_BEAMS), dtype=torch.float32, device=dev) for f in ("wave", "lane", "rays")}
        d_hit = torch.empty((B, N_BEAMS, 2), dtype=torch.float32, device=dev)
        d_begin = torch.empty((B, N_BEAMS, 2), dtype=torch.float32, device=dev)
        d_end = torch.empty((B, N_BEAMS, 2), dtype=torch.float32, device=dev)
    sp = s.cuda_stream

    def cast(form, lvl, n=N_BEAMS, hit=False):
        maps[form].cast_scans_device(lvl, B, d_poses.data_ptr(), d_angles.data_ptr(), n, RANGE_MAX, ranges[form].data_ptr(),
                                     d_hit.data_ptr() if hit else 0, sp)

    def fill():
        with torch.cuda.stream(s):
            end_points(torch, d_poses, d_angles, d_begin, d_end)

    def rays(lvl, hit=False):
        maps["wave"].ray_distances_device(lvl, B * N_BEAMS, d_begin.data_ptr(), d_end.data_ptr(), ranges["rays"].data_ptr(),
                                          d_hit.data_ptr() if hit else 0, stream=sp)

    def timed(fn, repeats):
        for _ in range(2):
            fn()
        s.synchronize()
        out = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            fn()
            e1.record(s)
            e1.synchronize()
            out.append(e0.elapsed_time(e1) * 1e3)
        return out

    if args.short_fans:
        half = (args.repeats + 1) // 2
        for n in (1, 4, 16, 32, 48, 64, 65, 72, 80, 96, 112, 128, 129, 160, 192):
            t = {"wave": [], "lane": []}
            for _ in range(2):
                for form in t:
                    t[form] += timed(lambda: cast(form, 0, n), half)
            print(json.dumps({"level": 0, "poses": B, "beams": n, "cast_wave_us": stats(t["wave"]), "cast_lane_us": stats(t["lane"])}),
                  flush=True)
    for lvl in () if args.short_fans else (0, 2):
        if args.profile_steps:
            fill()
            for _ in range(args.profile_steps):
                for hit in (False, True):
                    cast("wave", lvl, hit=hit)
                    cast("lane", lvl, hit=hit)
                    rays(lvl, hit=hit)
            s.synchronize()
            continue
        # alternate the forms repeat by repeat: other work shares the machine
        t = {k: [] for k in ("wave", "lane", "fill", "rays", "wave_hit", "lane_hit", "rays_hit")}
        half = (args.repeats + 1) // 2
        for _ in range(2):
            t["wave"] += timed(lambda: cast("wave", lvl), half)
            t["lane"] += timed(lambda: cast("lane", lvl), half)
            t["fill"] += timed(fill, half)
            t["rays"] += timed(lambda: rays(lvl), half)
            t["wave_hit"] += timed(lambda: cast("wave", lvl, hit=True), half)
            t["lane_hit"] += timed(lambda: cast("lane", lvl, hit=True), half)
            t["rays_hit"] += timed(lambda: rays(lvl, hit=True), half)
        s.synchronize()
        r_wave, r_lane, r_rays = (ranges[f].cpu().numpy() for f in ("wave", "lane", "rays"))
        res = maps["wave"].map_metadata(lvl)[2]
        cells = np.where(r_wave >= 0, np.rint(r_wave / np.float32(res)), -1).astype(np.int64).reshape(-1)
        edges = [0, 1, 64, 128, 256, 512, 1024, 2048, 5001]
        hist = {"no_hit": int((cells < 0).sum())}
        for lo, hi in zip(edges[:-1], edges[1:]):
            hist[f"hit_{lo}_{hi - 1}_cells"] = int(((cells >= lo) & (cells < hi)).sum())
        out = {"level": lvl, "poses": B, "beams": N_BEAMS, "range_max_m": RANGE_MAX, "rays": B * N_BEAMS, "repeats": len(t["wave"]),
               "cast_wave_us": stats(t["wave"]), "cast_lane_us": stats(t["lane"]),
               "cast_wave_with_hit_us": stats(t["wave_hit"]), "cast_lane_with_hit_us": stats(t["lane_hit"]),
               "two_step_fill_us": stats(t["fill"]), "two_step_ray_kernel_us": stats(t["rays"]),
               "two_step_ray_kernel_with_hit_us": stats(t["rays_hit"]),
               "two_step_total_us": round(stats(t["fill"])["median"] + stats(t["rays"])["median"], 1),
               "wave_and_lane_bits_equal": bool(np.array_equal(r_wave.view(np.uint32), r_lane.view(np.uint32))),
               "two_step_ranges_equal_fraction": round(float((r_rays == r_wave).mean()), 6),  # (torch's sin/cos are not glibc's)
               "hit_distance_histogram": hist}
        if not args.skip_host:
            fill()
            s.synchronize()
            hb, he = d_begin.cpu().numpy().reshape(-1, 2), d_end.cpu().numpy().reshape(-1, 2)
            host = []
            for k in range(3 + 1):
                t0 = time.perf_counter()
                maps["wave"].ray_distances(lvl, hb, he)
                host.append((time.perf_counter() - t0) * 1e6)
            out["hsm_ray_distances_host_arrays_whole_call_us"] = stats(host[1:])
        print(json.dumps(out), flush=True)
    for m in maps.values():
        m.close()


if __name__ == "__main__":
    main()
