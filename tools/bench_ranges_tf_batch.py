#!/usr/bin/env python
"""Raw LaserScans through the node's default tf path, batched: hsm_ingest_batch_ranges_tf_device on 4096 x 1081 beams with one
laser -> base transform per scan (2048^2 map, 3 levels, the seeded world, query poses and range noise of
tools/bench_ranges_batch.py), one process, legs alternated:
  1   the conversion alone (three launches), event-timed on the caller's stream
  2   the conversion followed by hsm_match_batch_device on its outputs, one stream, event-timed
  3   the same batch through hsm_match_batch_ranges_device, the non-tf conversion + match: the yardstick for what the fp64 path
      adds; and hsm_match_batch_device alone on the container of leg 1, so that both conversions can be read as differences
  4   hsm_match_batch_ranges_tf, the host entry (4 B per beam and 96 B per scan cross), wall clock
  5   the per-scan loop hsm_ingest_laser_scan_tf + hsm_match_ingested over the first --loop-scans scans, wall clock per scan
      (--loop-only runs this leg alone: it needs nothing this tool's commit added, so it also runs on the parent commit)
Prints ONE JSON line: medians, the differences, and whether legs 2, 4 and 5 gave the same poses bit for bit."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GATES = (np.float32(0.4 * 0.4), np.float32(30.0 * 30.0), -1.0, 1.0)  # the node's defaults (HectorMappingRos.cpp:95-108)
CUTOFF = 30.0


def mount_rows(rng, batch):
    """one laser -> base transform per scan: the mount 12 cm ahead of and 30 cm above base_link, base_link attitude (roll,
    pitch within 0.03 rad) changing every scan"""
    T = np.empty((batch, 12), np.float64)
    for b in range(batch):
        r, p = rng.uniform(-0.03, 0.03, 2)
        cr, sr, cp, sp = np.cos(r), np.sin(r), np.cos(p), np.sin(p)
        R = np.array([[cp, sp * sr, sp * cr], [0.0, cr, -sr], [-sp, cp * sr, cp * cr]])
        T[b] = np.concatenate([R, np.array([[0.12], [-0.05], [0.3]])], 1).reshape(12)
    return T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--loop-scans", type=int, default=256)
    ap.add_argument("--loop-only", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from bench_ranges_batch import raw_ranges
    from hector_slam_amd import capi, synth
    from hsm_bench import common as hb
    B, n, levels = hb.BATCH_PER_GPU, hb.N_BEAMS, 3
    bp, bs, truth, _, init = hb.make_inputs(0, B)[:5]
    world = synth.World.make(40.0, 30.0, seed=1234)
    ranges = raw_ranges(world, truth, n)
    T = mount_rows(np.random.default_rng(1241), B)
    m = capi.MapRepMultiMap(hb.RESOLUTION, hb.MAP_SIZE, hb.MAP_SIZE, levels)
    m.setUpdateFactorFree(0.4)
    m.setUpdateFactorOccupied(0.9)
    m.build_map(bp, bs)
    m.synchronize()
    a0, inc = (float(np.float32(x)) for x in synth.SCAN_SHAPES[n])
    geom = (a0, inc, 0.4, 30.0)
    scale = m.getScaleToMap()
    u = lambda x: np.ascontiguousarray(x).view(np.uint32)  # noqa: E731

    def loop(count):
        poses = np.empty((count, 3), np.float32)
        t0 = time.perf_counter()
        for b in range(count):
            m.ingest_laser_scan_tf(ranges[b], *geom, CUTOFF, T[b], *GATES)
            poses[b] = m.match_ingested(init[b])[0]
        return (time.perf_counter() - t0) / count, poses

    line = {"tool": "bench_ranges_tf_batch", "batch": B, "beams": n, "map": f"{hb.MAP_SIZE}^2 x{levels}", "reps": a.reps,
            "loop_scans": a.loop_scans}
    if a.loop_only:
        loop(16)
        t = [loop(a.loop_scans)[0] for _ in range(3)]
        line["per_scan_loop_us_per_scan"] = float(np.median(t)) * 1e6
        ok = True
    else:
        dev = torch.device("cuda")
        d_begin, d_ranges, d_T = (torch.from_numpy(x).to(dev) for x in (init, ranges, T))
        d_pts = torch.empty((B * n, 2), dtype=torch.float32, device=dev)
        d_offs = torch.empty(B + 1, dtype=torch.int32, device=dev)
        d_counts = torch.empty(B, dtype=torch.int32, device=dev)
        d_origo = torch.empty((B, 2), dtype=torch.float32, device=dev)
        d_pose = torch.empty((B, 3), dtype=torch.float32, device=dev)
        d_cov = torch.zeros((B, 9), dtype=torch.float32, device=dev)
        ws_bytes = capi.match_batch_ranges_workspace(B, n)
        d_ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream()
        s = stream.cuda_stream
        torch.cuda.synchronize()

        def convert():
            m.ingest_batch_ranges_tf_device(B, d_ranges.data_ptr(), n, *geom, CUTOFF, d_T.data_ptr(), False, *GATES, scale,
                                            d_pts.data_ptr(), d_offs.data_ptr(), d_counts.data_ptr(), d_origo.data_ptr(), s)

        def match():
            m.match_batch_device(B, d_begin.data_ptr(), d_pts.data_ptr(), d_offs.data_ptr(), n, d_pose.data_ptr(), d_cov.data_ptr(), s)

        def ranges_device():
            m.match_batch_ranges_device(B, d_begin.data_ptr(), d_ranges.data_ptr(), n, *geom, scale, d_pose.data_ptr(),
                                        d_cov.data_ptr(), d_counts.data_ptr(), d_ws.data_ptr(), ws_bytes, s)

        def timed(*calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for c in calls:
                c()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e-3

        t = {k: [] for k in ("1_tf_conversion", "2_tf_conversion_then_match", "3_ranges_device_non_tf", "3_match_batch_device",
                             "4_host_entry")}
        for rep in range(a.reps + 1):  # rep 0 warms every path up (tables, staging blocks) and is not counted
            r1 = timed(convert)
            r2 = timed(convert, match)
            pose2 = d_pose.cpu().numpy()
            kept = int(d_offs[-1].item())
            r3m = timed(match)
            r3 = timed(ranges_device)
            t0 = time.perf_counter()
            pose4 = m.match_batch_ranges_tf(init, ranges, *geom, CUTOFF, T, *GATES)[0]
            r4 = time.perf_counter() - t0
            if rep:
                for k, v in zip(t, (r1, r2, r3, r3m, r4)):
                    t[k].append(v)
        loop(16)
        per_scan, pose5 = loop(a.loop_scans)
        med = {k: float(np.median(v)) for k, v in t.items()}
        ok = bool(np.array_equal(u(pose2), u(pose4)) and np.array_equal(u(pose2[:a.loop_scans]), u(pose5)))
        line.update({
            "median_us": {k: v * 1e6 for k, v in med.items()},
            "per_scan_loop_us_per_scan": per_scan * 1e6,
            "tf_conversion_in_sequence_us": (med["2_tf_conversion_then_match"] - med["3_match_batch_device"]) * 1e6,
            "non_tf_conversion_in_sequence_us": (med["3_ranges_device_non_tf"] - med["3_match_batch_device"]) * 1e6,
            "bytes_MB": {"ranges_read_twice": 2 * ranges.nbytes / 1e6, "unit_vectors": 16 * n / 1e6, "transforms": T.nbytes / 1e6,
                         "endpoints_written": kept * 8 / 1e6},
            "kept_beams": kept,
            "legs_2_4_5_bit_identical": ok,
        })
    s = json.dumps(line)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")
    m.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
