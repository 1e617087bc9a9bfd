#!/usr/bin/env python
"""Raw LaserScans in, poses out: the host-pointer batch entries and the device entry on the bench's 4096 x 1081-beam batch
(2048^2 map, level 0, the same seeded world, query poses and range noise as bench.py), one process, legs alternated:
  A   hsm_match_batch with host endpoints (8 B/beam): on one endpoint array converted once and reused across repetitions (as
      tools/bench_host_batch.py does), and, separately, the node's conversion on the CPU (synth.ranges_to_csr) followed by
      hsm_match_batch on the array it just produced
  B   hsm_match_batch_ranges: the raw ranges (4 B/beam) cross, conversion and match on the device
  C   hsm_match_batch_ranges_device with the ranges in HBM, event-timed, next to hsm_match_batch_device on the same scans
      already ingested (the CSR container of leg A in HBM): the difference is the ingestion's cost inside the sequence; and
      with the ranges in pinned host memory (read once over the link into the workspace)
Prints ONE JSON line: medians, bytes moved, GN it/s, and whether every leg gave the same poses and covariances bit for bit.
The ingestion kernels' own times come from a separate `rocprofv3 --kernel-trace --stats` run of this script (--reps 3)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def raw_ranges(world, truth, n):
    """bench.make_inputs' query scans before the conversion: the same ray caster, noise stream and clamp (pad_to_full)"""
    from hector_slam_amd import synth
    ang = synth.beam_angles(n)
    rng_q = np.random.default_rng(1237)  # hsm_bench.common.make_inputs, rank 0
    out = np.empty((truth.shape[0], n), np.float32)
    for b, p in enumerate(truth):
        r = world.raycast(p, ang)
        r = r + rng_q.normal(0.0, 0.01, size=r.shape)
        out[b] = np.clip(r, 0.45, 30.0 - 0.2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from hector_slam_amd import capi, synth
    from hsm_bench import common as hb
    B, n = hb.BATCH_PER_GPU, hb.N_BEAMS
    bp, bs, truth, init = hb.make_inputs(0, B)[:4]
    world = synth.World.make(40.0, 30.0, seed=1234)
    ranges = raw_ranges(world, truth, n)
    m = capi.MapRepMultiMap(hb.RESOLUTION, hb.MAP_SIZE, hb.MAP_SIZE, 1)
    m.setUpdateFactorFree(0.4)
    m.setUpdateFactorOccupied(0.9)
    m.build_map(bp, bs)
    m.synchronize()
    a0, inc = (float(np.float32(x)) for x in synth.SCAN_SHAPES[n])
    geom = (a0, inc, 0.4, 30.0)
    scale = m.getScaleToMap()

    # device buffers of leg C
    dev = torch.device("cuda")
    d_begin = torch.from_numpy(init).to(dev)
    d_ranges = torch.from_numpy(ranges).to(dev)
    h_ranges = torch.from_numpy(ranges).pin_memory()  # device-accessible pinned host memory
    counts, offs, pts = synth.ranges_to_csr(ranges, *geom, scale)
    d_pts = torch.from_numpy(pts).to(dev)
    d_offs = torch.from_numpy(offs).to(dev)
    d_pose = torch.empty((B, 3), dtype=torch.float32, device=dev)
    d_cov = torch.zeros((B, 9), dtype=torch.float32, device=dev)
    d_counts = torch.empty(B, dtype=torch.int32, device=dev)
    ws_bytes = capi.match_batch_ranges_workspace(B, n)
    d_ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream()
    torch.cuda.synchronize()

    def leg_c(ranges_entry, src=None):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        d_cov.zero_()
        e0.record(stream)
        if ranges_entry:
            r = src if src is not None else d_ranges
            m.match_batch_ranges_device(B, d_begin.data_ptr(), r.data_ptr(), n, *geom, scale, d_pose.data_ptr(), d_cov.data_ptr(),
                                        d_counts.data_ptr(), d_ws.data_ptr(), ws_bytes, stream.cuda_stream)
        else:
            m.match_batch_device(B, d_begin.data_ptr(), d_pts.data_ptr(), d_offs.data_ptr(), n, d_pose.data_ptr(),
                                 d_cov.data_ptr(), stream.cuda_stream)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3, d_pose.cpu().numpy(), d_cov.cpu().numpy()

    t = {k: [] for k in ("A_match_batch", "A_convert", "A_convert_then_match_batch", "B_match_batch_ranges", "C_ranges_device",
                         "C_ranges_device_pinned_input", "C_match_batch_device")}
    res = {}
    for rep in range(a.reps + 1):  # rep 0 warms every path up (tables, staging blocks) and is not counted
        s0 = time.perf_counter()
        pose_a, cov_a = m.match_batch(init, pts, offs)  # the same endpoint array every repetition
        s1 = time.perf_counter()
        c_a, o_a, p_a = synth.ranges_to_csr(ranges, *geom, scale)
        s2 = time.perf_counter()
        pose_f, cov_f = m.match_batch(init, p_a, o_a)  # the array the conversion just produced
        s3 = time.perf_counter()
        pose_b, cov_b, cnt_b = m.match_batch_ranges(init, ranges, *geom)
        s4 = time.perf_counter()
        tc, pose_c, cov_c = leg_c(True)
        cnt_c = d_counts.cpu().numpy()
        tp, pose_p, cov_p = leg_c(True, h_ranges)
        cnt_p = d_counts.cpu().numpy()
        tm, pose_m, cov_m = leg_c(False)
        if rep:
            t["A_match_batch"].append(s1 - s0)
            t["A_convert"].append(s2 - s1)
            t["A_convert_then_match_batch"].append(s3 - s1)
            t["B_match_batch_ranges"].append(s4 - s3)
            t["C_ranges_device"].append(tc)
            t["C_ranges_device_pinned_input"].append(tp)
            t["C_match_batch_device"].append(tm)
        res = {"A": (pose_a, cov_a), "A_converted": (pose_f, cov_f), "B": (pose_b, cov_b), "C": (pose_c, cov_c),
               "C_pinned": (pose_p, cov_p), "C_match": (pose_m, cov_m)}
    u = lambda x: np.ascontiguousarray(x).view(np.uint32)  # noqa: E731
    same = all(np.array_equal(u(res[k][0]), u(res["A"][0])) and np.array_equal(u(res[k][1]), u(res["A"][1])) for k in res)
    med = {k: float(np.median(v)) for k, v in t.items()}
    it = B * m.gn_iterations_per_match()
    total = int(offs[-1])
    line = {
        "tool": "bench_ranges_batch", "batch": B, "beams": n, "map": f"{hb.MAP_SIZE}^2 x1", "reps": a.reps,
        "median_ms": {k: v * 1e3 for k, v in med.items()},
        "GN_it_per_s": {k: it / v for k, v in med.items() if k != "A_convert"},
        "ingestion_overhead_in_sequence_us": (med["C_ranges_device"] - med["C_match_batch_device"]) * 1e6,
        "ingestion_overhead_pinned_input_us": (med["C_ranges_device_pinned_input"] - med["C_match_batch_device"]) * 1e6,
        "bytes_host_to_device_MB": {"A_endpoints": (pts.nbytes + offs.nbytes) / 1e6, "B_ranges": ranges.nbytes / 1e6},
        "bytes_device_ingestion_MB": {"ranges_read_device_input": 2 * ranges.nbytes / 1e6,
                                      "pinned_input_link_read_and_copy_write_read": 3 * ranges.nbytes / 1e6,
                                      "endpoints_written": total * 8 / 1e6, "counts_offsets": 12 * B / 1e6},
        "kept_beams": total,
        "counts_equal_reference": bool(np.array_equal(c_a, cnt_b) and np.array_equal(c_a, cnt_c) and np.array_equal(c_a, cnt_p)),
        "all_legs_bit_identical": bool(same),
        "kernel_last_launch": m.last_launch_config()["kernel"],
    }
    s = json.dumps(line)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")
    m.close()
    return 0 if same and line["counts_equal_reference"] else 1


if __name__ == "__main__":
    sys.exit(main())
