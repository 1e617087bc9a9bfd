"""Time the window search behind hsm_relocalize_device on the 3-level 2048^2 map of the benchmark scene with a 1081-beam scan.

Device events around each launch on one stream, after warm-up, --repeats times; every figure is the median with its p10 - p90
spread (one device, one run: other work shares the machine).  One JSON line per measurement:

  (a) window score, W in {1 089, 4 225, 35 301, 269 001}, levels 2 and 0:
        hsm_score_window_device with a lane per hypothesis (HSM_WINDOW_FORM=lane), with a wavefront per hypothesis (=wave), and
        the route that existed before: the window's poses filled by torch ops, then hsm_score_batch_device with the shared scan
        (the fill, the kernel, and their sum).  The three must give the same bits: `bits_equal`.
  (b) hsm_select_topk_device, K = 16, over the same W.
  (c) hsm_relocalize_device, K = 16, against the four public calls queued separately from the host, per W on level 2.

  python tools/bench_relocalize.py [--repeats 30] [--k 16]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LEVELS = 3
# (hx, hy, ht): 33 * 33 * 1, 65 * 65 * 1, 41 * 41 * 21, 81 * 81 * 41
WINDOWS = ((16, 16, 0), (32, 32, 0), (20, 20, 10), (40, 40, 20))
STEP = (0.05, 0.05, 0.0125)


def stats(us):
    us = np.sort(np.asarray(us, np.float64))
    return {"median": round(float(np.median(us)), 1), "p10": round(float(np.percentile(us, 10)), 1),
            "p90": round(float(np.percentile(us, 90)), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--k", type=int, default=16)
    args = ap.parse_args()
    import torch
    from hector_slam_amd import capi
    from hsm_bench import common
    bp, bs, truth, init_l0, _, pts, offs = common.make_inputs(0, 64)[:7]
    scan = np.ascontiguousarray(pts[offs[0]:offs[1]], np.float32)
    centre = (np.asarray(truth[0], np.float32) + np.float32([0.6, -0.4, 0.2])).astype(np.float32)
    maps = {}
    for form in ("wave", "lane", "auto"):  # "auto": the form is picked by W, as a caller's context would
        os.environ["HSM_WINDOW_FORM"] = form
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
    os.environ.pop("HSM_WINDOW_FORM")
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream()
    sp = s.cuda_stream
    K, n = args.k, scan.shape[0]
    Wmax = max((2 * a + 1) * (2 * b + 1) * (2 * c + 1) for a, b, c in WINDOWS)
    with torch.cuda.stream(s):
        d_c, d_pts = torch.from_numpy(centre).to(dev), torch.from_numpy(scan).to(dev)
        d_step = torch.tensor(STEP, dtype=torch.float32, device=dev)
        out = {f: torch.empty((2, Wmax), dtype=torch.float32, device=dev) for f in ("wave", "lane", "batch")}
        d_poses = torch.empty((Wmax, 3), dtype=torch.float32, device=dev)
        kidx = torch.empty(K, dtype=torch.int32, device=dev)
        kscore, kpose = torch.empty(K, dtype=torch.float32, device=dev), torch.empty((K, 3), dtype=torch.float32, device=dev)
        cand, cov, lh0 = (torch.empty(sh, dtype=torch.float32, device=dev) for sh in ((K, 3), (K, 9), (K,)))
        best_pose, best_score = torch.empty(3, dtype=torch.float32, device=dev), torch.empty(1, dtype=torch.float32, device=dev)
        best_index = torch.empty(1, dtype=torch.int32, device=dev)
        topk_ws = torch.empty(capi.MapRepMultiMap.select_topk_workspace(Wmax, K) // 4, dtype=torch.int32, device=dev)
        reloc_ws = torch.empty(capi.MapRepMultiMap.relocalize_workspace(Wmax, K) // 4, dtype=torch.int32, device=dev)
    s.synchronize()

    def timed(fn):
        for _ in range(2):
            fn()
        s.synchronize()
        t = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            fn()
            e1.record(s)
            e1.synchronize()
            t.append(e0.elapsed_time(e1) * 1e3)
        return t

    for half in WINDOWS:
        hx, hy, ht = half
        nx, ny, nt = 2 * hx + 1, 2 * hy + 1, 2 * ht + 1
        W = nx * ny * nt

        def window(form, lvl):
            maps[form].score_window_device(lvl, d_c.data_ptr(), STEP, half, d_pts.data_ptr(), n, out[form][0].data_ptr(),
                                           out[form][1].data_ptr(), sp)

        def fill():
            with torch.cuda.stream(s):
                p = d_poses[:W].view(nt, ny, nx, 3)
                ar = lambda m_, h_: (torch.arange(m_, device=dev, dtype=torch.int32) - h_).to(torch.float32)  # noqa: E731
                p[..., 0] = (d_c[0] + ar(nx, hx) * d_step[0])[None, None, :]
                p[..., 1] = (d_c[1] + ar(ny, hy) * d_step[1])[None, :, None]
                p[..., 2] = (d_c[2] + ar(nt, ht) * d_step[2])[:, None, None]

        def batch(lvl):
            maps["wave"].score_batch_device(lvl, W, d_poses.data_ptr(), d_pts.data_ptr(), 0, n, out["batch"][0].data_ptr(),
                                            out["batch"][1].data_ptr(), sp)

        for lvl in (2, 0):
            t = {k: [] for k in ("lane", "wave", "fill", "batch")}
            t["lane"] = timed(lambda: window("lane", lvl))
            t["wave"] = timed(lambda: window("wave", lvl))
            t["fill"] = timed(fill)
            t["batch"] = timed(lambda: batch(lvl))
            s.synchronize()
            r = {f: out[f][:, :W].cpu().numpy().view(np.uint32) for f in out}
            print(json.dumps({"measure": "a_window_score", "level": lvl, "window": half, "W": W, "beams": n, "repeats": args.repeats,
                              "window_lane_us": stats(t["lane"]), "window_wave_us": stats(t["wave"]),
                              "torch_fill_us": stats(t["fill"]), "score_batch_us": stats(t["batch"]),
                              "fill_plus_score_batch_us": round(stats(t["fill"])["median"] + stats(t["batch"])["median"], 1),
                              "bits_equal": bool(np.array_equal(r["lane"], r["wave"]) and np.array_equal(r["lane"], r["batch"]))}),
                  flush=True)

        def topk():
            maps["lane"].select_topk_device(W, out["lane"][0].data_ptr(), K, kidx.data_ptr(), kscore.data_ptr(), topk_ws.data_ptr(),
                                            topk_ws.numel() * 4, sp)
        window("lane", 2)
        print(json.dumps({"measure": "b_topk", "W": W, "k": K, "select_topk_us": stats(timed(topk))}), flush=True)

        def one_call():
            maps["auto"].relocalize_device(2, d_c.data_ptr(), STEP, half, K, d_pts.data_ptr(), n, reloc_ws.data_ptr(),
                                           reloc_ws.numel() * 4, cand.data_ptr(), cov.data_ptr(), lh0.data_ptr(), best_pose.data_ptr(),
                                           best_score.data_ptr(), best_index.data_ptr(), sp)

        def four_calls():
            m = maps["auto"]
            m.score_window_device(2, d_c.data_ptr(), STEP, half, d_pts.data_ptr(), n, out["wave"][0].data_ptr(), 0, sp)
            m.select_topk_device(W, out["wave"][0].data_ptr(), K, kidx.data_ptr(), kscore.data_ptr(), topk_ws.data_ptr(),
                                 topk_ws.numel() * 4, sp)
            m.window_poses_device(d_c.data_ptr(), STEP, half, kidx.data_ptr(), K, kpose.data_ptr(), sp)
            m.match_score_batch_device(K, kpose.data_ptr(), d_pts.data_ptr(), 0, n, cand.data_ptr(), cov.data_ptr(), 0, lh0.data_ptr(),
                                       0, 1, 0, K, best_index.data_ptr(), best_score.data_ptr(), best_pose.data_ptr(), sp)
        t1, t4 = timed(one_call), timed(four_calls)
        s.synchronize()
        err = (best_pose.cpu().numpy() - np.asarray(truth[0], np.float32))
        print(json.dumps({"measure": "c_relocalize", "search_level": 2, "W": W, "k": K, "relocalize_one_call_us": stats(t1),
                          "four_calls_us": stats(t4), "winner_off_truth_m": round(float(np.hypot(err[0], err[1])), 4),
                          "winner_off_truth_rad": round(float(abs(err[2])), 5)}), flush=True)
    for m in maps.values():
        m.close()


if __name__ == "__main__":
    main()
