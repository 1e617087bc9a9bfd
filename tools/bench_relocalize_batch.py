"""Time hsm_relocalize_batch_device against one hsm_relocalize_device call per scan, on the 3-level 2048^2 map of the benchmark
scene with 1081-beam scans, K = 16, the window searched on level 2.

Device events on one stream around the whole of a leg (all its launches, queued from the host without a wait in between), after
two warm-up rounds, --repeats times; every figure is the median with its p10 - p90 spread (one device, one run: other work
shares the machine).  One JSON line per (W, B), W in {1 089, 4 225}, B in {1, 8, 64, 512}:

  one_call_us        hsm_relocalize_batch_device, B scans (CSR) in B windows
  queued_calls_us    B hsm_relocalize_device calls queued back to back: the route that existed before, and the yardstick
  score_lane_us / score_wave_us   hsm_score_windows_batch_device alone in each form (HSM_WINDOW_FORM); `score_bits_equal`
  topk_groups_us     hsm_select_topk_groups_device alone, B groups of W
  rest_us            one_call - the score in the form the call picks - the top-K: start poses, the scans laid out K times,
                     match + score on level 0 + winners
  equal_to_queued    the one call's winners and candidates have the bits of the queued calls'

  python tools/bench_relocalize_batch.py [--repeats 30] [--k 16] [--batches 1,8,64,512]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LEVELS = 3
SEARCH_LEVEL = 2
WINDOWS = ((16, 16, 0), (32, 32, 0))  # 33 * 33, 65 * 65
STEP = (0.05, 0.05, 0.0125)
LANE_MIN = 1 << 16  # kWindowLaneMin of csrc/window.hip: which form the one call picks


def stats(us):
    us = np.sort(np.asarray(us, np.float64))
    return {"median": round(float(np.median(us)), 1), "p10": round(float(np.percentile(us, 10)), 1),
            "p90": round(float(np.percentile(us, 90)), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--batches", default="1,8,64,512")
    args = ap.parse_args()
    batches = [int(b) for b in args.batches.split(",")]
    import torch
    from hector_slam_amd import capi
    from hsm_bench import common
    bp, bs, truth, _, _, pts, offs = common.make_inputs(0, 64)[:7]
    n_scans = len(offs) - 1
    maps = {}
    for form in ("wave", "lane", "auto"):  # "auto": the form is picked by B * W, as a caller's context would
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
    K = args.k
    M = capi.MapRepMultiMap

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
        W = M.window_count(half)
        for B in batches:
            which = [b % n_scans for b in range(B)]
            scans = [np.ascontiguousarray(pts[offs[q]:offs[q + 1]], np.float32) for q in which]
            lens = np.array([len(x) for x in scans])
            h_offs = np.zeros(B + 1, np.int32)
            h_offs[1:] = np.cumsum(lens)
            total = int(h_offs[-1])
            centres = np.stack([np.asarray(truth[q], np.float32) for q in which]) + np.float32([0.6, -0.4, 0.2])
            f = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)  # noqa: E731
            i = lambda *sh: torch.empty(sh, dtype=torch.int32, device=dev)  # noqa: E731
            with torch.cuda.stream(s):
                d_c = torch.from_numpy(np.ascontiguousarray(centres, np.float32)).to(dev)
                d_pts, d_offs = torch.from_numpy(np.concatenate(scans)).to(dev), torch.from_numpy(h_offs).to(dev)
                one = dict(cand=f(B, K, 3), cov=f(B, K, 9), lh=f(B, K), ci=i(B, K), bp=f(B, 3), bs=f(B), bi=i(B))
                que = dict(cand=f(B, K, 3), cov=f(B, K, 9), lh=f(B, K), bp=f(B, 3), bs=f(B), bi=i(B))
                for d in (one, que):
                    d["bp"].fill_(0.0)
                ws = i(M.relocalize_batch_workspace(B, W, K, total) // 4)
                ws1 = i(M.relocalize_workspace(W, K) // 4)
                score = {form: f(B, W) for form in ("lane", "wave")}
                tk_ws = i(M.select_topk_groups_workspace(B, W, K) // 4)
                tk_idx, tk_score = i(B, K), f(B, K)
            s.synchronize()

            def one_call():
                maps["auto"].relocalize_batch_device(SEARCH_LEVEL, B, d_c.data_ptr(), STEP, half, K, d_pts.data_ptr(), d_offs.data_ptr(),
                                                     0, total, ws.data_ptr(), ws.numel() * 4, one["cand"].data_ptr(),
                                                     one["cov"].data_ptr(), one["lh"].data_ptr(), one["ci"].data_ptr(),
                                                     one["bp"].data_ptr(), one["bs"].data_ptr(), one["bi"].data_ptr(), sp)

            def queued_calls():
                m = maps["auto"]
                for b in range(B):
                    m.relocalize_device(SEARCH_LEVEL, d_c[b].data_ptr(), STEP, half, K, d_pts[h_offs[b]].data_ptr(), int(lens[b]),
                                        ws1.data_ptr(), ws1.numel() * 4, que["cand"][b].data_ptr(), que["cov"][b].data_ptr(),
                                        que["lh"][b].data_ptr(), que["bp"][b].data_ptr(), que["bs"][b:].data_ptr(),
                                        que["bi"][b:].data_ptr(), sp)

            def score_alone(form):
                maps[form].score_windows_batch_device(SEARCH_LEVEL, B, d_c.data_ptr(), STEP, half, d_pts.data_ptr(), d_offs.data_ptr(), 0,
                                                      score[form].data_ptr(), 0, sp)

            def topk():
                maps["auto"].select_topk_groups_device(B, W, score["wave"].data_ptr(), K, tk_idx.data_ptr(), tk_score.data_ptr(),
                                                       tk_ws.data_ptr(), tk_ws.numel() * 4, sp)

            t = {"one": timed(one_call), "queued": timed(queued_calls), "lane": timed(lambda: score_alone("lane")),
                 "wave": timed(lambda: score_alone("wave")), "topk": timed(topk)}
            s.synchronize()
            u32 = lambda x: x.cpu().numpy().view(np.uint32)  # noqa: E731
            equal = all(np.array_equal(u32(one[key]), u32(que[key])) for key in que)
            picked = "lane" if B * W >= LANE_MIN else "wave"
            med = {key: stats(v) for key, v in t.items()}
            print(json.dumps({"W": W, "B": B, "k": K, "beams": int(lens.max()), "repeats": args.repeats, "one_call_us": med["one"],
                              "queued_calls_us": med["queued"], "score_lane_us": med["lane"], "score_wave_us": med["wave"],
                              "score_form_picked": picked, "topk_groups_us": med["topk"],
                              "rest_us": round(med["one"]["median"] - med[picked]["median"] - med["topk"]["median"], 1),
                              "score_bits_equal": bool(np.array_equal(u32(score["lane"]), u32(score["wave"]))),
                              "equal_to_queued": bool(equal)}), flush=True)
    for m in maps.values():
        m.close()


if __name__ == "__main__":
    main()
