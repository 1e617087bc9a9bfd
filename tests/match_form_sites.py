"""The launch sites behind tests/golden/match_forms.json: which matcher form the host runtime picks for which call.

One module for the recorder (tests/tools/record_match_forms.py), the CPU test of the plan (tests/test_match_plan.py) and the GPU
test (tests/test_gpu_match_forms.py), so that the three cannot drift.  A site is a plain dict:

    id       unique name
    entry    "batch" (match_batch_device, ONE shared scan and `batch` start poses) or "single" (matchData)
    map      "small" (256 x 256 cells), "small2" (the same, two levels) or "large" (4096 x 2304: level 0 beyond 2^23 cells)
    layout   "quad" | "plane"
    parity   "auto" | "exact" | "fast" | "relaxed"
    n        beams of the scan
    batch_cu [a, b]: the batch is a * CU + b start poses, CU the device's compute units (single: [0, 1])
    env      the knobs hsm_create reads, as {name: value}
    probe    a clock probe is set for the launch (set_clock_probe)

Every launch is a few milliseconds on an empty map: the form depends on the call's shape alone, never on what the map holds.
"""
import os

from support import layout_of

KNOBS = ("HSM_EXACT_CHAIN_WAVE", "HSM_EXACT_SPLIT_TAIL", "HSM_EXACT_CACHED", "HSM_EXACT_DENSE", "HSM_EXACT_DENSE_MIN",
         "HSM_TEXEL_CACHE", "HSM_BPL", "HSM_SPB_LARGE", "HSM_EXACT_SPEC", "HSM_EXACT_SPEC1", "HSM_COOP_MIN", "HSM_WPS")
# ... and what else of the environment would change a form: cleared while a context is created
OTHER_ENV = ("HSM_LAYOUT", "HSM_PARITY", "HSM_BATCH_ORDER", "HSM_BATCH_ORDER_MIN", "HSM_XCD_CHUNK_EXACT")
BEAMS = (64, 128, 192, 320, 576, 832, 1081, 1089, 2162, 4095, 4096, 16384)
SINGLE_BEAMS = (360, 720, 1081, 2048, 4096, 16384)
# batch sizes as a * CU + b: groups of four scans on both sides of 2, 3 and 4 workgroups per CU, and the split-tail remainders
BATCHES = ((0, 1), (0, 16), (1, 0), (1, 1), (8, 0), (8, 4), (12, 0), (12, 4), (16, 0), (16, 4), (24, 0), (24, 4), (28, 4),
           (0, 5000), (0, 20000))
MAPS = {"small": (256, 256, 1), "small2": (256, 256, 2), "large": (4096, 2304, 1)}
FAMILIES = ("team", "team_exact", "cached", "exact_cached", "exact_cached_cw", "exact_dense", "spec", "spec1", "coop")
LAYOUT_CODE = {"quad": 1, "plane": 2}


def _site(out, entry, map_name, layout, parity, n, batch_cu=(0, 1), env=None, probe=False):
    env = dict(env or {})
    tag = ",".join(f"{k[4:].lower()}={v}" for k, v in sorted(env.items()))
    a, b = batch_cu
    bs = (f"{a}cu+{b}" if b else f"{a}cu") if a else str(b)
    sid = f"{entry}:{map_name}:{layout}:{parity}:n{n}:b{bs}" + (f":{tag}" if tag else "") + (":probe" if probe else "")
    if any(s["id"] == sid for s in out):
        return
    out.append({"id": sid, "entry": entry, "map": map_name, "layout": layout, "parity": parity, "n": int(n),
                "batch_cu": [int(a), int(b)], "env": env, "probe": bool(probe)})


def sites():
    """the list, a few hundred sites: the axes crossed where they interact, every knob at the sites it affects"""
    out = []
    # every batch size: the exact-order batch forms and the fast ones, on a map within the L2s and on one beyond
    for m in ("small", "large"):
        for bc in BATCHES:
            for parity in ("auto", "fast"):
                _site(out, "batch", m, "quad", parity, 1081, bc)
    # every scan length (beams per lane on both sides of 2, 3, 5, 9, 13 and 17, and the streaming tail) at the batch sizes
    # that change the form
    for n in BEAMS:
        for bc in ((0, 1), (0, 16), (1, 1), (8, 0), (12, 0), (16, 0), (0, 5000)):
            for parity in ("auto", "fast"):
                _site(out, "batch", "small", "quad", parity, n, bc)
        for bc in ((0, 16), (0, 5000)):
            for parity in ("auto", "fast"):
                _site(out, "batch", "small", "plane", parity, n, bc)
    for n in (576, 832, 1081, 1089, 2162):
        for bc in ((8, 0), (12, 0), (16, 0)):
            for parity in ("auto", "fast"):
                _site(out, "batch", "large", "quad", parity, n, bc)
    for n in (832, 1081):
        for parity in ("auto", "fast"):
            _site(out, "batch", "large", "plane", parity, n, (16, 0))
    for parity in ("exact", "relaxed"):
        for n in (320, 1081, 4096):
            for bc in ((0, 16), (16, 0)):
                _site(out, "batch", "small", "quad", parity, n, bc)
        _site(out, "batch", "small", "plane", parity, 1081, (16, 0))
        _site(out, "batch", "large", "quad", parity, 1081, (16, 0))
    # the single-scan entry
    for n in SINGLE_BEAMS:
        for parity in ("auto", "exact", "fast"):
            for layout in ("quad", "plane"):
                _site(out, "single", "small", layout, parity, n)
        _site(out, "single", "small2", "quad", "auto", n)
        _site(out, "single", "small2", "quad", "relaxed", n)
    _site(out, "single", "large", "quad", "auto", 1081)
    _site(out, "single", "large", "quad", "fast", 1081)
    # each knob on its own, at the sites it affects
    for bc in ((0, 16), (8, 0), (12, 0), (16, 4), (0, 5000)):
        _site(out, "batch", "small", "quad", "auto", 1081, bc, {"HSM_EXACT_CHAIN_WAVE": 0})
    _site(out, "batch", "small", "quad", "auto", 2162, (1, 1), {"HSM_EXACT_CHAIN_WAVE": 0})
    for bc in ((16, 4), (24, 4), (28, 4), (0, 5000), (0, 20000)):
        _site(out, "batch", "small", "quad", "auto", 1081, bc, {"HSM_EXACT_SPLIT_TAIL": 0})
    _site(out, "batch", "large", "quad", "auto", 1081, (24, 4), {"HSM_EXACT_SPLIT_TAIL": 0})
    for n, bc in ((1081, (0, 16)), (1081, (16, 0)), (320, (0, 5000)), (2162, (1, 1))):
        _site(out, "batch", "small", "quad", "auto", n, bc, {"HSM_EXACT_CACHED": 0})
    for n in (4096, 16384):
        for bc in ((0, 1), (0, 16), (1, 1)):
            _site(out, "batch", "small", "quad", "auto", n, bc, {"HSM_EXACT_DENSE": 0})
        _site(out, "single", "small", "quad", "auto", n, env={"HSM_EXACT_DENSE": 0})
    for n in (2048, 2162):
        for bc in ((0, 1), (0, 16), (1, 1)):
            _site(out, "batch", "small", "quad", "auto", n, bc, {"HSM_EXACT_DENSE_MIN": 2048})
    for n in (1081, 2048):
        _site(out, "single", "small", "quad", "auto", n, env={"HSM_EXACT_DENSE_MIN": 2048})
    for m in ("small", "large"):
        for n in (320, 576, 1081):
            _site(out, "batch", m, "quad", "fast", n, (16, 0), {"HSM_TEXEL_CACHE": 0})
    for parity, n, bc in (("fast", 320, (0, 16)), ("fast", 1081, (16, 0)), ("auto", 1081, (16, 0)), ("auto", 1081, (0, 16))):
        _site(out, "batch", "small", "quad", parity, n, bc, {"HSM_BPL": 0})
    _site(out, "batch", "large", "quad", "fast", 1081, (16, 0), {"HSM_BPL": 0})
    for parity in ("auto", "fast"):
        _site(out, "single", "small", "quad", parity, 360, env={"HSM_BPL": 0})
    for n in (320, 576, 1081, 1089):
        _site(out, "batch", "large", "quad", "fast", n, (16, 0), {"HSM_SPB_LARGE": 4})
    for n in (4096, 16384):
        for bc in ((0, 1), (0, 16)):
            _site(out, "batch", "small", "quad", "auto", n, bc, {"HSM_EXACT_SPEC": 1})
            _site(out, "batch", "small", "plane", "auto", n, bc, {"HSM_EXACT_SPEC": 1})
        _site(out, "single", "small", "quad", "auto", n, env={"HSM_EXACT_SPEC": 1})
    _site(out, "batch", "small", "quad", "fast", 4096, (0, 16), {"HSM_EXACT_SPEC": 1})
    for n in (360, 1081, 2048, 4096):
        for layout in ("quad", "plane"):
            _site(out, "single", "small", layout, "auto", n, env={"HSM_EXACT_SPEC1": 1})
    _site(out, "single", "small", "quad", "fast", 1081, env={"HSM_EXACT_SPEC1": 1})
    _site(out, "batch", "small", "quad", "auto", 1081, (0, 1), {"HSM_EXACT_SPEC1": 1})
    for n in (720, 1081, 4096):
        for parity in ("auto", "fast"):
            _site(out, "single", "small", "quad", parity, n, env={"HSM_COOP_MIN": 1024})
    _site(out, "single", "small", "plane", "fast", 1081, env={"HSM_COOP_MIN": 1024})
    _site(out, "single", "small", "quad", "fast", 4096, env={"HSM_COOP_MIN": 100000})
    for wps in (1, 2, 4, 8, 16):
        for parity in ("auto", "fast"):
            for n in (128, 1081, 4096):
                _site(out, "batch", "small", "quad", parity, n, (0, 16), {"HSM_WPS": wps})
            _site(out, "batch", "small", "quad", parity, 1081, (16, 0), {"HSM_WPS": wps})
            for n in (1081, 4096):
                _site(out, "single", "small", "quad", parity, n, env={"HSM_WPS": wps})
        _site(out, "batch", "large", "quad", "fast", 1081, (16, 0), {"HSM_WPS": wps})
    # a launch with a clock probe: the headline form has an instantiation that carries the stamps, the others take it as they are
    for parity, bc in (("auto", (16, 0)), ("auto", (16, 4)), ("auto", (0, 16)), ("fast", (16, 0))):
        _site(out, "batch", "small", "quad", parity, 1081, bc, probe=True)
    _site(out, "batch", "large", "quad", "auto", 1081, (16, 0), probe=True)
    _site(out, "single", "small", "quad", "auto", 1081, probe=True)
    return out


def batch_of(site, cu):
    a, b = site["batch_cu"]
    return a * cu + b


def portable(site, cu, recorded_cu):
    """does the recorded answer hold on a device of `cu` compute units?  A batch given in CUs moves with the device (only its
    grid changes: scaled_grid); up to 16 scans behave alike on any device of more than 16 CUs; a batch given as a plain number
    (5000, 20 000) sits elsewhere among the thresholds of another device"""
    return cu == recorded_cu or site["batch_cu"][0] > 0 or (site["batch_cu"][1] <= 16 and cu > 16)


def scaled_grid(site, expect, cu, recorded_cu):
    """the recorded grid on a device of `cu` compute units: every form's grid is ceil(batch / scans per workgroup) -- the split
    launch's two grids add up to that as well -- and the scans per workgroup (1, 4 or 8) follow from the recorded pair"""
    grid = expect["config"][3]
    if cu == recorded_cu or site["batch_cu"][0] == 0:
        return grid
    b0, b1 = batch_of(site, recorded_cu), batch_of(site, cu)
    spb = [k for k in (1, 4, 8) if (b0 + k - 1) // k == grid]
    assert len(spb) == 1, (site["id"], grid, b0)
    return (b1 + spb[0] - 1) // spb[0]


def context_key(site):
    return (site["map"], site["layout"], tuple(sorted(site["env"].items())))


class Runner:
    """runs sites on the device: one context at a time (run the sites sorted by context_key), the large map among them"""

    def __init__(self, capi):
        import torch
        self.capi, self.torch = capi, torch
        self.key, self.ctx, self.cu = None, None, None
        self.bufs = {}
        # (hsm_set_clock_probe asks for four words; the speculative-carry kernels write eight: room to spare)
        self.stamps = torch.zeros(8192, dtype=torch.int64, device="cuda:0")
        self.contexts_created = {}

    def context(self, site):
        key = context_key(site)
        if key != self.key:
            self.close()
            sx, sy, levels = MAPS[site["map"]]
            saved = {k: os.environ.pop(k, None) for k in KNOBS + OTHER_ENV}
            try:
                for k, v in site["env"].items():
                    os.environ[k] = str(v)
                self.ctx = self.capi.MapRepMultiMap(0.05, sx, sy, levels, device=0,
                                                    layout=layout_of(self.capi, site["layout"]))
            finally:
                for k, v in saved.items():
                    os.environ.pop(k, None)
                    if v is not None:
                        os.environ[k] = v
            self.key = key
            self.contexts_created[key] = self.contexts_created.get(key, 0) + 1
        return self.ctx

    def compute_units(self):
        if self.cu is None:
            g = self.capi.MapRepMultiMap(0.05, 256, 256, 1, device=0)
            self.cu = g.device_info()["compute_units"]
            g.close()
        return self.cu

    def close(self):
        if self.ctx is not None:
            self.torch.cuda.synchronize()
            self.ctx.close()
        self.ctx, self.key = None, None

    def scan(self, n):
        """n endpoints on a ring of 2 m around the sensor, in level-0 cells: inside every map used here"""
        import numpy as np
        t = np.arange(n, dtype=np.float64) * (2.0 * np.pi / max(n, 1))
        return np.stack([40.0 * np.cos(t), 40.0 * np.sin(t)], 1).astype(np.float32)

    def buf(self, name, floats):
        have = self.bufs.get(name)
        if have is None or have.numel() < floats:
            have = self.bufs[name] = self.torch.zeros(max(floats, 1), dtype=self.torch.float32, device="cuda:0")
        return have

    def run(self, site):
        """-> {"kernel", "config": the five hsm_last_launch_config values, "parity": hsm_last_launch_parity as a word}"""
        capi, torch = self.capi, self.torch
        g = self.context(site)
        g.set_parity({"auto": capi.PARITY_AUTO, "exact": capi.PARITY_EXACT, "fast": capi.PARITY_FAST,
                      "relaxed": capi.PARITY_RELAXED}[site["parity"]])
        g.set_clock_probe(self.stamps.data_ptr() if site["probe"] else 0)
        pts = self.scan(site["n"])
        try:
            if site["entry"] == "single":
                g.matchData([0.0, 0.0, 0.0], pts)
            else:
                batch = batch_of(site, self.compute_units())
                d_pts = self.buf("pts", 2 * site["n"])
                d_pts[:2 * site["n"]] = torch.from_numpy(pts.reshape(-1))
                d_begin, d_out = self.buf("begin", 3 * batch), self.buf("out", 3 * batch)
                g.match_batch_device(batch, d_begin.data_ptr(), d_pts.data_ptr(), 0, site["n"], d_out.data_ptr(), 0)
                torch.cuda.synchronize()
            c = g.last_launch_config()
        finally:
            g.set_clock_probe(0)
        return {"kernel": c["kernel"],
                "config": [LAYOUT_CODE[c["layout"]], c["waves_per_scan"], c["block"], c["grid"],
                           -c["beams_per_lane"] if c["texel_cache"] else c["beams_per_lane"]],
                "parity": c["parity_effective"]}


def run_all(capi, site_list):
    """every site of the list, grouped by context; -> {id: answer}"""
    r = Runner(capi)
    got = {}
    try:
        for s in sorted(site_list, key=lambda s: (context_key(s), s["id"])):
            got[s["id"]] = r.run(s)
    finally:
        r.close()
    return got, r
