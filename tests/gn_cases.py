"""Maps and scans of the float64 checks of one Gauss-Newton evaluation (gn_f64.py).  A test helper, not a conftest:
the CPU self-check (test_gn_f64_reference.py) and the GPU cases (test_gpu_parity.py) build the same scans from the same
seeds, so the margin the CPU test asserts is the margin of the scans the GPU sees.

Maps: every cell of every level an independent random log-odds value, so that the probability changes from cell to cell
and almost every beam that lands on the map has a gradient a lost beam would show in H.  Scans: endpoints placed in map
coordinates around the start pose, plus the edges where kernels go wrong -- endpoints off the map (terms exactly zero),
on exact cell corners (fractions 0) and on the last interpolable row and column (coordinate == size - 2, which reads the
level's last row / column).  Beams whose every term is zero are kept; of the others only those whose single-beam change
of H or dTr exceeds twice the bound of the case's depth (gn_f64.Eval64.beam_margin)."""
from __future__ import annotations

import numpy as np

import gn_f64

RES = 0.05


class World:
    """a random multi-level map in the CPU oracle; gpu() makes a context holding the same levels"""

    def __init__(self, kind: str, size: int, levels: int, seed: int, size_y: int | None = None):
        """size_y: the map's height where it differs from its width (None: a square map, the random numbers of before)"""
        from oracle import pyoracle
        pyoracle.build()
        self.kind, self.size, self.levels = kind, size, levels
        self.size_y = size if size_y is None else size_y
        self.o = pyoracle.Oracle(kind, RES, size, self.size_y, levels)
        rng = np.random.default_rng(seed)
        self.lv = []
        for lvl in range(levels):
            sx, sy, _, _ = self.o.level_info(lvl)
            lo = rng.uniform(-2.5, 2.5, (sy, sx)).astype(np.float32)
            ui = np.zeros((sy, sx), np.int32)
            self.o.upload_level(lvl, lo, ui)
            self.lv.append((lo, ui))
        self._prob = {}

    def prob(self, level):
        """the level's probability plane (getGridProbability of the log-odds, host libm): what the relaxed model samples"""
        if level not in self._prob:
            from oracle import pyoracle
            lo = self.lv[level][0]
            self._prob[level] = pyoracle.libm_expf(lo.reshape(-1), self.kind)[1].reshape(lo.shape)
        return self._prob[level]

    def gpu(self, capi, **kw):
        kw.setdefault("parity", capi.PARITY_FAST)
        g = capi.MapRepMultiMap(RES, self.size, self.size_y, self.levels, **kw)
        for lvl in range(self.levels):
            g.upload_level(lvl, *self.lv[lvl])
        return g

    def limits(self, level):
        sx, sy, _, _ = self.o.level_info(level)
        return sx, sy

    def start_pose(self, level, rng, theta=None):
        """a world pose whose level-`level` map position lies well inside the map; theta 0 puts corner beams exactly"""
        sx, sy = self.limits(level)
        m = np.array([rng.uniform(0.3, 0.7) * sx, rng.uniform(0.3, 0.7) * sy,
                      0.0 if theta is None else theta], np.float32)
        return self.o.world_coords_pose(level, m)


def _targets(sx, sy, e, m, rng, radius):
    """m candidate endpoint positions (map frame, float64) and their kind: 0 interior, 1 corner, 2 edge, 3 off"""
    limx, limy = sx - 2.0, sy - 2.0
    kinds = rng.choice(4, m, p=[0.82, 0.06, 0.06, 0.06])
    t = np.empty((m, 2))
    lo = np.maximum(np.asarray(e[:2], np.float64) - radius, 0.0)
    hi = np.minimum(np.asarray(e[:2], np.float64) + radius, [limx, limy])
    t[:, 0] = rng.uniform(lo[0], hi[0], m)
    t[:, 1] = rng.uniform(lo[1], hi[1], m)
    c = kinds == 1
    t[c] = np.floor(t[c])
    ed = np.nonzero(kinds == 2)[0]
    half = rng.random(ed.size) < 0.5
    t[ed[half], 0] = limx - rng.choice([0.0, 0.0, 0.25, 1.0], half.sum())
    t[ed[~half], 1] = limy - rng.choice([0.0, 0.0, 0.25, 1.0], (~half).sum())
    off = np.nonzero(kinds == 3)[0]
    side = rng.integers(0, 4, off.size)
    t[off[side == 0], 0] = limx + rng.uniform(0.01, 3.0, (side == 0).sum())
    t[off[side == 1], 1] = limy + rng.uniform(0.01, 3.0, (side == 1).sum())
    t[off[side == 2], 0] = -rng.uniform(0.01, 3.0, (side == 2).sum())
    t[off[side == 3], 1] = -rng.uniform(0.01, 3.0, (side == 3).sum())
    return t, kinds


def make_scan(w: World, level: int, world_pose, n: int, d_of_n, rng, relaxed=False, extra_poses=()):
    """n level-scaled endpoints for a scan matched from `world_pose` on `level`: every beam significant at depth
    d_of_n(n) (at the start pose and at every pose of `extra_poses` -- the hypotheses of a shared scan) or all-zero.
    Returns (pts (n, 2) float32, [Eval64 per pose])."""
    if n == 0:
        return np.zeros((0, 2), np.float32), []
    poses = [world_pose] + list(extra_poses)
    pm = [w.o.map_coords_pose(level, p) for p in poses]
    e = pm[0]
    sx, sy = w.limits(level)
    radius = max(min(sx, sy) * 0.45, 8.0)
    d = d_of_n(n)
    rp = w.prob(level) if relaxed else None  # (the relaxed form's own factors: gn_f64.relaxed_factors)
    have = np.zeros((0, 2), np.float32)
    for _ in range(8):
        m = 3 * (n - have.shape[0]) + 16
        t, kinds = _targets(sx, sy, e, m, rng, radius)
        th = float(e[2])
        # p = R(-theta) (t - e): at theta == 0 exactly t - e in fp32, which lands on t exactly for corner / edge targets
        dx, dy = t[:, 0] - float(e[0]), t[:, 1] - float(e[1])
        if th == 0.0:
            p = np.stack([dx, dy], 1).astype(np.float32)
        else:
            c, s = np.cos(th), np.sin(th)
            p = np.stack([c * dx + s * dy, -s * dx + c * dy], 1).astype(np.float32)
        keep = np.ones(m, bool)
        for q in pm:
            ev = gn_f64.Eval64(w.o, level, q, p, w.kind, rp)
            keep &= (~ev.nonzero()) | (ev.beam_margin(d) > 1.5)
        have = np.concatenate([have, p[keep]])[:n]
        if have.shape[0] == n:
            break
    assert have.shape[0] == n, "could not find enough significant beams"
    have = have[rng.permutation(n)]
    return np.ascontiguousarray(have), [gn_f64.Eval64(w.o, level, q, have, w.kind, rp) for q in pm]


# ------------------------------------------------------------------------------------------------------------------------
# the batched fast-mode cases (one GN step through hsm_debug_set_schedule).  Each: the context's options, the level, the
# scan lengths of the batch, and the launch it must take: kernel name, waves per scan, block, beams per lane, texel cache.
def _cached(bpl, spb=4):
    return dict(kernel="gn_match_cached_kernel", waves_per_scan=1, block=64 * spb, beams_per_lane=bpl, texel_cache=True)


def _plain(w, bpl, spb):
    return dict(kernel="gn_match_kernel", waves_per_scan=w, block=64 * w * spb, beams_per_lane=bpl, texel_cache=False)


BATCH_CASES = []
for lvl in (0, 2):
    for lay in ("quad", "plane"):
        BATCH_CASES += [
            dict(id=f"cached4x17-{lay}-L{lvl}", world="pyr", level=lvl, wps=1, layout=lay, sizes=[1000, 700, 577, 1088, 901] * 2 + [1088, 640, 1001],
                 expect=_cached(17)),
            dict(id=f"cached4x9-{lay}-L{lvl}", world="pyr", level=lvl, wps=1, layout=lay, sizes=[500, 321, 576, 400] * 2 + [576, 333, 449],
                 expect=_cached(9)),
        ]
BATCH_CASES += [
    dict(id="relaxed4x17-L0", world="pyr", level=0, wps=1, layout="quad", parity="relaxed", sizes=[1000, 800, 1088, 577, 999] * 2 + [700],
         expect=_cached(17)),
    dict(id="relaxed4x9-L2", world="pyr", level=2, wps=1, layout="quad", parity="relaxed", sizes=[500, 576, 321, 450, 333] * 2 + [512],
         expect=_cached(9)),
    # ragged CSR batch on the headline form: empty, single-beam, two-beam and wave-boundary scans
    dict(id="cached4x17-ragged-L0", world="pyr", level=0, wps=1, layout="quad", sizes=[0, 1, 2, 63, 64, 65, 1000, 0, 127, 128, 129, 1088, 577],
         expect=_cached(17)),
    # shared scan (offsets = NULL): one scan, B start poses
    dict(id="cached4x17-shared-L0", world="pyr", level=0, wps=1, layout="quad", sizes=[1000] * 9, shared=True, expect=_cached(17)),
    dict(id="plain1x4x2-L0", world="pyr", level=0, wps=1, layout="quad", sizes=[100, 128, 65, 90, 2], expect=_plain(1, 2, 4)),
    dict(id="plain1x4x3-L1", world="pyr", level=1, wps=1, layout="quad", sizes=[150, 192, 129, 160, 191, 180, 140], expect=_plain(1, 3, 4)),
    dict(id="plain1x4x5-L0", world="pyr", level=0, wps=1, layout="plane", sizes=[300, 320, 193, 250, 319], expect=_plain(1, 5, 4)),
    dict(id="plain1x4x0-L0", world="pyr", level=0, wps=1, layout="quad", sizes=[1440, 2162, 1089, 1500, 2000], expect=_plain(1, 0, 4)),
    dict(id="plain1x4x0-plane-L2", world="pyr", level=2, wps=1, layout="plane", sizes=[1440, 2162, 1200], expect=_plain(1, 0, 4)),
    dict(id="nocache1x4x17-L0", world="pyr", level=0, wps=1, layout="quad", env={"HSM_TEXEL_CACHE": "0"}, sizes=[1000, 700, 1088, 600, 999],
         expect=_plain(1, 17, 4)),
    # level 0 above 2^23 cells: eight scans per workgroup
    dict(id="cached8x17-big", world="big", level=0, wps=1, layout="quad", sizes=[1000, 1088, 700] * 4 + [900] * 5, expect=_cached(17, 8)),
    dict(id="cached8x9-big-plane", world="big", level=0, wps=1, layout="plane", sizes=[500, 576, 400] * 3 + [333] * 4, expect=_cached(9, 8)),
    dict(id="cached8x17-big-morton", world="big", level=0, wps=1, layout="quad", order="morton", sizes=[1000, 1088, 800] * 4 + [900] * 9,
         expect=_cached(17, 8)),
    dict(id="cached8x9-big-auto", world="big", level=0, wps=1, layout="quad", order="auto-interleaved", sizes=[500] * 41,
         expect=_cached(9, 8)),
]
# team batches: W waves per scan, beam counts that select each beams-per-lane instantiation (3 / 5 / 9 / 17 / streamed)
for W in (2, 4, 8, 16):
    T = 64 * W
    for bpl, n in ((3, 3 * T - 1), (5, 5 * T - 1), (9, 8 * T + 1), (17, 17 * T - 3), (0, 17 * T + 65)):
        BATCH_CASES.append(dict(id=f"team{W}x{bpl}", world="pyr", level=0 if W <= 4 else 1, wps=W, layout="quad" if W != 4 else "plane",
                                sizes=[n, n - 2 * T if bpl else n - T] + ([n - 1] if W <= 4 else []), expect=_plain(W, bpl, 1)))

# rectangular maps: the texel-cache forms on a wide and a tall pyramid (an axis swap reads the wrong texels on one of the two),
# and the large-map forms on a map whose width alone sets the batch sort's tile shift
for wname in ("wide", "tall"):
    for lvl in (0, 2):
        for lay in ("quad", "plane"):
            BATCH_CASES += [
                dict(id=f"cached4x17-{lay}-L{lvl}-{wname}", world=wname, level=lvl, wps=1, layout=lay,
                     sizes=[1000, 700, 577, 1088, 901] * 2 + [1088, 640, 1001], expect=_cached(17)),
                dict(id=f"cached4x9-{lay}-L{lvl}-{wname}", world=wname, level=lvl, wps=1, layout=lay,
                     sizes=[500, 321, 576, 400] * 2 + [576, 333, 449], expect=_cached(9)),
            ]
BATCH_CASES += [
    dict(id="cached8x17-bigwide", world="bigwide", level=0, wps=1, layout="quad", sizes=[1000, 1088, 700] * 4 + [900] * 5,
         expect=_cached(17, 8)),
    dict(id="cached8x17-bigwide-auto", world="bigwide", level=0, wps=1, layout="quad", order="auto-interleaved", sizes=[1000] * 41,
         expect=_cached(17, 8)),
]


def batch_depth(case, n):
    return gn_f64.depth_team(n, case["wps"])


# the single-scan team cases (match_level, max_iter = 0): W = 1 .. 16, n = 64 W k +- 1 and n < 64
SINGLE_CASES = [(W, n) for W in (1, 2, 4, 8, 16) for n in (37, 64 * W * 2 - 1, 64 * W * 3 + 1)]
# the cooperative matcher: K = 16, 64, and several beams per lane
COOP_SIZES = (4096, 16384, 20000)

_WORLDS: dict = {}


def world(name: str, kind: str = "ho") -> World:
    key = (name, kind)
    if key not in _WORLDS:
        if name == "pyr":
            _WORLDS[key] = World(kind, 512, 3, seed=2024)
        elif name == "flat1":
            _WORLDS[key] = World(kind, 384, 1, seed=77)
        elif name == "wide":  # rectangles: 640 x 192 / 320 x 96 / 160 x 48, and the transpose
            _WORLDS[key] = World(kind, 640, 3, seed=640, size_y=192)
        elif name == "tall":
            _WORLDS[key] = World(kind, 192, 3, seed=192, size_y=640)
        elif name == "bigwide":  # 8192 x 1040 > 2^23 cells: the large-map forms, a batch-sort tile shift set by the width alone
            _WORLDS[key] = World(kind, 8192, 1, seed=8192, size_y=1040)
        else:  # "big": 4096^2 level 0 = 2^24 cells (> 2^23: the large-map forms)
            _WORLDS[key] = World(kind, 4096, 1, seed=4096)
    return _WORLDS[key]


def batch_inputs(case, kind: str = "ho"):
    """(world, init world poses (B, 3), list of level-scaled scans, [[Eval64 per pose] per scan], seed-stable)"""
    w = world(case["world"], kind)
    lvl = case["level"]
    rng = np.random.default_rng([ord(ch) for ch in case["id"]])
    sizes = case["sizes"]
    relaxed = case.get("parity") == "relaxed"
    dn = lambda n: batch_depth(case, n)  # noqa: E731
    if case.get("shared"):
        init = [w.start_pose(lvl, rng, theta=float(rng.uniform(-0.5, 0.5)))]
        for j in range(1, len(sizes)):
            init.append(init[0] + np.array([rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02), rng.uniform(-0.01, 0.01)], np.float32))
        pts, evs = make_scan(w, lvl, init[0], sizes[0], dn, rng, relaxed, extra_poses=init[1:])
        return w, np.asarray(init, np.float32), [pts] * len(sizes), [[e] for e in evs]
    init, scans, evs = [], [], []
    if case.get("order") == "auto-interleaved":
        # two tiles, alternating: the automatic order sorts this batch (changes between neighbours >> distinct tiles)
        a, b = w.start_pose(lvl, rng, 0.1), w.start_pose(lvl, rng, -0.1)
    for j, n in enumerate(sizes):
        if case.get("order") == "auto-interleaved":
            p0 = (a if j % 2 == 0 else b) + np.array([rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), 0.0], np.float32)
        else:
            p0 = w.start_pose(lvl, rng, theta=0.0 if j % 3 == 0 else float(rng.uniform(-2.5, 2.5)))
        pts, ev = make_scan(w, lvl, p0, n, dn, rng, relaxed)
        init.append(p0)
        scans.append(pts)
        evs.append(ev)
    return w, np.asarray(init, np.float32), scans, evs


def _world_seed(name):
    return [] if name == "pyr" else [ord(ch) for ch in name]


def single_inputs(W: int, n: int, kind: str = "ho", world_name: str = "pyr"):
    """one scan for match_level(0, ..., max_iter = 0) on W waves: (world, init world pose, level-0 scan, Eval64)"""
    w = world(world_name, kind)
    rng = np.random.default_rng([W, n, 1] + _world_seed(world_name))
    p0 = w.start_pose(0, rng, theta=0.0 if n % 2 else float(rng.uniform(-2.5, 2.5)))
    pts, evs = make_scan(w, 0, p0, n, lambda m: gn_f64.depth_team(m, W), rng)
    return w, p0, pts, evs[0]


def coop_inputs(n: int, kind: str = "ho", world_name: str = "pyr"):
    """one dense scan for the cooperative matcher (match_level on level 0)"""
    w = world(world_name, kind)
    rng = np.random.default_rng([n, 2] + _world_seed(world_name))
    p0 = w.start_pose(0, rng, theta=float(rng.uniform(-2.5, 2.5)))
    pts, evs = make_scan(w, 0, p0, n, lambda m: gn_f64.depth_coop(m, gn_f64.coop_workgroups(m)), rng)
    return w, p0, pts, evs[0]


def trace_inputs(n: int = 1081, kind: str = "ho"):
    """one scan on the one-level map for the hook trace (hsm_match_trace); significant at the depth of any team width"""
    w = world("flat1", kind)
    rng = np.random.default_rng([n, 3])
    p0 = w.start_pose(0, rng, theta=0.3)
    pts, evs = make_scan(w, 0, p0, n, lambda m: max(gn_f64.depth_team(m, W) for W in (1, 2, 4, 8, 16)), rng)
    return w, p0, pts, evs[0]


def eval_inputs(n: int, level: int, kind: str = "ho", world_name: str = "pyr"):
    """one scan for hsm_hessian_derivs (gn_eval_kernel)"""
    w = world(world_name, kind)
    rng = np.random.default_rng([n, level, 4] + _world_seed(world_name))
    p0 = w.start_pose(level, rng, theta=float(rng.uniform(-2.5, 2.5)))
    pts, evs = make_scan(w, level, p0, n, gn_f64.depth_eval, rng)
    return w, p0, pts, evs[0]


EVAL_CASES = [(37, 0), (1081, 0), (1024, 1), (5000, 2)]

# the single-scan forms on rectangles, each case naming its world: team widths (match_level, max_iter = 0), the cooperative
# matcher, gn_eval_kernel on the coarsest level of the wide pyramid
RECT_SINGLE_CASES = [("wide", 1, 1081), ("tall", 2, 64 * 2 * 3 + 1), ("wide", 4, 64 * 4 * 2 - 1), ("tall", 8, 1081),
                     ("wide", 16, 64 * 16 * 3 + 1), ("tall", 16, 37)]
RECT_COOP_CASES = [("tall", 16384)]
RECT_EVAL_CASES = [("wide", 2000, 2)]
