"""Rectangular maps (tests/rect_cases.py: wide / tall, sx % 4 != 0, strips whose coarsest level is 6 cells across, and two
maps above 2^23 cells), each with its transpose, in the library's DEFAULT mode (the reference's summation order): every
entry point bit-identical to the CPU checker.  The library keeps x and y apart in the level limits, the tiled texel plane,
the edge-copied last texel column and row, the update boxes, the key-row clears, the mark tiles and the batch sort's tiles;
on a square map a mixed-up axis there cannot be seen.

Every test asserts the launch it took (last_launch_config), so a routing change cannot quietly test another kernel.  Where the
checker is the reference itself ("hr"), the restatement runs one step ahead of it on every match: after a map read at a NaN
coordinate there (a singular H, where the reference would index its grid with (int)NaN and crash) the restatement -- pinned
to the reference by tests/test_oracle_vs_reference.py -- is the checker for the rest of the test, NaN pattern for NaN pattern."""
import numpy as np
import pytest
from hypothesis import HealthCheck, given, seed, settings

import rect_cases
from conftest import bits, oracle_kinds
from support import capi, kind, new_context, same
from edge_cases import begin_cells, border_fan, probe_coords, world_pose_of_cell

pytestmark = pytest.mark.gpu

RES = rect_cases.RES
ZERO2 = np.zeros(2, np.float32)
RANGE_MIN, RANGE_MAX = 0.4, 30.0


class Ref:
    """the CPU checker of `kind`; for "hr" with the restatement stepped ahead of it (see the module docstring)"""

    def __init__(self, oracle_mod, kind, sx, sy, levels, start=(0.5, 0.5), free=0.4, occ=0.9):
        self.o = oracle_mod.Oracle(kind, RES, sx, sy, levels, start)
        self.guard = oracle_mod.Oracle("ho", RES, sx, sy, levels, start) if kind == "hr" else None
        self.kind, self.levels = kind, levels
        for x in self.all():
            x.set_update_factor_free(free)
            x.set_update_factor_occupied(occ)

    def all(self):
        return (self.o,) if self.guard is None else (self.o, self.guard)

    def match(self, pose, pts, origo=ZERO2):
        """-> (pose, cov): the reference's; where its result would be undefined, the restatement's -- which then stays the
        checker (it holds the same map, and a skipped match would leave the reference's coarse levels on stale containers)"""
        if self.guard is None:
            return self.o.match(pose, pts, origo, cov=np.zeros(9, np.float32))
        u0 = self.guard.undefined_reads()
        p, c = self.guard.match(pose, pts, origo, cov=np.zeros(9, np.float32))
        if self.guard.undefined_reads() != u0:
            self.o, self.guard = self.guard, None
            return p, c
        return self.o.match(pose, pts, origo, cov=np.zeros(9, np.float32))

    def update(self, pose, pts, origo=ZERO2):
        for x in self.all():
            x.update_by_scan(pose, pts, origo)
            x.on_map_updated()

    def upload(self, lvl, lo, ui):
        for x in self.all():
            x.upload_level(lvl, lo, ui)


def assert_match(pg, cg, po, co, what):
    if np.isfinite(po).all():
        assert same(pg, po) and same(cg, co), (what, pg, po)
    else:  # a singular H: the reference divides by a zero determinant; NaN payloads are not pinned
        assert np.array_equal(np.isnan(pg), np.isnan(po)), (what, pg, po)


def new_ctx(capi, sx, sy, levels, layout="quad", start=(0.5, 0.5), free=0.4, occ=0.9, **kw):
    g = new_context(capi, RES, sx, sy, levels, start, layout, (free, occ), **kw)
    assert g.parity() == capi.PARITY_AUTO
    assert [g.level_info(l)[:2] for l in range(levels)] == [(sx >> l, sy >> l) for l in range(levels)]
    return g


def check_maps(oracle_mod, g, ref, rng, what, probes=True):
    """every level bit-identical, the mark planes clear, the probability plane and the sampled texels along the four borders"""
    for lvl in range(ref.levels):
        (lo_g, ui_g), (lo_o, ui_o) = g.download_level(lvl), ref.o.download_level(lvl)
        assert np.array_equal(ui_g, ui_o), (what, lvl, int((ui_g != ui_o).sum()))
        assert same(lo_g, lo_o), (what, lvl, int((bits(lo_g) != bits(lo_o)).sum()))
        assert g.debug_marks_nonzero(lvl) == (0, 0), (what, lvl)
        if not probes:
            continue
        _, prob = oracle_mod.libm_expf(lo_o.reshape(-1), "ho")
        assert np.array_equal(bits(g.download_prob(lvl)).reshape(-1), bits(prob)), (what, lvl)
        lsx, lsy = lo_o.shape[1], lo_o.shape[0]
        pc = probe_coords(lsx, lsy, rng)
        got = g.eval_beams(lvl, np.zeros(3, np.float32), pc)
        assert same(got[:, :3], ref.o.interp(lvl, pc)), (what, lvl)


def expect_single(g, n, what):
    cfg = g.last_launch_config()
    assert cfg["parity_effective"] == "exact", (what, cfg)
    if n >= 4096:
        assert cfg["kernel"] == "gn_match_exact_dense_kernel" and cfg["block"] == 1024, (what, cfg)
    else:
        assert cfg["kernel"] == "gn_match_kernel (exact order)", (what, cfg)


def expect_batch(g, what, texel_cache=True):
    cfg = g.last_launch_config()
    assert cfg["parity_effective"] == "exact", (what, cfg)
    if texel_cache:
        assert cfg["kernel"] == "gn_match_exact_cached_kernel (chain wavefront)" and cfg["block"] == 320, (what, cfg)
    else:
        assert cfg["kernel"] == "gn_match_kernel (exact order)" and not cfg["texel_cache"], (what, cfg)
    return cfg


# ---------------------------------------------------------------------------------------------- a. the SLAM loop from empty
@pytest.mark.parametrize("layout", ["quad", "plane", "quad-texel-pass"])
@pytest.mark.parametrize("beams", [1081, 5000])
@pytest.mark.parametrize("geom", rect_cases.SMALL, ids=rect_cases.gid)
def test_slam_loop_from_an_empty_map(capi, oracle_mod, kind, geom, beams, layout, monkeypatch):
    """match -> update at the matched pose, 8 scans from an empty map, a laser origin off the robot's centre: every pose and
    covariance, and after every update every level, the mark planes, the probability plane and the texels along the borders.
    1081 beams: the team matcher and the keyed update; 5000: the dense matcher and the byte-map update.  "quad-texel-pass":
    HSM_SCATTER_TEXELS_MAX=0, every update rewrites its box's texels in update_texels_kernel instead of the apply pass"""
    sx, sy, levels = geom
    if layout == "quad-texel-pass":
        monkeypatch.setenv("HSM_SCATTER_TEXELS_MAX", "0")
    g = new_ctx(capi, sx, sy, levels, layout.split("-")[0])
    ref = Ref(oracle_mod, kind, sx, sy, levels)
    _, poses, scans = rect_cases.scene(sx, sy, 8, beams, seed=sx * 31 + sy + beams)
    rng = np.random.default_rng([sx, sy, beams])
    origos = rng.uniform(-1, 1, (8, 2)).astype(np.float32)
    pose = poses[0].copy()
    dense = 0
    for t in range(8):
        hint = pose + (poses[t] - poses[max(t - 1, 0)])
        po, co = ref.match(hint, scans[t], origos[t])
        pg, cg = g.matchData(hint, scans[t], None, origos[t])
        expect_single(g, scans[t].shape[0], (geom, t))
        dense += scans[t].shape[0] >= 4096
        assert_match(pg, cg, po, co, (geom, layout, t))
        if not np.isfinite(po).all():
            po = hint
        ref.update(po, scans[t], origos[t])
        g.updateByScan(scans[t], po, origos[t])
        check_maps(oracle_mod, g, ref, rng, (geom, layout, beams, t))
        pose = po
    assert dense == (8 if beams > 4096 else 0), dense
    _, ui = ref.o.download_level(0)
    assert (ui >= 0).sum() > 50, "the loop mapped nothing"
    g.close()


# --------------------------------------------------------------------------------------------- b. sparse fans at the borders
@pytest.mark.parametrize("layout", ["quad", "plane"])
@pytest.mark.parametrize("geom", rect_cases.SMALL, ids=rect_cases.gid)
def test_sparse_border_fans(capi, oracle_mod, kind, geom, layout):
    """1500-beam fans (the keyed update) ending on and 0.5 .. 6 cells beyond the four borders, from begin cells next to and
    off every border: every level bit-identical after every update, and the fans reach x = 0, x = sx - 1, y = 0, y = sy - 1"""
    sx, sy, levels = geom
    g = new_ctx(capi, sx, sy, levels, layout)
    ref = Ref(oracle_mod, kind, sx, sy, levels)
    rng = np.random.default_rng(sx * 1000 + sy)
    for k, (cx, cy) in enumerate(begin_cells(sx, sy)):
        th = float(rng.uniform(-np.pi, np.pi)) if k % 3 else 0.0
        pose = world_pose_of_cell(RES, sx, sy, cx, cy, th)
        pts = border_fan(rng, sx, sy, cx, cy, th, 1500)
        og = ZERO2 if k % 4 else np.array([0.3, -0.2], np.float32)
        po, co = ref.match(pose, pts, og)
        pg, cg = g.matchData(pose, pts, None, og)
        expect_single(g, pts.shape[0], (geom, k))
        assert_match(pg, cg, po, co, (geom, layout, k))
        ref.update(pose, pts, og)
        g.updateByScan(pts, pose, og)
        check_maps(oracle_mod, g, ref, rng, (geom, layout, k), probes=k == len(begin_cells(sx, sy)) - 1)
    _, ui = ref.o.download_level(0)
    assert (ui[0] >= 0).any() and (ui[-1] >= 0).any() and (ui[:, 0] >= 0).any() and (ui[:, -1] >= 0).any(), geom
    g.close()


# ----------------------------------------------------------------------------------------------------------- shared builds
def built_pair(capi, oracle_mod, kind, geom, layout="quad", n_build=10, n_query=24, beams=1081):
    """a map made by n_build updates on both sides (bit-identical), then n_query scans of the same loop from perturbed starts"""
    sx, sy, levels = geom
    g = new_ctx(capi, sx, sy, levels, layout)
    ref = Ref(oracle_mod, kind, sx, sy, levels)
    _, poses, scans = rect_cases.scene(sx, sy, n_build + n_query, beams, seed=sx * 17 + sy)
    for t in range(0, n_build + n_query, (n_build + n_query) // n_build):
        # (the coarse levels are updated with the containers of the last matchData: MapRepMultiMap.h:127,143)
        po, co = ref.match(poses[t], scans[t])
        pg, cg = g.matchData(poses[t], scans[t])
        expect_single(g, scans[t].shape[0], (geom, "build", t))
        assert_match(pg, cg, po, co, (geom, "build", t))
        ref.update(poses[t], scans[t])
        g.updateByScan(scans[t], poses[t])
    check_maps(None, g, ref, None, (geom, "build"), probes=False)
    rng = np.random.default_rng([sx, sy, 3])
    qi = [t for t in range(n_build + n_query) if t % ((n_build + n_query) // n_build)][:n_query]
    init = np.stack([poses[t] + np.array([rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), rng.uniform(-0.02, 0.02)],
                                         np.float32) for t in qi]).astype(np.float32)
    return g, ref, init, [scans[t] for t in qi], [poses[t] for t in qi]


# ------------------------------------------------------------------------------------------------------------ c. batches
@pytest.mark.parametrize("geom", rect_cases.SMALL, ids=rect_cases.gid)
def test_batches(capi, oracle_mod, kind, geom, monkeypatch):
    """hsm_match_batch on a rectangle: a ragged batch (empty, 1, 63 / 64 / 65 beams, full) and a shared scan, each scan
    bit-identical to the checker's matchData; the given / Morton / automatic order (every batch sorted where the order asks for
    it) give the same bits; hsm_match_batch_ranges on raw ranges equals the endpoint entry"""
    from hector_slam_amd import synth
    g, ref, init, scans, truth = built_pair(capi, oracle_mod, kind, geom)
    sx, sy, levels = geom
    rng = np.random.default_rng([sx, sy, 5])
    query = []
    for q, sq in enumerate(scans):
        n = [sq.shape[0], 0, 1, 63, 64, 65, 700, sq.shape[0]][q % 8]
        query.append(np.ascontiguousarray(sq[np.sort(rng.choice(sq.shape[0], size=min(n, sq.shape[0]), replace=False))]))
    pts, offs = synth.pack_scans(query)
    pb, cb = g.match_batch(init, pts, offs)
    expect_batch(g, geom)
    assert not g.last_launch_sorted()
    for q, sq in enumerate(query):
        po, co = ref.match(init[q], sq)
        if sq.shape[0] == 0:
            assert same(pb[q], init[q]), q
            continue
        assert_match(pb[q], cb[q], po, co, (geom, q, sq.shape[0]))
    # the shared-scan form: nine start poses of one scan
    hyp = (np.repeat(init[:1], 9, 0) + np.linspace(-0.05, 0.05, 9, dtype=np.float32)[:, None]).astype(np.float32)
    ph, ch = g.match_batch(hyp, scans[0], None)
    expect_batch(g, (geom, "shared"))
    for k in range(9):
        po, co = ref.match(hyp[k], scans[0])
        assert_match(ph[k], ch[k], po, co, (geom, "shared", k))
    # batch orders: the same bits whichever order the batch runs in
    monkeypatch.setenv("HSM_BATCH_ORDER_MIN", "1")
    for order, sorted_ in (("given", False), ("morton", True), ("auto", False)):  # (auto sorts maps above 2^23 cells only)
        monkeypatch.setenv("HSM_BATCH_ORDER", order)
        m = new_ctx(capi, sx, sy, levels)
        for lvl in range(levels):
            m.upload_level(lvl, *ref.o.download_level(lvl))
        p2, c2 = m.match_batch(init, pts, offs)
        expect_batch(m, (geom, order))
        assert m.last_launch_sorted() == sorted_, order
        assert same(p2, pb) and same(c2, cb), order
        m.close()
    monkeypatch.delenv("HSM_BATCH_ORDER")
    # raw LaserScan ranges, with a driver's drop-outs: the ranges entry == the endpoint entry on the node's conversion
    n = 1081
    a0, inc = synth.SCAN_SHAPES[n] if n in synth.SCAN_SHAPES else (-np.pi, 2.0 * np.pi / n)
    a0, inc = float(np.float32(a0)), float(np.float32(inc))
    world = rect_cases.world_for(sx, sy, RES, 0.9, sx * 17 + sy)
    r = np.stack([world.raycast(p, synth.beam_angles(n)) for p in truth]) + rng.normal(0.0, 0.01, (len(truth), n))
    r = r.astype(np.float32)
    drop = rng.random(r.shape)
    r[drop < 0.02] = np.inf
    r[(drop >= 0.02) & (drop < 0.03)] = np.nan
    pr, cr, cnt = g.match_batch_ranges(init, r, a0, inc, RANGE_MIN, RANGE_MAX)
    expect_batch(g, (geom, "ranges"))
    counts, roffs, rpts = synth.ranges_to_csr(r, a0, inc, RANGE_MIN, RANGE_MAX, g.getScaleToMap())
    assert np.array_equal(cnt, counts)
    pe, ce = g.match_batch(init, rpts, roffs)
    assert same(pr, pe) and same(cr, ce)
    g.close()


# ------------------------------------------------------------------------------------------------------------- d. probes
def border_states(sx, sy, rng):
    """map-frame states next to all four borders and the corners, plus the centre"""
    xy = [(1.5, sy * 0.5), (sx - 2.5, sy * 0.5), (sx * 0.5, 1.5), (sx * 0.5, sy - 2.5), (1.2, 1.3), (sx - 2.2, sy - 2.4),
          (sx * 0.5, sy * 0.5), (sx - 2.0, 0.4)]
    return np.array([(x, y, rng.uniform(-np.pi, np.pi)) for x, y in xy], np.float32)


@pytest.mark.parametrize("layout", ["quad", "plane"])
@pytest.mark.parametrize("geom", rect_cases.SMALL, ids=rect_cases.gid)
def test_probes(capi, oracle_mod, kind, geom, layout):
    """hessian_derivs, likelihood / residual states, the sigma-point covariances and the occupancy grid at states along the
    four borders; ray distances; row and cell windows in the far corner; the update boxes"""
    g, ref, init, scans, _ = built_pair(capi, oracle_mod, kind, geom, layout)
    sx, sy, levels = geom
    o = ref.o
    rng = np.random.default_rng([sx, sy, 9])
    for lvl in range(levels):
        lsx, lsy = sx >> lvl, sy >> lvl
        f = np.float32(1.0 / 2 ** lvl)
        states = border_states(lsx, lsy, rng)
        cloud = (states[rng.integers(0, len(states), 300)] + rng.normal(0, [2.0, 2.0, 0.05], (300, 3))).astype(np.float32)
        states = np.concatenate([states, cloud, np.array([[-50.0, 3.0, 0.1]], np.float32)])
        for q in range(3):
            pts = scans[q][: [1081, 300, 65][q]]
            for s in states[:8]:
                Hg, dg = g.hessian_derivs(lvl, s, pts * f)
                Ho, do = o.hessian_derivs(lvl, s, pts * f)
                assert same(Hg, Ho) and same(dg, do), (geom, lvl, q, s)
            assert same(g.likelihood_states(lvl, states, pts), o.likelihood_states(lvl, states, pts * f)), (geom, lvl, q)
            assert same(g.residual_states(lvl, states, pts), o.residual_states(lvl, states, pts * f)), (geom, lvl, q)
            cm, cw, lh = g.covariance_for_poses(lvl, states[:24], pts)
            om, ow, ol = o.covariance_for_poses(lvl, states[:24], pts * f)
            assert same(lh, ol) and same(cm, om) and same(cw, ow), (geom, lvl, q)
        grid = o.occupancy_grid(lvl)
        assert np.array_equal(g.occupancy_grid(lvl), grid), (geom, lvl)
        # ray distances on the level's grid: rays inside, leaving and starting outside the map, axis-aligned, zero length
        ox, oy, res = g.map_metadata(lvl)
        n = 4000
        ext = np.array([lsx * res, lsy * res])
        begin = (np.array([ox, oy]) + rng.uniform(-0.05, 1.05, (n, 2)) * ext).astype(np.float32)
        ang = rng.uniform(0, 2 * np.pi, n)
        length = rng.uniform(0.0, 1.2, n) * ext.max()
        end = (begin + np.stack([np.cos(ang), np.sin(ang)], 1) * length[:, None]).astype(np.float32)
        end[:40] = begin[:40]
        end[40:80, 1] = begin[40:80, 1]
        end[80:120, 0] = begin[80:120, 0]
        dist, hit = g.ray_distances(lvl, begin, end)
        rd, rh = oracle_mod.ray_distances("ho", grid, (ox, oy), res, begin, end)
        assert same(dist, rd), (geom, lvl, int((bits(dist) != bits(rd)).sum()))
        has = rd >= 0
        assert same(hit[has], rh[has]) and np.isnan(hit[~has]).all(), (geom, lvl)
        assert 0 < has.sum() < n, has.mean()
        # windows in the far corner
        lo_o, ui_o = o.download_level(lvl)
        y0 = max(lsy - 5, 0)
        assert same(g.download_rows(lvl, y0, lsy), lo_o[y0:]), (geom, lvl)
        x0, y0 = max(lsx - 7, 0), max(lsy - 3, 0)
        cells = np.zeros((lsy - y0, lsx - x0, 2), np.int32)
        capi._check(g._lib.hsm_download_cells(g._h, lvl, x0, y0, lsx - 1, lsy - 1, cells.ctypes.data, lsx - x0), "download_cells")
        assert same(cells[..., 0].view(np.float32), lo_o[y0:, x0:]) and np.array_equal(cells[..., 1], ui_o[y0:, x0:]), (geom, lvl)
    # update boxes: each contains every cell the update changed, and is no wider than the hull of the in-map end cells and the
    # begin cell (coarser levels may derive their box from the finer one's: one cell more on each side)
    for lvl in range(levels):
        g.take_dirty_bbox(lvl)
    for q in range(6):
        pose, pts = init[q], scans[q]
        before = [o.download_level(lvl) for lvl in range(levels)]
        ref.match(pose, pts)
        o = ref.o  # (the checker the match left: see Ref.match)
        g.matchData(pose, pts)
        ref.update(pose, pts)
        g.updateByScan(pts, pose)
        g.synchronize()
        for lvl in range(levels):
            lo_o, ui_o = o.download_level(lvl)
            ys, xs = np.nonzero((ui_o != before[lvl][1]) | (bits(lo_o) != bits(before[lvl][0])))
            bb, dirty = g.last_update_bbox(lvl), g.take_dirty_bbox(lvl)
            if xs.size == 0:
                continue
            assert np.array_equal(bb, dirty), (geom, q, lvl, bb, dirty)
            assert bb[0] <= xs.min() and bb[2] >= xs.max() and bb[1] <= ys.min() and bb[3] >= ys.max(), (geom, q, lvl, bb)
            mp = o.map_coords_pose(lvl, pose).astype(np.float64)
            p = pts.astype(np.float64) / 2 ** lvl
            ex = np.cos(mp[2]) * p[:, 0] - np.sin(mp[2]) * p[:, 1] + mp[0] + 0.5
            ey = np.sin(mp[2]) * p[:, 0] + np.cos(mp[2]) * p[:, 1] + mp[1] + 0.5
            cx, cy = np.floor(ex), np.floor(ey)
            inmap = (cx >= 0) & (cx < sx >> lvl) & (cy >= 0) & (cy < sy >> lvl)
            hx = np.concatenate([cx[inmap], [np.floor(mp[0] + 0.5)]])
            hy = np.concatenate([cy[inmap], [np.floor(mp[1] + 0.5)]])
            slack = 1 if lvl == 0 else 2  # (fp32 rounding at a cell border; the derived box of a coarser level)
            assert bb[0] >= hx.min() - slack and bb[2] <= hx.max() + slack and bb[1] >= hy.min() - slack and bb[3] <= hy.max() + slack, \
                (geom, q, lvl, bb, (hx.min(), hy.min(), hx.max(), hy.max()))
    check_maps(oracle_mod, g, ref, rng, (geom, "after the box updates"))
    g.close()


# -------------------------------------------------------------------------------------------------- e. large rectangles
@pytest.mark.parametrize("geom", rect_cases.LARGE, ids=rect_cases.gid)
def test_large_rectangle_batches(capi, oracle_mod, kind, geom, monkeypatch):
    """level 0 above 2^23 cells, random log-odds uploaded on both sides: a batch of 80 scans (endpoints on the last row and
    column, on cell corners and off the map) bit-identical; the automatic order sorts such a map's batches (above
    HSM_BATCH_ORDER_MIN) -- with a tile shift set by the longer edge only -- and gives the same bits"""
    import gn_cases
    from hector_slam_amd import synth
    sx, sy, _ = geom
    rng = np.random.default_rng([sx, sy])
    lo = rng.uniform(-2.5, 2.5, (sy, sx)).astype(np.float32)
    ui = np.zeros((sy, sx), np.int32)
    ref = Ref(oracle_mod, kind, sx, sy, 1)
    ref.upload(0, lo, ui)
    g = new_ctx(capi, sx, sy, 1)
    g.upload_level(0, lo, ui)
    init, query = [], []
    for j in range(80):
        m = np.array([rng.uniform(0.05, 0.95) * sx, rng.uniform(0.05, 0.95) * sy, 0.0 if j % 3 == 0 else rng.uniform(-3, 3)], np.float32)
        n = [1081, 700, 64, 1000, 1088][j % 5]
        t, _ = gn_cases._targets(sx, sy, m.astype(np.float64), n, rng, radius=300.0)
        c, s = np.cos(float(m[2])), np.sin(float(m[2]))
        dx, dy = t[:, 0] - float(m[0]), t[:, 1] - float(m[1])
        query.append(np.ascontiguousarray(np.stack([c * dx + s * dy, -s * dx + c * dy], 1).astype(np.float32)))
        init.append(ref.o.world_coords_pose(0, m))
    init = np.stack(init).astype(np.float32)
    # the scans do reach the last row / column and leave the map
    allw = np.concatenate([q.astype(np.float64) @ np.array([[np.cos(p[2]), np.sin(p[2])], [-np.sin(p[2]), np.cos(p[2])]])
                           + ref.o.map_coords_pose(0, p)[:2] for q, p in zip(query, init)])
    assert (np.abs(allw[:, 0] - (sx - 2)) < 1e-3).any() and (np.abs(allw[:, 1] - (sy - 2)) < 1e-3).any()
    assert ((allw[:, 0] > sx - 2) | (allw[:, 1] > sy - 2) | (allw < 0).any(1)).sum() > 80
    pts, offs = synth.pack_scans(query)
    pb, cb = g.match_batch(init, pts, offs)
    expect_batch(g, geom)
    assert not g.last_launch_sorted()  # (80 scans: below the default HSM_BATCH_ORDER_MIN)
    for q in range(len(query)):
        po, co = ref.match(init[q], query[q])
        assert_match(pb[q], cb[q], po, co, (geom, q))
    monkeypatch.setenv("HSM_BATCH_ORDER_MIN", "1")
    m2 = new_ctx(capi, sx, sy, 1)
    m2.upload_level(0, lo, ui)
    assert m2.batch_order() == capi.ORDER_AUTO
    p2, c2 = m2.match_batch(init, pts, offs)
    expect_batch(m2, (geom, "auto"))
    assert m2.last_launch_sorted(), "the automatic order sorts batches on maps above 2^23 cells"
    assert same(p2, pb) and same(c2, cb)
    m2.close()
    g.close()


# ----------------------------------------------------------------------------------------------- f. the key generation wrap
@pytest.mark.parametrize("geom", [(640, 192, 3), (192, 640, 3), (333, 90, 2), (90, 333, 2)], ids=rect_cases.gid)
def test_update_serial_wrap(capi, oracle_mod, kind, geom):
    """the 12-bit update generation wraps after 4095 updates and the key rows the updates used are cleared, sx cells per row:
    updates across the wrap bit-exact on every level (1081 and 5000 beams: the keyed and the byte-map update)"""
    sx, sy, levels = geom
    g = new_ctx(capi, sx, sy, levels)
    ref = Ref(oracle_mod, kind, sx, sy, levels)
    _, poses, scans = rect_cases.scene(sx, sy, 16, 1081, seed=sx + 3 * sy)
    _, _, dense = rect_cases.scene(sx, sy, 16, 5000, seed=sx + 3 * sy)
    rng = np.random.default_rng(sx + sy)
    for t in range(16):
        if t == 4:
            for lvl in range(levels):
                capi._check(g._lib.hsm_debug_set_update_serial(g._h, lvl, 4093 - lvl), "set serial")  # wraps at t = 6..8
        pts = dense[t] if t % 3 == 2 else scans[t]
        po, co = ref.match(poses[t], pts)
        pg, cg = g.matchData(poses[t], pts)
        expect_single(g, pts.shape[0], (geom, t))
        assert_match(pg, cg, po, co, (geom, t))
        ref.update(poses[t], pts)
        g.updateByScan(pts, poses[t])
        check_maps(oracle_mod, g, ref, rng, (geom, t), probes=t == 15)
    for lvl in range(levels):
        assert np.array_equal(g.occupancy_grid(lvl), ref.o.occupancy_grid(lvl))
    g.close()


# ---------------------------------------------------------------------------------------------------- g. hsm_create limits
def test_create_validation_is_symmetric(capi, oracle_mod, kind):
    """a level with fewer than 2 rows or columns is refused on either axis; 2 rows or columns are accepted on either axis, and
    a match plus an update on such a map stay bit-exact"""
    for sx, sy in ((1024, 6), (6, 1024)):
        with pytest.raises(capi.HsmError, match="too many levels"):
            capi.MapRepMultiMap(RES, sx, sy, 3)
    for sx, sy in ((1024, 8), (8, 1024)):
        g = new_ctx(capi, sx, sy, 3)
        ref = Ref(oracle_mod, kind, sx, sy, 3)
        _, poses, scans = rect_cases.scene(sx, sy, 4, 1081, seed=sx * sy)
        for t in range(4):
            po, co = ref.match(poses[t], scans[t])
            pg, cg = g.matchData(poses[t], scans[t])
            expect_single(g, scans[t].shape[0], (sx, sy, t))
            assert_match(pg, cg, po, co, (sx, sy, t))
            ref.update(poses[t], scans[t])
            g.updateByScan(scans[t], poses[t])
            check_maps(oracle_mod, g, ref, None, (sx, sy, t), probes=False)
        _, ui = ref.o.download_level(2)
        assert ui.shape == (sy >> 2, sx >> 2) and (ui >= 0).any()
        g.close()
    # the level count: 8 at most, and no level below 2 cells on either axis
    with pytest.raises(capi.HsmError, match="bad map geometry"):
        capi.MapRepMultiMap(RES, 4096, 4096, 9)
    for sx, sy in ((255, 255), (256, 255), (255, 256)):
        with pytest.raises(capi.HsmError, match="too many levels"):
            capi.MapRepMultiMap(RES, sx, sy, 8)
    g = new_ctx(capi, 256, 511, 8)
    o = oracle_mod.Oracle(kind, RES, 256, 511, 8)
    assert [g.level_info(l) for l in range(8)] == [o.level_info(l) for l in range(8)]
    assert g.level_info(7)[:2] == (2, 3) and g.getMapLevels() == 8
    g.close()


# ------------------------------------------------------------------------------------------------ h. the seeded property
@seed(rect_cases.RECT_SEED)
@settings(max_examples=20, deadline=None, database=None, suppress_health_check=list(HealthCheck))
@given(g=rect_cases.rect_geometry())
def test_default_mode_equals_reference_for_random_rectangles(oracle_mod, g):
    """the examples tests/test_oracle_vs_reference.py pins on the CPU: the library default (no parity argument), every pose,
    covariance and map of the loop bit-identical, the mark planes clear after every update"""
    from hector_slam_amd import capi

    def make_gpu(res, sx, sy, levels, start, free, occ):
        m = capi.MapRepMultiMap(res, sx, sy, levels, start)
        assert m.parity() == capi.PARITY_AUTO
        m.setUpdateFactorFree(free)
        m.setUpdateFactorOccupied(occ)

        def match(h, sc, og):
            out = m.matchData(h, sc, None, og)
            assert m.last_launch_config()["parity_effective"] == "exact"
            return out

        def check(gg, t):
            for lvl in range(levels):
                assert m.debug_marks_nonzero(lvl) == (0, 0), (gg, t, lvl)
        return {"match": match, "update": lambda p, sc, og: m.updateByScan(sc, p, og), "level": m.download_level, "keep": m,
                "check": check}
    kind = oracle_kinds()[-1]
    rect_cases.run_loop(g, make_gpu, rect_cases.oracle_impl(oracle_mod, kind),
                        make_guard=rect_cases.oracle_impl(oracle_mod, "ho") if kind == "hr" else None)
