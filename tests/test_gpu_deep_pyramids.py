"""Deep pyramids (tests/deep_cases.py: 6 to 8 levels, coarsest levels of 64 x 64 down to 2 x 2 cells, odd sizes on the way down,
and one 4096^2 map of 8 levels) in the library's DEFAULT mode (the reference's summation order): every entry point bit-identical
to the CPU checker on every level, the deepest included.  What depends on the level count or on a level's size -- the LevelView
parameter block, the update launches' per-level grid dimension, the per-level slices of the beam records and update boxes, the
boxes the coarse levels derive from level 0, the 2^-l container scale, the mark / quad tiles and the row-aligned apply path on a
level smaller than one tile, the retained scan for seven coarse containers -- is not reached by the rest of the suite, which stops
at 3 levels and at 8 cells.

Every case is checked on the CPU first (deep_cases.check: no level empty, the reference's H regular for at least half of the
query scans on every level of 16 cells or more, no map read at a NaN coordinate), so a comparison here is not one of zeros; where
the checker is the reference itself ("hr") the restatement runs ahead of it on every new input, and a NaN read there fails the
test: the reference would crash on it, and that is a mistake in the case list."""
import ctypes as C

import numpy as np
import pytest

import deep_cases
import gn_f64
import select_rule
from conftest import bits
from support import capi, dev, kind, new_context, same

pytestmark = pytest.mark.gpu

RES = deep_cases.RES
ZERO2 = np.zeros(2, np.float32)
HSM_ERR_INVALID = -1
SENTINEL = -777.0
LAYOUTS = ["quad", "plane"]
BIG = [(2048, 2048, 6), deep_cases.LARGE]  # the batch sizes of the benchmark (4096) run on these two


_CASES: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_caches():
    """the cases and batch references (a 4096^2 x 8-level checker among them) live as long as this module's tests"""
    yield
    _CASES.clear()
    _BATCH_REF.clear()
    _BATCH_HO.clear()


def case_of(oracle_mod, geom):
    """the geometry's scene, checked on the CPU (a case the reference is undefined on, or blind on, fails here)"""
    if geom not in _CASES:
        c = deep_cases.case(geom)
        share = deep_cases.check(oracle_mod, c)
        print(f"{deep_cases.gid(geom)}: share of the query scans with a regular reference H per level "
              f"{ {l: round(float(s), 2) for l, s in share.items()} }")
        _CASES[geom] = c
    return _CASES[geom]


class Ref:
    """the CPU checker of `kind` holding the case's built map; for "hr" with the restatement alongside, asked first"""

    def __init__(self, oracle_mod, kind, case, build=True):
        make = deep_cases.built_oracle if build else (lambda m, k, c: deep_cases.new_oracle(m, k, c.geom))
        self.o = make(oracle_mod, kind, case)
        self.guard = make(oracle_mod, "ho", case) if kind == "hr" else None
        self.levels = case.levels

    def all(self):
        return (self.o,) if self.guard is None else (self.guard, self.o)

    def defined(self, what, since=0):
        g = self.guard or self.o
        assert g.undefined_reads() == since, (what, "the reference is undefined on this input: a mistake in the case list")

    def match(self, pose, pts, origo=ZERO2):
        u0 = (self.guard or self.o).undefined_reads()
        for x in self.all():
            out = x.match(pose, pts, origo, cov=np.zeros(9, np.float32))
            self.defined(("match", pose), u0)
        return out

    def match_many(self, init, pts, offs, known=None, every=1):
        """the checker's matchData of every scan of a CSR batch (`known`: the restatement's result, where a caller holds it;
        `every`: the reference runs on every n-th of the rows it is defined on -- the restatement, pinned to it on these very
        cases by tests/test_oracle_vs_reference.py, stands for the others).  A scan of one beam (and now and then one of a few dozen) gives
        a singular H: the reference divides by a zero determinant and then indexes its grid with (int)NaN.  Those rows are the
        restatement's (non-finite: compared NaN for NaN), and the reference is run on the others only."""
        first = self.guard or self.o
        out = first.match_many(init, pts, offs) if known is None else known.copy()
        if self.guard is not None:
            ok = np.flatnonzero(np.isfinite(out).all(1))[::every]
            from hector_slam_amd import synth
            sub_pts, sub_offs = synth.pack_scans([pts[offs[b]:offs[b + 1]] for b in ok])
            got = self.o.match_many(np.ascontiguousarray(init[ok]), sub_pts, sub_offs)
            assert every == 1 or same(got, out[ok]), "restatement != reference"
            out[ok] = got
        return out

    def match_level(self, lvl, init, pts_level, it):
        """the checker's single-level matchData; the restatement's where the reference would read the map at a NaN coordinate"""
        first = self.guard or self.o
        u0 = first.undefined_reads()
        out = first.match_level(lvl, init, pts_level, it)
        if self.guard is None or first.undefined_reads() != u0 or not np.isfinite(out[0]).all():
            return out
        return self.o.match_level(lvl, init, pts_level, it)

    def update(self, pose, pts, origo=ZERO2):
        for x in self.all():
            x.update_by_scan(pose, pts, origo)
            x.on_map_updated()

    def build(self, poses, scans, origo=ZERO2):
        """every level at the given pose with the level-scaled container: what hsm_update_by_scans_device integrates"""
        for x in self.all():
            x.build_map(np.asarray(poses, np.float32).reshape(-1, 3), scans, origo)


def new_ctx(capi, geom, layout="quad", **kw):
    sx, sy, levels = geom
    g = new_context(capi, RES, sx, sy, levels, layout=layout, **kw)
    assert g.parity() == capi.PARITY_AUTO and g.getMapLevels() == levels
    assert [g.level_info(l)[:2] for l in range(levels)] == deep_cases.level_sizes(sx, sy, levels)
    return g


def uploaded_ctx(capi, geom, o, layout="quad", **kw):
    g = new_ctx(capi, geom, layout, **kw)
    for lvl in range(geom[2]):
        g.upload_level(lvl, *o.download_level(lvl))
    g.synchronize()
    return g


def built_ctx(capi, case, layout="quad"):
    """the case's map made by the library itself: hsm_update_by_scan_level on every level, as the checker's build_map"""
    g = new_ctx(capi, case.geom, layout)
    g.build_map(case.build_poses, case.build_scans)
    g.synchronize()
    return g


def check_planes(g, o, levels, what, update_index=None):
    """log-odds and update index of every level bit-identical, the mark planes clear, hsm_update_index as counted"""
    for lvl in range(levels):
        (lo_g, ui_g), (lo_o, ui_o) = g.download_level(lvl), o.download_level(lvl)
        assert np.array_equal(ui_g, ui_o), (what, lvl, int((ui_g != ui_o).sum()))
        assert same(lo_g, lo_o), (what, lvl, int((bits(lo_g) != bits(lo_o)).sum()))
        assert g.debug_marks_nonzero(lvl) == (0, 0), (what, lvl)
        if update_index is not None:
            assert g.getUpdateIndex(lvl) == update_index, (what, lvl, g.getUpdateIndex(lvl), update_index)


def oracle_planes(o, levels):
    return [o.download_level(lvl) for lvl in range(levels)]


def changed_cells(p0, p1):
    (lo0, ui0), (lo1, ui1) = p0, p1
    return np.nonzero((ui0 != ui1) | (bits(lo0) != bits(lo1)))


def check_boxes(g, before, after, what, before_last=None):
    """hsm_take_dirty_bbox of every level contains every cell the update(s) since `before` changed; hsm_last_update_bbox, the box
    of the last scan integrated, every cell that scan changed: all of them after a single scan, those since `before_last` (the
    planes before the last scan of a call of several)"""
    changed = 0
    for lvl in range(len(before)):
        last, dirty = g.last_update_bbox(lvl), g.take_dirty_bbox(lvl)
        shape = before[lvl][0].shape
        for name, bb, (ys, xs) in (("dirty", dirty, changed_cells(before[lvl], after[lvl])),
                                   ("last", last, changed_cells((before_last or before)[lvl], after[lvl]))):
            if xs.size == 0:
                continue
            changed += name == "dirty"
            assert bb[0] <= xs.min() and bb[2] >= xs.max() and bb[1] <= ys.min() and bb[3] >= ys.max(), \
                (what, name, lvl, bb, (xs.min(), ys.min(), xs.max(), ys.max()))
            assert bb[0] >= 0 and bb[1] >= 0 and bb[2] < shape[1] and bb[3] < shape[0], (what, name, lvl, bb)
        assert np.array_equal(g.take_dirty_bbox(lvl), np.int32([0, 0, -1, -1])), (what, lvl)
    return changed


def assert_match(pg, cg, po, co, what):
    assert np.isfinite(po).all(), (what, po)  # (deep_cases.check: none of these inputs makes the reference's H singular)
    assert same(pg, po) and same(cg, co), (what, pg, po)


# ------------------------------------------------------------------------------------------ 1. the SLAM loop on a built map
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("geom", deep_cases.GEOMETRIES, ids=deep_cases.gid)
def test_slam_loop_on_a_built_map(capi, oracle_mod, kind, geom, layout):
    """hsm_match, then hsm_update_by_scan at the matched pose, 8 steps with a laser origin off the robot's centre, one of them a
    scan of more than 4096 beams (the dense matcher and the byte-map mark path): every pose and covariance, and after every
    update the log-odds and update index of every level, hsm_update_index, the two boxes and the mark planes"""
    case = case_of(oracle_mod, geom)
    L = case.levels
    ref = Ref(oracle_mod, kind, case)
    g = built_ctx(capi, case, layout)
    n = len(case.build_scans)
    check_planes(g, ref.o, L, (geom, "built"), update_index=n - 1)
    for lvl in range(L):
        assert (ref.o.download_level(lvl)[0] != 0).any(), (geom, lvl)
        g.take_dirty_bbox(lvl)
    steps, dense, boxed = 8, 0, 0
    for t in range(steps):
        q = t % len(case.query_scans)
        hint, pts = (case.dense_pose, case.dense) if t == steps // 2 else (case.query_init[q], case.query_scans[q])
        before = oracle_planes(ref.o, L)
        po, co = ref.match(hint, pts, case.origo)
        pg, cg = g.matchData(hint, pts, None, case.origo)
        cfg = g.last_launch_config()
        assert cfg["parity_effective"] == "exact", cfg
        if pts.shape[0] >= 4096:
            assert cfg["kernel"] == "gn_match_exact_dense_kernel", cfg
            dense += 1
        assert_match(pg, cg, po, co, (geom, layout, t))
        ref.update(po, pts, case.origo)
        g.updateByScan(pts, po, case.origo)
        g.synchronize()
        check_planes(g, ref.o, L, (geom, layout, t), update_index=n + t)
        boxed += check_boxes(g, before, oracle_planes(ref.o, L), (geom, layout, t))
    assert dense == 1 and boxed >= steps * 4, (dense, boxed)  # (a level of a few cells does not change on every update)
    g.close()


# ------------------------------------------------------------------------------------------------------------ 2. the trace
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("geom", deep_cases.GEOMETRIES, ids=deep_cases.gid)
def test_match_trace_has_a_record_for_every_step_of_every_level(capi, oracle_mod, kind, geom, layout):
    """hsm_match_trace with room for 6 + 4 (L - 1) records (34 on 8 levels): as many records as hsm_gn_iterations_per_match;
    record k's H is the checker's getCompleteHessianDerivs at the estimate step k started from (the level's start pose, then the
    record before), its estimate the checker's single-level matchData of as many iterations, taken to the world frame; the last
    record of a level carries the covariance that level's matchData returns.  One record short: refused, nothing written."""
    case = case_of(oracle_mod, geom)
    L = case.levels
    ref = Ref(oracle_mod, kind, case)
    o = ref.o
    g = uploaded_ctx(capi, geom, o, layout)
    lib = capi.load_library()
    cap = deep_cases.gn_steps(L)
    assert g.gn_iterations_per_match() == cap and (L < 8 or cap == 34)
    for q in (0, 5, 10, 15):
        init, pts = case.query_init[q], np.ascontiguousarray(case.query_scans[q], np.float32)
        po, co = ref.match(init, pts)
        pose, cov, trace, nst = np.zeros(3, np.float32), np.zeros(9, np.float32), np.zeros(cap * 12, np.float32), C.c_int(-1)
        capi._check(lib.hsm_match_trace(g._h, init, pts.ctypes.data, pts.shape[0], ZERO2, pose, cov, trace, cap, C.byref(nst)),
                    "hsm_match_trace")
        assert nst.value == cap
        assert_match(pose, cov, po, co, (geom, q))
        trace = trace.reshape(cap, 12)
        chain, est, _ = deep_cases.level_chain(o, init, pts, L)
        assert same(est, po)
        k = 0
        for lvl, start, p, it in chain:
            at = o.map_coords_pose(lvl, start)
            for j in range(it + 1):
                Ho, _ = o.hessian_derivs(lvl, at, p)
                assert same(trace[k, 3:].reshape(3, 3).T, Ho), (geom, q, "H", lvl, j)
                wo, cj = o.match_level(lvl, start, p, j)
                w = o.world_coords_pose(lvl, trace[k, :3])
                w[2] = np.float32(o.normalize_angle(w[2]))
                assert same(w, wo), (geom, q, "estimate", lvl, j, w, wo)
                at = trace[k, :3].copy()
                k += 1
            assert same(trace[k - 1, 3:], cj), (geom, q, "the level's covariance", lvl)
        assert k == cap
        # one record short of what the match writes
        pose2, cov2, short, nst2 = np.full(3, SENTINEL, np.float32), np.full(9, SENTINEL, np.float32), \
            np.full((cap - 1) * 12, SENTINEL, np.float32), C.c_int(-5)
        rc = lib.hsm_match_trace(g._h, init, pts.ctypes.data, pts.shape[0], ZERO2, pose2, cov2, short, cap - 1, C.byref(nst2))
        assert rc == HSM_ERR_INVALID and nst2.value == -5
        assert (pose2 == SENTINEL).all() and (cov2 == SENTINEL).all() and (short == SENTINEL).all()
    g.close()


# ---------------------------------------------------------------------------------------------------------- 3. the batches
def batch_inputs(case, B, seed):
    """B hints within +-0.15 m / +-0.05 rad of the query poses, each with its scan cut to a length of the cycle
    (whole, 0, 1, 63, 64, 65, 700, whole).  The 4096 batch takes every second beam of the scans (541 beams: the checker's time
    is the test's time there); the batches of 16 and 257 carry the whole 1081."""
    from hector_slam_amd import synth
    rng = np.random.default_rng([case.geom[0], case.geom[1], B, seed])
    Q = len(case.query_scans)
    truth = np.stack([case.query_truth[b % Q] for b in range(B)])
    init = synth.perturb_poses(truth, rng)
    scans = []
    for b in range(B):
        sq = case.query_scans[b % Q][:: 2 if B >= 4096 else 1]
        n = [sq.shape[0], 0, 1, 63, 64, 65, 700, sq.shape[0]][(b // Q + b) % 8] if b % 3 == 1 else sq.shape[0]
        scans.append(sq[:n])
    return init, scans


_BATCH_REF: dict = {}
_BATCH_HO: dict = {}  # (geom, B) -> the restatement's poses, computed once for both checkers


def batch_reference(oracle_mod, kind, case, B):
    """(init, scans, packed points, offsets, the checker's poses, its (pose, cov) of the first 16 one by one); cached for the
    second layout"""
    from hector_slam_amd import synth
    key = (case.geom, kind, B)
    if key not in _BATCH_REF:
        ref = Ref(oracle_mod, kind, case)
        init, scans = batch_inputs(case, B, 1)
        pts, offs = synth.pack_scans(scans)
        known = _BATCH_HO.get((case.geom, B), (None, None))
        every = 16 if B >= 4096 else 1  # (the reference on every 16th scan of the 4096 batch, on every scan of the others)
        poses = ref.match_many(init, pts, offs, known[0], every)
        first = [ref.match(init[b], scans[b]) if np.isfinite(poses[b]).all() else None for b in range(16)]
        hyp = synth.perturb_poses(np.repeat(case.query_truth[3:4], B if B <= 257 else 16, 0), np.random.default_rng(B))
        shared = case.query_scans[3]
        hp = ref.match_many(hyp, *synth.pack_scans([shared] * len(hyp)), known[1])
        if kind == "ho":
            _BATCH_HO[(case.geom, B)] = (poses, hp)
        _BATCH_REF[key] = dict(ref=ref, init=init, scans=scans, pts=pts, offs=offs, poses=poses, first=first, hyp=hyp, shared=shared,
                               hyp_poses=hp)
    return _BATCH_REF[key]


def device_batch(g, init, pts, offs, shared_n=0):
    """hsm_match_batch_device on torch buffers -> (poses, covs) on the host"""
    import torch
    B = len(init)
    d_i, d_p = dev(init), dev(pts if len(pts) else np.zeros((1, 2), np.float32))
    d_o = None if offs is None else dev(offs)
    pose = torch.full((B, 3), SENTINEL, dtype=torch.float32, device="cuda:0")
    cov = torch.full((B, 9), SENTINEL, dtype=torch.float32, device="cuda:0")
    s = torch.cuda.current_stream()
    g.match_batch_device(B, d_i.data_ptr(), d_p.data_ptr(), 0 if d_o is None else d_o.data_ptr(), shared_n, pose.data_ptr(),
                         cov.data_ptr(), s.cuda_stream)
    s.synchronize()
    return pose.cpu().numpy(), cov.cpu().numpy()


def same_rows(pg, po):
    """rows bit for bit where the checker's are finite, NaN for NaN elsewhere (a singular H: NaN payloads are not pinned)"""
    fin = np.isfinite(po).all(1)
    return bool((bits(pg[fin]) == bits(po[fin])).all() and np.array_equal(np.isnan(pg[~fin]), np.isnan(po[~fin])))


def check_batch(r, pb, cb, what):
    lens = np.diff(r["offs"])
    fin = np.isfinite(r["poses"]).all(1)
    assert fin[lens == lens.max()].mean() >= 0.95 and fin[lens == 0].all(), (what, fin.mean())  # (the whole scans)
    bad = np.flatnonzero((bits(pb) != bits(r["poses"])).any(1) & fin)
    assert bad.size == 0, (what, f"{bad.size} of {len(pb)} poses differ", bad[:8], lens[bad[:8]])
    assert np.array_equal(np.isnan(pb[~fin]), np.isnan(r["poses"][~fin])), what
    assert same(pb[lens == 0], r["init"][lens == 0])
    for b, first in enumerate(r["first"]):
        if lens[b] and first is not None:
            assert same(cb[b], first[1]), (what, "covariance", b)
    assert (lens == 0).any() and (lens == 1).any()
    moved = (bits(r["poses"]) != bits(r["init"])).any(1)
    assert moved[lens > 1].mean() > 0.9, what  # (the matches do take steps)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("geom", deep_cases.GEOMETRIES + [deep_cases.LARGE], ids=deep_cases.gid)
def test_batches(capi, oracle_mod, kind, geom, layout, monkeypatch):
    """hsm_match_batch and hsm_match_batch_device against the checker's match_many: 16 and 257 scans (4096 too on the two large
    maps) in CSR form with scans of 0 and 1 beams among them, and the shared-scan form; on the 4096^2 map also the Morton and
    the automatic order on a shuffled batch"""
    case = case_of(oracle_mod, geom)
    sizes = (16, 257, 4096) if geom in BIG else (16, 257)
    g = None
    for B in sizes:
        r = batch_reference(oracle_mod, kind, case, B)
        if g is None:
            g = uploaded_ctx(capi, geom, r["ref"].o, layout)
        pb, cb = g.match_batch(r["init"], r["pts"], r["offs"])
        cfg = g.last_launch_config()
        assert cfg["parity_effective"] == "exact", cfg
        check_batch(r, pb, cb, (geom, layout, B, "host arrays"))
        pd, cd = device_batch(g, r["init"], r["pts"], r["offs"], 1081)
        assert g.last_launch_config()["parity_effective"] == "exact"
        live = (np.diff(r["offs"]) > 0) & np.isfinite(pb).all(1)
        assert same_rows(pd, pb) and same(cd[live], cb[live]), (geom, layout, B, "device pointers")
        ph, ch = g.match_batch(r["hyp"], r["shared"], None)
        assert same_rows(ph, r["hyp_poses"]) and np.isfinite(r["hyp_poses"]).all(1).mean() >= 0.75, (geom, layout, B, "shared scan")
        pdh, cdh = device_batch(g, r["hyp"], r["shared"], None, len(r["shared"]))
        assert same_rows(pdh, ph) and same(cdh[np.isfinite(ph).all(1)], ch[np.isfinite(ph).all(1)]), (geom, layout, B, "shared scan, device pointers")
    if geom == deep_cases.LARGE:
        B = 4096
        perm = np.random.default_rng(5).permutation(B)
        init = r["init"][perm]
        from hector_slam_amd import synth
        pts, offs = synth.pack_scans([r["scans"][b] for b in perm])
        monkeypatch.setenv("HSM_BATCH_ORDER_MIN", "1")
        for order in ("morton", "auto"):
            m = uploaded_ctx(capi, geom, r["ref"].o, layout)
            if order == "morton":
                m.set_batch_order(capi.ORDER_MORTON)
            assert m.batch_order() == (capi.ORDER_MORTON if order == "morton" else capi.ORDER_AUTO)
            p2, c2 = m.match_batch(init, pts, offs)
            if layout == "quad":  # (the batch order applies to the texel-cache forms: every batch of the quad layout)
                assert m.last_launch_sorted(), order
            fin = np.isfinite(p2).all(1)
            assert same_rows(p2, r["poses"][perm]) and same(c2[fin], cb[perm][fin]), (geom, layout, order)
            m.close()
    g.close()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("geom", deep_cases.GEOMETRIES + [deep_cases.LARGE], ids=deep_cases.gid)
def test_fast_mode_batch_one_step_against_float64(capi, oracle_mod, geom, layout):
    """HSM_PARITY_FAST: one Gauss-Newton step of a batch on level 3 and on the deepest level (hsm_debug_set_schedule): H entry by
    entry within the float64 bound of the launched form's addition depth (tests/gn_f64.py), the step through check_step"""
    from hector_slam_amd import synth
    case = case_of(oracle_mod, geom)
    L = case.levels
    o = deep_cases.built_oracle(oracle_mod, "ho", case)
    g = uploaded_ctx(capi, geom, o, layout)
    g.set_parity(capi.PARITY_FAST)
    init, scans = batch_inputs(case, 16, 2)
    pts, offs = synth.pack_scans(scans)
    for lvl in (3, L - 1):
        g.debug_set_schedule(lvl, 1)
        pose, cov = g.match_batch(init, pts, offs)
        cfg = g.last_launch_config()
        assert cfg["parity_effective"] == "fast" and cfg["kernel"] in ("gn_match_cached_kernel", "gn_match_kernel"), cfg
        W = cfg["waves_per_scan"]
        assert W >= 1, cfg
        regular = stepped = 0
        f = np.float32(1.0 / 2.0 ** lvl)
        for b, sb in enumerate(scans):
            if sb.shape[0] == 0:
                assert same(pose[b], init[b])
                continue
            start = o.map_coords_pose(lvl, init[b])
            ev = gn_f64.Eval64(o, lvl, start, sb * f, "ho")
            d = gn_f64.depth_team(sb.shape[0], W)
            Hg = cov[b].reshape(3, 3).T
            gn_f64.check_H(Hg, ev, d, f"{geom} L{lvl} scan {b}")
            if int(ev.nonzero().sum()) >= 3 and Hg[0, 0] != 0 and Hg[1, 1] != 0:
                regular += 1
                if np.isfinite(pose[b]).all():
                    end = g.getMapCoordsPose(lvl, pose[b])
                    # (a step across +-pi: normalize_angle wrapped the result; taken back to the start's turn, in fp32)
                    end[2] += np.float32(2 * np.pi) * np.float32(np.round((float(start[2]) - float(end[2])) / (2 * np.pi)))
                    stepped += gn_f64.check_step(Hg, start, end, ev, d, f"{geom} L{lvl} scan {b}")
            elif Hg[0, 0] == 0 or Hg[1, 1] == 0:  # the reference's own test for taking a step: none, and no sum in the result
                assert same(pose[b], o.match_level(lvl, init[b], sb * f, 0)[0]), (geom, lvl, b)
        if min(geom[0] >> lvl, geom[1] >> lvl) >= 16:
            assert regular >= 6 and stepped >= regular - 1, (geom, lvl, regular, stepped)
        g.debug_set_schedule(-1)
    g.close()


# ----------------------------------------------------------------------------------------------------------- 4. raw ranges
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("geom", [(2048, 2048, 6), (640, 192, 7)], ids=deep_cases.gid)
def test_batch_of_raw_ranges(capi, oracle_mod, kind, geom, layout):
    """hsm_match_batch_ranges, 257 raw LaserScans with a driver's drop-outs: the counts and every pose and covariance are those of
    the node's conversion (synth.ranges_to_csr) matched by the checker"""
    from hector_slam_amd import synth
    case = case_of(oracle_mod, geom)
    ref = Ref(oracle_mod, kind, case)
    g = uploaded_ctx(capi, geom, ref.o, layout)
    B, n = 257, 1081
    rng = np.random.default_rng([geom[0], geom[1], 4])
    Q = len(case.query_scans)
    truth = np.stack([case.query_truth[b % Q] for b in range(B)])
    init = synth.perturb_poses(truth, rng)
    a0, inc = (float(np.float32(v)) for v in synth.SCAN_SHAPES[n])
    rays = {q: case.world.raycast(case.query_truth[q], synth.beam_angles(n)) for q in range(Q)}
    r = (np.stack([rays[b % Q] for b in range(B)]) + rng.normal(0.0, 0.01, (B, n))).astype(np.float32)
    drop = rng.random(r.shape)
    r[drop < 0.02] = np.inf
    r[(drop >= 0.02) & (drop < 0.03)] = np.nan
    range_min, range_max = 0.4, float(max(geom[0], geom[1]) * RES)
    pr, cr, cnt = g.match_batch_ranges(init, r, a0, inc, range_min, range_max)
    assert g.last_launch_config()["parity_effective"] == "exact"
    counts, offs, pts = synth.ranges_to_csr(r, a0, inc, range_min, range_max, g.getScaleToMap())
    assert np.array_equal(cnt, counts) and counts.min() > 900
    po = ref.match_many(init, pts, offs)
    assert np.isfinite(po).all(1).mean() >= 0.95
    assert same_rows(pr, po), (geom, int((bits(pr) != bits(po)).any(1).sum()))
    for b in np.flatnonzero(np.isfinite(po).all(1))[::16]:
        _, co = ref.match(init[b], pts[offs[b]:offs[b + 1]])
        assert same(cr[b], co), b
    g.close()


# ------------------------------------------------------------------------------------------------- 5. probes on every level
def level_states(o, case, lvl, rng):
    """map-frame states of `lvl`: the query hints, a cloud around them, the level's corners and one state far outside"""
    lsx, lsy = case.geom[0] >> lvl, case.geom[1] >> lvl
    hints = np.stack([o.map_coords_pose(lvl, p) for p in case.query_init[:8]])
    cloud = (hints[rng.integers(0, 8, 40)] + rng.normal(0, [1.0, 1.0, 0.05], (40, 3))).astype(np.float32)
    corners = np.array([(0.4, 0.3, 0.1), (lsx - 1.5, lsy - 1.5, -2.0), (lsx * 0.5, lsy * 0.5, 1.0), (-50.0, 3.0, 0.1)], np.float32)
    return np.concatenate([hints, cloud, corners]).astype(np.float32)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("geom", deep_cases.GEOMETRIES, ids=deep_cases.gid)
def test_probes_on_every_level(capi, oracle_mod, kind, geom, layout):
    """every probe with level = 0 .. L - 1: hessian_derivs, eval_beams, match_level, likelihood / residual states, the
    sigma-point covariances, hsm_score_batch_device, hsm_match_score_batch_device scoring on the deepest level with groups, the
    occupancy grid, ray distances, row and cell downloads of the whole level, and the two coordinate transforms"""
    import torch
    from hector_slam_amd import synth
    case = case_of(oracle_mod, geom)
    L = case.levels
    ref = Ref(oracle_mod, kind, case)
    o = ref.o
    g = uploaded_ctx(capi, geom, o, layout)
    rng = np.random.default_rng([geom[0], geom[1], 9])
    for lvl in range(L):
        nonzero_H = 0
        lsx, lsy = geom[0] >> lvl, geom[1] >> lvl
        f = np.float32(1.0 / 2.0 ** lvl)
        states = level_states(o, case, lvl, rng)
        for q in range(3):
            pts = case.query_scans[q][: [1081, 300, 65][q]]
            pl = pts * f
            for s in states[:4]:
                Hg, dg = g.hessian_derivs(lvl, s, pl)
                Ho, do = o.hessian_derivs(lvl, s, pl)
                assert same(Hg, Ho) and same(dg, do), (geom, lvl, q, s)
                nonzero_H += bool(Ho[0, 0] != 0)
            assert same(g.likelihood_states(lvl, states, pts), o.likelihood_states(lvl, states, pl)), (geom, lvl, q)
            assert same(g.residual_states(lvl, states, pts), o.residual_states(lvl, states, pl)), (geom, lvl, q)
            cm, cw, lh = g.covariance_for_poses(lvl, states[:24], pts)
            om, ow, ol = o.covariance_for_poses(lvl, states[:24], pl)
            assert same(lh, ol) and same(cm, om) and same(cw, ow), (geom, lvl, q)
            # hsm_score_batch_device: world poses, level-0 points
            world = np.stack([o.world_coords_pose(lvl, s) for s in states]).astype(np.float32)
            pm = np.stack([o.map_coords_pose(lvl, w) for w in world]).astype(np.float32)
            lhs, res = g.score_batch(lvl, world, pts)
            assert capi.load_library().hsm_last_launch_kernel(g._h) == b"score_batch_kernel"
            assert same(lhs, o.likelihood_states(lvl, pm, pl)) and same(res, o.residual_states(lvl, pm, pl)), (geom, lvl, q)
            for it in (0, 3):
                pg, cg = g.match_level(lvl, case.query_init[q], pl, it)
                po, co = ref.match_level(lvl, case.query_init[q], pl, it)
                if np.isfinite(po).all():
                    assert same(pg, po) and same(cg, co), (geom, lvl, q, it)
                else:
                    assert np.array_equal(np.isnan(pg), np.isnan(po)), (geom, lvl, q, it)
        # per-beam values at a hint, and on and beyond the level's last row and column
        pl = case.query_scans[0] * f
        pm = o.map_coords_pose(lvl, case.query_init[0])
        got = g.eval_beams(lvl, pm, pl)
        edge = rng.uniform(-1.5, [lsx + 1.5, lsy + 1.5], (400, 2)).astype(np.float32)
        edge[:6] = [(0, 0), (lsx - 2, lsy - 2), (lsx - 1, lsy - 1), (lsx - 2, 0), (0, lsy - 2), (lsx - 1.999, 0.5)]
        assert same(g.eval_beams(lvl, np.zeros(3, np.float32), edge)[:, :3], o.interp(lvl, edge)), (geom, lvl)
        ev = gn_f64.Eval64(o, lvl, pm, pl, "ho")  # (the transform of the reference, fp32)
        assert same(got[:, :3], o.interp(lvl, ev.coords)), (geom, lvl, "eval_beams at a hint")
        # transforms
        for w in rng.uniform(-12, 12, (20, 3)).astype(np.float32):
            m_g, m_o = g.getMapCoordsPose(lvl, w), o.map_coords_pose(lvl, w)
            assert same(m_g, m_o) and same(g.getWorldCoordsPose(lvl, m_o), o.world_coords_pose(lvl, m_o)), (geom, lvl, w)
        # grids and windows: the whole level
        grid = o.occupancy_grid(lvl)
        assert np.array_equal(g.occupancy_grid(lvl), grid), (geom, lvl)
        lo_o, ui_o = o.download_level(lvl)
        assert same(g.download_rows(lvl, 0, lsy), lo_o), (geom, lvl)
        cells = np.zeros((lsy, lsx, 2), np.int32)
        capi._check(g._lib.hsm_download_cells(g._h, lvl, 0, 0, lsx - 1, lsy - 1, cells.ctypes.data, lsx), "download_cells")
        assert same(cells[..., 0].view(np.float32), lo_o) and np.array_equal(cells[..., 1], ui_o), (geom, lvl)
        _, prob = oracle_mod.libm_expf(lo_o.reshape(-1), "ho")
        assert same(g.download_prob(lvl).reshape(-1), prob), (geom, lvl)
        # ray distances on the level's grid
        ox, oy, res = g.map_metadata(lvl)
        n = 2000
        ext = np.array([lsx * res, lsy * res])
        begin = (np.array([ox, oy]) + rng.uniform(-0.05, 1.05, (n, 2)) * ext).astype(np.float32)
        ang = rng.uniform(0, 2 * np.pi, n)
        end = (begin + np.stack([np.cos(ang), np.sin(ang)], 1) * (rng.uniform(0.0, 1.2, n) * ext.max())[:, None]).astype(np.float32)
        end[:40] = begin[:40]
        end[40:80, 1] = begin[40:80, 1]
        end[80:120, 0] = begin[80:120, 0]
        dist, hit = g.ray_distances(lvl, begin, end)
        rd, rh = oracle_mod.ray_distances("ho", grid, (ox, oy), res, begin, end)
        assert same(dist, rd), (geom, lvl, int((bits(dist) != bits(rd)).sum()))
        has = rd >= 0
        assert same(hit[has], rh[has]) and np.isnan(hit[~has]).all(), (geom, lvl)
        if min(lsx, lsy) >= 16:
            assert 0 < has.sum() < n, (geom, lvl, has.mean())
            assert nonzero_H >= 6, (geom, lvl, nonzero_H)  # (of 12: the probes at the hints are not ones of zeros)
    # match -> score on the deepest level -> select, one call on one stream: the 16 hints of the case in 4 groups of 4
    G, K = 4, 4
    init = case.query_init[:G * K]
    scans = case.query_scans[:G * K]
    pts, offs = synth.pack_scans(scans)
    poses = ref.match_many(init, pts, offs)
    assert np.isfinite(poses).all(), geom
    f = np.float32(1.0 / 2.0 ** (L - 1))
    lh_o = np.array([o.likelihood_states(L - 1, o.map_coords_pose(L - 1, p)[None], s * f)[0] for p, s in zip(poses, scans)], np.float32)
    res_o = np.array([o.residual_states(L - 1, o.map_coords_pose(L - 1, p)[None], s * f)[0] for p, s in zip(poses, scans)], np.float32)
    idx_o, best_o = select_rule.select_best(lh_o, groups=G, group_size=K)
    B = G * K
    d_i, d_p, d_o = dev(init), dev(pts), dev(offs)
    full = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float32, device="cuda:0")  # noqa: E731
    pose, lh, res, best, best_pose = full(B, 3), full(B), full(B), full(G), full(G, 3)
    idx = torch.full((G,), 99, dtype=torch.int32, device="cuda:0")
    s = torch.cuda.current_stream()
    g.match_score_batch_device(B, d_i.data_ptr(), d_p.data_ptr(), d_o.data_ptr(), 1081, pose.data_ptr(), 0, L - 1, lh.data_ptr(),
                               res.data_ptr(), G, 0, K, idx.data_ptr(), best.data_ptr(), best_pose.data_ptr(), s.cuda_stream)
    s.synchronize()
    assert same(pose.cpu().numpy(), poses), (geom, "match_score: poses")
    assert same(lh.cpu().numpy(), lh_o) and same(res.cpu().numpy(), res_o), (geom, "match_score: scores on the deepest level")
    assert np.array_equal(idx.cpu().numpy(), idx_o) and same(best.cpu().numpy(), best_o), (geom, idx.cpu().numpy(), idx_o)
    assert same(best_pose.cpu().numpy(), select_rule.winner_poses(idx_o, poses, np.full((G, 3), SENTINEL, np.float32)))
    g.close()


# --------------------------------------------------------------------------------------------- 6. device-resident integration
def device_update(g, poses, scans=None, shared=None, max_beams=0, origo=None):
    """hsm_update_by_scans_device on torch buffers (CSR scans, or one shared scan); returns the buffers (they outlive the update)"""
    import torch
    from hector_slam_amd import synth
    s = torch.cuda.current_stream()
    d_p = dev(np.asarray(poses, np.float32).reshape(-1, 3))
    if shared is None:
        pts, offs = synth.pack_scans(scans)
        d_pts, d_offs = dev(pts if len(pts) else np.zeros((1, 2), np.float32)), dev(offs)
        g.update_by_scans_device(len(d_p), d_p.data_ptr(), d_pts.data_ptr(), d_offs.data_ptr(), 0, max_beams, origo, s.cuda_stream)
    else:
        a = np.asarray(shared, np.float32).reshape(-1, 2)
        d_pts, d_offs = dev(a), None
        g.update_by_scans_device(len(d_p), d_p.data_ptr(), d_pts.data_ptr(), 0, len(a), max_beams, origo, s.cuda_stream)
    return d_p, d_pts, d_offs


def host_update(capi, g, poses, scans, origo=ZERO2):
    """per scan hsm_retain_scan (what matchData leaves for the coarse levels) + hsm_update_by_scan"""
    og = np.ascontiguousarray(origo, np.float32)
    for p, sc in zip(np.asarray(poses, np.float32).reshape(-1, 3), scans):
        a = np.ascontiguousarray(sc, np.float32).reshape(-1, 2)
        capi._check(g._lib.hsm_retain_scan(g._h, a.ctypes.data if a.size else None, a.shape[0], og), "hsm_retain_scan")
        g.updateByScan(a, p, og)


def trajectory(case):
    """40 posed scans (the build and the query scans at their true poses), one of them at a NaN pose and one empty"""
    poses = np.concatenate([case.build_poses, case.query_truth]).astype(np.float32)
    scans = list(case.build_scans) + list(case.query_scans)
    poses[5] = [np.nan, 0.5, 0.1]
    scans[9] = np.zeros((0, 2), np.float32)
    return poses[:40], scans[:40]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("geom", deep_cases.GEOMETRIES, ids=deep_cases.gid)
def test_device_resident_integration(capi, oracle_mod, kind, geom, layout):
    """hsm_update_by_scans_device from an empty map: a trajectory of 40 posed scans in one call (a NaN pose and an empty scan in
    the list), then one scan at eight poses in the shared form with a laser origin, then host updates (a 1081-beam and a dense
    scan) and device-side updates again -- after each, every level's planes, update index, boxes and mark planes"""
    case = case_of(oracle_mod, geom)
    L = case.levels
    ref = Ref(oracle_mod, kind, case, build=False)
    g = new_ctx(capi, geom, layout)
    poses, scans = trajectory(case)
    assert len(poses) >= 32 and np.isnan(poses[5, 0]) and len(scans[9]) == 0
    for lvl in range(L):
        g.take_dirty_bbox(lvl)
    done = 0

    def step(what, run, p, sc, origo=ZERO2):
        nonlocal done
        before = oracle_planes(ref.o, L)
        keep = run()
        ref.build(p[:-1], sc[:-1], origo)
        before_last = oracle_planes(ref.o, L)
        ref.build(p[-1:], sc[-1:], origo)
        g.synchronize()
        done += len(p)
        check_planes(g, ref.o, L, (geom, layout, what), update_index=done - 1)
        n = check_boxes(g, before, oracle_planes(ref.o, L), (geom, layout, what), before_last)
        assert n >= L - 2, what  # (a level of 2 rows need not change)
        del keep

    step("trajectory, CSR", lambda: device_update(g, poses, scans, max_beams=1081), poses, scans)
    rng = np.random.default_rng(3)
    hyp = (case.query_truth[2][None, :] + rng.normal(0, [0.05, 0.05, 0.02], (8, 3))).astype(np.float32)
    step("shared scan", lambda: device_update(g, hyp, shared=case.query_scans[2], origo=case.origo), hyp, [case.query_scans[2]] * 8,
         case.origo)
    step("host update", lambda: host_update(capi, g, case.query_truth[4:5], case.query_scans[4:5]), case.query_truth[4:5],
         case.query_scans[4:5])
    step("dense host update", lambda: host_update(capi, g, case.dense_pose[None], [case.dense]), case.dense_pose[None], [case.dense])
    step("device-side again", lambda: device_update(g, case.query_truth[6:9], case.query_scans[6:9]), case.query_truth[6:9],
         case.query_scans[6:9])
    for lvl in range(L):
        assert (ref.o.download_level(lvl)[0] != 0).any(), (geom, lvl)
    # the texels the updates wrote: a batched match on the result
    from hector_slam_amd import synth
    pts, offs = synth.pack_scans(case.query_scans)
    pb, _ = g.match_batch(case.query_init, pts, offs)
    assert same_rows(pb, ref.match_many(case.query_init, pts, offs)), geom
    g.close()


# ------------------------------------------------------------------------------------------- 7. the key generation wrap
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("geom", deep_cases.GEOMETRIES, ids=deep_cases.gid)
def test_update_serial_wrap_on_a_deep_level(capi, oracle_mod, kind, geom, layout):
    """the 12-bit update generation of level L - 1 and of level 3 set to 4094: it wraps on the second of four updates, through
    the host entry on one context and through the device entry on another; every level's planes after each"""
    case = case_of(oracle_mod, geom)
    L = case.levels
    ref = Ref(oracle_mod, kind, case, build=False)
    host, devc = new_ctx(capi, geom, layout), new_ctx(capi, geom, layout)
    first = (case.build_poses[:6], case.build_scans[:6])
    keep = [device_update(m, *first) for m in (host, devc)]
    ref.build(*first)
    for m in (host, devc):
        m.synchronize()
        check_planes(m, ref.o, L, (geom, "before the wrap"), update_index=5)
        for lvl in sorted({L - 1, 3}):
            capi._check(m._lib.hsm_debug_set_update_serial(m._h, lvl, 4094), "hsm_debug_set_update_serial")
    nxt = (np.concatenate([case.query_truth[:3], case.dense_pose[None]]), case.query_scans[:3] + [case.dense])
    for k in range(4):
        one = (nxt[0][k:k + 1], nxt[1][k:k + 1])
        host_update(capi, host, *one)
        keep.append(device_update(devc, *one))
        ref.build(*one)
        for m, name in ((host, "host"), (devc, "device")):
            m.synchronize()
            check_planes(m, ref.o, L, (geom, layout, name, "update", k), update_index=6 + k)
    for m in (host, devc):
        for lvl in range(L):
            assert np.array_equal(m.occupancy_grid(lvl), ref.o.occupancy_grid(lvl)), (geom, lvl)
        m.close()


# ------------------------------------------------------------------------------------------------- 8. upload and rebuild
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("geom", deep_cases.GEOMETRIES, ids=deep_cases.gid)
def test_uploaded_pyramid_equals_the_maintained_one(capi, oracle_mod, kind, geom, layout):
    """hsm_upload_level of the checker's planes on all L levels of a fresh context: hsm_download_prob and the matches carry the
    bits of the context that made the same map update by update"""
    case = case_of(oracle_mod, geom)
    L = case.levels
    ref = Ref(oracle_mod, kind, case)
    kept = built_ctx(capi, case, layout)
    fresh = uploaded_ctx(capi, geom, ref.o, layout)
    check_planes(fresh, ref.o, L, (geom, "uploaded"))
    for lvl in range(L):
        pk, pf = kept.download_prob(lvl), fresh.download_prob(lvl)
        assert same(pk, pf), (geom, lvl, int((bits(pk) != bits(pf)).sum()))
        _, prob = oracle_mod.libm_expf(ref.o.download_level(lvl)[0].reshape(-1), "ho")
        assert same(pf.reshape(-1), prob), (geom, lvl)
    for q in range(8):
        po, co = ref.match(case.query_init[q], case.query_scans[q])
        for m, name in ((fresh, "uploaded"), (kept, "maintained")):
            pg, cg = m.matchData(case.query_init[q], case.query_scans[q])
            assert_match(pg, cg, po, co, (geom, layout, name, q))
    kept.close()
    fresh.close()
