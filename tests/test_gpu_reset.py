"""hsm_reset of a context that has been used, against checkers that went through the same history and the same reset().

The cases are tests/reset_cases.py's, pinned on the CPU by tests/test_reset_reference.py: three maps (64 x 64 x 2, 96 x 40 x 3 in
the sensitive frame, (333, 90, 6); the latter two in both layouts), each plain, moved (hsm_shift_map) and frozen (stamps ahead
of the counter).  The history ends in a gated device-side call and no host query follows it, so the gate's count and the
update boxes are still on the device when hsm_reset runs; a publish box is pending, the key generation is about to wrap,
the matchers hold a cached permutation, a cached sensor geometry and buffers grown past anything used afterwards, and the
batch order stays sorted.

  1. the reset itself, the readers on the blank map, the rebuild by six updates across the key wrap, the readers again: in
     the library's default mode and in HSM_PARITY_EXACT against the checkers; in HSM_PARITY_FAST and HSM_PARITY_RELAXED, where
     no checker gives the bits, against a never-used context of the same geometry and layout that goes through the same
     readers and the same six updates (cells, probabilities and outputs, not stamps)
  2. a match queued on a caller's stream in front of the reset sees the old map, one queued behind it the blank one; a reset
     while such a stream is being captured is refused and changes nothing
  3. a reset context as the source of a merge, as the destination of a copy, and of a copy of boxes
  4. a group of two replicas: process_scan, both members reset, process_scan again

Every comparison is on uint32 views, against oracle_kinds()[-1] where a checker gives the bits.  No tolerance anywhere.
"""
import numpy as np
import pytest

import merge_cases
import moved_entry_cases as mec
import newer_entry_cases as nec
import reset_cases as rc
import shift_cases as sc
import test_gpu_moved_entries as tmoved
import test_gpu_score_batch as tsb
import test_gpu_shift_map as tshift
import test_gpu_window as tw
import topk_rule
from conftest import bits, oracle_kinds
from support import capi, dev, pack, same, stream_ptr

pytestmark = pytest.mark.gpu
KIND = oracle_kinds()[-1]
F = np.float32
EMPTY = [0, 0, -1, -1]
HSM_ERR_INVALID = -1
SORTED_BATCH = 1024
new_ctx, levels_of, assert_planes, whole = tshift.new_ctx, tshift.levels_of, tshift.assert_planes, tshift.whole
box, posed_update, export_device = tmoved.box, tmoved.posed_update, tmoved.export_device


class Device:
    """a context going through reset_cases' steps; `keep` holds the device buffers of queued calls until the context closes"""

    def __init__(self, capi, oracle_mod, m, layout, start=None, parity=None):
        import torch
        self.capi, self.py, self.m, self.sorted = capi, oracle_mod, m, None
        self.g = new_ctx(capi, m, layout, start=None if start is None else (float(start[0]), float(start[1])))
        if parity is not None:
            self.g.set_parity(parity)
        self.g.set_update_gate(*mec.trajectory(oracle_mod, m).thresholds)
        self.keep, self.applied = [], []
        self.grids = [torch.full((m.dims(lvl)[1], m.dims(lvl)[0]), 55, dtype=torch.int8, device="cuda:0") for lvl in range(m.levels)]
        self.d_box = torch.zeros(4, dtype=torch.int32, device="cuda:0")

    def step(self, op):
        g, m, name = self.g, self.m, op[0]
        if name == "load":
            tshift.load(g, op[1])
        elif name == "match":
            return g.matchData(op[1], op[2])
        elif name == "update":
            g.updateByScan(op[2], op[1])
        elif name == "shift":
            g.shift_map(mec.case_plan(m, op[1])[0])
        elif name == "batches":
            self.batches()
        elif name == "export":
            for lvl in range(m.levels):
                g.occupancy_changes_device(lvl, self.grids[lvl].data_ptr(), self.d_box.data_ptr(), stream_ptr())
        elif name == "serial":
            g.synchronize()
            for lvl in range(m.levels):
                self.capi._check(g._lib.hsm_debug_set_update_serial(g._h, lvl, 4093 - lvl), "set serial")
        elif name in ("device", "gated"):
            k = posed_update(g, op[1], op[2], gated=name == "gated")
            self.keep.append(k)
            if name == "gated":
                self.applied.append(k[4])
        return None

    def batches(self):
        """what the matchers keep between launches: a permutation of 1024 sorted scans, a sensor geometry, grown buffers"""
        g, q = self.g, rc.reader_inputs(self.py, self.m)
        rng = np.random.default_rng(3101)
        res = self.m.resolution
        cloud = lambda n: (q["centre"].astype(np.float64) + rng.uniform(-1, 1, (n, 3)) * [3 * res, 3 * res, 0.05]).astype(F)  # noqa: E731
        g.set_batch_order(self.capi.ORDER_MORTON)
        # 1024 scans (the Morton sort takes batches of HSM_BATCH_ORDER_MIN = 1024 and more) from start poses all over the window
        sx, sy = self.m.dims(0)
        spread = np.stack([g.getWorldCoordsPose(0, F([x, y, a])) for x, y, a in
                           rng.uniform([2, 2, -3], [sx - 3, sy - 3, 3], (SORTED_BATCH, 3))]).astype(F)
        g.match_batch(spread, q["pts"][:64])
        self.sorted = bool(g.last_launch_sorted())
        ranges = (np.hypot(q["pts"][:, 0], q["pts"][:, 1]) * res).astype(F)
        g.match_batch_ranges(cloud(5), np.tile(ranges, (5, 1)), -2.3, float(F(4.6 / 199)), float(F(0.5 * res)), float(F(400.0 * res)))
        g.match_batch(cloud(320), np.concatenate([q["pts"], q["pts"]]))   # 320 x 400 beams: more than anything behind the reset

    def close(self):
        self.g.close()
        self.keep.clear()


def used(capi, oracle_mod, m, layout, variant, parity=None):
    d = Device(capi, oracle_mod, m, layout, parity=parity)
    for op in rc.history(oracle_mod, m, variant):
        d.step(op)
    return d


def assert_prob(oracle_mod, g, planes, what):
    for lvl, (lo, _) in enumerate(planes):
        _, prob = oracle_mod.libm_expf(lo.reshape(-1), "ho")
        assert same(g.download_prob(lvl).reshape(-1), prob), (what, lvl, "probability")
        assert g.debug_marks_nonzero(lvl) == (0, 0), (what, lvl)


def same_or_nan(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F).reshape(np.shape(a))
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a)[~nan], bits(b)[~nan])


def check_readers(capi, g, m, q, want, what, blank):
    import torch
    rows = [k for k, x in enumerate(want["match"]) if x is not None]
    assert len(rows) >= 7
    assert g.batch_order() == capi.ORDER_MORTON   # the order that sorted the 1024 scans before the reset is still set
    pose, cov = g.match_batch(q["poses"][rows], *pack([q["scans"][k] for k in rows]))
    # this only says that the eight-scan launch did not sort.  That the 1024's cached permutation (quad layout; the plane
    # layout's form leaves none) is not applied to it shows in the rows below: a permuted row would carry another row's bits
    assert not g.last_launch_sorted(), what
    for j, k in enumerate(rows):
        assert same(pose[j], want["match"][k][0]) and same(cov[j], want["match"][k][1]), (what, "match_batch row", k)
    pose, cov = g.matchData(q["centre"], q["pts"])
    assert same(pose, want["single"][0]) and same(cov, want["single"][1]), (what, "matchData")
    lens = [len(s) for s in q["scans"]]
    pts, offs = pack(q["scans"])
    got_scores = []
    for lvl in range(m.levels):
        got_scores.append(tsb.score(g, lvl, q["poses"], pts, offs)[0])
        tsb.assert_scores(f"{what} score batch level {lvl}", tsb.score(g, lvl, q["poses"], pts, offs), want["score"][lvl], lens)
        got = tw.score_window(g, lvl, q["centre"], q["step"], rc.WINDOW_HALF, q["pts"])
        tw.assert_same_scores(f"{what} window level {lvl}", got, want["window"][lvl], len(q["pts"]))
        for k in rc.TOPK:
            idx, best = tw.run_topk(g, capi, got[0], k)
            want_idx, want_best = topk_rule.topk(want["window"][lvl][0], k)
            assert np.array_equal(idx, want_idx) and same(best, want_best), (what, "top k", lvl, k, idx, want_idx)
            if blank and (bits(want["window"][lvl][0]) == bits(want["window"][lvl][0][0])).all():   # all tied: by index alone
                assert np.array_equal(idx, np.arange(k)), (what, lvl, k, idx)
        st, lh, res, covs = want["states"][lvl]
        assert tw.same_bits(g.likelihood_states(lvl, st, q["pts"]), lh), (what, lvl, "likelihood states")
        assert tw.same_bits(g.residual_states(lvl, st, q["pts"]), res), (what, lvl, "residual states")
        for a, b in zip(g.covariance_for_poses(lvl, st, q["pts"]), covs):
            assert tw.same_bits(a, b), (what, lvl, "covariance for poses")
        assert np.array_equal(g.occupancy_grid(lvl), want["grid"][lvl]), (what, lvl, "occupancy grid")
        cw, cm, l7, lh = g.covariance_batch(lvl, q["poses"], pts, offs)
        for a, key in ((cw, "cw"), (cm, "cm"), (l7, "l7"), (lh, "lh")):
            assert same_or_nan(a, want["cov"][lvl][key]), (what, lvl, "covariance batch", key)
        reach, want_ranges, want_hit = want["cast"][lvl]
        ranges, hit = g.cast_scans(lvl, q["poses"], q["angles"], reach)
        assert same(ranges, want_ranges) and tw.same_bits(hit, want_hit), (what, lvl, "cast scans")
        begin, end, want_dist, want_hit = want["rays"][lvl]
        dist, hit = g.ray_distances(lvl, begin, end)
        assert same(dist, want_dist) and tw.same_bits(hit, want_hit), (what, lvl, "ray distances")
        if blank:   # no ray hits anything
            assert (ranges < 0).all() and np.isnan(hit).all() and (dist < 0).all(), (what, lvl)
        d_s, idx = dev(got_scores[lvl]), torch.full((2,), 99, dtype=torch.int32, device="cuda:0")
        g.select_best_device(2, 0, len(rc.CSR_LENS) // 2, d_s.data_ptr(), 0, idx.data_ptr(), 0, 0, stream_ptr())
        assert np.array_equal(idx.cpu().numpy(), want["best"][lvl][0]), (what, lvl, "select best", idx, want["best"][lvl][0])
    tmoved.check_ranges(capi, g, q, want)
    a0, inc, rmin, rmax = q["laser"]
    pose, cov, counts = g.match_batch_ranges(q["starts"], q["ranges"], a0, inc, rmin, rmax)   # the host form: hsm_match_batch_ranges
    assert np.array_equal(counts, want["counts"]), (what, "match_batch_ranges counts")
    assert same(pose, np.stack([p for p, _ in want["ranges_match"]])) and same(cov, np.stack([c for _, c in want["ranges_match"]])), (what, "match_batch_ranges")
    pose, cov, counts, origo = g.match_batch_ranges_tf(q["starts"], q["ranges"], a0, inc, *q["tf_lim"], q["tf_rows"], *q["tf_gates"])
    assert np.array_equal(counts, [len(c) for c, _, _ in want["tf"]]) and same(origo, np.stack([o for _, o, _ in want["tf"]])), (what, "tf counts, origos")
    assert same(pose, np.stack([r[0] for _, _, r in want["tf"]])) and same(cov, np.stack([r[1] for _, _, r in want["tf"]])), (what, "match_batch_ranges_tf")
    check_chains(g, m, q, want["chain"], [want["match"][k] for k in want["chain"]["rows"]], what)
    tmoved.check_reloc(capi, g, q, want)
    if blank and (bits(want["reloc"]["scores"]) == bits(want["reloc"]["scores"][0])).all():   # all tied: the first k places
        assert np.array_equal(want["reloc"]["index"], np.arange(mec.RELOC_K)), want["reloc"]["index"]
    g.matchData(q["centre"], q["pts"])   # (the container the next host update finds retained is the scan's, as on the checker)


def chains(g, m, q, rows):
    """hsm_match_score_batch (host arrays; scored on the coarsest level) and hsm_match_cov_batch_device (level 0) over the
    hypotheses `rows` as one group -> (the score chain's dict, the covariance chain's dict)"""
    import torch
    B = len(rows)
    pts, offs = pack([q["scans"][k] for k in rows])
    sc_ = g.match_score_batch(q["poses"][rows], pts, offs, score_level=m.levels - 1, group_size=B)
    d_b, d_pts, d_offs = dev(q["poses"][rows]), dev(pts), dev(offs)
    out = {k: torch.full((B, w), -777.0, device="cuda:0") for k, w in (("pose", 3), ("cov", 9), ("cw", 9), ("cm", 9), ("l7", 7), ("lh", 1))}
    out["cov"].zero_()   # a scan with no beam leaves its Hessian row as it finds it (the host forms hand in zeros)
    idx = torch.full((1,), 99, dtype=torch.int32, device="cuda:0")
    g.match_cov_batch_device(B, d_b.data_ptr(), d_pts.data_ptr(), d_offs.data_ptr(), rc.CSR_LENS[-1], out["pose"].data_ptr(),
                             out["cov"].data_ptr(), 0, out["cw"].data_ptr(), out["cm"].data_ptr(), out["l7"].data_ptr(),
                             out["lh"].data_ptr(), 1, 0, B, idx.data_ptr(), 0, 0, stream_ptr())
    torch.cuda.synchronize()
    cv = {k: v.cpu().numpy() for k, v in out.items()}
    cv["best_index"] = idx.cpu().numpy()
    return sc_, cv


def check_chains(g, m, q, want, matches, what):
    rows = want["rows"]
    lens = [len(q["scans"][k]) for k in rows]
    sc_, cv = chains(g, m, q, rows)
    poses, covs = np.stack([p for p, _ in matches]), np.stack([c for _, c in matches])
    for r, name in ((sc_, "match_score_batch"), (cv, "match_cov_batch_device")):
        assert same(r["pose"], poses) and same(r["cov"], covs), (what, name, "poses and Hessians")
    tsb.assert_scores(f"{what} match_score_batch", (sc_["likelihood"], sc_["residual"]), want["score"], lens)
    assert np.array_equal(sc_["best_index"], want["score_best"][0]) and same_or_nan(sc_["best_score"], want["score_best"][1]), (what, sc_["best_index"])
    for key in ("cw", "cm", "l7", "lh"):
        assert same_or_nan(cv[key], want["cov"][key]), (what, "match_cov_batch_device", key)
    assert np.array_equal(cv["best_index"], want["cov_best"][0]), (what, cv["best_index"], want["cov_best"][0])


def outputs(capi, g, m, q, rows):
    """every reader whose bits depend on the parity mode, and the rest of check_readers' entries with them -> {name: array}"""
    out = {}
    pose, cov = g.match_batch(q["poses"][rows], *pack([q["scans"][k] for k in rows]))
    out.update(batch_pose=pose, batch_cov=cov)
    out["single_pose"], out["single_cov"] = g.matchData(q["centre"], q["pts"])
    a0, inc, rmin, rmax = q["laser"]
    out["ranges_pose"], out["ranges_cov"], out["ranges_counts"] = g.match_batch_ranges(q["starts"], q["ranges"], a0, inc, rmin, rmax)
    out["tf_pose"], out["tf_cov"], out["tf_counts"], out["tf_origo"] = g.match_batch_ranges_tf(
        q["starts"], q["ranges"], a0, inc, *q["tf_lim"], q["tf_rows"], *q["tf_gates"])
    sc_, cv = chains(g, m, q, rows)
    out.update({"score_chain_" + k: v for k, v in sc_.items()})
    out.update({"cov_chain_" + k: v for k, v in cv.items()})
    pts, offs = pack(q["scans"])
    for lvl in range(m.levels):
        out[f"score_{lvl}"], out[f"residual_{lvl}"] = tsb.score(g, lvl, q["poses"], pts, offs)
        win = tw.score_window(g, lvl, q["centre"], q["step"], rc.WINDOW_HALF, q["pts"])
        out[f"window_{lvl}"] = win[0]
        for k in rc.TOPK:
            out[f"topk_{lvl}_{k}"], out[f"topk_score_{lvl}_{k}"] = tw.run_topk(g, capi, win[0], k)
        for key, a in zip(("cw", "cm", "l7", "lh"), g.covariance_batch(lvl, q["poses"], pts, offs)):
            out[f"cov_{key}_{lvl}"] = a
        out[f"grid_{lvl}"] = g.occupancy_grid(lvl)
    g.matchData(q["centre"], q["pts"])   # (the container the next host update finds retained is the scan's)
    return out


def assert_same_outputs(what, a, b):
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert (same_or_nan(x, y) if x.dtype == F else np.array_equal(x, y)), (what, k)


# ---- 1. the reset, the blank map, the rebuild ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parity", ["auto", "exact"])
@pytest.mark.parametrize("m,layout,variant", rc.CASES, ids=rc.CASE_IDS)
def test_reset_of_a_used_context(capi, oracle_mod, m, layout, variant, parity):
    r, q = rc.run_checker(oracle_mod, KIND, m, variant), rc.reader_inputs(oracle_mod, m)
    mode = None if parity == "auto" else capi.PARITY_EXACT   # auto: the library's default, never set
    d = used(capi, oracle_mod, m, layout, variant, mode)
    g = d.g
    fresh = Device(capi, oracle_mod, m, layout, start=r["start"], parity=mode)   # never used: the box model of the six updates
    try:
        assert g.parity() == (capi.PARITY_AUTO if mode is None else mode)
        # the quad layout's batch form takes its scans through a permutation and leaves one cached behind; the plane layout's
        # form takes none (MatchPlan::wants_perm), so there the step leaves only the setting
        assert d.sorted == (layout == "quad"), "the 1024-scan batch of the history: hsm_last_launch_sorted"
        g.reset()   # no host query since the gated call: the gate's count and the update boxes are still on the device
        # (a) the count is in the counters.  The fold is lazy everywhere (hsm_update_index folds what is outstanding, too), so this
        # holds the count across the reset whoever folds it; the dirty and publish boxes below are hsm_reset's alone
        for lvl in range(m.levels):
            assert g.getUpdateIndex(lvl) == r["index_before"], (lvl, g.getUpdateIndex(lvl), r["index_before"])
        assert np.array_equal(d.applied[0].cpu().numpy(), r["flags"][0].astype(np.int32))
        pose, total = g.update_gate_state()
        assert same(pose, F([rc.FLT_MAX] * 3)) and total == r["gate_count_before"], (pose, total)
        assert same(g.map_start(), r["start"]), (g.map_start(), r["start"])   # reset clears cells, not geometry
        assert_planes("blank", levels_of(g, m.levels), r["blank"])
        assert_prob(oracle_mod, g, r["blank"], "blank")
        for lvl in range(m.levels):
            assert (bits(g.download_prob(lvl)) == bits(F(0.5))).all(), lvl
            assert box(g.last_update_bbox(lvl)) == EMPTY, (lvl, g.last_update_bbox(lvl))
            assert box(g.take_dirty_bbox(lvl)) == whole(m, lvl) and box(g.take_dirty_bbox(lvl)) == EMPTY, lvl
            if lvl % 2 == 0:   # the device form on the even levels, the host form on the odd ones
                assert export_device(g, lvl, d.grids[lvl], d.d_box) == whole(m, lvl), lvl
                assert export_device(g, lvl, d.grids[lvl], d.d_box) == EMPTY, lvl
                grid = d.grids[lvl].cpu().numpy()
            else:
                grid = np.full((m.dims(lvl)[1], m.dims(lvl)[0]), 55, np.int8)
                assert box(g.occupancy_changes(lvl, grid)) == whole(m, lvl) and box(g.occupancy_changes(lvl, grid)) == EMPTY, lvl
                d.grids[lvl].copy_(dev(grid))
            assert (grid == -1).all(), lvl
        check_readers(capi, g, m, q, r["readers_blank"], "blank", True)   # (b)
        for lvl in range(m.levels):   # the fresh context: its first export and dirty box are the whole level, too
            fresh.g.take_dirty_bbox(lvl)
            export_device(fresh.g, lvl, fresh.grids[lvl], fresh.d_box)
        fresh.g.matchData(q["centre"], q["pts"])
        for op in rc.after_sequence(oracle_mod, m):   # (c)
            d.step(op)
            fresh.step(op)
        g.synchronize()
        assert np.array_equal(d.applied[1].cpu().numpy(), r["flags"][1].astype(np.int32))
        assert_planes("rebuilt", levels_of(g, m.levels), r["rebuilt"])
        assert_prob(oracle_mod, g, r["rebuilt"], "rebuilt")
        pose, total = g.update_gate_state()
        assert same(pose, r["gate_last"]) and total == r["gate_count"], (pose, r["gate_last"], total, r["gate_count"])
        for lvl in range(m.levels):
            assert g.getUpdateIndex(lvl) == r["index_after"], lvl
            st = r["rebuilt"][lvl][1]
            last = st >= 3 * r["index_after"] + 1   # the cells the last scan marked
            # the boxes are those of a never-used context after the same six updates, and they hold the changed cells
            got, model = box(g.last_update_bbox(lvl)), box(fresh.g.last_update_bbox(lvl))
            assert got == model, (lvl, "last update box", got, model)
            if last.any():
                ys, xs = np.nonzero(last)
                assert got[0] <= xs.min() and got[1] <= ys.min() and got[2] >= xs.max() and got[3] >= ys.max(), (lvl, got)
            dirty, model = box(g.take_dirty_bbox(lvl)), box(fresh.g.take_dirty_bbox(lvl))
            assert dirty == model, (lvl, "dirty box", dirty, model)
            got, model = export_device(g, lvl, d.grids[lvl], d.d_box), export_device(fresh.g, lvl, fresh.grids[lvl], fresh.d_box)
            assert got == model, (lvl, "exported box", got, model)
            ys, xs = np.nonzero(st != -1)
            if len(xs):
                assert got != EMPTY and got[0] <= xs.min() and got[1] <= ys.min() and got[2] >= xs.max() and got[3] >= ys.max(), (lvl, got)
            assert np.array_equal(d.grids[lvl].cpu().numpy(), r["readers_rebuilt"]["grid"][lvl]), (lvl, "exported cells")
        check_readers(capi, g, m, q, r["readers_rebuilt"], "rebuilt", False)   # (d)
    finally:
        d.close()
        fresh.close()


@pytest.mark.parametrize("parity", ["fast", "relaxed"])
@pytest.mark.parametrize("m,layout,variant", rc.CASES, ids=rc.CASE_IDS)
def test_reset_in_fast_parity_equals_a_fresh_context(capi, oracle_mod, m, layout, variant, parity):
    """no checker gives the bits of these modes: the reset context against a never-used one of the same geometry, layout, start
    and mode -- the readers on the blank map, the cells and probabilities the six updates build, the readers on those"""
    mode = capi.PARITY_FAST if parity == "fast" else capi.PARITY_RELAXED
    r, q = rc.run_checker(oracle_mod, KIND, m, variant), rc.reader_inputs(oracle_mod, m)
    rows = r["readers_rebuilt"]["chain"]["rows"]
    d = used(capi, oracle_mod, m, layout, variant, mode)
    fresh = Device(capi, oracle_mod, m, layout, start=r["start"], parity=mode)
    try:
        d.g.reset()
        assert d.g.parity() == mode and fresh.g.parity() == mode   # the setting stays
        fresh.g.set_batch_order(capi.ORDER_MORTON)
        assert same(d.g.map_start(), fresh.g.map_start())
        for lvl in range(m.levels):
            assert (bits(d.g.download_prob(lvl)) == bits(F(0.5))).all(), lvl
        assert_same_outputs("blank", outputs(capi, d.g, m, q, rows), outputs(capi, fresh.g, m, q, rows))
        for op in rc.after_sequence(oracle_mod, m):
            d.step(op)
            fresh.step(op)
        d.g.synchronize()
        fresh.g.synchronize()
        assert np.array_equal(d.applied[1].cpu().numpy(), fresh.applied[0].cpu().numpy())
        for lvl in range(m.levels):
            assert same(d.g.download_level(lvl)[0], fresh.g.download_level(lvl)[0]), (lvl, "cells")
            assert same(d.g.download_level(lvl)[0], r["rebuilt"][lvl][0]), (lvl, "cells against the checker: updates have one mode")
            assert same(d.g.download_prob(lvl), fresh.g.download_prob(lvl)), (lvl, "probabilities")
            assert d.g.debug_marks_nonzero(lvl) == (0, 0), lvl
        assert_same_outputs("rebuilt", outputs(capi, d.g, m, q, rows), outputs(capi, fresh.g, m, q, rows))
    finally:
        d.close()
        fresh.close()


# ---- 2. ordering ---------------------------------------------------------------------------------------------------------------------------
def test_reset_is_ordered_behind_a_match_queued_on_a_caller_stream(capi, oracle_mod):
    import torch
    m, variant = mec.M96, "plain"
    r, q = rc.run_checker(oracle_mod, KIND, m, variant), rc.reader_inputs(oracle_mod, m)
    rows = [k for k, x in enumerate(r["readers_blank"]["match"]) if x is not None and len(q["scans"][k]) > 1]
    pts, offs = pack([q["scans"][k] for k in rows])
    B = len(rows)
    d = used(capi, oracle_mod, m, "quad", variant)
    g = d.g
    try:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            d_b, d_pts, d_offs = dev(q["poses"][rows]), dev(pts), dev(offs)
            out = [torch.full((B, 3), -777.0, device="cuda:0") for _ in range(3)]

        def match(k):
            g.match_batch_device(B, d_b.data_ptr(), d_pts.data_ptr(), d_offs.data_ptr(), 0, out[k].data_ptr(), 0, s.cuda_stream)
        match(0)
        s.synchronize()
        old = out[0].cpu().numpy()
        blank = np.stack([r["readers_blank"]["match"][k][0] for k in rows])
        assert not same(old, blank), "the old map and the blank one give the same poses: the check below would be blind"
        match(1)
        g.reset()   # no wait in between: hsm_reset orders itself behind the foreign match
        match(2)
        s.synchronize()
        assert same(out[1].cpu().numpy(), old), "a match queued in front of the reset saw cleared cells"
        assert same(out[2].cpu().numpy(), blank), "a match queued behind the reset saw the old map"
    finally:
        d.close()


def test_reset_while_a_caller_stream_captures_is_refused(capi, oracle_mod):
    """hsm_reset is a map update: while a stream this context has matched on is being captured it fails with HSM_ERR_INVALID and
    changes nothing; after the capture it runs (tests/test_gpu_capture_state.py holds the same for the updates, not for reset)"""
    import torch
    m, variant = mec.M96, "plain"
    q = rc.reader_inputs(oracle_mod, m)
    d = used(capi, oracle_mod, m, "quad", variant)
    g = d.g
    try:
        g.synchronize()
        before = [g.download_level(lvl) + (g.download_prob(lvl),) for lvl in range(m.levels)]
        index, gate = [g.getUpdateIndex(lvl) for lvl in range(m.levels)], g.update_gate_state()
        B = len(q["poses"])
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            d_b, d_pts, out = dev(q["poses"]), dev(q["pts"]), torch.full((B, 3), -777.0, device="cuda:0")

        def launch():
            g.match_batch_device(B, d_b.data_ptr(), d_pts.data_ptr(), 0, len(q["pts"]), out.data_ptr(), 0, s.cuda_stream)
        launch()   # an eager match first: the stream is one this context has matched on
        s.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            launch()
            with pytest.raises(capi.HsmError) as e:
                g.reset()
            assert f"({HSM_ERR_INVALID})" in str(e.value) and "captur" in str(e.value), str(e.value)
            launch()
        torch.cuda.synchronize()
        after = [g.download_level(lvl) + (g.download_prob(lvl),) for lvl in range(m.levels)]
        for lvl, (a, b) in enumerate(zip(before, after)):
            assert np.array_equal(a[1], b[1]) and same(a[0], b[0]) and same(a[2], b[2]), (lvl, "a refused reset changed the map")
        assert [g.getUpdateIndex(lvl) for lvl in range(m.levels)] == index
        assert same(g.update_gate_state()[0], gate[0]) and g.update_gate_state()[1] == gate[1]
        del graph
        g.reset()   # the capture has ended: accepted
        for lvl in range(m.levels):
            lo, st = g.download_level(lvl)
            assert (bits(lo) == 0).all() and (st == -1).all(), lvl
    finally:
        d.close()


# ---- 3. as a merge or copy partner -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["quad", "plane"])
def test_reset_context_as_merge_source_and_copy_destination(capi, oracle_mod, layout):
    m = mec.M96
    planes = sc.old_planes(oracle_mod, m)
    d = used(capi, oracle_mod, m, layout, "frozen")
    e = used(capi, oracle_mod, m, layout, "plain")
    full = tshift.load(new_ctx(capi, m, layout), planes)
    try:
        d.g.reset()
        e.g.reset()
        index = [full.getUpdateIndex(lvl) for lvl in range(m.levels)]
        geom = nec.geometry_of(m)
        blank = [np.zeros_like(lo) for lo, _ in planes]
        for name in ("identity", "theta_0.3"):   # an all-unknown source, by merge_cases' model: the cells stay, and a level
            tx, ty, th = dict(merge_cases.TRANSFORMS)[name]   # whose box is not empty counts one update
            t = F([tx * m.resolution / merge_cases.RES, ty * m.resolution / merge_cases.RES, th])
            model = merge_cases.merge_pyramid([lo for lo, _ in planes], blank, geom, geom, t)
            capi.merge_map(full, d.g, t)
            full.synchronize()
            for lvl, (lo, bx) in enumerate(model):
                assert same(lo, planes[lvl][0]), (name, lvl, "the model itself changes a cell")
                index[lvl] += 0 if tuple(bx) == merge_cases.EMPTY else 1
            assert any(tuple(bx) != merge_cases.EMPTY for _, bx in model), name
            assert_planes("merged " + name, levels_of(full, m.levels), planes)
            assert [full.getUpdateIndex(lvl) for lvl in range(m.levels)] == index, name
        d.g.copy_map_from(full)   # the reset context equals the source afterwards
        d.g.synchronize()
        assert_planes("copied", levels_of(d.g, m.levels), planes)
        assert_prob(oracle_mod, d.g, planes, "copied")
        boxes = np.array([[1, 1, (m.dims(lvl)[0] - 1) // 2, (m.dims(lvl)[1] - 1) // 2] for lvl in range(m.levels)], np.int32)
        e.g.copy_map_from(full, boxes)   # outside the boxes: blank cells, not the cells from before the reset
        e.g.synchronize()
        want = []
        for lvl, (lo, st) in enumerate(planes):
            wl, ws = np.zeros_like(lo), np.full_like(st, -1)
            x0, y0, x1, y1 = boxes[lvl]
            wl[y0:y1 + 1, x0:x1 + 1], ws[y0:y1 + 1, x0:x1 + 1] = lo[y0:y1 + 1, x0:x1 + 1], st[y0:y1 + 1, x0:x1 + 1]
            want.append((wl, ws))
        assert_planes("boxes copied", levels_of(e.g, m.levels), want)
        assert_prob(oracle_mod, e.g, want, "boxes copied")
    finally:
        d.close()
        e.close()
        full.close()


# ---- 4. a group of two replicas -----------------------------------------------------------------------------------------------------------
def test_group_members_reset_between_process_scans(capi, oracle_mod):
    """MapRepGroup(.., [0, 0]) as tests/test_gpu_map_frames.py builds it: matchData on replica 0 and updateByScan on both per scan,
    hsm_reset of both members, the same again.  Poses, Hessians and both replicas' planes are the checker's, whose counters
    and retained containers went through the same reset()"""
    m = rc.GROUP_MAP
    r, t = rc.group_case(oracle_mod, KIND), mec.trajectory(oracle_mod, m)
    grp = capi.MapRepGroup(m.resolution, m.geom[0], m.geom[1], m.geom[2], [0, 0], startCoords=m.start)
    try:
        grp.set_update_factors(*tshift.fc.FACTORS)
        members = [grp.member(0), grp.member(1)]
        for g in members:
            tshift.load(g, rc.start_planes(oracle_mod, m, "plain"))
        row = 0
        for part, ks in enumerate(rc.GROUP_SCANS):
            for k in ks:
                pose, cov = grp.process_scan(t.world[k], t.scans[k])
                assert same(pose, r["poses"][row]) and same(cov, r["covs"][row]), (k, pose, r["poses"][row])
                row += 1
            if part == 0:
                for i, g in enumerate(members):
                    assert_planes(f"replica {i} before the reset", levels_of(g, m.levels), r["before"])
                for g in members:
                    g.reset()
                for i, g in enumerate(members):
                    assert_planes(f"replica {i} blank", levels_of(g, m.levels), r["blank"])
        grp.synchronize()
        for i, g in enumerate(members):
            assert_planes(f"replica {i}", levels_of(g, m.levels), r["end"])
            assert_prob(oracle_mod, g, r["end"], f"replica {i}")
            assert g.getUpdateIndex(0) == r["index"], (i, g.getUpdateIndex(0), r["index"])
    finally:
        grp.close()
