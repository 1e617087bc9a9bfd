"""The covariance batch entries and the merge on every map shape of the suite's geometry files, on the MI355X (cases:
tests/newer_entry_cases.py, pinned on the CPU by tests/test_newer_entries_reference.py).

Covariance (hsm_covariance_batch_device, hsm_covariance_batch, hsm_match_cov_batch_device): four frames on 90 x 24 x 2 and
96 x 40 x 3, the deep pyramids (333, 90, 6), (90, 333, 6) and (256, 256, 8) on every level down to 10 x 2, 2 x 10 and 2 x 2 cells,
and two maps after a window move; against the checker oracle_kinds()[-1] bit for bit.  A row is NaN where the checker's is and
nowhere else: the rows of empty scans, and the covariances (not the likelihoods, which are 0) of rows whose seven likelihoods are
all 0 -- every row on a level with a side of 2 cells, where lim = 0 puts every beam at every sigma point off the level.  The sign
and payload of an invalid operation's NaN are the processor's choice, so such words are compared as NaN, every other word bit
for bit.

Merge (hsm_merge_map, hsm_merge_map_box): the pairs of newer_entry_cases.PAIRS -- an inexact scale and a start outside the
map, the far frame, six and eight levels, a strip of 2050 tiles that sends map_merge_cells_kernel's tile loop on its second trip
(test_merged_state_is_the_models_on_every_new_pair[strip-identity-*]) -- and merges between contexts that have moved, against
the numpy model of tests/merge_cases.py bit for bit over all cells; again in a child process with HSM_COPY_STAGE=1.

No tolerance anywhere in this file.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import moved_entry_cases as mec
import newer_entry_cases as nc
import select_rule
import shift_cases as sc
import test_gpu_covariance_batch as tcb
import test_gpu_entry_geometries as tge
import test_gpu_merge_map as tgm
import test_gpu_score_batch as tsb
import test_gpu_shift_map as tshift
from conftest import bits, oracle_kinds
from support import capi, dev, pack, single_update

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIND = oracle_kinds()[-1]
F = np.float32
SENTINEL, KEYS = tcb.SENTINEL, tcb.KEYS
cov_dev, reference = tcb.cov_dev, tcb.reference
MOVE = "x3_y-2"


def assert_rows(what, got, ref, lens, keys=KEYS):
    """test_gpu_covariance_batch.assert_same where the reference's covariance may be NaN for a scan that is not empty: every
    row was written; a word is NaN where the reference's is and only there; every other word carries its bits; the
    likelihoods are NaN for the empty scans alone"""
    empty = np.asarray(lens) == 0
    for k in keys:
        a, b = got[k], ref[k]
        assert not (a == SENTINEL).any(), f"{what}: rows of {k} never written"
        assert np.isnan(a[empty]).all() and np.isnan(b[empty]).all(), (what, k)
        odd = np.isnan(a) != np.isnan(b)
        assert not odd.any(), f"{what}: {k}: NaN where the reference has none, or none where it has one, rows {np.unique(np.argwhere(odd)[:, 0])[:5]}"
        bad = (bits(a) != bits(b)) & ~np.isnan(b)
        assert not bad.any(), f"{what}: {k}: {int(bad.sum())} words differ, rows {np.unique(np.argwhere(bad)[:, 0])[:5]}"
    for k in keys:
        if k in ("l7", "lh"):
            assert np.isfinite(got[k][~empty]).all(), (what, k)


def parity_of(capi, name):
    return {"exact": capi.PARITY_EXACT, "fast": capi.PARITY_FAST, "relaxed": capi.PARITY_RELAXED}[name]


# ---- covariance: the reference order -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parity", ["default", "exact"])
@pytest.mark.parametrize("m,layout", nc.COV_MAP_LAYOUTS, ids=nc.COV_IDS)
def test_reference_order_carries_the_checkers_bits_on_every_level(capi, oracle_mod, m, layout, parity):
    o = m.checker(oracle_mod, KIND)
    g = tge.new_ctx(capi, oracle_mod, m, layout)
    if parity == "exact":
        g.set_parity(capi.PARITY_EXACT)
    lib = capi.load_library()
    for lvl in range(m.levels):
        want = nc.expected_cov(oracle_mod, m, lvl, KIND)
        for name, poses, scans in nc.cov_batches(oracle_mod, m, lvl):
            lens = [len(s) for s in scans]
            shared = name.startswith("shared")
            got = cov_dev(g, lvl, poses, scans[0]) if shared else cov_dev(g, lvl, poses, *pack(scans))
            assert lib.hsm_last_launch_kernel(g._h) == b"covariance_batch_kernel"
            assert lib.hsm_last_launch_parity(g._h) == capi.PARITY_EXACT
            assert_rows(f"{name}, level {lvl}", got, want[name], lens)
            if shared:
                assert_rows(f"{name} as CSR, level {lvl}", cov_dev(g, lvl, poses, *pack(scans)), want[name], lens)
    lvl = m.levels - 1   # every output alone gives the same bits
    _, poses, scans = nc.cov_batches(oracle_mod, m, lvl)[0]
    pts, offs = pack(scans)
    for i, k in enumerate(KEYS):
        alone = cov_dev(g, lvl, poses, pts, offs, want=tuple(j == i for j in range(4)))
        assert_rows(f"{k} alone, level {lvl}", alone, nc.expected_cov(oracle_mod, m, lvl, KIND)["csr"], nc.CSR_LENS, keys=(k,))
        assert all((alone[j] == SENTINEL).all() for j in KEYS if j != k)
    g.close()


# ---- covariance: the tree order ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parity", ["fast", "relaxed"])
@pytest.mark.parametrize("m,layout", nc.TREE_MAP_LAYOUTS, ids=["%s-%s" % (m.id, layout) for m, layout in nc.TREE_MAP_LAYOUTS])
def test_tree_order_gives_the_probes_bits_on_host_converted_poses(capi, oracle_mod, m, layout, parity):
    g = tge.new_ctx(capi, oracle_mod, m, layout)
    g.set_parity(parity_of(capi, parity))
    for lvl in range(m.levels):
        c = nc.cov_level_case(oracle_mod, m, lvl)
        poses, scans = np.concatenate([c["csr"][0], c["border"][0]]), c["csr"][1] + c["border"][1]
        got = cov_dev(g, lvl, poses, *pack(scans))
        assert capi.load_library().hsm_last_launch_parity(g._h) == parity_of(capi, parity)
        want = dict(cm=[], cw=[], l7=[])
        for w, s in zip(poses, scans):   # the per-scan probe on the host's getMapCoordsPose
            cm, cw, l7 = g.covariance_for_poses(lvl, g.getMapCoordsPose(lvl, w)[None], s)
            want["cm"].append(cm[0]), want["cw"].append(cw[0]), want["l7"].append(l7[0])
        want = {k: np.stack(v) for k, v in want.items()}
        want["lh"] = want["l7"][:, 6]
        assert_rows(f"{parity}, level {lvl}", got, want, [len(s) for s in scans])
    g.close()


# ---- covariance: relations -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parity", ["default", "exact", "fast", "relaxed"])
@pytest.mark.parametrize("m", nc.LH_MAPS, ids=[m.id for m in nc.LH_MAPS])
def test_pose_likelihood_is_the_scores_likelihood(capi, oracle_mod, m, parity):
    g = tge.new_ctx(capi, oracle_mod, m)
    if parity != "default":
        g.set_parity(parity_of(capi, parity))
    for lvl in range(m.levels):
        c = nc.cov_level_case(oracle_mod, m, lvl)
        poses, scans = np.concatenate([c["csr"][0], c["border"][0]]), c["csr"][1] + c["border"][1]
        pts, offs = pack(scans)
        got = cov_dev(g, lvl, poses, pts, offs)
        lh, _ = tsb.score(g, lvl, poses, pts, offs)
        empty = np.array([len(s) == 0 for s in scans])
        assert np.isnan(got["lh"][empty]).all() and np.isnan(lh[empty]).all() and np.isnan(got["l7"][empty]).all()
        assert np.array_equal(bits(got["lh"][~empty]), bits(got["l7"][~empty, 6])), lvl
        assert np.array_equal(bits(got["lh"][~empty]), bits(lh[~empty])), lvl
    g.close()


class ChainBuffers(tcb.ChainBuffers):
    """test_gpu_covariance_batch.ChainBuffers on newer_entry_cases.chain_case: its groups and scan lengths scaled to the map's scan"""
    G, K = nc.CHAIN_GROUPS, nc.CHAIN_K

    def __init__(self, starts, scans):
        import torch
        self.h_init = np.ascontiguousarray(starts, F)
        self.h_pts, self.h_offs = pack(scans)
        self.B = len(self.h_init)
        self.init, self.pts, self.offs = dev(self.h_init), dev(self.h_pts), dev(self.h_offs)
        f = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float32, device="cuda:0")  # noqa: E731
        B, G = self.B, self.G
        self.pose, self.hess, self.cw, self.cm, self.l7, self.lh = f(B, 3), f(B, 9), f(B, 9), f(B, 9), f(B, 7), f(B)
        self.idx = torch.full((G,), 99, dtype=torch.int32, device="cuda:0")
        self.best, self.best_pose = f(G), f(G, 3)


@pytest.mark.parametrize("m", nc.CHAIN_MAPS, ids=[m.id for m in nc.CHAIN_MAPS])
def test_match_cov_is_the_three_calls_and_the_checkers_covariance(capi, oracle_mod, m):
    import torch
    o = m.checker(oracle_mod, KIND)
    g = tge.new_ctx(capi, oracle_mod, m)
    s = torch.cuda.Stream()
    starts, scans = nc.chain_case(oracle_mod, m)
    for lvl in (0, m.levels - 1):
        a, b = ChainBuffers(starts, scans), ChainBuffers(starts, scans)
        torch.cuda.synchronize()
        a.three_calls(g, s, level=lvl)
        b.one_call(g, s, level=lvl)
        s.synchronize()
        ra, rb = a.host(), b.host()
        tcb.assert_same_results(f"one call, level {lvl}", rb, ra)
        K = a.K
        assert not (ra["pose"] == SENTINEL).any() and np.isfinite(ra["pose"]).all(), "the matches are defined"
        assert_rows(f"matched poses, level {lvl}", dict(cw=ra["cw"], cm=ra["cm"], l7=ra["l7"], lh=ra["lh"]),
                    reference(o, lvl, ra["pose"], scans), np.diff(a.h_offs))
        idx, best = select_rule.select_best(ra["lh"], groups=a.G, group_size=K)
        assert np.array_equal(ra["idx"], idx) and idx[2] == -1 and (idx[:2] >= 0).all()
        assert np.array_equal(bits(ra["best"][:2]), bits(best[:2])) and np.isnan(ra["best"][2])
        assert np.array_equal(bits(ra["best_pose"][:2]), bits(ra["pose"][idx[:2]]))
    g.close()


# ---- covariance on a moved map -------------------------------------------------------------------------------------------------------------
MOVED_COV = [(m, layout) for m, layout in mec.MAP_LAYOUTS if m in (mec.M96, mec.DEEP)]


@pytest.mark.parametrize("m,layout", MOVED_COV, ids=["%s-%s" % (m.id, layout) for m, layout in MOVED_COV])
def test_covariance_on_a_moved_map(capi, oracle_mod, m, layout):
    o = mec.reader_checker(oracle_mod, KIND, m, MOVE)
    g = tshift.load(tshift.new_ctx(capi, m, layout), sc.old_planes(oracle_mod, m))
    g.shift_map(mec.case_plan(m, MOVE)[0])
    for lvl in range(m.levels):
        poses, scans = nc.cov_level_case(oracle_mod, m, lvl)["csr"]   # world poses: the world does not move with the window
        pts, offs = pack(scans)
        want = reference(o, lvl, poses, scans)
        assert_rows(f"moved CSR, level {lvl}", cov_dev(g, lvl, poses, pts, offs), want, nc.CSR_LENS)
        maps = nc.border_map_poses(m.dims(lvl))   # the borders of the MOVED window
        bposes = np.stack([o.world_coords_pose(lvl, p) for p in maps]).astype(F)
        bscans = [scans[-1]] * len(maps)
        assert_rows(f"moved borders, level {lvl}", cov_dev(g, lvl, bposes, *pack(bscans)), reference(o, lvl, bposes, bscans),
                    [len(s) for s in bscans])
        if lvl == 1:
            host = dict(zip(KEYS, g.covariance_batch(lvl, poses, pts, offs)))
            assert_rows(f"host form, level {lvl}", host, want, nc.CSR_LENS)
    g.close()


# ---- merge -----------------------------------------------------------------------------------------------------------------------------------
def minus_ones(lo):
    return np.full(lo.shape, -1, np.int32)


def loaded(capi, geom, layout, planes):
    g = tgm.new_ctx(capi, geom, layout)
    for lvl, lo in enumerate(planes):
        g.upload_level(lvl, lo, minus_ones(lo))
    return g


def probe_scan(geom):
    """a fan of 120 end points 6 .. 14 level-0 cells out, and six world poses round the window's centre"""
    rng = np.random.default_rng(2950)
    a = np.linspace(-2.2, 2.2, 120)
    r = 10.0 + 4.0 * np.sin(3.0 * a)
    pts = np.ascontiguousarray(np.stack([r * np.cos(a), r * np.sin(a)], 1), F)
    c = nc.level0_centre(geom)
    res = float(F(geom[0]))
    starts = (np.array([c[0], c[1], 0.4])[None] + rng.uniform(-1, 1, (6, 3)) * [3 * res, 3 * res, 0.3]).astype(F)
    return starts, pts


def assert_reads_alike(dst, exp, geom, what, reads):
    """test_gpu_merge_map.assert_reads_alike on a geometry of its own: a score on every level; a match and a cast besides where
    level 0 has READS_MIN_SIDE cells both ways"""
    starts, pts = probe_scan(geom)
    for lvl in range(geom[3]):
        sa, sb = dst.score_batch(lvl, starts, pts), exp.score_batch(lvl, starts, pts)
        assert np.array_equal(bits(sa[0]), bits(sb[0])) and np.array_equal(bits(sa[1]), bits(sb[1])), (what, "score", lvl)
    if not reads:
        return
    a, b = dst.match_batch(starts, pts), exp.match_batch(starts, pts)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1])), (what, "match", a[0], b[0])
    angles = np.linspace(-3.1, 3.1, 48).astype(F)
    rmax = 30.0 * float(F(geom[0]))
    for lvl in range(geom[3]):
        ca, cb = dst.cast_scans(lvl, starts[:3], angles, rmax), exp.cast_scans(lvl, starts[:3], angles, rmax)
        assert np.array_equal(bits(ca[0]), bits(cb[0])) and np.array_equal(bits(ca[1]), bits(cb[1])), (what, "cast", lvl)


def check_merge(capi, dst, src, case, layout, what, reads):
    """the merge of `case` queued on dst and held to the model: log-odds bit for bit over all cells, stamps untouched, the
    probability plane, the dirty box, hsm_merge_map_box, the update index, src unchanged, and the reads of a context
    uploaded from the model"""
    gd, t, model = case["gd"], case["t"], case["model"]
    levels = gd[3]
    index = [dst.getUpdateIndex(lvl) for lvl in range(levels)]
    for lvl in range(levels):
        dst.take_dirty_bbox(lvl)
        assert capi.merge_map_box(dst, src, t, lvl).tolist() == list(model[lvl][1]), (what, lvl, "hsm_merge_map_box")
    starts = dst.map_start().copy(), src.map_start().copy()
    capi.merge_map(dst, src, t)
    assert np.array_equal(bits(dst.map_start()), bits(starts[0])) and np.array_equal(bits(src.map_start()), bits(starts[1]))
    for lvl, (lo, st) in enumerate(tgm.planes(dst)):
        want, box = model[lvl]
        differ = int((bits(lo) != bits(want)).sum())
        assert differ == 0, (what, lvl, "log odds", differ, "of", lo.size, "box", box)
        assert (st == -1).all(), (what, lvl, "stamps")
        assert np.array_equal(bits(dst.download_prob(lvl)), bits(tgm.grid_probability(capi, dst, want))), (what, lvl, "probabilities")
        assert dst.getUpdateIndex(lvl) == index[lvl] + 1, (what, lvl, "update index")
        assert dst.take_dirty_bbox(lvl).tolist() == list(box), (what, lvl, "dirty box")
    for lvl, (lo, st) in enumerate(tgm.planes(src)):
        assert np.array_equal(bits(lo), bits(case["src"][lvl])) and (st == -1).all(), (what, lvl, "src")
    exp = loaded(capi, gd, layout, [w for w, _ in model])
    assert_reads_alike(dst, exp, gd, what, reads)
    return exp


@pytest.mark.parametrize("pair,name,layout", nc.MERGE_RUNS, ids=nc.MERGE_RUN_IDS)
def test_merged_state_is_the_models_on_every_new_pair(capi, pair, name, layout):
    case = nc.merge_case(pair, name)
    dst, src = loaded(capi, case["gd"], layout, case["dst"]), loaded(capi, case["gs"], layout, case["src"])
    reads = min(case["gd"][1], case["gd"][2]) >= nc.READS_MIN_SIDE
    exp = check_merge(capi, dst, src, case, layout, (pair, name, layout), reads)
    for g in (dst, src, exp):
        g.close()


@pytest.mark.parametrize("m,move,side,layout", nc.MOVED_RUNS, ids=nc.MOVED_RUN_IDS)
def test_moved_merge_is_the_shifted_model(capi, oracle_mod, m, move, side, layout):
    case = nc.moved_case(oracle_mod, m, move, side)
    geom = nc.geometry_of(m)
    dst, src = loaded(capi, geom, layout, case["old_dst"]), loaded(capi, geom, layout, case["old_src"])
    for g, moved in ((dst, side in ("dst", "both")), (src, side in ("src", "both"))):
        if moved:
            assert g.shift_map(case["start"]) == tuple(case["d0"])
    for lvl, (lo, _) in enumerate(tgm.planes(dst)):   # the move itself: what the merge starts from
        assert np.array_equal(bits(lo), bits(case["dst"][lvl])), (lvl, "dst before the merge")
    exp = check_merge(capi, dst, src, case, layout, (m.id, move, side, layout), True)
    for g in (dst, src, exp):
        g.close()


def test_staged_route_gives_the_same_bits_on_the_new_pairs():
    """the pair and the moved tests again with HSM_COPY_STAGE=1: every merge goes through the staging patch"""
    if os.environ.get("HSM_COPY_STAGE") == "1":
        pytest.fail("the child run must not select this test")
    env = dict(os.environ, HSM_COPY_STAGE="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__),
                        "-k", "every_new_pair or moved_merge"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "%d passed" % (len(nc.MERGE_RUNS) + len(nc.MOVED_RUNS)) in r.stdout, r.stdout[-2000:]


@pytest.mark.parametrize("pair", ("tiny", "deep"))
def test_an_update_after_the_merge_leaves_the_same_planes_on_all_levels(capi, pair):
    """texels and probabilities of the coarse levels: one updateByScan on dst and on a context uploaded from the model"""
    case = nc.merge_case(pair, "theta_0.3")
    gd = case["gd"]
    dst, src = loaded(capi, gd, "quad", case["dst"]), loaded(capi, case["gs"], "quad", case["src"])
    exp = loaded(capi, gd, "quad", [w for w, _ in case["model"]])
    capi.merge_map(dst, src, case["t"])
    starts, pts = probe_scan(gd)
    for g in (dst, exp):
        single_update(capi, g, starts[0], pts)
    touched = 0
    for lvl in range(gd[3]):
        (lo, st), (lo_e, st_e) = dst.download_level(lvl), exp.download_level(lvl)
        assert np.array_equal(bits(lo), bits(lo_e)) and np.array_equal(st, st_e), (lvl, "the update after the merge")
        assert np.array_equal(bits(dst.download_prob(lvl)), bits(exp.download_prob(lvl))), (lvl, "probabilities")
        touched += int((st != -1).sum())
    assert touched > 0, "the scan marks cells"
    for g in (dst, src, exp):
        g.close()
