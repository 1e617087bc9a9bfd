"""hsm_score_window* / hsm_window_poses_device / hsm_select_topk_device / hsm_relocalize* on the MI355X.

Window scores carry the CPU reference's bits (`likelihood_states` / `residual_states` at `map_coords_pose(window pose)` with the
level-scaled container) in BOTH kernel forms, and the bits hsm_score_batch_device gives on the written-out poses; a scan of 0
beams gives NaN likelihoods (compared as NaN: the payload of an invalid operation's NaN is the processor's choice) and residual
+0.  The K best follow tests/topk_rule.py.  The relocalisation equals the four public calls and the reference composition of
tests/test_window_model.py on the committed case of tests/window_cases.py.  Every output buffer is filled with a sentinel
before a launch so that a row no launch wrote shows.
"""
import numpy as np
import pytest

import select_rule
import topk_rule
import window_cases
from conftest import bits, make_oracle, oracle_kinds
from support import capi, dev, layout_of, stream_ptr
from test_window_model import reference_relocalize

pytestmark = pytest.mark.gpu

HSM_ERR_INVALID = -1
SENTINEL = -777.0
LENS = (0, 1, 63, 64, 65, 200)
FORMS = ("lane", "wave")
KERNEL = {"lane": b"score_window_lane_kernel", "wave": b"score_window_wave_kernel"}


def gpu_for(capi, sc, o, sx=None, sy=None, stamps=True, **kw):
    g = capi.MapRepMultiMap(sc.resolution, sx or sc.map_size, sy or sc.map_size, sc.levels, **kw)
    g.setUpdateFactorFree(0.4)
    g.setUpdateFactorOccupied(0.9)
    for lvl in range(sc.levels):
        lo, ui = o.download_level(lvl)
        g.upload_level(lvl, lo, ui if stamps else None)
    g.synchronize()
    return g


def forced(monkeypatch, form):
    if form is None:
        monkeypatch.delenv("HSM_WINDOW_FORM", raising=False)
    else:
        monkeypatch.setenv("HSM_WINDOW_FORM", form)


def score_window(g, level, centre, step, half, pts, want=(True, True)):
    """hsm_score_window_device on torch buffers -> (likelihood, residual) on the host"""
    import torch
    W = window_cases.window_count(half)
    d_c, d_pts = dev(np.asarray(centre, np.float32)), dev(np.asarray(pts, np.float32).reshape(-1, 2))
    out = torch.full((2, W), SENTINEL, dtype=torch.float32, device="cuda:0")
    g.score_window_device(level, d_c.data_ptr(), step, half, d_pts.data_ptr() if len(pts) else 0, len(pts),
                          out[0].data_ptr() if want[0] else 0, out[1].data_ptr() if want[1] else 0, stream_ptr())
    r = out.cpu().numpy()
    return r[0], r[1]


def written_poses(g, centre, step, half, index=None, count=None):
    import torch
    n = window_cases.window_count(half) if index is None and count is None else (len(index) if count is None else count)
    d_c = dev(np.asarray(centre, np.float32))
    d_i = None if index is None else dev(np.asarray(index, np.int32))
    out = torch.full((n, 3), SENTINEL, dtype=torch.float32, device="cuda:0")
    g.window_poses_device(d_c.data_ptr(), step, half, 0 if d_i is None else d_i.data_ptr(), n, out.data_ptr(), stream_ptr())
    return out


def score_batch(g, level, d_poses, pts):
    import torch
    B = d_poses.shape[0]
    d_pts = dev(np.asarray(pts, np.float32).reshape(-1, 2))
    out = torch.full((2, B), SENTINEL, dtype=torch.float32, device="cuda:0")
    g.score_batch_device(level, B, d_poses.data_ptr(), d_pts.data_ptr() if len(pts) else 0, 0, len(pts), out[0].data_ptr(),
                         out[1].data_ptr(), stream_ptr())
    r = out.cpu().numpy()
    return r[0], r[1]


def oracle_window(o, level, poses, pts):
    pm = np.stack([o.map_coords_pose(level, p) for p in poses]).astype(np.float32)
    pl = np.asarray(pts, np.float32).reshape(-1, 2) * np.float32(1.0 / 2 ** level)
    return o.likelihood_states(level, pm, pl), o.residual_states(level, pm, pl)


def assert_same_scores(what, got, ref, n):
    (lh, res), (rlh, rres) = got, ref
    assert not (lh == SENTINEL).any() and not (res == SENTINEL).any(), f"{what}: rows never written"
    bad = bits(res) != bits(rres)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {len(res)} residuals differ, first {np.flatnonzero(bad)[:5]}"
    if n == 0:
        assert np.isnan(lh).all() and np.isnan(rlh).all() and (bits(res) == 0).all(), what
        return
    bad = bits(lh) != bits(rlh)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {len(lh)} likelihoods differ, first {np.flatnonzero(bad)[:5]}"


_REFS = {}


def window_reference(o, kind, tag, level, centre, step, half, pts):
    """the oracle's scores of a window, computed once and shared by the layouts and forms"""
    key = (kind, tag, level, tuple(half), len(pts))
    if key not in _REFS:
        _REFS[key] = oracle_window(o, level, window_cases.window_poses(centre, step, half), pts)
    return _REFS[key]


# ---- 1: both forms against both oracle kinds and against the batched score -----------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("layout", ["quad", "plane"])
@pytest.mark.parametrize("kind", oracle_kinds())
def test_window_scores_are_bit_identical_in_both_forms(capi, oracle_mod, pyramid_scene, monkeypatch, kind, layout, form):
    sc = pyramid_scene
    o = make_oracle(oracle_mod, kind, sc)
    forced(monkeypatch, form)
    g = gpu_for(capi, sc, o, layout=layout_of(capi, layout))
    lib = capi.load_library()
    truth = sc.query_truth[1].astype(np.float32)
    centre = (truth + np.float32([0.03, -0.02, 0.01])).astype(np.float32)
    edge = np.float32([12.0, 12.1, 0.3])  # the map ends at 12.8 m: the far corner of the (3, 2, 1) window below lies outside
    for lvl in range(sc.levels):
        for half in window_cases.WINDOWS:
            for n in LENS:
                pts = sc.query_scans[1][:n]
                got = score_window(g, lvl, centre, window_cases.STEP, half, pts)
                assert lib.hsm_last_launch_kernel(g._h) == KERNEL[form] and lib.hsm_last_launch_parity(g._h) == capi.PARITY_EXACT
                what = f"{kind} {layout} {form} level {lvl} window {half} {n} beams"
                assert_same_scores(what, got, window_reference(o, kind, "centre", lvl, centre, window_cases.STEP, half, pts), n)
                d_poses = written_poses(g, centre, window_cases.STEP, half)
                assert np.array_equal(bits(d_poses.cpu().numpy()), bits(window_cases.window_poses(centre, window_cases.STEP, half)))
                assert_same_scores(what + " (batched score)", got, score_batch(g, lvl, d_poses, pts), n)
        pts = sc.query_scans[1][:200]
        step = (0.5, 0.5, 0.1)
        got = score_window(g, lvl, edge, step, (3, 2, 1), pts)
        ref = window_reference(o, kind, "edge", lvl, edge, step, (3, 2, 1), pts)
        assert_same_scores(f"{kind} {layout} {form} level {lvl} over the map's edge", got, ref, 200)
        assert got[1].max() > got[1].min()
        only_lh, _ = score_window(g, lvl, edge, step, (3, 2, 1), pts, want=(True, False))
        _, only_res = score_window(g, lvl, edge, step, (3, 2, 1), pts, want=(False, True))
        assert np.array_equal(bits(only_lh), bits(got[0])) and np.array_equal(bits(only_res), bits(got[1]))
    if form == "lane" and layout == "quad":  # the host form
        lh, res = g.score_window(0, centre, window_cases.STEP, (3, 2, 1), sc.query_scans[1][:200])
        want = score_window(g, 0, centre, window_cases.STEP, (3, 2, 1), sc.query_scans[1][:200])
        assert np.array_equal(bits(lh), bits(want[0])) and np.array_equal(bits(res), bits(want[1]))
    g.close()


def test_default_form_is_chosen_by_the_window_size(capi, oracle_mod, small_scene, monkeypatch):
    """below the threshold a wavefront per hypothesis, from it on a lane per hypothesis: the same bits across it"""
    sc = small_scene
    o = make_oracle(oracle_mod, "ho", sc)
    lib = capi.load_library()
    pts = sc.query_scans[0][:65]
    centre = sc.query_truth[0].astype(np.float32)
    half, step = (40, 40, 5), (0.05, 0.05, 0.02)  # 72 171 hypotheses
    res = {}
    for form in (None, "lane", "wave"):
        forced(monkeypatch, form)
        g = gpu_for(capi, sc, o)
        res[form] = score_window(g, 0, centre, step, half, pts)
        if form is None:
            assert lib.hsm_last_launch_kernel(g._h) == KERNEL["lane"]
            score_window(g, 0, centre, step, (3, 2, 1), pts)
            assert lib.hsm_last_launch_kernel(g._h) == KERNEL["wave"]
        g.close()
    for form in ("lane", "wave"):
        assert np.array_equal(bits(res[form][0]), bits(res[None][0])) and np.array_equal(bits(res[form][1]), bits(res[None][1]))
    assert np.unique(res[None][1]).size > 1000


# ---- 2: a centre that is not finite ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_non_finite_centre_gives_the_batched_scores_bits(capi, oracle_mod, pyramid_scene, monkeypatch, form):
    sc = pyramid_scene
    o = make_oracle(oracle_mod, "ho", sc)
    forced(monkeypatch, form)
    g = gpu_for(capi, sc, o)
    truth = sc.query_truth[2].astype(np.float32)
    pts = sc.query_scans[2][:65]
    for a in range(3):
        for v in (np.nan, np.inf, -np.inf):
            centre = truth.copy()
            centre[a] = v
            got = score_window(g, 1, centre, window_cases.STEP, (3, 2, 1), pts)
            want = score_batch(g, 1, written_poses(g, centre, window_cases.STEP, (3, 2, 1)), pts)
            for k in range(2):
                both_nan = np.isnan(got[k]) & np.isnan(want[k])
                assert (both_nan | (bits(got[k]) == bits(want[k]))).all(), (a, v, k)
    g.close()


# ---- 3: the parity modes change nothing -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_parity_modes_keep_the_reference_order(capi, oracle_mod, pyramid_scene, monkeypatch, form):
    sc = pyramid_scene
    o = make_oracle(oracle_mod, "ho", sc)
    forced(monkeypatch, form)
    g = gpu_for(capi, sc, o)
    lib = capi.load_library()
    centre = sc.query_truth[1].astype(np.float32)
    pts = sc.query_scans[1][:200]
    want = score_window(g, 0, centre, window_cases.STEP, (3, 2, 1), pts)
    for mode in (capi.PARITY_FAST, capi.PARITY_RELAXED):
        g.set_parity(mode)
        got = score_window(g, 0, centre, window_cases.STEP, (3, 2, 1), pts)
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1])), mode
        assert lib.hsm_last_launch_parity(g._h) == capi.PARITY_EXACT and lib.hsm_last_launch_kernel(g._h) == KERNEL[form]
    g.close()


# ---- 4: a rectangular map -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_rectangular_map(capi, oracle_mod, monkeypatch, form):
    import rect_cases
    sx, sy, levels = 333, 90, 2
    world, truth, scans_all = rect_cases.scene(sx, sy, 24, 1081, seed=3)
    o = oracle_mod.Oracle(oracle_kinds()[-1], rect_cases.RES, sx, sy, levels)
    o.set_update_factor_free(0.4)
    o.set_update_factor_occupied(0.9)
    o.build_map(truth[:16], scans_all[:16])
    forced(monkeypatch, form)
    g = capi.MapRepMultiMap(rect_cases.RES, sx, sy, levels)
    for lvl in range(levels):
        g.upload_level(lvl, *o.download_level(lvl))
    centre = truth[17].astype(np.float32)
    pts = scans_all[17][:200]
    for lvl in range(levels):
        got = score_window(g, lvl, centre, window_cases.STEP, (3, 2, 1), pts)
        ref = oracle_window(o, lvl, window_cases.window_poses(centre, window_cases.STEP, (3, 2, 1)), pts)
        assert_same_scores(f"rectangular, level {lvl}", got, ref, 200)
        assert got[0][52] > 0.05  # (the centre sees the map: the case is not all out-of-map zeros)
    g.close()


# ---- 5: the K best --------------------------------------------------------------------------------------------------------------
def run_topk(g, capi, scores, k, want_score=True):
    """exact-size workspace full of garbage, with a guard behind it"""
    import torch
    s = np.asarray(scores, np.float32)
    d_s = dev(s) if s.size else torch.zeros(1, dtype=torch.float32, device="cuda:0")
    nbytes = capi.MapRepMultiMap.select_topk_workspace(s.size, k)
    assert nbytes > 0 and nbytes % 8 == 0
    garbage = np.random.default_rng(s.size + k).integers(0, 2**32, nbytes // 4 + 16, dtype=np.uint32)
    ws = dev(garbage.view(np.int32))
    idx = torch.full((k,), 99, dtype=torch.int32, device="cuda:0")
    best = torch.full((k,), SENTINEL, dtype=torch.float32, device="cuda:0")
    g.select_topk_device(s.size, d_s.data_ptr() if s.size else 0, k, idx.data_ptr(), best.data_ptr() if want_score else 0,
                         ws.data_ptr(), nbytes, stream_ptr())
    assert np.array_equal(ws.cpu().numpy().view(np.uint32)[nbytes // 4:], garbage[nbytes // 4:]), "wrote behind the workspace"
    return idx.cpu().numpy(), best.cpu().numpy()


def test_topk_follows_the_rule(capi, oracle_mod, small_scene):
    import torch
    g = gpu_for(capi, small_scene, make_oracle(oracle_mod, "ho", small_scene, build=False))
    for name, s in topk_rule.topk_cases():
        for k in (1, 8, 64):
            idx, best = run_topk(g, capi, s, k)
            want_idx, want_best = topk_rule.topk(s, k)
            assert np.array_equal(idx, want_idx), (name, k, idx[:10], want_idx[:10])
            none = want_idx < 0
            assert np.isnan(best[none]).all() and np.array_equal(bits(best[~none]), bits(want_best[~none])), (name, k)
        idx, best = run_topk(g, capi, s, 8, want_score=False)
        assert np.array_equal(idx, topk_rule.topk(s, 8)[0]) and (best == SENTINEL).all(), name
        if s.size:  # k == 1 is hsm_select_best_device's winner
            one = torch.full((1,), 99, dtype=torch.int32, device="cuda:0")
            g.select_best_device(1, 0, s.size, dev(s).data_ptr(), 0, one.data_ptr(), 0, 0, stream_ptr())
            assert run_topk(g, capi, s, 1)[0][0] == one.cpu().numpy()[0] == select_rule.select_best(s, groups=1, group_size=s.size)[0][0]
    g.close()


# ---- 6: window indices as poses ---------------------------------------------------------------------------------------------------
def test_window_poses_of_given_indices(capi, oracle_mod, small_scene):
    g = gpu_for(capi, small_scene, make_oracle(oracle_mod, "ho", small_scene, build=False))
    centre = np.float32([1.2345678, -2.7182817, 0.31415927])
    for half in window_cases.WINDOWS:
        W = window_cases.window_count(half)
        index = np.array([0, W - 1, -1, W, W // 2, W // 2, -7, 2**31 - 1, 0] + list(range(min(W, 300))), np.int32)
        got = written_poses(g, centre, window_cases.STEP, half, index).cpu().numpy()
        want = window_cases.window_poses(centre, window_cases.STEP, half, index)
        outside = (index < 0) | (index >= W)
        assert np.isnan(got[outside]).all() and np.array_equal(bits(got[~outside]), bits(want[~outside])), half
        part = written_poses(g, centre, window_cases.STEP, half, count=(W + 1) // 2).cpu().numpy()
        assert np.array_equal(bits(part), bits(window_cases.window_poses(centre, window_cases.STEP, half)[:(W + 1) // 2]))
    g.close()


# ---- 7: the relocalisation --------------------------------------------------------------------------------------------------------
class RelocBuffers:
    def __init__(self, capi, centre, scan, step, half, k):
        import torch
        self.step, self.half, self.k, self.n = step, half, k, len(scan)
        self.W = window_cases.window_count(half)
        self.centre, self.pts = dev(np.asarray(centre, np.float32)), dev(np.asarray(scan, np.float32).reshape(-1, 2))
        f = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float32, device="cuda:0")  # noqa: E731
        i = lambda *shape: torch.full(shape, 99, dtype=torch.int32, device="cuda:0")  # noqa: E731
        self.cand, self.cov, self.lh0, self.best_pose, self.best_score, self.best_index = f(k, 3), f(k, 9), f(k), f(3), f(1), i(1)
        self.ws_bytes = capi.MapRepMultiMap.relocalize_workspace(self.W, k)
        self.ws = torch.full((self.ws_bytes // 4,), -1, dtype=torch.int32, device="cuda:0")
        # what the four separate calls need on top
        self.scores, self.kidx, self.kscore, self.start = f(self.W), i(k), f(k), f(k, 3)
        self.topk_bytes = capi.MapRepMultiMap.select_topk_workspace(self.W, k)
        self.topk_ws = torch.zeros(self.topk_bytes // 4, dtype=torch.int32, device="cuda:0")

    def pts_ptr(self):
        return self.pts.data_ptr() if self.n else 0

    def one_call(self, g, level, s):
        g.relocalize_device(level, self.centre.data_ptr(), self.step, self.half, self.k, self.pts_ptr(), self.n, self.ws.data_ptr(),
                            self.ws_bytes, self.cand.data_ptr(), self.cov.data_ptr(), self.lh0.data_ptr(), self.best_pose.data_ptr(),
                            self.best_score.data_ptr(), self.best_index.data_ptr(), s)

    def four_calls(self, g, level, s):
        g.score_window_device(level, self.centre.data_ptr(), self.step, self.half, self.pts_ptr(), self.n, self.scores.data_ptr(), 0, s)
        g.select_topk_device(self.W, self.scores.data_ptr(), self.k, self.kidx.data_ptr(), self.kscore.data_ptr(),
                             self.topk_ws.data_ptr(), self.topk_bytes, s)
        g.window_poses_device(self.centre.data_ptr(), self.step, self.half, self.kidx.data_ptr(), self.k, self.start.data_ptr(), s)
        g.match_score_batch_device(self.k, self.start.data_ptr(), self.pts_ptr(), 0, self.n, self.cand.data_ptr(), self.cov.data_ptr(),
                                   0, self.lh0.data_ptr(), 0, 1, 0, self.k, self.best_index.data_ptr(), self.best_score.data_ptr(),
                                   self.best_pose.data_ptr(), s)

    def host(self):
        r = {k: getattr(self, k).cpu().numpy() for k in ("cand", "cov", "lh0", "best_pose", "best_score", "best_index")}
        return r

    def refill(self):
        for t in (self.cand, self.cov, self.lh0, self.best_pose, self.best_score):
            t.fill_(SENTINEL)
        self.best_index.fill_(99)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != np.float32:
        return np.array_equal(a, b)
    return bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def test_relocalize_equals_the_four_calls_and_the_reference(capi, oracle_mod, pyramid_scene):
    import torch
    sc = pyramid_scene
    kind = oracle_kinds()[-1]
    o = make_oracle(oracle_mod, kind, sc)
    g = gpu_for(capi, sc, o)
    truth, centre, scan = window_cases.reloc_case(sc)
    step, half, k, lvl = window_cases.RELOC_STEP, window_cases.RELOC_HALF, window_cases.RELOC_K, sc.levels - 1
    s = torch.cuda.Stream()
    one, four = (RelocBuffers(capi, centre, scan, step, half, k) for _ in range(2))
    torch.cuda.synchronize()
    one.one_call(g, lvl, s.cuda_stream)
    four.four_calls(g, lvl, s.cuda_stream)
    s.synchronize()
    r1, r4 = one.host(), four.host()
    kidx = four.kidx.cpu().numpy()
    place = int(r4["best_index"][0])
    assert 0 <= place < k
    r4["best_index"] = kidx[[place]]  # the fourth call names the place among the k; the one call the window index behind it
    for key in r1:
        assert not (r1[key] == (99 if key == "best_index" else SENTINEL)).any(), key
        assert same_bits(r1[key], r4[key]), key
    ref = reference_relocalize(o, sc, centre, scan, step, half, k)
    assert np.array_equal(bits(four.scores.cpu().numpy()), bits(ref["scores"]))
    assert np.array_equal(kidx, ref["index"]) and np.array_equal(bits(four.kscore.cpu().numpy()), bits(ref["top"]))
    assert np.array_equal(bits(four.start.cpu().numpy()), bits(ref["start"]))
    assert np.array_equal(bits(r1["cand"]), bits(ref["cand"])) and np.array_equal(bits(r1["cov"]), bits(ref["cov"]))
    assert np.array_equal(bits(r1["lh0"]), bits(ref["lh0"]))
    assert r1["best_index"][0] == ref["best_index"] and bits(r1["best_score"])[0] == bits(ref["best_score"])
    assert np.array_equal(bits(r1["best_pose"]), bits(ref["best_pose"]))
    assert np.hypot(*(r1["best_pose"][:2] - truth[:2])) <= sc.resolution
    # the host form
    h = g.relocalize(lvl, centre, step, half, k, scan)
    assert same_bits(h["cand_pose"], r1["cand"]) and same_bits(h["cand_cov"], r1["cov"]) and same_bits(h["cand_likelihood"], r1["lh0"])
    assert same_bits(h["best_pose"], r1["best_pose"]) and bits(h["best_score"]) == bits(r1["best_score"])[0]
    assert h["best_index"] == r1["best_index"][0]
    g.close()


def test_relocalize_with_fewer_scores_than_places(capi, oracle_mod, pyramid_scene):
    """a window of three poses and k = 8: five NaN starts, which the matcher survives and which never win; an empty scan: every
    window score is NaN, no winner"""
    import torch
    sc = pyramid_scene
    o = make_oracle(oracle_mod, oracle_kinds()[-1], sc)
    g = gpu_for(capi, sc, o)
    truth, _, scan = window_cases.reloc_case(sc)
    centre = (truth + np.float32([0.05, 0.0, 0.0])).astype(np.float32)
    step, half, k = (0.05, 0.05, 0.01), (1, 0, 0), 8
    b = RelocBuffers(capi, centre, scan, step, half, k)
    torch.cuda.synchronize()
    b.one_call(g, 0, stream_ptr())
    torch.cuda.synchronize()
    r = b.host()
    ref = reference_relocalize(o, sc, centre, scan, step, half, k, search_level=0)
    assert (ref["index"][:3] >= 0).all() and (ref["index"][3:] == -1).all()
    assert np.array_equal(bits(r["cand"][:3]), bits(ref["cand"][:3])) and np.array_equal(bits(r["cov"][:3]), bits(ref["cov"][:3]))
    assert np.array_equal(bits(r["lh0"][:3]), bits(ref["lh0"][:3]))
    assert not np.isfinite(r["cand"][3:]).all(axis=1).any()          # a NaN start stays a non-finite row ...
    assert (np.isnan(r["lh0"][3:]) | (r["lh0"][3:] <= 0.0)).all()    # ... that scores nothing
    assert r["best_index"][0] == ref["best_index"] and np.array_equal(bits(r["best_pose"]), bits(ref["best_pose"]))
    assert bits(r["best_score"])[0] == bits(ref["best_score"])
    e = RelocBuffers(capi, centre, scan[:0], step, half, k)
    torch.cuda.synchronize()
    e.one_call(g, 0, stream_ptr())
    torch.cuda.synchronize()
    r = e.host()
    assert r["best_index"][0] == -1 and np.isnan(r["best_score"][0]) and (r["best_pose"] == SENTINEL).all()
    assert np.isnan(r["lh0"]).all()
    # four ordinary matches afterwards: the context is as it was
    got = g.match_batch(np.stack([sc.query_truth[q] for q in range(4)]), sc.query_scans[0], want_cov=False)[0]
    want = np.stack([o.match(sc.query_truth[q], sc.query_scans[0])[0] for q in range(4)])
    assert np.array_equal(bits(got), bits(want))
    g.close()


# ---- 8: ordering against map updates -------------------------------------------------------------------------------------------
def oracle_update(o, pose, pts):
    o.update_by_scan(pose, pts)
    o.on_map_updated()


def test_window_scores_are_ordered_against_queued_updates(capi, oracle_mod, pyramid_scene):
    """an update queued on the context, then a window score on a caller's stream with no host wait: the updated map's scores; a
    score queued first, then an update: the scores of the map before it"""
    import torch
    from hector_slam_amd import synth
    sc = pyramid_scene
    o = make_oracle(oracle_mod, oracle_kinds()[-1], sc)
    g = gpu_for(capi, sc, o, stamps=False)  # (log-odds alone: the updates below are meant to change the map)
    rng = np.random.default_rng(8)
    sfac = float(np.float32(1.0) / np.float32(sc.resolution))
    dense = [synth.make_scan(sc.world, sc.build_poses[t], 16384, sfac, rng) for t in range(6)]
    centre = sc.query_truth[0].astype(np.float32)
    pts = sc.query_scans[0][:200]
    half, step = (20, 10, 2), window_cases.STEP  # 4305 hypotheses
    poses = window_cases.window_poses(centre, step, half)
    W = len(poses)
    d_c, d_pts = dev(centre), dev(pts)
    s = torch.cuda.Stream()
    outs = [torch.full((2, W), SENTINEL, dtype=torch.float32, device="cuda:0") for _ in range(3)]
    torch.cuda.synchronize()

    def launch(out):
        g.score_window_device(0, d_c.data_ptr(), step, half, d_pts.data_ptr(), len(pts), out[0].data_ptr(), out[1].data_ptr(),
                              s.cuda_stream)
    refs = []
    for t in range(3):
        g.updateByScan(dense[t], sc.build_poses[t])  # queued, not waited for
        oracle_update(o, sc.build_poses[t], dense[t])
    launch(outs[0])                                   # behind the three updates
    refs.append(oracle_window(o, 0, poses, pts))
    g.updateByScan(dense[3], sc.build_poses[3])       # behind the score: it must not rewrite the map under it
    oracle_update(o, sc.build_poses[3], dense[3])
    launch(outs[1])
    refs.append(oracle_window(o, 0, poses, pts))
    launch(outs[2])                                   # score queued ...
    g.updateByScan(dense[4], sc.build_poses[4])       # ... then an update: the score sees the map before it
    g.updateByScan(dense[5], sc.build_poses[5])
    refs.append(refs[-1])
    s.synchronize()
    g.synchronize()
    for k in range(3):
        r = outs[k].cpu().numpy()
        assert_same_scores(f"launch {k}", (r[0], r[1]), refs[k], len(pts))
    assert not np.array_equal(bits(refs[0][0]), bits(refs[1][0]))  # the updates do change these scores
    for t in (4, 5):
        oracle_update(o, sc.build_poses[t], dense[t])
    assert np.array_equal(bits(g.download_level(0)[0]), bits(o.download_level(0)[0]))
    g.close()


# ---- 9: graph capture -------------------------------------------------------------------------------------------------------------
def test_relocalize_captured_in_a_graph_and_replayed(capi, oracle_mod, pyramid_scene):
    import torch
    sc = pyramid_scene
    o = make_oracle(oracle_mod, oracle_kinds()[-1], sc)
    g = gpu_for(capi, sc, o)
    truth, centre, scan = window_cases.reloc_case(sc)
    step, half, k, lvl = window_cases.RELOC_STEP, window_cases.RELOC_HALF, window_cases.RELOC_K, sc.levels - 1
    s = torch.cuda.Stream()
    buf = RelocBuffers(capi, centre, scan, step, half, k)
    torch.cuda.synchronize()
    buf.one_call(g, lvl, s.cuda_stream)  # eager first: nothing is allocated under capture
    s.synchronize()
    eager = buf.host()
    graph = torch.cuda.CUDAGraph()
    idx0 = g.getUpdateIndex(0)
    with torch.cuda.graph(graph, stream=s):
        buf.one_call(g, lvl, s.cuda_stream)
        with pytest.raises(capi.HsmError) as e:
            g.updateByScan(sc.build_scans[0], sc.build_poses[0])
        assert f"({HSM_ERR_INVALID})" in str(e.value) and "captur" in str(e.value), str(e.value)
    assert g.getUpdateIndex(0) == idx0
    with torch.cuda.stream(s):
        buf.refill()
        graph.replay()
    s.synchronize()
    got = buf.host()
    for key in got:
        assert same_bits(got[key], eager[key]), key
    for rep, q in enumerate((1, 2)):  # a new centre and a new scan (of the same length) in the same buffers
        t2 = sc.query_truth[q].astype(np.float32)
        c2 = (t2 + np.float32([0.8, -0.6, -0.4]) * np.float32(1 - 2 * rep)).astype(np.float32)
        scan2 = sc.query_scans[q]
        assert len(scan2) == len(scan)
        want = RelocBuffers(capi, c2, scan2, step, half, k)
        torch.cuda.synchronize()
        want.one_call(g, lvl, s.cuda_stream)
        s.synchronize()
        with torch.cuda.stream(s):
            buf.centre.copy_(dev(c2))
            buf.pts.copy_(dev(scan2))
            buf.refill()
            graph.replay()
        s.synchronize()
        got, w = buf.host(), want.host()
        assert got["best_index"][0] >= 0 and not same_bits(got["best_pose"], eager["best_pose"])
        for key in got:
            assert same_bits(got[key], w[key]), (rep, key)
    del graph
    g.updateByScan(sc.build_scans[0], sc.build_poses[0])  # the capture has ended: accepted
    g.synchronize()
    g.close()


# ---- 10: refusals -----------------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing(capi, oracle_mod, small_scene):
    import ctypes as C
    import torch
    sc = small_scene
    g = gpu_for(capi, sc, make_oracle(oracle_mod, "ho", sc, build=False))
    lib = capi.load_library()
    buf = torch.full((4096,), SENTINEL, dtype=torch.float32, device="cuda:0")
    idx = torch.full((64,), 99, dtype=torch.int32, device="cuda:0")
    p, ip = buf.data_ptr(), idx.data_ptr()
    st = (C.c_float * 3)(0.1, 0.1, 0.1)
    hf = (C.c_int * 3)(1, 1, 1)
    F3, I3 = C.c_float * 3, C.c_int * 3
    huge = I3(40000, 40000, 0)  # 80001^2 > INT_MAX
    sw = lib.hsm_score_window_device
    bad = [
        sw(g._h, 5, p, st, hf, p, 1, p, None, None), sw(g._h, -1, p, st, hf, p, 1, p, None, None),       # level
        sw(g._h, 0, p, st, I3(1, -1, 1), p, 1, p, None, None),                                             # negative half-extent
        sw(g._h, 0, p, st, huge, p, 1, p, None, None),                                                     # W > INT_MAX
        sw(g._h, 0, p, F3(0.1, float("inf"), 0.1), hf, p, 1, p, None, None),                               # non-finite step
        sw(g._h, 0, p, F3(float("nan"), 0.1, 0.1), hf, p, 1, p, None, None),
        sw(g._h, 0, p, st, hf, p, -1, p, None, None),                                                      # n < 0
        sw(g._h, 0, p, st, hf, p, 1, None, None, None),                                                    # both outputs NULL
        sw(g._h, 0, None, st, hf, p, 1, p, None, None),                                                    # NULL centre
        sw(g._h, 0, p, st, hf, None, 1, p, None, None),                                                    # NULL points, n > 0
        sw(g._h, 0, p, None, hf, p, 1, p, None, None), sw(g._h, 0, p, st, None, p, 1, p, None, None),
        lib.hsm_score_window(g._h, 0, None, st, hf, None, 0, None, None),
        lib.hsm_window_poses_device(g._h, p, st, hf, None, 28, p, None),                                   # 28 > W without indices
        lib.hsm_window_poses_device(g._h, p, st, hf, ip, -1, p, None),
        lib.hsm_window_poses_device(g._h, p, st, hf, ip, 4, None, None),
        lib.hsm_window_poses_device(g._h, None, st, hf, ip, 4, p, None),
        lib.hsm_select_topk_device(g._h, -1, p, 4, ip, p, p, 1 << 12, None),
        lib.hsm_select_topk_device(g._h, 100, p, 0, ip, p, p, 1 << 12, None),
        lib.hsm_select_topk_device(g._h, 100, p, 65, ip, p, p, 1 << 12, None),
        lib.hsm_select_topk_device(g._h, 100, None, 4, ip, p, p, 1 << 12, None),
        lib.hsm_select_topk_device(g._h, 100, p, 4, None, p, p, 1 << 12, None),
        lib.hsm_select_topk_device(g._h, 100, p, 4, ip, p, None, 1 << 12, None),
        lib.hsm_select_topk_device(g._h, 100, p, 4, ip, p, p, lib.hsm_select_topk_workspace(100, 4) - 1, None),
    ]
    rl = lib.hsm_relocalize_device
    need = lib.hsm_relocalize_workspace(27, 4)
    ok = dict(level=0, c=p, st=st, hf=hf, k=4, pts=p, n=1, ws=p + 8192, wsb=need, cand=p, cov=None, lh=p, bp=p, bs=None, bi=ip)
    for change in (dict(level=3), dict(c=None), dict(hf=I3(-1, 0, 0)), dict(hf=huge), dict(st=F3(0.1, 0.1, float("-inf"))),
                   dict(k=0), dict(k=65), dict(pts=None), dict(n=-1), dict(ws=None), dict(wsb=need - 1), dict(ws=p + 8196),
                   dict(cand=None), dict(lh=None), dict(bp=None), dict(bi=None)):
        a = dict(ok, **change)
        bad.append(rl(g._h, a["level"], a["c"], a["st"], a["hf"], a["k"], a["pts"], a["n"], a["ws"], a["wsb"], a["cand"], a["cov"],
                      a["lh"], a["bp"], a["bs"], a["bi"], None))
    assert bad and all(rc == HSM_ERR_INVALID for rc in bad), bad
    assert lib.hsm_window_poses_device(g._h, p, st, hf, ip, 0, None, None) == 0  # count == 0
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all() and (idx == 99).all()
    g.close()
