"""hsm_score_windows_batch_device / hsm_select_topk_groups_device / hsm_relocalize_batch* on the MI355X.

What holds the batched entries is what already holds the single ones (tests/test_gpu_window.py): window b of a batch carries
the bits hsm_score_window_device gives for centre b and scan b in BOTH kernel forms and both layouts, and one window per shape
the CPU reference's bits; every group of the grouped top-K follows tests/topk_rule.py (and, for K = 1, tests/select_rule.py) and
equals hsm_select_topk_device on that group; the batched relocalisation equals one hsm_relocalize_device call per scan.  Every
output buffer is filled with a sentinel before a launch so that a row no launch wrote shows.

The relocalisation in HSM_PARITY_FAST: the matcher's tree sums depend on the width of the team of wavefronts a launch gives a
scan, which the plan takes from the number of pairs and the scan length (csrc/match_plan.h, choose_wps).  The three scans here
are 1081, 1000 and 900 beams: K = 8 pairs of each, and the 24 pairs of the batch with their mean length of 994, all plan four
wavefronts per scan and five beams per lane, so the batch has the single calls' bits in that mode too.
"""
import ctypes as C

import numpy as np
import pytest

import select_rule
import topk_rule
import window_cases
from conftest import bits, make_oracle, oracle_kinds
from support import capi, dev, layout_of, pack, same, stream_ptr
from test_gpu_window import RelocBuffers, SENTINEL, forced, gpu_for, oracle_window, score_window

pytestmark = pytest.mark.gpu

HSM_ERR_INVALID = -1
FORMS = ("lane", "wave")
KERNEL = {"lane": b"score_windows_batch_lane_kernel", "wave": b"score_windows_batch_wave_kernel"}
LANE_MIN = 1 << 16  # kWindowBatchLaneMin of csrc/window.hip
SCAN_LENS = (1081, 67, 0, 130)
INT_MAX_9 = (2**31 - 1) // 9

_ORACLES = {}
_REFS = {}


def built_oracle(oracle_mod, kind, scene, tag):
    """one checker with the scene's map per (scene, kind), shared by the tests of this file: none of them changes it"""
    if (tag, kind) not in _ORACLES:
        _ORACLES[tag, kind] = make_oracle(oracle_mod, kind, scene)
    return _ORACLES[tag, kind]


def score_windows_batch(g, level, centres, step, half, pts, offs=None, shared_n=0, want=(True, True)):
    """hsm_score_windows_batch_device on torch buffers -> (likelihood [B, W], residual [B, W]) on the host"""
    import torch
    c = np.asarray(centres, np.float32).reshape(-1, 3)
    B, W = len(c), window_cases.window_count(half)
    d_c, d_pts = dev(c), dev(np.asarray(pts, np.float32).reshape(-1, 2))
    d_o = None if offs is None else dev(np.asarray(offs, np.int32))
    out = torch.full((2, B, W), SENTINEL, dtype=torch.float32, device="cuda:0")
    g.score_windows_batch_device(level, B, d_c.data_ptr(), step, half, d_pts.data_ptr() if len(pts) else 0,
                                 0 if d_o is None else d_o.data_ptr(), shared_n, out[0].data_ptr() if want[0] else 0,
                                 out[1].data_ptr() if want[1] else 0, stream_ptr())
    r = out.cpu().numpy()
    return r[0], r[1]


# ---- 1: the scores ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("layout", ["quad", "plane"])
def test_batched_window_scores_are_the_single_calls_bits(capi, oracle_mod, pyramid_scene, monkeypatch, layout, form):
    sc = pyramid_scene
    refs = {kind: built_oracle(oracle_mod, kind, sc, "pyramid") for kind in oracle_kinds()}
    forced(monkeypatch, form)
    g = gpu_for(capi, sc, refs[oracle_kinds()[-1]], layout=layout_of(capi, layout))
    lib = capi.load_library()
    scans = [sc.query_scans[q][:n] for q, n in enumerate(SCAN_LENS)]
    pts, offs = pack(scans)
    centres = np.stack([sc.query_truth[q] for q in range(4)]).astype(np.float32) + np.float32([0.03, -0.02, 0.01])
    centres[1, 2] = np.inf  # one centre that is not finite: its scores are whatever the single call gives
    for lvl in range(sc.levels):
        for half in window_cases.WINDOWS:
            got = score_windows_batch(g, lvl, centres, window_cases.STEP, half, pts, offs)
            assert lib.hsm_last_launch_kernel(g._h) == KERNEL[form] and lib.hsm_last_launch_parity(g._h) == capi.PARITY_EXACT
            what = f"{layout} {form} level {lvl} window {half}"
            for b in range(4):
                one = score_window(g, lvl, centres[b], window_cases.STEP, half, scans[b])
                assert not (got[0][b] == SENTINEL).any() and not (got[1][b] == SENTINEL).any(), f"{what}: rows never written"
                assert same(got[0][b], one[0]) and same(got[1][b], one[1]), (what, b)
            assert np.isnan(got[0][2]).all() and (bits(got[1][2]) == 0).all(), what  # the empty scan: NaN and +0
            for kind, o in refs.items():  # window 0, 1081 beams, against the reference
                if (kind, lvl, half) not in _REFS:  # computed once, shared by the layouts and forms
                    _REFS[kind, lvl, half] = oracle_window(o, lvl, window_cases.window_poses(centres[0], window_cases.STEP, half), scans[0])
                rlh, rres = _REFS[kind, lvl, half]
                assert same(got[0][0], rlh) and same(got[1][0], rres), (what, kind)
    # either output alone; and one shared scan is a CSR batch of copies of it
    half = window_cases.WINDOWS[0]
    both = score_windows_batch(g, 1, centres, window_cases.STEP, half, pts, offs)
    only_lh, untouched = score_windows_batch(g, 1, centres, window_cases.STEP, half, pts, offs, want=(True, False))
    assert same(only_lh, both[0]) and (untouched == SENTINEL).all()
    untouched, only_res = score_windows_batch(g, 1, centres, window_cases.STEP, half, pts, offs, want=(False, True))
    assert same(only_res, both[1]) and (untouched == SENTINEL).all()
    for n in (200, 0):
        cpts, coffs = pack([scans[0][:n]] * 4)
        shared = score_windows_batch(g, 1, centres, window_cases.STEP, half, scans[0][:n], None, n)
        copies = score_windows_batch(g, 1, centres, window_cases.STEP, half, cpts, coffs)
        assert same(shared[0], copies[0]) and same(shared[1], copies[1]), n
    if form == "wave" and layout == "quad":  # the wrapper that takes host arrays
        lh, res = g.score_windows_batch(1, centres, window_cases.STEP, half, pts, offs)
        assert same(lh, both[0]) and same(res, both[1])
    g.close()


def test_default_form_follows_batch_times_window(capi, oracle_mod, small_scene, monkeypatch):
    """1 089 hypotheses a window: 60 windows stay below the threshold (a wavefront per hypothesis), 61 reach it (a lane per
    hypothesis); the windows both launches share have the same bits"""
    sc = small_scene
    forced(monkeypatch, None)
    g = gpu_for(capi, sc, built_oracle(oracle_mod, "ho", sc, "small"))
    lib = capi.load_library()
    half, step = (16, 16, 0), (0.05, 0.05, 0.02)
    W = window_cases.window_count(half)
    below, at = (LANE_MIN - 1) // W, (LANE_MIN + W - 1) // W
    assert W == 1089 and below * W < LANE_MIN <= at * W and at == below + 1
    pts = sc.query_scans[0][:65]
    rng = np.random.default_rng(5)
    centres = (sc.query_truth[0].astype(np.float32) + rng.uniform(-0.5, 0.5, (at, 3)).astype(np.float32)).astype(np.float32)
    lo = score_windows_batch(g, 0, centres[:below], step, half, pts, None, len(pts))
    assert lib.hsm_last_launch_kernel(g._h) == KERNEL["wave"]
    hi = score_windows_batch(g, 0, centres, step, half, pts, None, len(pts))
    assert lib.hsm_last_launch_kernel(g._h) == KERNEL["lane"]
    assert same(hi[0][:below], lo[0]) and same(hi[1][:below], lo[1])
    assert not (hi[1] == SENTINEL).any() and np.unique(hi[1]).size > 1000
    g.close()


# ---- 2: the grouped top-K ---------------------------------------------------------------------------------------------------
def topk_groups_scores(size, k):
    """six groups of `size` scores: 16 values (ties), all NaN, three valid scores at the most (fewer than k from k = 8 on),
    signed zeros alone, NaNs sprinkled over distinct values, one value everywhere"""
    rng = np.random.default_rng(1000 + size)
    nan = np.float32(np.nan)
    s = np.empty((6, size), np.float32)
    s[0] = rng.integers(0, 16, size).astype(np.float32) / np.float32(16)
    s[1] = nan
    s[2] = nan
    s[2, rng.permutation(size)[:3]] = np.float32([0.25, 0.75, 0.25])[:min(size, 3)]
    s[3] = np.where(rng.integers(0, 2, size) == 0, np.float32(0.0), np.float32(-0.0))
    s[4] = rng.permutation(size).astype(np.float32)
    s[4, rng.random(size) < 0.3] = nan
    s[5] = np.float32(0.5)
    return s


@pytest.mark.parametrize("size", [1, 63, 65, 16385])
def test_grouped_topk_follows_the_rule_in_every_group(capi, oracle_mod, small_scene, size):
    import torch
    g = gpu_for(capi, small_scene, make_oracle(oracle_mod, "ho", small_scene, build=False))
    M = capi.MapRepMultiMap
    for k in (1, 8, 64):
        s = topk_groups_scores(size, k)
        G = len(s)
        nbytes = M.select_topk_groups_workspace(G, size, k)
        assert nbytes > 0 and nbytes % 8 == 0
        garbage = np.random.default_rng(size + k).integers(0, 2**32, nbytes // 4 + 16, dtype=np.uint32)
        ws = dev(garbage.view(np.int32))
        d_s = dev(s)
        idx = torch.full((G, k), 99, dtype=torch.int32, device="cuda:0")
        best = torch.full((G, k), SENTINEL, dtype=torch.float32, device="cuda:0")
        g.select_topk_groups_device(G, size, d_s.data_ptr(), k, idx.data_ptr(), best.data_ptr(), ws.data_ptr(), nbytes, stream_ptr())
        assert np.array_equal(ws.cpu().numpy().view(np.uint32)[nbytes // 4:], garbage[nbytes // 4:]), "wrote behind the workspace"
        idx, best = idx.cpu().numpy(), best.cpu().numpy()
        # the single entry on every group, with a workspace of its own
        one_bytes = M.select_topk_workspace(size, k)
        assert M.select_topk_groups_workspace(1, size, k) == one_bytes
        ws1 = torch.zeros(one_bytes // 4, dtype=torch.int32, device="cuda:0")
        idx1 = torch.full((k,), 99, dtype=torch.int32, device="cuda:0")
        best1 = torch.full((k,), SENTINEL, dtype=torch.float32, device="cuda:0")
        for grp in range(G):
            want_idx, want_best = topk_rule.topk(s[grp], k)
            none = want_idx < 0
            assert np.array_equal(idx[grp], want_idx), (size, k, grp, idx[grp][:10], want_idx[:10])
            assert np.isnan(best[grp][none]).all() and same(best[grp][~none], want_best[~none]), (size, k, grp)
            g.select_topk_device(size, d_s[grp].data_ptr(), k, idx1.data_ptr(), best1.data_ptr(), ws1.data_ptr(), one_bytes, stream_ptr())
            assert np.array_equal(idx1.cpu().numpy(), idx[grp]) and same(best1.cpu().numpy(), best[grp]), (size, k, grp)
        if k == 1:
            win, win_score = select_rule.select_best(s.reshape(-1), groups=G, group_size=size)
            rel = np.where(win >= 0, win - np.arange(G) * size, -1)
            assert np.array_equal(idx[:, 0], rel), (size, rel, idx[:, 0])
            assert same(best[win >= 0, 0], win_score[win >= 0])
        # without the scores; and one group through the grouped entry is the single entry
        idx2 = torch.full((G, k), 99, dtype=torch.int32, device="cuda:0")
        g.select_topk_groups_device(G, size, d_s.data_ptr(), k, idx2.data_ptr(), 0, ws.data_ptr(), nbytes, stream_ptr())
        assert np.array_equal(idx2.cpu().numpy(), idx)
        g.select_topk_groups_device(1, size, d_s[0].data_ptr(), k, idx1.data_ptr(), best1.data_ptr(), ws1.data_ptr(), one_bytes,
                                    stream_ptr())
        assert np.array_equal(idx1.cpu().numpy(), idx[0]) and same(best1.cpu().numpy(), best[0])
    g.close()


# ---- 3: the relocalisation --------------------------------------------------------------------------------------------------
class BatchBuffers:
    """the device arrays of one hsm_relocalize_batch_device call; `scans` None: the one scan `shared` for every centre"""

    def __init__(self, capi, centres, scans, step, half, k, shared=None):
        import torch
        c = np.asarray(centres, np.float32).reshape(-1, 3)
        self.B, self.step, self.half, self.k = len(c), step, half, k
        self.W = window_cases.window_count(half)
        self.centres = dev(c)
        if scans is None:
            p, self.total, self.shared_n, self.offs = np.asarray(shared, np.float32).reshape(-1, 2), 0, len(shared), None
        else:
            p, o = pack(scans)
            self.total, self.shared_n, self.offs = int(o[-1]), 0, dev(o)
        self.n_pts = len(p)
        self.pts = dev(p) if len(p) else torch.zeros((1, 2), dtype=torch.float32, device="cuda:0")
        f = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float32, device="cuda:0")  # noqa: E731
        i = lambda *shape: torch.full(shape, 99, dtype=torch.int32, device="cuda:0")  # noqa: E731
        B = self.B
        self.cand, self.cov, self.lh0, self.cand_index = f(B, k, 3), f(B, k, 9), f(B, k), i(B, k)
        self.best_pose, self.best_score, self.best_index = f(B, 3), f(B), i(B)
        self.ws_bytes = capi.MapRepMultiMap.relocalize_batch_workspace(B, self.W, k, self.total)
        assert self.ws_bytes > 0 and self.ws_bytes % 8 == 0
        self.guard = 64
        self.ws = torch.full((self.ws_bytes // 4 + self.guard,), -1, dtype=torch.int32, device="cuda:0")

    KEYS = ("cand", "cov", "lh0", "cand_index", "best_pose", "best_score", "best_index")

    def call(self, g, level, s):
        g.relocalize_batch_device(level, self.B, self.centres.data_ptr(), self.step, self.half, self.k,
                                  self.pts.data_ptr() if self.n_pts else 0, 0 if self.offs is None else self.offs.data_ptr(),
                                  self.shared_n, self.total, self.ws.data_ptr(), self.ws_bytes, self.cand.data_ptr(),
                                  self.cov.data_ptr(), self.lh0.data_ptr(), self.cand_index.data_ptr(), self.best_pose.data_ptr(),
                                  self.best_score.data_ptr(), self.best_index.data_ptr(), s)

    def host(self):
        assert (self.ws[self.ws_bytes // 4:] == -1).all(), "wrote behind the workspace"
        return {k: getattr(self, k).cpu().numpy() for k in self.KEYS}

    def refill(self):
        for t in (self.cand, self.cov, self.lh0, self.best_pose, self.best_score):
            t.fill_(SENTINEL)
        self.cand_index.fill_(99)
        self.best_index.fill_(99)


def single_calls(capi, g, level, centres, scans, step, half, k, s):
    """one hsm_relocalize_device call per scan -> the batch's outputs stacked (cand_index: score + top-K on their own)"""
    import torch
    out = {key: [] for key in BatchBuffers.KEYS}
    for c, scan in zip(centres, scans):
        b = RelocBuffers(capi, c, scan, step, half, k)
        torch.cuda.synchronize()
        b.one_call(g, level, s)
        g.score_window_device(level, b.centre.data_ptr(), step, half, b.pts_ptr(), b.n, b.scores.data_ptr(), 0, s)
        g.select_topk_device(b.W, b.scores.data_ptr(), k, b.kidx.data_ptr(), b.kscore.data_ptr(), b.topk_ws.data_ptr(), b.topk_bytes, s)
        torch.cuda.synchronize()
        r = b.host()
        for key in ("cand", "cov", "lh0", "best_pose"):
            out[key].append(r[key])
        out["best_score"].append(r["best_score"][0])
        out["best_index"].append(r["best_index"][0])
        out["cand_index"].append(b.kidx.cpu().numpy())
    return {key: np.stack(v) for key, v in out.items()}


def assert_same_outputs(got, want, what):
    for key in BatchBuffers.KEYS:
        if got[key].dtype == np.float32:
            assert same(got[key], want[key]), (what, key)
        else:
            assert np.array_equal(got[key], want[key]), (what, key, got[key], want[key])


def reloc_batch_case(sc):
    """three scans of the pyramid scene in their windows: the committed case, and two other queries truncated to 1000 and 900
    beams whose centres lie off their truths"""
    truth, centre, scan = window_cases.reloc_case(sc)
    scans = [scan, sc.query_scans[5][:1000], sc.query_scans[7][:900]]
    centres = np.stack([centre, sc.query_truth[5] + np.float32([0.8, -0.6, -0.4]), sc.query_truth[7] + np.float32([-0.6, 0.4, 0.3])])
    return truth, centres.astype(np.float32), scans


@pytest.mark.parametrize("mode", ["default", "fast"])
def test_relocalize_batch_equals_one_call_per_scan(capi, oracle_mod, pyramid_scene, mode):
    import torch
    sc = pyramid_scene
    g = gpu_for(capi, sc, built_oracle(oracle_mod, oracle_kinds()[-1], sc, "pyramid"))
    if mode == "fast":
        g.set_parity(capi.PARITY_FAST)
    truth, centres, scans = reloc_batch_case(sc)
    step, half, k, lvl = window_cases.RELOC_STEP, window_cases.RELOC_HALF, window_cases.RELOC_K, sc.levels - 1
    s = torch.cuda.Stream()
    b = BatchBuffers(capi, centres, scans, step, half, k)
    torch.cuda.synchronize()
    b.call(g, lvl, s.cuda_stream)
    s.synchronize()
    got = b.host()
    for key in got:
        assert got[key].dtype != np.float32 or not (got[key] == SENTINEL).any(), key
    want = single_calls(capi, g, lvl, centres, scans, step, half, k, s.cuda_stream)
    assert_same_outputs(got, want, mode)
    # the committed case ends where the reference composition does (tests/test_window_model.py)
    d = np.hypot(*(got["best_pose"][0, :2] - truth[:2]))
    a = abs((got["best_pose"][0, 2] - truth[2] + np.pi) % (2 * np.pi) - np.pi)
    assert d <= sc.resolution and a <= 0.02, (d, a)
    assert (got["best_index"] >= 0).all() and all(got["best_index"][i] in got["cand_index"][i] for i in range(3))
    if mode == "default":
        # the host entry
        pts, offs = pack(scans)
        h = g.relocalize_batch(lvl, centres, step, half, k, pts, offs)
        for key, hk in (("cand", "cand_pose"), ("cov", "cand_cov"), ("lh0", "cand_likelihood"), ("cand_index", "cand_index"),
                        ("best_pose", "best_pose"), ("best_score", "best_score"), ("best_index", "best_index")):
            assert same(h[hk], got[key]) if got[key].dtype == np.float32 else np.array_equal(h[hk], got[key]), key
        # one shared scan at two centres, nothing copied
        sh = BatchBuffers(capi, centres[:2], None, step, half, k, shared=scans[0])
        torch.cuda.synchronize()
        sh.call(g, lvl, s.cuda_stream)
        s.synchronize()
        assert_same_outputs(sh.host(), single_calls(capi, g, lvl, centres[:2], [scans[0]] * 2, step, half, k, s.cuda_stream), "shared")
        hs = g.relocalize_batch(lvl, centres[:2], step, half, k, scans[0])
        assert same(hs["cand_pose"], sh.host()["cand"]) and np.array_equal(hs["best_index"], sh.host()["best_index"])
    g.close()


def test_a_scan_without_scores_has_no_winner_and_disturbs_nobody(capi, oracle_mod, pyramid_scene):
    """the middle scan is empty: every score of its window is NaN, its index -1, its best pose left as it was; its neighbours
    have the bits of a call of their own.  A window of three poses and k = 8: five unfilled places per scan"""
    import torch
    sc = pyramid_scene
    g = gpu_for(capi, sc, built_oracle(oracle_mod, oracle_kinds()[-1], sc, "pyramid"))
    truth, centres, scans = reloc_batch_case(sc)
    scans = [scans[0], scans[1][:0], scans[2]]
    for step, half, k, lvl in ((window_cases.RELOC_STEP, window_cases.RELOC_HALF, window_cases.RELOC_K, sc.levels - 1),
                               ((0.05, 0.05, 0.01), (1, 0, 0), 8, 0)):
        b = BatchBuffers(capi, centres, scans, step, half, k)
        torch.cuda.synchronize()
        b.call(g, lvl, stream_ptr())
        torch.cuda.synchronize()
        got = b.host()
        assert got["best_index"][1] == -1 and np.isnan(got["best_score"][1]) and (got["best_pose"][1] == SENTINEL).all()
        assert (got["cand_index"][1] == -1).all() and np.isnan(got["lh0"][1]).all()
        want = single_calls(capi, g, lvl, centres[[0, 2]], [scans[0], scans[2]], step, half, k, stream_ptr())
        for key in BatchBuffers.KEYS:
            a, w = got[key][[0, 2]], want[key]
            if a.dtype == np.float32:
                assert ((bits(a) == bits(w)) | (np.isnan(a) & np.isnan(w))).all(), (half, key)  # (unfilled places: NaN rows)
            else:
                assert np.array_equal(a, w), (half, key)
        assert (got["best_index"][[0, 2]] >= 0).all()
    g.close()


def test_relocalize_batch_captured_in_a_graph_and_replayed(capi, oracle_mod, pyramid_scene):
    import torch
    sc = pyramid_scene
    g = gpu_for(capi, sc, built_oracle(oracle_mod, oracle_kinds()[-1], sc, "pyramid"))
    _, centres, scans = reloc_batch_case(sc)
    step, half, k, lvl = window_cases.RELOC_STEP, window_cases.RELOC_HALF, window_cases.RELOC_K, sc.levels - 1
    s = torch.cuda.Stream()
    buf = BatchBuffers(capi, centres, scans, step, half, k)
    torch.cuda.synchronize()
    buf.call(g, lvl, s.cuda_stream)  # eager first: nothing is allocated under capture
    s.synchronize()
    eager = buf.host()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        buf.call(g, lvl, s.cuda_stream)
    with torch.cuda.stream(s):
        buf.refill()
        graph.replay()
    s.synchronize()
    assert_same_outputs(buf.host(), eager, "replay")
    # new centres in the same buffers: every scan is now searched around another scan's place
    c2 = (centres[[1, 2, 0]] + np.float32([[0.2, 0.2, -0.1], [-0.4, 0.2, 0.1], [0.2, -0.4, 0.05]])).astype(np.float32)
    want = BatchBuffers(capi, c2, scans, step, half, k)
    torch.cuda.synchronize()
    want.call(g, lvl, s.cuda_stream)
    s.synchronize()
    with torch.cuda.stream(s):
        buf.centres.copy_(dev(c2))
        buf.refill()
        graph.replay()
    s.synchronize()
    got = buf.host()
    assert not same(got["cand"], eager["cand"])
    assert_same_outputs(got, want.host(), "replay with new centres")
    del graph
    g.close()


def test_relocalize_batch_is_ordered_behind_queued_updates(capi, oracle_mod, pyramid_scene):
    """updates queued on the context, then the batch on a caller's stream with no host wait: what the same call gives once
    everything has been waited for, and not what it gave before the updates"""
    import torch
    from hector_slam_amd import synth
    sc = pyramid_scene
    g = gpu_for(capi, sc, built_oracle(oracle_mod, oracle_kinds()[-1], sc, "pyramid"), stamps=False)
    rng = np.random.default_rng(8)
    sfac = float(np.float32(1.0) / np.float32(sc.resolution))
    dense = [synth.make_scan(sc.world, sc.build_poses[t], 16384, sfac, rng) for t in range(3)]
    _, centres, scans = reloc_batch_case(sc)
    step, half, k, lvl = window_cases.RELOC_STEP, (3, 3, 2), window_cases.RELOC_K, sc.levels - 1
    s = torch.cuda.Stream()
    before, behind, after = (BatchBuffers(capi, centres, scans, step, half, k) for _ in range(3))
    torch.cuda.synchronize()
    before.call(g, lvl, s.cuda_stream)
    s.synchronize()
    for t in range(3):
        g.updateByScan(dense[t], sc.build_poses[t])  # queued, not waited for
    behind.call(g, lvl, s.cuda_stream)
    s.synchronize()
    g.synchronize()
    after.call(g, lvl, s.cuda_stream)
    s.synchronize()
    assert_same_outputs(behind.host(), after.host(), "behind the updates")
    assert not same(before.host()["lh0"], after.host()["lh0"])  # the updates do change these scores
    g.close()


def test_refusals_launch_nothing(capi, oracle_mod, small_scene):
    import torch
    sc = small_scene
    g = gpu_for(capi, sc, make_oracle(oracle_mod, "ho", sc, build=False))
    lib = capi.load_library()
    buf = torch.full((1 << 16,), SENTINEL, dtype=torch.float32, device="cuda:0")
    idx = torch.full((256,), 99, dtype=torch.int32, device="cuda:0")
    offs = dev(np.array([0, 1, 2], np.int32))
    p, ip, op = buf.data_ptr(), idx.data_ptr(), offs.data_ptr()
    F3, I3 = C.c_float * 3, C.c_int * 3
    st, hf = F3(0.1, 0.1, 0.1), I3(1, 1, 1)
    huge = I3(40000, 40000, 0)  # 80001^2 > INT_MAX
    wide = I3(16383, 0, 0)      # 32767 hypotheses: 65540 windows of them are more than INT_MAX
    bad = []
    ok = dict(level=0, B=2, c=p, st=st, hf=hf, pts=p, offs=op, n=0, lh=p, res=None)
    for change in (dict(level=1), dict(level=-1), dict(B=-1), dict(c=None), dict(st=None), dict(hf=None), dict(hf=I3(0, -1, 0)),
                   dict(hf=huge), dict(hf=wide, B=65540), dict(st=F3(0.1, float("nan"), 0.1)), dict(lh=None),
                   dict(offs=None, n=-1), dict(offs=None, n=4, pts=None)):
        a = dict(ok, **change)
        bad.append(lib.hsm_score_windows_batch_device(g._h, a["level"], a["B"], a["c"], a["st"], a["hf"], a["pts"], a["offs"], a["n"],
                                                      a["lh"], a["res"], None))
    need = lib.hsm_select_topk_groups_workspace(3, 100, 4)
    ok = dict(G=3, size=100, s=p, k=4, idx=ip, ws=p + 8192, wsb=need)
    for change in (dict(G=-1), dict(size=-1), dict(k=0), dict(k=65), dict(s=None), dict(idx=None), dict(ws=None), dict(wsb=need - 1),
                   dict(ws=p + 8194), dict(G=3, size=2**30), dict(G=2**26, k=64, size=1)):
        a = dict(ok, **change)
        bad.append(lib.hsm_select_topk_groups_device(g._h, a["G"], a["size"], a["s"], a["k"], a["idx"], None, a["ws"], a["wsb"], None))
    need = lib.hsm_relocalize_batch_workspace(2, 27, 4, 2)
    ok = dict(level=0, B=2, c=p, st=st, hf=hf, k=4, pts=p, offs=op, n=0, total=2, ws=p + 8192, wsb=need, cand=p, cov=None, lh=p,
              ci=None, bp=p, bs=None, bi=ip)
    for change in (dict(level=3), dict(B=-1), dict(c=None), dict(hf=I3(-1, 0, 0)), dict(hf=huge), dict(hf=wide, B=65540),
                   dict(st=F3(0.1, 0.1, float("-inf"))), dict(k=0), dict(k=65), dict(offs=None, n=-1), dict(offs=None, n=4, pts=None),
                   dict(total=-1), dict(total=2**29), dict(ws=None), dict(wsb=need - 1), dict(ws=p + 8196), dict(cand=None),
                   dict(lh=None), dict(bp=None), dict(bi=None), dict(B=INT_MAX_9 // 4 + 1, hf=I3(0, 0, 0))):
        a = dict(ok, **change)
        bad.append(lib.hsm_relocalize_batch_device(g._h, a["level"], a["B"], a["c"], a["st"], a["hf"], a["k"], a["pts"], a["offs"],
                                                   a["n"], a["total"], a["ws"], a["wsb"], a["cand"], a["cov"], a["lh"], a["ci"],
                                                   a["bp"], a["bs"], a["bi"], None))
    host = np.zeros(64, np.float32)
    hidx = np.zeros(8, np.int32)
    hp, hip_ = host.ctypes.data, hidx.ctypes.data
    down = np.array([0, 2, 1], np.int32)
    for B, c, offs_h, cand in ((-1, hp, None, hp), (2, None, None, hp), (2, hp, down.ctypes.data, hp), (2, hp, None, None)):
        bad.append(lib.hsm_relocalize_batch(g._h, 0, B, c, st, hf, 4, hp, offs_h, 1, cand, None, hp, None, hp, None, hip_))
    assert bad and all(rc == HSM_ERR_INVALID for rc in bad), bad
    # nothing to do is not an error
    assert lib.hsm_score_windows_batch_device(g._h, 0, 0, None, st, hf, None, None, 0, p, None, None) == 0
    assert lib.hsm_select_topk_groups_device(g._h, 0, 100, None, 4, None, None, None, 0, None) == 0
    assert lib.hsm_relocalize_batch_device(g._h, 0, 0, None, st, hf, 4, None, None, 0, 0, p + 8192, 1 << 12, p, None, p, None, p, None,
                                           ip, None) == 0
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all() and (idx == 99).all() and not host.any() and not hidx.any()
    g.close()

