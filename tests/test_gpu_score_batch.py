"""hsm_score_batch_device / hsm_select_best_device / hsm_match_score_batch* on the MI355X.

Default mode: likelihood and residual of every hypothesis carry the CPU reference's bits
(`o.likelihood_states(level, o.map_coords_pose(level, pose)[None], pts * 2^-level)`); a scan of 0 beams gives NaN in both (the sign
and payload of an invalid operation's NaN are the processor's choice -- x86 produces 0xffc00000 -- so NaN rows are compared as
NaN, every other row bit for bit) and residual +0.  Winners are the numpy rule of tests/select_rule.py.  Every output buffer
is filled with a sentinel before a launch so that a row no launch wrote shows.
"""
import numpy as np
import pytest

import select_rule
from conftest import bits, make_oracle, oracle_kinds
from support import capi, dev, layout_of, pack, stream_ptr
from test_score_batch_abi import selection_cases, wide_start_hypotheses

pytestmark = pytest.mark.gpu

HSM_ERR_INVALID = -1
SENTINEL = -777.0
LENS = (0, 1, 63, 64, 65, 700, 1081)
FAR_MAP = np.array([[-50.0, 3.0, 0.1], [1e6, 1e6, 0.0]], np.float32)  # (almost) every beam leaves the map


def gpu_for(capi, sc, o, sx=None, sy=None, stamps=True, **kw):
    """a context holding the oracle's map; stamps=False: the log-odds only, every stamp stays -1"""
    g = capi.MapRepMultiMap(sc.resolution, sx or sc.map_size, sy or sc.map_size, sc.levels, **kw)
    g.setUpdateFactorFree(0.4)
    g.setUpdateFactorOccupied(0.9)
    for lvl in range(sc.levels):
        lo, ui = o.download_level(lvl)
        g.upload_level(lvl, lo, ui if stamps else None)
    g.synchronize()
    return g


def score(g, level, poses, pts, offs=None, stream=None, want=(True, True)):
    """hsm_score_batch_device on torch buffers -> (likelihood, residual) on the host"""
    import torch
    B = len(poses)
    s = stream or torch.cuda.current_stream()
    with torch.cuda.stream(s):
        d_p, d_pts = dev(np.asarray(poses, np.float32).reshape(-1, 3)), dev(np.asarray(pts, np.float32).reshape(-1, 2))
        d_offs = None if offs is None else dev(np.asarray(offs, np.int32))
        out = torch.full((2, max(B, 1)), SENTINEL, dtype=torch.float32, device="cuda:0")
        g.score_batch_device(level, B, d_p.data_ptr(), d_pts.data_ptr() if len(pts) else 0,
                             0 if d_offs is None else d_offs.data_ptr(), len(pts) if d_offs is None else 0,
                             out[0].data_ptr() if want[0] else 0, out[1].data_ptr() if want[1] else 0, s.cuda_stream)
        r = out.cpu().numpy()
    return r[0, :B], r[1, :B]


def reference(o, level, poses, scans):
    """per hypothesis: the reference's likelihood and residual at getMapCoordsPose(pose) with the level-scaled container"""
    f = np.float32(1.0 / 2 ** level)
    lh, res = np.empty(len(poses), np.float32), np.empty(len(poses), np.float32)
    for b, (p, s) in enumerate(zip(poses, scans)):
        pm = o.map_coords_pose(level, p)[None]
        pl = np.asarray(s, np.float32).reshape(-1, 2) * f
        lh[b] = o.likelihood_states(level, pm, pl)[0]
        res[b] = o.residual_states(level, pm, pl)[0]
    return lh, res


def assert_scores(what, got, ref, lens):
    """every row: the reference's bits; NaN likelihood exactly where the scan is empty (and residual +0 there)"""
    lens = np.asarray(lens)
    (lh, res), (rlh, rres) = got, ref
    assert not (lh == SENTINEL).any() and not (res == SENTINEL).any(), f"{what}: rows never written"
    empty = lens == 0
    assert np.array_equal(np.isnan(lh), empty) and np.array_equal(np.isnan(rlh), empty), what
    bad = (bits(lh) != bits(rlh)) & ~empty
    assert not bad.any(), f"{what}: {int(bad.sum())} of {len(lh)} likelihoods differ, first {np.flatnonzero(bad)[:5]}"
    bad = bits(res) != bits(rres)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {len(res)} residuals differ, first {np.flatnonzero(bad)[:5]}"
    assert (bits(res[empty]) == 0).all()


def hypotheses(o, sc, level, rng, lens=LENS, cloud=12):
    """(poses, scans): for every scan length the truth, a cloud around it and the two far poses"""
    poses, scans = [], []
    for k, n in enumerate(lens):
        q = k % len(sc.query_scans)
        truth = sc.query_truth[q]
        far = np.stack([o.world_coords_pose(level, m) for m in FAR_MAP])
        around = (truth[None, :] + rng.normal(0, [0.1, 0.1, 0.05], (cloud, 3))).astype(np.float32)
        for p in np.concatenate([truth[None, :], around, far]).astype(np.float32):
            poses.append(p)
            scans.append(sc.query_scans[q][:n])
    return np.stack(poses), scans


# ---- 1, 2: CSR batches and the shared scan, every level, both layouts -----------------------------------------------------------
@pytest.mark.parametrize("layout", ["quad", "plane"])
@pytest.mark.parametrize("kind", oracle_kinds())
def test_csr_batch_is_bit_identical_on_every_level(capi, oracle_mod, pyramid_scene, kind, layout):
    sc = pyramid_scene
    o = make_oracle(oracle_mod, kind, sc)
    g = gpu_for(capi, sc, o, layout=layout_of(capi, layout))
    rng = np.random.default_rng(17)
    for lvl in range(sc.levels):
        poses, scans = hypotheses(o, sc, lvl, rng)
        pts, offs = pack(scans)
        got = score(g, lvl, poses, pts, offs)
        assert g.last_launch_config() is not None
        assert capi.load_library().hsm_last_launch_kernel(g._h) == b"score_batch_kernel"
        assert capi.load_library().hsm_last_launch_parity(g._h) == capi.PARITY_EXACT
        assert_scores(f"level {lvl}", got, reference(o, lvl, poses, scans), [len(s) for s in scans])
        far_full = [b for b, s in enumerate(scans) if len(s) == 1081][-1]  # the (1e6, 1e6) pose: every beam outside, M = 0
        assert got[0][far_full] == 0.0 and got[1][far_full] == 1081.0
        # either output alone
        only_lh, _ = score(g, lvl, poses, pts, offs, want=(True, False))
        _, only_res = score(g, lvl, poses, pts, offs, want=(False, True))
        assert np.array_equal(bits(only_lh), bits(got[0])) and np.array_equal(bits(only_res), bits(got[1]))
    g.close()


@pytest.mark.parametrize("layout", ["quad", "plane"])
@pytest.mark.parametrize("kind", oracle_kinds())
def test_shared_scan_gives_the_csr_bits_and_the_old_entry_points_bits(capi, oracle_mod, pyramid_scene, kind, layout):
    sc = pyramid_scene
    o = make_oracle(oracle_mod, kind, sc)
    g = gpu_for(capi, sc, o, layout=layout_of(capi, layout))
    rng = np.random.default_rng(18)
    for lvl in range(sc.levels):
        for n in LENS:
            poses, _ = hypotheses(o, sc, lvl, rng, lens=(n,), cloud=40)
            pts = sc.query_scans[0][:n]
            shared = score(g, lvl, poses, pts)
            scans = [pts] * len(poses)
            assert_scores(f"shared, level {lvl}, {n} beams", shared, reference(o, lvl, poses, scans), [n] * len(poses))
            csr = score(g, lvl, poses, *pack(scans))
            pm = np.stack([g.getMapCoordsPose(lvl, p) for p in poses]).astype(np.float32)
            old = g.likelihood_states(lvl, pm, pts), g.residual_states(lvl, pm, pts)
            for other in (csr, old):
                assert np.array_equal(bits(shared[1]), bits(other[1])), (lvl, n)
                if n:
                    assert np.array_equal(bits(shared[0]), bits(other[0])), (lvl, n)
                else:
                    assert np.isnan(other[0]).all()
    lh, res = g.score_batch(0, poses, pts)  # the array methods
    want = score(g, 0, poses, pts)
    assert np.array_equal(bits(lh), bits(want[0])) and np.array_equal(bits(res), bits(want[1]))
    lh, res = g.score_batch(0, poses, *pack([pts[:700]] * len(poses)))
    want = score(g, 0, poses, pts[:700])
    assert np.array_equal(bits(lh), bits(want[0])) and np.array_equal(bits(res), bits(want[1]))
    g.close()


def test_argument_errors_launch_nothing(capi, oracle_mod, small_scene):
    import torch
    sc = small_scene
    o = make_oracle(oracle_mod, "ho", sc)
    g = gpu_for(capi, sc, o)
    lib = capi.load_library()
    buf = torch.full((64,), SENTINEL, dtype=torch.float32, device="cuda:0")
    idx = torch.full((4,), 99, dtype=torch.int32, device="cuda:0")
    p = buf.data_ptr()
    assert lib.hsm_score_batch_device(g._h, 5, 1, p, p, None, 1, p, None, None) == HSM_ERR_INVALID   # level
    assert lib.hsm_score_batch_device(g._h, -1, 1, p, p, None, 1, p, None, None) == HSM_ERR_INVALID
    assert lib.hsm_score_batch_device(g._h, 0, -1, p, p, None, 1, p, None, None) == HSM_ERR_INVALID  # batch < 0
    assert lib.hsm_score_batch_device(g._h, 0, 1, p, p, None, 1, None, None, None) == HSM_ERR_INVALID  # both outputs NULL
    assert lib.hsm_score_batch_device(g._h, 0, 1, None, p, None, 1, p, None, None) == HSM_ERR_INVALID  # poses
    assert lib.hsm_score_batch_device(g._h, 0, 1, p, None, None, 1, p, None, None) == HSM_ERR_INVALID  # points
    assert lib.hsm_score_batch_device(g._h, 0, 1, p, p, None, -1, p, None, None) == HSM_ERR_INVALID
    assert lib.hsm_score_batch_device(g._h, 0, 0, None, None, None, 0, p, None, None) == 0           # batch == 0
    assert lib.hsm_select_best_device(g._h, -1, None, 1, p, None, idx.data_ptr(), None, None, None) == HSM_ERR_INVALID
    assert lib.hsm_select_best_device(g._h, 1, None, 1, p, None, None, None, None, None) == HSM_ERR_INVALID
    assert lib.hsm_select_best_device(g._h, 1, None, 1, p, None, idx.data_ptr(), None, p, None) == HSM_ERR_INVALID  # pose out, no poses
    assert lib.hsm_select_best_device(g._h, 0, None, 1, None, None, idx.data_ptr(), None, None, None) == 0
    assert lib.hsm_match_score_batch_device(g._h, 4, p, p, None, 1, p, None, 0, None, p, 2, None, 2, idx.data_ptr(), None, None,
                                            None) == HSM_ERR_INVALID  # ranking needs the likelihoods
    assert lib.hsm_match_score_batch_device(g._h, 4, p, p, None, 1, p, None, 0, p, None, 3, None, 2, idx.data_ptr(), None, None,
                                            None) == HSM_ERR_INVALID  # 3 groups of 2 in a batch of 4
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all() and (idx == 99).all()
    g.close()


# ---- 3: full size -------------------------------------------------------------------------------------------------------------
def test_full_size_4096_hypotheses_and_a_ragged_4097_batch(capi, oracle_mod):
    """the benchmark workload's 2048^2 single-level map: 4096 hypotheses of one 1081-beam scan, 4096 distinct scans, and a ragged
    batch of 4097 scans -- every hypothesis compared"""
    from hsm_bench import common
    bp, bs, truth, init_l0, _, pts, offs = common.make_inputs(0, 4096)[:7]
    o = oracle_mod.Oracle("ho", common.RESOLUTION, common.MAP_SIZE, common.MAP_SIZE, 1)
    o.set_update_factor_free(0.4)
    o.set_update_factor_occupied(0.9)
    o.build_map(bp, bs)
    g = capi.MapRepMultiMap(common.RESOLUTION, common.MAP_SIZE, common.MAP_SIZE, 1)
    g.upload_level(0, *o.download_level(0))
    B = 4096
    scan = pts[offs[0]:offs[1]]
    pm = np.stack([o.map_coords_pose(0, p) for p in init_l0]).astype(np.float32)
    ref = o.likelihood_states(0, pm, scan), o.residual_states(0, pm, scan)
    assert_scores("4096 hypotheses of one scan", score(g, 0, init_l0, scan), ref, [len(scan)] * B)
    scans = [pts[offs[b]:offs[b + 1]] for b in range(B)]
    assert_scores("4096 distinct scans", score(g, 0, init_l0, pts, offs), reference(o, 0, init_l0, scans), np.diff(offs))
    rng = np.random.default_rng(23)
    ragged = [scans[b % B][:int(n)] for b, n in enumerate(rng.integers(0, 1082, 4097))]
    poses = np.concatenate([init_l0, truth[:1]])
    assert_scores("ragged 4097", score(g, 0, poses, *pack(ragged)), reference(o, 0, poses, ragged), [len(s) for s in ragged])
    g.close()


# ---- 4: the chain -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain_case(oracle_mod, pyramid_scene):
    """64 groups x 32 wide starts (the recipe of test_score_batch_abi, scans 0..3 sixteen times over with fresh starts), the
    reference's poses, likelihoods and winners"""
    sc = pyramid_scene
    kind = oracle_kinds()[-1]
    o = make_oracle(oracle_mod, kind, sc)
    init, scans = [], []
    for rep in range(16):
        for q, h in enumerate(wide_start_hypotheses(sc, seed=5 + rep)):
            init.append(h)
            scans += [sc.query_scans[q]] * len(h)
    init = np.concatenate(init).astype(np.float32)
    pts, offs = pack(scans)
    poses = o.match_many(init, pts, offs)
    lh, res = reference(o, 0, poses, scans)
    return dict(o=o, init=init, scans=scans, pts=pts, offs=offs, poses=poses, lh=lh, res=res,
                win=select_rule.select_best(lh, groups=64, group_size=32))


class ChainBuffers:
    def __init__(self, c, G=64):
        import torch
        B = len(c["init"])
        self.B, self.G = B, G
        self.init, self.pts, self.offs = dev(c["init"]), dev(c["pts"]), dev(c["offs"])
        f = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float32, device="cuda:0")  # noqa: E731
        self.pose, self.cov, self.lh, self.res = f(B, 3), f(B, 9), f(B), f(B)
        self.idx = torch.full((G,), 99, dtype=torch.int32, device="cuda:0")
        self.best, self.best_pose = f(G), f(G, 3)

    def three_calls(self, g, s):
        g.match_batch_device(self.B, self.init.data_ptr(), self.pts.data_ptr(), self.offs.data_ptr(), 1081, self.pose.data_ptr(),
                             self.cov.data_ptr(), s.cuda_stream)
        g.score_batch_device(0, self.B, self.pose.data_ptr(), self.pts.data_ptr(), self.offs.data_ptr(), 0, self.lh.data_ptr(),
                             self.res.data_ptr(), s.cuda_stream)
        g.select_best_device(self.G, 0, self.B // self.G, self.lh.data_ptr(), self.pose.data_ptr(), self.idx.data_ptr(),
                             self.best.data_ptr(), self.best_pose.data_ptr(), s.cuda_stream)

    def one_call(self, g, s):
        g.match_score_batch_device(self.B, self.init.data_ptr(), self.pts.data_ptr(), self.offs.data_ptr(), 1081,
                                   self.pose.data_ptr(), self.cov.data_ptr(), 0, self.lh.data_ptr(), self.res.data_ptr(), self.G, 0,
                                   self.B // self.G, self.idx.data_ptr(), self.best.data_ptr(), self.best_pose.data_ptr(),
                                   s.cuda_stream)

    def host(self):
        return {k: getattr(self, k).cpu().numpy() for k in ("pose", "cov", "lh", "res", "idx", "best", "best_pose")}


def assert_same_results(what, a, b):
    for k in a:
        assert np.array_equal(bits(a[k]) if a[k].dtype == np.float32 else a[k], bits(b[k]) if b[k].dtype == np.float32 else b[k]), (what, k)


def test_match_score_select_chain_on_one_stream(capi, pyramid_scene, chain_case):
    import torch
    c, sc = chain_case, pyramid_scene
    g = gpu_for(capi, sc, c["o"])
    s = torch.cuda.Stream()
    buf = ChainBuffers(c)
    torch.cuda.synchronize()
    buf.three_calls(g, s)  # no host wait between the three
    s.synchronize()
    r = buf.host()
    assert np.array_equal(bits(r["pose"]), bits(c["poses"]))
    assert np.array_equal(bits(r["lh"]), bits(c["lh"])) and np.array_equal(bits(r["res"]), bits(c["res"]))
    idx, best = c["win"]
    assert (idx >= 0).all() and np.array_equal(r["idx"], idx) and np.array_equal(bits(r["best"]), bits(best))
    assert np.array_equal(bits(r["best_pose"]), bits(c["poses"][idx]))
    ties = sum(np.unique(c["lh"][k * 32:(k + 1) * 32]).size < 32 for k in range(64))
    assert ties > 32  # the ranking rule is exercised: most groups hold bit-identical likelihoods
    # the one-call form, and the host form on either route (CSR staging; the shared scan through pinned memory)
    buf2 = ChainBuffers(c)
    torch.cuda.synchronize()
    buf2.one_call(g, s)
    s.synchronize()
    assert_same_results("one call", buf2.host(), r)
    h = g.match_score_batch(c["init"], c["pts"], c["offs"], score_level=0, group_size=32)
    for k, hk in (("pose", "pose"), ("cov", "cov"), ("lh", "likelihood"), ("res", "residual"), ("best", "best_score"),
                  ("best_pose", "best_pose")):
        assert np.array_equal(bits(h[hk]), bits(r[k])), hk
    assert np.array_equal(h["best_index"], r["idx"])
    goffs = np.arange(0, 2049, 32, dtype=np.int32)
    h2 = g.match_score_batch(c["init"], c["pts"], c["offs"], group_offsets=goffs)
    assert np.array_equal(h2["best_index"], r["idx"]) and np.array_equal(bits(h2["best_pose"]), bits(r["best_pose"]))
    one = slice(0, 32)  # group 0: 32 hypotheses of scan 0 -> the shared-scan route
    h3 = g.match_score_batch(c["init"][one], c["scans"][0], score_level=0, group_size=32)
    assert np.array_equal(bits(h3["pose"]), bits(r["pose"][one])) and np.array_equal(bits(h3["likelihood"]), bits(r["lh"][one]))
    assert np.array_equal(bits(h3["cov"]), bits(r["cov"][one])) and np.array_equal(bits(h3["residual"]), bits(r["res"][one]))
    assert h3["best_index"][0] == r["idx"][0] and np.array_equal(bits(h3["best_pose"][0]), bits(r["best_pose"][0]))
    g.close()


def test_host_entry_gives_the_device_entrys_bits_with_every_optional_array(capi, oracle_mod, small_scene):
    """hsm_match_batch and hsm_match_score_batch stage their arrays through one plan (stage_layout.h match_batch_stage): a CSR
    batch through device memory, hypotheses of one scan through pinned memory.  With every combination of the optional arrays
    either route gives the bits of the _device entry called on the same inputs uploaded by hand, and an in/out array the call
    must leave alone -- the covariance of the empty scan, the winner pose of a group without a finite score -- keeps the
    caller's values, as does every array of a ranking that was not asked for."""
    import itertools
    from hector_slam_amd import synth
    sc = small_scene
    g = gpu_for(capi, sc, make_oracle(oracle_mod, "ho", sc))
    lib = capi.load_library()
    rng = np.random.default_rng(31)
    B, lens = 8, (0, 1, 63, 64, 65, 181, 200, 200)
    sfac = float(np.float32(1.0) / np.float32(sc.resolution))
    scan = np.ascontiguousarray(synth.make_scan(sc.world, sc.query_truth[0], 200, sfac, rng, pad_to_full=True), np.float32)
    assert scan.shape == (200, 2)
    init = (sc.query_truth[0][None, :] + rng.uniform(-1, 1, (B, 3)) * [0.1, 0.1, 0.03]).astype(np.float32)
    routes = {"csr": pack([scan[:n] for n in lens]), "shared": (scan, None)}
    # (groups, group offsets, group size): eight groups of one -- on the CSR route the first holds the empty scan alone, whose score
    # is NaN -- and four ragged groups, the first the same and the third empty
    rankings = {"none": (0, None, 0), "group_size": (B, None, 1), "group_offsets": (4, np.array([0, 1, 4, 4, 8], np.int32), 0)}
    stream = stream_ptr()

    def fresh(G):
        f = lambda *shape: np.full(shape, SENTINEL, np.float32)  # noqa: E731
        return dict(pose=f(B, 3), cov=f(B, 9), lh=f(B), res=f(B), idx=np.full(max(G, 1), 99, np.int32), best=f(max(G, 1)),
                    best_pose=f(max(G, 1), 3))

    def run(route, scored, want, rank):
        """the host entry on numpy arrays and the _device entry on their uploads -> both sets of arrays, every one of them
        pre-filled with the sentinel and handed over only where `want` says so"""
        pts, offs = routes[route]
        G, goffs, gsize = rankings[rank]
        host, up = fresh(G), {k: dev(v) for k, v in fresh(G).items()}
        d_init, d_pts = dev(init), dev(pts)
        d_offs, d_goffs = (None if a is None else dev(a) for a in (offs, goffs))
        hp = lambda a, on=True: a.ctypes.data if on and a is not None else None  # noqa: E731
        dp = lambda t, on=True: t.data_ptr() if on and t is not None else None  # noqa: E731
        n_host, n_dev = (len(pts), len(pts)) if offs is None else (0, max(lens))  # (a CSR device call: the sizing hint)
        if not scored:
            rc = lib.hsm_match_batch(g._h, B, init.reshape(-1), hp(pts), hp(offs), n_host, host["pose"].reshape(-1),
                                     hp(host["cov"], want["cov"]))
            rd = lib.hsm_match_batch_device(g._h, B, dp(d_init), dp(d_pts), dp(d_offs), n_dev, dp(up["pose"]),
                                            dp(up["cov"], want["cov"]), stream or None)
        else:
            rc = lib.hsm_match_score_batch(g._h, B, hp(init), hp(pts), hp(offs), n_host, hp(host["pose"]), hp(host["cov"], want["cov"]),
                                           0, hp(host["lh"]), hp(host["res"], want["res"]), G, hp(goffs), gsize, hp(host["idx"]),
                                           hp(host["best"], want["best"]), hp(host["best_pose"], want["best_pose"]))
            rd = lib.hsm_match_score_batch_device(g._h, B, dp(d_init), dp(d_pts), dp(d_offs), n_dev, dp(up["pose"]),
                                                  dp(up["cov"], want["cov"]), 0, dp(up["lh"]), dp(up["res"], want["res"]), G,
                                                  dp(d_goffs), gsize, dp(up["idx"]), dp(up["best"], want["best"]),
                                                  dp(up["best_pose"], want["best_pose"]), stream or None)
        assert rc == 0 and rd == 0, (route, scored, want, rank, rc, rd, lib.hsm_last_error())
        return host, {k: v.cpu().numpy() for k, v in up.items()}

    def check(route, scored, want, rank):
        what = (route, scored, want, rank)
        G = rankings[rank][0]
        host, device = run(route, scored, want, rank)
        assert_same_results(what, host, device)
        untouched = lambda a: (a == (99 if a.dtype == np.int32 else SENTINEL)).all()  # noqa: E731
        assert not (host["pose"] == SENTINEL).any(), what
        empty_scans = [b for b, n in enumerate(lens) if n == 0] if route == "csr" else []
        for b in range(B):  # in/out: the matcher leaves an empty scan's covariance as the caller had it
            assert untouched(host["cov"][b]) == (not want["cov"] or b in empty_scans), (what, b)
        assert untouched(host["lh"]) == (not scored) and untouched(host["res"]) == (not (scored and want["res"])), what
        if not G:
            assert untouched(host["idx"]) and untouched(host["best"]) and untouched(host["best_pose"]), what
            return
        _, goffs, gsize = rankings[rank]
        want_idx, _ = select_rule.select_best(host["lh"], **(dict(groups=G, group_size=gsize) if goffs is None else dict(group_offsets=goffs)))
        assert np.array_equal(host["idx"], want_idx), what
        no_winner = want_idx < 0
        # (the cases do hold such groups: the empty scan alone, whose score is NaN, and the empty group)
        assert all(no_winner[k] for k in {"group_size": empty_scans, "group_offsets": [2] + [0] * (route == "csr")}[rank]), what
        for k in range(G):  # in/out: a group without a finite score keeps the caller's winner pose
            assert untouched(host["best_pose"][k]) == (not want["best_pose"] or no_winner[k]), (what, k)
        assert untouched(host["best"]) == (not want["best"]), what

    for route in routes:
        for cov in (True, False):
            check(route, False, dict(cov=cov, res=False, best=False, best_pose=False), "none")
        for cov, res, rank, best, best_pose in itertools.product((True, False), (True, False), rankings, (True, False), (True, False)):
            check(route, True, dict(cov=cov, res=res, best=best, best_pose=best_pose), rank)
    g.close()


# ---- 5: selection alone -----------------------------------------------------------------------------------------------------
def run_select(g, scores, poses=None, groups=None, group_size=None, group_offsets=None):
    import torch
    s = np.asarray(scores, np.float32)
    G = groups if group_offsets is None else len(group_offsets) - 1
    d_s = dev(s) if s.size else torch.zeros(1, dtype=torch.float32, device="cuda:0")
    d_offs = None if group_offsets is None else dev(np.asarray(group_offsets, np.int32))
    d_p = None if poses is None else dev(poses)
    idx = torch.full((G,), 99, dtype=torch.int32, device="cuda:0")
    best = torch.full((G,), SENTINEL, dtype=torch.float32, device="cuda:0")
    bp = torch.full((G, 3), SENTINEL, dtype=torch.float32, device="cuda:0")
    g.select_best_device(G, 0 if d_offs is None else d_offs.data_ptr(), group_size or 0, d_s.data_ptr(),
                         0 if d_p is None else d_p.data_ptr(), idx.data_ptr(), best.data_ptr(), 0 if d_p is None else bp.data_ptr(),
                         stream_ptr())
    return idx.cpu().numpy(), best.cpu().numpy(), bp.cpu().numpy()


def assert_selection(g, scores, **kw):
    s = np.asarray(scores, np.float32)
    poses = np.random.default_rng(s.size).normal(size=(max(s.size, 1), 3)).astype(np.float32)
    idx, best, bp = run_select(g, s, poses, **kw)
    want_idx, want_best = select_rule.select_best(s, **kw)
    assert np.array_equal(idx, want_idx), (idx, want_idx)
    none = want_idx < 0
    assert np.isnan(best[none]).all() and np.array_equal(bits(best[~none]), bits(want_best[~none]))
    assert np.array_equal(bits(bp), bits(select_rule.winner_poses(want_idx, poses, np.full((len(idx), 3), SENTINEL, np.float32))))
    return idx


def test_selection_kernel_follows_the_rule(capi, oracle_mod, small_scene):
    g = gpu_for(capi, small_scene, make_oracle(oracle_mod, "ho", small_scene, build=False))
    for name, scores, kw, want in selection_cases():
        assert assert_selection(g, scores, **kw).tolist() == want, name
    rng = np.random.default_rng(41)
    big = rng.uniform(0, 1, 100_000).astype(np.float32)
    big[rng.integers(0, 100_000, 500)] = np.nan
    big[[77_777, 12_345]] = 2.0  # the maximum, planted twice
    assert assert_selection(g, big, groups=1, group_size=100_000).tolist() == [12_345]
    assert assert_selection(g, big, group_offsets=[0, 100_000]).tolist() == [12_345]
    ones = rng.uniform(0, 1, 4096).astype(np.float32)
    ones[::97] = np.nan
    want = np.where(np.isnan(ones), -1, np.arange(4096))
    assert np.array_equal(assert_selection(g, ones, groups=4096, group_size=1), want)
    assert np.array_equal(assert_selection(g, ones, group_offsets=np.arange(4097)), want)
    # both launch shapes on the same ragged data: many ties, NaNs, empty groups
    many = rng.integers(0, 5, 60_000).astype(np.float32)
    many[rng.integers(0, 60_000, 3000)] = np.nan
    cuts = np.sort(rng.integers(0, 60_001, 1500))
    a = assert_selection(g, many, group_offsets=np.concatenate([[0], cuts, [60_000]]))      # >= 1024 groups: a wavefront each
    b = assert_selection(g, many, group_offsets=np.concatenate([[0], cuts[:500], [60_000]]))  # a workgroup each
    assert np.array_equal(a[:500], b[:500])
    assert_selection(g, many, groups=40, group_size=1500)
    assert_selection(g, many, groups=58, group_size=1024)
    g.close()


# ---- 6: ordering against map updates ------------------------------------------------------------------------------------------
def oracle_update(o, pose, pts):
    o.update_by_scan(pose, pts)
    o.on_map_updated()  # (as HectorSlamProcessor::update does: the probability cache of the reference is per map generation)


def test_scores_are_ordered_against_queued_updates(capi, oracle_mod, pyramid_scene):
    """an update queued on the context, then a score on a caller's stream with no host wait: the updated map's scores; a score
    queued first, then an update: the scores of the map before it"""
    import torch
    from hector_slam_amd import synth
    sc = pyramid_scene
    o = make_oracle(oracle_mod, oracle_kinds()[-1], sc)
    # The context's update counter starts at 0, the checker's has counted its build scans: the checker's stamps, restored here,
    # would lie ahead of this context's marks and freeze the cells as they do in the reference (capi.h hsm_upload_level;
    # tests/test_gpu_restored_stamps.py).  The updates below are meant to change the map: the log-odds alone, stamps of -1.
    g = gpu_for(capi, sc, o, stamps=False)
    rng = np.random.default_rng(8)
    sfac = float(np.float32(1.0) / np.float32(sc.resolution))
    dense = [synth.make_scan(sc.world, sc.build_poses[t], 16384, sfac, rng) for t in range(6)]  # long-running updates
    poses, scans = hypotheses(o, sc, 0, rng, lens=(1081, 700), cloud=100)
    pts, offs = pack(scans)
    d_p, d_pts, d_offs = dev(poses), dev(pts), dev(offs)
    s = torch.cuda.Stream()
    B = len(poses)
    outs = [torch.full((2, B), SENTINEL, dtype=torch.float32, device="cuda:0") for _ in range(3)]
    torch.cuda.synchronize()

    def launch(out):
        g.score_batch_device(0, B, d_p.data_ptr(), d_pts.data_ptr(), d_offs.data_ptr(), 0, out[0].data_ptr(), out[1].data_ptr(),
                             s.cuda_stream)
    refs = []
    for t in range(3):
        g.updateByScan(dense[t], sc.build_poses[t])  # queued, not waited for
        oracle_update(o, sc.build_poses[t], dense[t])
    launch(outs[0])                                   # behind the three updates
    refs.append(reference(o, 0, poses, scans))
    g.updateByScan(dense[3], sc.build_poses[3])       # behind the score: it must not rewrite the map under it
    oracle_update(o, sc.build_poses[3], dense[3])
    launch(outs[1])
    refs.append(reference(o, 0, poses, scans))
    launch(outs[2])                                   # score queued ...
    g.updateByScan(dense[4], sc.build_poses[4])       # ... then an update: the score sees the map before it
    g.updateByScan(dense[5], sc.build_poses[5])
    refs.append(refs[-1])
    s.synchronize()
    g.synchronize()
    lens = [len(x) for x in scans]
    for k in range(3):
        r = outs[k].cpu().numpy()
        assert_scores(f"launch {k}", (r[0], r[1]), refs[k], lens)
    assert not np.array_equal(bits(refs[0][0]), bits(refs[1][0]))  # the updates do change these scores
    for t in (4, 5):
        oracle_update(o, sc.build_poses[t], dense[t])
    # ... and no update was disturbed by the scores around it (log-odds only: the update counters of a context that received
    # its map by upload do not count from the oracle's)
    assert np.array_equal(bits(g.download_level(0)[0]), bits(o.download_level(0)[0]))
    g.close()


# ---- 7: graph capture ---------------------------------------------------------------------------------------------------------
def test_chain_captured_in_a_graph_and_replayed_with_new_starts(capi, pyramid_scene, chain_case):
    import torch
    c, sc = chain_case, pyramid_scene
    g = gpu_for(capi, sc, c["o"])
    s = torch.cuda.Stream()
    buf = ChainBuffers(c)
    torch.cuda.synchronize()
    buf.three_calls(g, s)  # eager first: nothing is allocated under capture
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    idx0 = g.getUpdateIndex(0)
    with torch.cuda.graph(graph, stream=s):
        buf.three_calls(g, s)
        with pytest.raises(capi.HsmError) as e:
            g.updateByScan(sc.build_scans[0], sc.build_poses[0])
        assert f"({HSM_ERR_INVALID})" in str(e.value) and "captur" in str(e.value), str(e.value)
    assert g.getUpdateIndex(0) == idx0
    B = buf.B
    rng = np.random.default_rng(77)
    for rep in range(3):
        init = np.roll(c["init"], 7 * (rep + 1), axis=0) + rng.uniform(-0.02, 0.02, (B, 3)).astype(np.float32)
        want = ChainBuffers(dict(c, init=init))
        torch.cuda.synchronize()
        want.one_call(g, s)  # eager, buffers of its own
        s.synchronize()
        with torch.cuda.stream(s):
            buf.init.copy_(dev(init))
            for t in (buf.pose, buf.cov, buf.lh, buf.res, buf.best, buf.best_pose):
                t.fill_(SENTINEL)
            buf.idx.fill_(99)
            graph.replay()
        s.synchronize()
        got = buf.host()
        assert not (got["lh"] == SENTINEL).any() and not (got["idx"] == 99).any()
        assert_same_results(f"replay {rep}", got, want.host())
    del graph
    g.updateByScan(sc.build_scans[0], sc.build_poses[0])  # the capture has ended: accepted
    g.synchronize()
    g.close()


# ---- 8: the opt-in tree summation -----------------------------------------------------------------------------------------------
def test_fast_mode_within_the_old_kernels_bars(capi, oracle_mod, pyramid_scene):
    import torch
    sc = pyramid_scene
    o = make_oracle(oracle_mod, oracle_kinds()[-1], sc)
    g = gpu_for(capi, sc, o)
    g.set_parity(capi.PARITY_FAST)
    rng = np.random.default_rng(19)
    for lvl in range(sc.levels):
        poses, scans = hypotheses(o, sc, lvl, rng)
        lens = np.array([len(x) for x in scans])
        lh, res = score(g, lvl, poses, *pack(scans))
        assert capi.load_library().hsm_last_launch_parity(g._h) == capi.PARITY_FAST
        rlh, rres = reference(o, lvl, poses, scans)
        ok = lens > 0
        print(f"level {lvl}: max |lh - ref| {np.abs(lh[ok] - rlh[ok]).max():.3g}, max |res - ref| / n "
              f"{(np.abs(res[ok] - rres[ok]) / lens[ok]).max():.3g}")
        assert np.isnan(lh[~ok]).all() and (res[~ok] == 0).all()
        assert np.abs(lh[ok].astype(np.float64) - rlh[ok]).max() <= 1e-5
        assert (np.abs(res.astype(np.float64) - rres) <= 1e-5 * lens).all()
        # ranking: the rule applied to the DEVICE's own scores (near-ties may rank differently from the reference here)
        G = len(LENS)
        idx, best, _ = run_select(g, lh, groups=G, group_size=len(lh) // G)
        want = select_rule.select_best(lh, groups=G, group_size=len(lh) // G)
        assert np.array_equal(idx, want[0]) and np.array_equal(bits(best[idx >= 0]), bits(want[1][idx >= 0]))
    torch.cuda.synchronize()
    g.close()


# ---- 9: a rectangular map -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", [(333, 90, 2), (90, 333, 2)], ids=lambda g: "%dx%d_L%d" % g)
def test_rectangular_map(capi, oracle_mod, geom):
    """world -> map happens in the kernel now: the two axes must not be swapped or mixed"""
    import rect_cases
    sx, sy, levels = geom
    world, truth, scans_all = rect_cases.scene(sx, sy, 24, 1081, seed=3)
    for kind in oracle_kinds():
        o = oracle_mod.Oracle(kind, rect_cases.RES, sx, sy, levels)
        o.set_update_factor_free(0.4)
        o.set_update_factor_occupied(0.9)
        o.build_map(truth[:16], scans_all[:16])
        g = capi.MapRepMultiMap(rect_cases.RES, sx, sy, levels)
        for lvl in range(levels):
            g.upload_level(lvl, *o.download_level(lvl))
        rng = np.random.default_rng(29)
        for lvl in range(levels):
            poses, scans = [], []
            far = np.stack([o.world_coords_pose(lvl, m) for m in FAR_MAP])
            for k, n in enumerate(LENS):
                t = truth[16 + k]
                for p in np.concatenate([t[None], (t[None] + rng.normal(0, [0.1, 0.1, 0.05], (12, 3))), far]).astype(np.float32):
                    poses.append(p)
                    scans.append(scans_all[16 + k][:n])
            poses = np.stack(poses)
            got = score(g, lvl, poses, *pack(scans))
            assert_scores(f"{kind} level {lvl}", got, reference(o, lvl, poses, scans), [len(s) for s in scans])
            inside = [b for b, s in enumerate(scans) if len(s) == 1081][0]
            assert got[0][inside] > 0.05  # (the truth pose sees the map: the test is not all out-of-map zeros)
        g.close()
