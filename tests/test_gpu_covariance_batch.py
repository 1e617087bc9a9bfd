"""hsm_covariance_batch_device / hsm_match_cov_batch_device / hsm_covariance_batch on the MI355X.

Reference order (the default mode and HSM_PARITY_EXACT): per hypothesis, with that hypothesis's own scan, the map- and world-frame
covariances and all seven sigma-point likelihoods carry the bits of the CPU reference,
`o.covariance_for_poses(lvl, o.map_coords_pose(lvl, w)[None], pts * 2^-lvl)`.  A scan of 0 beams gives NaN everywhere (the sign and
payload of an invalid operation's NaN are the processor's choice, so those rows are compared as NaN, every other row bit for bit).
Tree order (fast, relaxed): the bits of hsm_covariance_for_poses in the same mode on the host-converted map poses, one call per scan:
the summation shape is the same.  Every output buffer is filled with a sentinel before a launch so that a row no launch wrote shows.
"""
import numpy as np
import pytest

import select_rule
from conftest import bits, make_oracle, oracle_kinds
from support import capi, dev, layout_of, pack
from test_gpu_score_batch import SENTINEL, gpu_for, oracle_update, score

pytestmark = pytest.mark.gpu

HSM_ERR_INVALID = -1
CSR_LENS = (0, 1, 63, 64, 65, 128, 129, 0, 181)  # the round boundaries of the chain; an empty scan first and one inside
SHARED_BATCHES = (1, 3, 4, 5)                    # the wavefront and workgroup boundaries
KEYS = ("cw", "cm", "l7", "lh")


def fan(sc, q, n=181):
    """n beams of query scan q spread over its whole fan"""
    return np.ascontiguousarray(sc.query_scans[q][::6][:n])


def cov_dev(g, level, poses, pts, offs=None, stream=None, want=(True, True, True, True)):
    """hsm_covariance_batch_device on torch buffers -> dict of host arrays cw [B,9], cm [B,9], l7 [B,7], lh [B]"""
    import torch
    poses = np.asarray(poses, np.float32).reshape(-1, 3)
    B = len(poses)
    s = stream or torch.cuda.current_stream()
    with torch.cuda.stream(s):
        d_p, d_pts = dev(poses), dev(np.asarray(pts, np.float32).reshape(-1, 2))
        d_offs = None if offs is None else dev(np.asarray(offs, np.int32))
        out = {k: torch.full((max(B, 1), w), SENTINEL, dtype=torch.float32, device="cuda:0") for k, w in zip(KEYS, (9, 9, 7, 1))}
        g.covariance_batch_device(level, B, d_p.data_ptr(), d_pts.data_ptr() if len(pts) else 0,
                                  0 if d_offs is None else d_offs.data_ptr(), len(pts) if d_offs is None else 0,
                                  *[out[k].data_ptr() if w else 0 for k, w in zip(KEYS, want)], s.cuda_stream)
        r = {k: v.cpu().numpy()[:B] for k, v in out.items()}
    r["lh"] = r["lh"][:, 0]
    return r


def reference(o, level, poses, scans):
    """per hypothesis, with its own scan: the reference's (cov_map, cov_world, seven likelihoods) at getMapCoordsPose(pose)"""
    f = np.float32(1.0 / 2 ** level)
    B = len(poses)
    cm, cw, l7 = np.empty((B, 9), np.float32), np.empty((B, 9), np.float32), np.empty((B, 7), np.float32)
    for b, (w, s) in enumerate(zip(poses, scans)):
        m, ww, l = o.covariance_for_poses(level, o.map_coords_pose(level, w)[None], np.asarray(s, np.float32).reshape(-1, 2) * f)
        cm[b], cw[b], l7[b] = np.reshape(m, 9), np.reshape(ww, 9), np.reshape(l, 7)
    return dict(cm=cm, cw=cw, l7=l7, lh=l7[:, 6].copy())


def assert_same(what, got, ref, lens, keys=KEYS):
    """rows of empty scans: NaN in both; every other row: the same bits"""
    empty = np.asarray(lens) == 0
    for k in keys:
        a, b = got[k], ref[k]
        assert not (a == SENTINEL).any(), f"{what}: rows of {k} never written"
        assert np.isnan(a[empty]).all() and np.isnan(b[empty]).all(), (what, k)
        bad = (bits(a) != bits(b))[~empty]
        assert not bad.any(), f"{what}: {k}: {int(bad.sum())} words differ, rows {np.unique(np.argwhere(bad)[:, 0])[:5]}"
    for k in keys:
        assert np.isfinite(got[k][~empty]).all(), (what, k)


def csr_case(sc, rng):
    """nine hypotheses of the nine scan lengths: the truth of their scan and small offsets from it"""
    poses, scans = [], []
    for k, n in enumerate(CSR_LENS):
        q = k % len(sc.query_scans)
        poses.append(sc.query_truth[q] + (rng.normal(0, [0.05, 0.05, 0.02]) if k % 2 else 0))
        scans.append(fan(sc, q, n))
    return np.asarray(poses, np.float32), scans


def border_case(o, sc, level):
    """map-frame poses one cell inside each edge and corner (the +- 1.5 cell sigma points leave the map, the pose does not), and a
    pose with a negative angle near -pi; as WORLD poses, each with a 181-beam fan"""
    size = sc.map_size >> level
    lim, mid = float(size - 2), size / 2.0
    lo, hi = 1.0, lim - 1.0
    maps = [(lo, mid, 0.3), (hi, mid, -2.0), (mid, lo, 1.2), (mid, hi, 2.9), (lo, lo, 0.8), (hi, lo, 2.2), (lo, hi, -0.7),
            (hi, hi, -2.4), (mid + 3.25, mid - 7.5, -3.1)]
    poses = np.stack([o.world_coords_pose(level, np.float32(m)) for m in maps]).astype(np.float32)
    for w, m in zip(poses, maps):  # the pose itself stays inside, a sigma point of each border pose does not
        pm = o.map_coords_pose(level, w)
        assert 0 <= pm[0] <= lim and 0 <= pm[1] <= lim, (level, m, pm)
    assert all(min(m[0], m[1]) - 1.5 < 0 or max(m[0], m[1]) + 1.5 > lim for m in maps[:8])
    return poses, [fan(sc, k % 4) for k in range(len(maps))]


# ---- reference order ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parity", ["default", "exact"])
@pytest.mark.parametrize("layout", ["quad", "plane"])
@pytest.mark.parametrize("kind", oracle_kinds())
def test_reference_order_is_bit_identical_on_every_level(capi, oracle_mod, pyramid_scene, kind, layout, parity):
    sc = pyramid_scene
    o = make_oracle(oracle_mod, kind, sc)
    g = gpu_for(capi, sc, o, layout=layout_of(capi, layout))
    if parity == "exact":
        g.set_parity(capi.PARITY_EXACT)
    lib = capi.load_library()
    rng = np.random.default_rng(2611)
    for lvl in range(sc.levels):
        poses, scans = csr_case(sc, rng)
        pts, offs = pack(scans)
        got = cov_dev(g, lvl, poses, pts, offs)
        assert lib.hsm_last_launch_kernel(g._h) == b"covariance_batch_kernel"
        assert lib.hsm_last_launch_parity(g._h) == capi.PARITY_EXACT
        ref = reference(o, lvl, poses, scans)
        assert_same(f"CSR, level {lvl}", got, ref, CSR_LENS)
        assert (got["lh"][np.asarray(CSR_LENS) > 60] > 0.05).all()  # the poses see the map: not all out-of-map zeros
        # every output alone gives the same bits
        for i, k in enumerate(KEYS):
            alone = cov_dev(g, lvl, poses, pts, offs, want=tuple(j == i for j in range(4)))
            assert_same(f"{k} alone, level {lvl}", alone, got, CSR_LENS, keys=(k,))
            assert all((alone[j] == SENTINEL).all() for j in KEYS if j != k)
        bposes, bscans = border_case(o, sc, lvl)
        bgot = cov_dev(g, lvl, bposes, *pack(bscans))
        bref = reference(o, lvl, bposes, bscans)
        assert_same(f"borders, level {lvl}", bgot, bref, [181] * len(bposes))
        scan = fan(sc, 1)
        for B in SHARED_BATCHES:
            sp = (sc.query_truth[1] + rng.normal(0, [0.05, 0.05, 0.02], (B, 3))).astype(np.float32)
            shared = cov_dev(g, lvl, sp, scan)
            assert_same(f"shared x{B}, level {lvl}", shared, reference(o, lvl, sp, [scan] * B), [181] * B)
            assert_same(f"shared x{B} against CSR", cov_dev(g, lvl, sp, *pack([scan] * B)), shared, [181] * B)
    g.close()


# ---- the tree order -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parity", ["fast", "relaxed"])
@pytest.mark.parametrize("layout", ["quad", "plane"])
def test_tree_order_gives_the_probes_bits(capi, oracle_mod, pyramid_scene, layout, parity):
    sc = pyramid_scene
    o = make_oracle(oracle_mod, "ho", sc)
    g = gpu_for(capi, sc, o, layout=layout_of(capi, layout))
    mode = capi.PARITY_FAST if parity == "fast" else capi.PARITY_RELAXED
    g.set_parity(mode)
    rng = np.random.default_rng(2612)
    for lvl in range(sc.levels):
        c_poses, c_scans = csr_case(sc, rng)
        b_poses, b_scans = border_case(o, sc, lvl)
        poses, scans = np.concatenate([c_poses, b_poses]), c_scans + b_scans
        got = cov_dev(g, lvl, poses, *pack(scans))
        assert capi.load_library().hsm_last_launch_parity(g._h) == mode
        want = dict(cm=[], cw=[], l7=[])
        for w, s in zip(poses, scans):  # the parent route: host-converted map pose, one call per scan
            cm, cw, l7 = g.covariance_for_poses(lvl, g.getMapCoordsPose(lvl, w)[None], s)
            want["cm"].append(cm[0]), want["cw"].append(cw[0]), want["l7"].append(l7[0])
        want = {k: np.stack(v) for k, v in want.items()}
        want["lh"] = want["l7"][:, 6]
        assert_same(f"{parity}, level {lvl}", got, want, [len(s) for s in scans])
    g.close()


# ---- relations ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parity", ["default", "exact", "fast", "relaxed"])
def test_pose_likelihood_is_the_scores_likelihood_in_every_mode(capi, oracle_mod, pyramid_scene, parity):
    sc = pyramid_scene
    o = make_oracle(oracle_mod, "ho", sc)
    g = gpu_for(capi, sc, o)
    if parity != "default":
        g.set_parity({"exact": capi.PARITY_EXACT, "fast": capi.PARITY_FAST, "relaxed": capi.PARITY_RELAXED}[parity])
    rng = np.random.default_rng(2613)
    for lvl in range(sc.levels):
        c_poses, c_scans = csr_case(sc, rng)
        b_poses, b_scans = border_case(o, sc, lvl)
        poses, scans = np.concatenate([c_poses, b_poses]), c_scans + b_scans
        pts, offs = pack(scans)
        got = cov_dev(g, lvl, poses, pts, offs)
        lh, _ = score(g, lvl, poses, pts, offs)
        empty = np.array([len(s) == 0 for s in scans])
        assert np.isnan(got["lh"][empty]).all() and np.isnan(lh[empty]).all() and np.isnan(got["l7"][empty]).all()
        assert np.array_equal(bits(got["lh"][~empty]), bits(got["l7"][~empty, 6])), lvl
        assert np.array_equal(bits(got["lh"][~empty]), bits(lh[~empty])), lvl
    g.close()


def test_host_form_equals_the_device_form(capi, oracle_mod, pyramid_scene):
    sc = pyramid_scene
    o = make_oracle(oracle_mod, "ho", sc)
    g = gpu_for(capi, sc, o)
    rng = np.random.default_rng(2614)
    poses, scans = csr_case(sc, rng)
    pts, offs = pack(scans)
    for lvl in (0, 2):
        host = dict(zip(KEYS, g.covariance_batch(lvl, poses, pts, offs)))
        assert_same(f"host CSR, level {lvl}", host, cov_dev(g, lvl, poses, pts, offs), CSR_LENS)
        scan = fan(sc, 2)
        host = dict(zip(KEYS, g.covariance_batch(lvl, poses[:5], scan)))
        assert_same(f"host shared, level {lvl}", host, cov_dev(g, lvl, poses[:5], scan), [181] * 5)
    cw, cm, l7, lh = g.covariance_batch(0, poses[:2], np.zeros((0, 2), np.float32))  # a shared scan of no beams
    assert np.isnan(cw).all() and np.isnan(cm).all() and np.isnan(l7).all() and np.isnan(lh).all()
    g.close()


class ChainBuffers:
    """3 groups of 8 hypotheses: two query scans from wide starts, and a group whose scans are all empty"""
    G, K = 3, 8

    def __init__(self, sc, seed=5, shift=0):
        import torch
        rng = np.random.default_rng(seed)
        init, scans = [], []
        for gi in range(self.G):
            q = gi + shift
            init.append(sc.query_truth[q] + rng.uniform(-1, 1, (self.K, 3)) * [0.3, 0.3, 0.15])
            scans += [sc.query_scans[q][:700] if gi < 2 else sc.query_scans[q][:0]] * self.K
        self.h_init = np.concatenate(init).astype(np.float32)
        self.h_pts, self.h_offs = pack(scans)
        self.B = len(self.h_init)
        self.init, self.pts, self.offs = dev(self.h_init), dev(self.h_pts), dev(self.h_offs)
        f = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float32, device="cuda:0")  # noqa: E731
        B, G = self.B, self.G
        self.pose, self.hess, self.cw, self.cm, self.l7, self.lh = f(B, 3), f(B, 9), f(B, 9), f(B, 9), f(B, 7), f(B)
        self.idx = torch.full((G,), 99, dtype=torch.int32, device="cuda:0")
        self.best, self.best_pose = f(G), f(G, 3)

    def three_calls(self, g, s, level=0):
        g.match_batch_device(self.B, self.init.data_ptr(), self.pts.data_ptr(), self.offs.data_ptr(), 700, self.pose.data_ptr(),
                             self.hess.data_ptr(), s.cuda_stream)
        g.covariance_batch_device(level, self.B, self.pose.data_ptr(), self.pts.data_ptr(), self.offs.data_ptr(), 0,
                                  self.cw.data_ptr(), self.cm.data_ptr(), self.l7.data_ptr(), self.lh.data_ptr(), s.cuda_stream)
        g.select_best_device(self.G, 0, self.K, self.lh.data_ptr(), self.pose.data_ptr(), self.idx.data_ptr(), self.best.data_ptr(),
                             self.best_pose.data_ptr(), s.cuda_stream)

    def one_call(self, g, s, level=0):
        g.match_cov_batch_device(self.B, self.init.data_ptr(), self.pts.data_ptr(), self.offs.data_ptr(), 700, self.pose.data_ptr(),
                                 self.hess.data_ptr(), level, self.cw.data_ptr(), self.cm.data_ptr(), self.l7.data_ptr(),
                                 self.lh.data_ptr(), self.G, 0, self.K, self.idx.data_ptr(), self.best.data_ptr(),
                                 self.best_pose.data_ptr(), s.cuda_stream)

    def refill(self):
        for t in (self.pose, self.hess, self.cw, self.cm, self.l7, self.lh, self.best, self.best_pose):
            t.fill_(SENTINEL)
        self.idx.fill_(99)

    def host(self):
        return {k: getattr(self, k).cpu().numpy() for k in ("pose", "hess", "cw", "cm", "l7", "lh", "idx", "best", "best_pose")}


def assert_same_results(what, a, b):
    for k in a:
        x, y = (bits(v) if v.dtype == np.float32 else v for v in (a[k], b[k]))
        assert np.array_equal(x, y), (what, k)  # (the same kernels on the same inputs: NaN rows carry the same bits too)


def test_match_cov_is_the_three_calls(capi, oracle_mod, pyramid_scene):
    import torch
    sc = pyramid_scene
    o = make_oracle(oracle_mod, "ho", sc)
    g = gpu_for(capi, sc, o)
    s = torch.cuda.Stream()
    a, b = ChainBuffers(sc), ChainBuffers(sc)
    torch.cuda.synchronize()
    a.three_calls(g, s)  # no host wait between the three
    b.one_call(g, s)
    s.synchronize()
    ra, rb = a.host(), b.host()
    assert_same_results("one call", rb, ra)
    K = a.K
    assert not (ra["pose"] == SENTINEL).any() and not (ra["lh"][:2 * K] == SENTINEL).any()
    # the matched poses' covariances are the reference's
    scans = [a.h_pts[a.h_offs[i]:a.h_offs[i + 1]] for i in range(a.B)]
    assert_same("matched poses", dict(cw=ra["cw"], cm=ra["cm"], l7=ra["l7"], lh=ra["lh"]), reference(o, 0, ra["pose"], scans),
                np.diff(a.h_offs))
    # the winners follow the rule on the device's likelihoods; the group of empty scans has none
    idx, best = select_rule.select_best(ra["lh"], groups=a.G, group_size=K)
    assert np.array_equal(ra["idx"], idx) and idx[2] == -1 and (idx[:2] >= 0).all()
    assert np.array_equal(bits(ra["best"][:2]), bits(best[:2])) and np.isnan(ra["best"][2])
    assert np.array_equal(bits(ra["best_pose"][:2]), bits(ra["pose"][idx[:2]])) and (ra["best_pose"][2] == SENTINEL).all()
    assert np.isnan(ra["cw"][2 * K:]).all() and np.isnan(ra["l7"][2 * K:]).all()
    # the Hessian stays optional, the ranking too
    c = ChainBuffers(sc)
    torch.cuda.synchronize()
    g.match_cov_batch_device(c.B, c.init.data_ptr(), c.pts.data_ptr(), c.offs.data_ptr(), 700, c.pose.data_ptr(), 0, 0,
                             c.cw.data_ptr(), 0, 0, 0, stream=s.cuda_stream)
    s.synchronize()
    rc = c.host()
    assert np.array_equal(bits(rc["pose"]), bits(ra["pose"])) and np.array_equal(bits(rc["cw"]), bits(ra["cw"]))
    assert (rc["hess"] == SENTINEL).all() and (rc["idx"] == 99).all() and (rc["lh"] == SENTINEL).all()
    g.close()


def test_match_and_covariance_captured_in_a_graph_and_replayed(capi, oracle_mod, pyramid_scene):
    import torch
    sc = pyramid_scene
    o = make_oracle(oracle_mod, "ho", sc)
    g = gpu_for(capi, sc, o)
    s = torch.cuda.Stream()
    buf = ChainBuffers(sc)
    torch.cuda.synchronize()
    buf.one_call(g, s)  # eager first: what the MATCH allocates exists before the capture; the covariance entry needs nothing
    s.synchronize()
    first = buf.host()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):  # (an allocation or a synchronisation under capture fails the capture)
        buf.one_call(g, s)
        with pytest.raises(capi.HsmError) as e:
            g.updateByScan(sc.build_scans[0], sc.build_poses[0])
        assert f"({HSM_ERR_INVALID})" in str(e.value) and "captur" in str(e.value), str(e.value)
    with torch.cuda.stream(s):
        buf.refill()
        graph.replay()
    s.synchronize()
    assert_same_results("replay of the captured inputs", buf.host(), first)
    # new poses and new scans, of other lengths, written into the same buffers
    new = ChainBuffers(sc, seed=9, shift=3)
    assert new.h_pts.shape == buf.h_pts.shape
    torch.cuda.synchronize()
    new.one_call(g, s)  # eager, buffers of its own
    s.synchronize()
    with torch.cuda.stream(s):
        buf.init.copy_(new.init), buf.pts.copy_(new.pts), buf.offs.copy_(new.offs)
        buf.refill()
        graph.replay()
    s.synchronize()
    got = buf.host()
    assert not np.array_equal(bits(got["pose"]), bits(first["pose"]))
    assert_same_results("replay with new inputs", got, new.host())
    del graph
    g.updateByScan(sc.build_scans[0], sc.build_poses[0])  # the capture has ended: accepted
    g.synchronize()
    g.close()


def test_covariance_is_ordered_behind_a_queued_update(capi, oracle_mod, pyramid_scene):
    import torch
    from hector_slam_amd import synth
    sc = pyramid_scene
    o = make_oracle(oracle_mod, oracle_kinds()[-1], sc)
    g = gpu_for(capi, sc, o, stamps=False)  # (log-odds only: test_gpu_score_batch.py has why)
    rng = np.random.default_rng(8)
    sfac = float(np.float32(1.0) / np.float32(sc.resolution))
    dense = synth.make_scan(sc.world, sc.build_poses[0], 16384, sfac, rng)  # a long-running update
    poses, scans = csr_case(sc, rng)
    pts, offs = pack(scans)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    before = cov_dev(g, 0, poses, pts, offs, stream=s)
    ref_before = reference(o, 0, poses, scans)
    g.updateByScan(dense, sc.build_poses[0])  # queued on the context's stream, not waited for ...
    after = cov_dev(g, 0, poses, pts, offs, stream=s)  # ... and the covariance on the caller's stream right behind it
    oracle_update(o, sc.build_poses[0], dense)
    ref_after = reference(o, 0, poses, scans)
    g.synchronize()
    assert_same("before the update", before, ref_before, CSR_LENS)
    assert_same("behind the update", after, ref_after, CSR_LENS)
    full = np.asarray(CSR_LENS) > 60
    assert not np.array_equal(bits(before["cw"][full]), bits(after["cw"][full]))  # the update does change these
    g.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_entry_and_launch_nothing(capi, oracle_mod, small_scene):
    import torch
    sc = small_scene
    g = gpu_for(capi, sc, make_oracle(oracle_mod, "ho", sc))
    lib = capi.load_library()
    buf = torch.full((256,), SENTINEL, dtype=torch.float32, device="cuda:0")
    idx = torch.full((4,), 99, dtype=torch.int32, device="cuda:0")
    p, ip = buf.data_ptr(), idx.data_ptr()

    def refused(rc, name):
        assert rc == HSM_ERR_INVALID and name.encode() in lib.hsm_last_error(), (rc, lib.hsm_last_error())

    dev_form = lib.hsm_covariance_batch_device
    name = "hsm_covariance_batch_device"
    refused(dev_form(None, 0, 1, p, p, None, 1, p, p, p, p, None), name)          # NULL context
    refused(dev_form(g._h, sc.levels, 1, p, p, None, 1, p, p, p, p, None), name)  # level past the pyramid
    refused(dev_form(g._h, -1, 1, p, p, None, 1, p, p, p, p, None), name)         # level below zero
    refused(dev_form(g._h, 0, -1, p, p, None, 1, p, p, p, p, None), name)         # batch < 0
    refused(dev_form(g._h, 0, 1, p, p, None, 1, None, None, None, None, None), name)  # all four outputs NULL
    refused(dev_form(g._h, 0, 1, p, p, None, -1, p, p, p, p, None), name)         # shared_n < 0 without offsets
    refused(dev_form(g._h, 0, 1, None, p, None, 1, p, p, p, p, None), name)       # NULL poses
    refused(dev_form(g._h, 0, 1, p, None, None, 1, p, p, p, p, None), name)       # NULL points, shared scan of 1 beam
    assert dev_form(g._h, 0, 0, None, None, None, 0, p, None, None, None, None) == 0  # batch == 0
    one = lib.hsm_match_cov_batch_device
    name = "hsm_match_cov_batch_device"
    refused(one(g._h, 4, p, p, None, 1, p, None, 1, p, p, p, p, 0, None, 0, None, None, None, None), name)    # level (one level here)
    refused(one(g._h, 4, p, p, None, 1, p, None, 0, None, None, None, None, 0, None, 0, None, None, None, None), name)  # no output
    refused(one(g._h, 4, None, p, None, 1, p, None, 0, p, p, p, p, 0, None, 0, None, None, None, None), name)  # NULL starts
    refused(one(g._h, 4, p, p, None, 1, p, None, 0, p, p, p, None, 2, None, 2, ip, None, None, None), name)   # ranking needs likelihoods
    refused(one(g._h, 4, p, p, None, 1, p, None, 0, p, p, p, p, 3, None, 2, ip, None, None, None), name)      # 3 groups of 2 in 4
    refused(one(g._h, 4, p, p, None, 1, p, None, 0, p, p, p, p, 2, None, 2, None, None, None, None), name)    # ranking needs d_out_index
    h = np.full(64, SENTINEL, np.float32)
    hp = h.ctypes.data
    name = "hsm_covariance_batch"
    refused(lib.hsm_covariance_batch(g._h, 1, 1, hp, hp, None, 1, hp, hp, hp, hp), name)
    refused(lib.hsm_covariance_batch(g._h, 0, -1, hp, hp, None, 1, hp, hp, hp, hp), name)
    refused(lib.hsm_covariance_batch(g._h, 0, 1, hp, hp, None, 1, None, None, None, None), name)
    refused(lib.hsm_covariance_batch(g._h, 0, 1, None, hp, None, 1, hp, hp, hp, hp), name)
    refused(lib.hsm_covariance_batch(g._h, 0, 1, hp, None, None, 1, hp, hp, hp, hp), name)
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all() and (idx == 99).all() and (h == SENTINEL).all()
    g.close()
