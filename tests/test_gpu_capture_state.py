"""Batched matches across hipGraph capture and the per-stream state the context keeps between launches: the Morton
permutation of a caller's stream (hsm_set_batch_order), the ordering of caller streams behind queued map updates, and the
product scratch of the speculative-carry form (HSM_EXACT_SPEC=1).  A capture must neither change that state as though the
captured work had run nor make a graph depend on state that a later eager launch rewrites or frees.

Every output row is compared, and every output buffer is filled with NaN before each launch, so that a row a launch never
wrote shows.  The default mode is held to the CPU reference's poses bit for bit ("hr" where oracle/_ref is present), both
modes to the eager caller-order launch of the same mode (pose and covariance, bit for bit).  Graphs are captured on one stream
each: they have no parallel branches.  Also: the sort kernel itself, through hsm_debug_batch_order."""
import threading

import numpy as np
import pytest

from conftest import bits, make_oracle, oracle_kinds
from support import capi

pytestmark = pytest.mark.gpu

KIND = oracle_kinds()[-1]  # "hr" (reference-compiled) where available
B = 4096
RANGE_MIN, RANGE_MAX = 0.4, 30.0
HSM_ERR_INVALID = -1


def oracle_poses(oracle_mod, sc, init, pts, offs, threads=16):
    """matchData of the CPU reference for every scan (one private oracle per thread)"""
    n = init.shape[0]
    T = max(1, min(threads, n // 64))
    out = np.empty((n, 3), np.float32)

    def work(t):
        o = make_oracle(oracle_mod, KIND, sc)
        b, e = n * t // T, n * (t + 1) // T
        out[b:e] = o.match_many(init[b:e], pts[offs[b]:offs[e]], offs[b:e + 1] - offs[b])

    th = [threading.Thread(target=work, args=(t,)) for t in range(T)]
    [x.start() for x in th]
    [x.join() for x in th]
    return out


class Inputs:
    """one batch on the device and how to launch it: CSR scans (hsm_match_batch_device) or raw LaserScan ranges
    (hsm_match_batch_ranges_device); `oracle` is the reference's pose of every scan"""

    def __init__(self, init, pts=None, offs=None, ranges=None, geom=None, scale=None, oracle=None):
        import torch
        dev = torch.device("cuda", 0)
        self.n = init.shape[0]
        self.oracle = oracle
        self.d_init = torch.from_numpy(np.ascontiguousarray(init)).to(dev)
        self.ranges = ranges is not None
        if self.ranges:
            self.nb = ranges.shape[1]
            self.geom, self.scale = geom, scale
            self.d_ranges = torch.from_numpy(np.ascontiguousarray(ranges)).to(dev)
            self.d_counts = torch.zeros(self.n, dtype=torch.int32, device=dev)
            self.ws_bytes = None
        else:
            self.d_pts = torch.from_numpy(np.ascontiguousarray(pts)).to(dev)
            self.d_offs = torch.from_numpy(np.ascontiguousarray(offs)).to(dev)

    def launch(self, g, batch, out, stream):
        import torch
        assert batch <= self.n and batch <= out.n
        if self.ranges:
            if self.ws_bytes is None:
                self.ws_bytes = g.match_batch_ranges_workspace(self.n, self.nb)
                self.d_ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device="cuda:0")
            g.match_batch_ranges_device(batch, self.d_init.data_ptr(), self.d_ranges.data_ptr(), self.nb, *self.geom, self.scale,
                                        out.pose.data_ptr(), out.cov.data_ptr(), self.d_counts.data_ptr(), self.d_ws.data_ptr(),
                                        self.ws_bytes, stream.cuda_stream)
        else:
            g.match_batch_device(batch, self.d_init.data_ptr(), self.d_pts.data_ptr(), self.d_offs.data_ptr(), 1081,
                                 out.pose.data_ptr(), out.cov.data_ptr(), stream.cuda_stream)


class Out:
    def __init__(self, n):
        import torch
        self.n = n
        self.pose = torch.empty((n, 3), dtype=torch.float32, device="cuda:0")
        self.cov = torch.empty((n, 9), dtype=torch.float32, device="cuda:0")

    def nan(self, stream=None):
        """NaN into every row, ordered on `stream` (the current one where None)"""
        import torch
        with torch.cuda.stream(stream or torch.cuda.current_stream()):
            self.pose.fill_(float("nan"))
            self.cov.fill_(float("nan"))

    def host(self, batch=None):
        b = self.n if batch is None else batch
        return self.pose[:b].cpu().numpy(), self.cov[:b].cpu().numpy()


def oracle_of(g, inp):
    """the reference's poses where the context runs the library default (the reference's order); None in fast mode"""
    from hector_slam_amd import capi
    return inp.oracle if g.parity() == capi.PARITY_AUTO else None


def check(what, got, want, oracle=None):
    """every row: written (no NaN left), pose and covariance the eager caller-order launch's bits, pose the reference's"""
    pose, cov = got
    unwritten = np.isnan(pose).any(1) | np.isnan(cov).any(1)
    assert not unwritten.any(), f"{what}: {int(unwritten.sum())} of {len(pose)} rows never written"
    dp = (bits(pose) != bits(want[0])).any(1)
    dc = (bits(cov) != bits(want[1])).any(1)
    assert not dp.any() and not dc.any(), f"{what}: {int(dp.sum())} poses / {int(dc.sum())} covariances of {len(pose)} differ"
    if oracle is not None:
        do = (bits(pose) != bits(oracle[:len(pose)])).any(1)
        assert not do.any(), f"{what}: {int(do.sum())} of {len(pose)} poses differ from the reference ({KIND})"


@pytest.fixture(scope="module")
def case(capi, oracle_mod):
    """a 1024^2 three-level map, 4096 query scans in three forms (equal CSR, ragged CSR, raw ranges), their reference poses; each
    form holds the batch twice (8192 scans: batches of either size)"""
    from hector_slam_amd import synth
    sc = synth.make_scene(n_beams=1081, map_size=1024, levels=3, resolution=0.05, n_build=60, n_query=B, room=(40.0, 30.0), seed=21)
    rng = np.random.default_rng(7)
    inputs = {}
    pts, offs = synth.pack_scans(sc.query_scans)
    inputs["csr"] = (sc.query_init, pts, offs)
    ragged = [s[: len(s) - int(rng.integers(0, 500))] for s in sc.query_scans]
    inputs["ragged"] = (sc.query_init, *synth.pack_scans(ragged))
    scans = {"csr": list(sc.query_scans), "ragged": ragged}
    # raw ranges at the query poses: the scene's ray caster, range noise, a driver's drop-outs
    ang = synth.beam_angles(1081)
    r = np.stack([sc.world.raycast(p, ang) for p in sc.query_truth]) + rng.normal(0.0, 0.01, (B, 1081))
    r = r.astype(np.float32)
    drop = rng.random(r.shape)
    r[drop < 0.02] = np.inf
    r[(drop >= 0.02) & (drop < 0.03)] = np.nan
    a0, inc = synth.SCAN_SHAPES[1081] if 1081 in synth.SCAN_SHAPES else (-np.pi, 2.0 * np.pi / 1081)
    geom = (float(np.float32(a0)), float(np.float32(inc)), RANGE_MIN, RANGE_MAX)
    o = make_oracle(oracle_mod, KIND, sc, build=False)
    conts = [o.laser_scan_to_container(r[b], *geom, sc.scale_to_map) for b in range(B)]
    assert min(c.shape[0] for c in conts) > 0
    refs = {}
    for k, (init, p, of) in inputs.items():
        refs[k] = oracle_poses(oracle_mod, sc, init, p, of)
    rp, ro = synth.pack_scans(conts)
    refs["ranges"] = oracle_poses(oracle_mod, sc, sc.query_init, rp, ro)
    init2 = np.concatenate([sc.query_init] * 2)
    dev = {k: Inputs(init2, *synth.pack_scans(scans[k] * 2), oracle=np.concatenate([refs[k]] * 2)) for k in inputs}
    dev["ranges"] = Inputs(init2, ranges=np.concatenate([r] * 2), geom=geom, scale=sc.scale_to_map,
                           oracle=np.concatenate([refs["ranges"]] * 2))
    # the same scans in another order (np.roll): another permutation out of the sort kernel, the reference rolled with them
    roll = np.roll(np.arange(B), 1000)
    rp2, ro2 = synth.pack_scans([sc.query_scans[i] for i in roll])
    dev["rolled"] = Inputs(sc.query_init[roll], rp2, ro2, oracle=refs["csr"][roll])
    return sc, dev


def new_ctx(capi, sc, mode):
    g = capi.MapRepMultiMap(sc.resolution, sc.map_size, sc.map_size, sc.levels)
    g.setUpdateFactorFree(0.4)
    g.setUpdateFactorOccupied(0.9)
    g.build_map(sc.build_poses, sc.build_scans)
    g.set_parity(mode)
    g.synchronize()
    return g


def given_order(capi, g, inp, batch):
    """the eager launch in the caller's order on a stream of its own: the bits every other launch must give"""
    import torch
    order = g.batch_order()
    g.set_batch_order(capi.ORDER_GIVEN)
    out, s = Out(batch), torch.cuda.Stream()
    out.nan()
    torch.cuda.synchronize()
    inp.launch(g, batch, out, s)
    torch.cuda.synchronize()
    assert not g.last_launch_sorted()
    want = out.host()
    check("caller's order", want, want, inp.oracle if g.parity() == capi.PARITY_AUTO else None)
    g.set_batch_order(order)
    return want


def modes(capi):
    return {"auto": capi.PARITY_AUTO, "fast": capi.PARITY_FAST}


# ---- permutation state across capture -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["csr", "ragged", "ranges"])
@pytest.mark.parametrize("mode", ["auto", "fast"])
def test_a_captured_sort_leaves_no_stale_permutation(capi, case, mode, variant):
    """eager 4096, eager 2048, captured 4096, eager 4096 on one stream, in that order (4096 first: every stale entry of the
    permutation is a valid scan index, so a stale one shows as rows never written, not as a read out of range).  The fast mode
    sorts batches of 4096 scans and more only (smaller ones run on teams of wavefronts): 8192, 4096, 8192, 8192 there"""
    import torch
    sc, dev = case
    inp = dev[variant]
    g = new_ctx(capi, sc, modes(capi)[mode])
    big, small = (B, B // 2) if mode == "auto" else (2 * B, B)
    want4, want2 = given_order(capi, g, inp, big), given_order(capi, g, inp, small)
    g.set_batch_order(capi.ORDER_MORTON)
    s = torch.cuda.Stream()
    out, out_g = Out(big), Out(big)
    out.nan(s)
    inp.launch(g, big, out, s)
    assert g.last_launch_sorted()
    s.synchronize()
    check(f"1. eager {big}", out.host(), want4, oracle_of(g, inp))
    out.nan(s)
    inp.launch(g, small, out, s)
    assert g.last_launch_sorted()
    s.synchronize()
    check(f"2. eager {small}", out.host(small), want2, oracle_of(g, inp))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        inp.launch(g, big, out_g, s)
    out.nan(s)
    inp.launch(g, big, out, s)
    assert g.last_launch_sorted()
    s.synchronize()
    check(f"4. eager {big} after a captured {big}", out.host(), want4, oracle_of(g, inp))
    out_g.nan()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    check(f"3. the captured {big}, replayed", out_g.host(), want4, oracle_of(g, inp))
    del graph
    g.close()


@pytest.mark.parametrize("mode", ["auto", "fast"])
def test_b_a_larger_eager_batch_does_not_free_what_a_graph_reads(capi, case, mode):
    """capture on a stream that holds a valid permutation, grow its buffer with an eager batch of 8192, replay the graph"""
    import torch
    sc, dev = case
    inp = inp8 = dev["csr"]
    g = new_ctx(capi, sc, modes(capi)[mode])
    want4, want8 = given_order(capi, g, inp, B), given_order(capi, g, inp8, 2 * B)
    g.set_batch_order(capi.ORDER_MORTON)
    s = torch.cuda.Stream()
    out, out_g, out8 = Out(B), Out(B), Out(2 * B)
    out.nan(s)
    inp.launch(g, B, out, s)
    assert g.last_launch_sorted()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        inp.launch(g, B, out_g, s)
    out8.nan(s)
    inp8.launch(g, 2 * B, out8, s)
    assert g.last_launch_sorted()
    s.synchronize()
    check("eager 4096", out.host(), want4, oracle_of(g, inp))
    check("eager 8192 after the capture", out8.host(), want8, oracle_of(g, inp8))
    for _ in range(2):
        out_g.nan()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        check("replay after the buffer grew", out_g.host(), want4, oracle_of(g, inp))
    del graph
    g.close()


@pytest.mark.parametrize("mode", ["auto", "fast"])
def test_c_eager_resorts_while_a_graph_replays(capi, case, mode):
    """a graph captured on `s`; then, interleaved, replays on another stream and eager launches on `s` that sort every time
    (refresh 1) a batch in another order: every graph row and every eager row right"""
    import torch
    sc, dev = case
    inp, rolled = dev["csr"], dev["rolled"]
    g = new_ctx(capi, sc, modes(capi)[mode])
    want, want_r = given_order(capi, g, inp, B), given_order(capi, g, rolled, B)
    g.set_batch_order(capi.ORDER_MORTON)
    s, r = torch.cuda.Stream(), torch.cuda.Stream()
    out, out_g = Out(B), Out(B)
    inp.launch(g, B, out, s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        inp.launch(g, B, out_g, s)
    g.set_batch_order_refresh(1)
    for it in range(3):
        out_g.nan(r)
        with torch.cuda.stream(r):
            graph.replay()
        out.nan(s)
        (rolled if it % 2 == 0 else inp).launch(g, B, out, s)
        assert g.last_launch_sorted()
        torch.cuda.synchronize()
        check(f"replay {it}", out_g.host(), want, oracle_of(g, inp))
        check(f"eager {it}", out.host(), want_r if it % 2 == 0 else want, oracle_of(g, rolled if it % 2 == 0 else inp))
    del graph
    g.close()


@pytest.mark.parametrize("mode", ["auto", "fast"])
def test_d_first_sorted_launch_in_a_capture_and_a_ninth_stream(capi, case, mode):
    """a stream whose first sorted launch is captured, then an eager launch of the same size on it; and a ninth caller stream
    (eight hold permutations): it keeps the caller's order, eager and captured"""
    import torch
    sc, dev = case
    inp = dev["csr"]
    g = new_ctx(capi, sc, modes(capi)[mode])
    want = given_order(capi, g, inp, B)
    g.set_batch_order(capi.ORDER_MORTON)
    streams = [torch.cuda.Stream() for _ in range(9)]
    out, out_g = Out(B), Out(B)
    for k, s in enumerate(streams):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            inp.launch(g, B, out_g, s)
        assert not g.last_launch_sorted()  # (a captured launch keeps the caller's order)
        out.nan(s)
        inp.launch(g, B, out, s)
        assert g.last_launch_sorted() == (k < 8), k
        s.synchronize()
        check(f"stream {k}: eager after its capture", out.host(), want, oracle_of(g, inp))
        out_g.nan()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        check(f"stream {k}: replay", out_g.host(), want, oracle_of(g, inp))
        del graph
    g.close()


# ---- update ordering across capture ---------------------------------------------------------------------------------------------

def _pair(capi, sc, monkeypatch, mode):
    monkeypatch.setenv("HSM_ASYNC_UPDATE", "0")
    ref = capi.MapRepMultiMap(sc.resolution, sc.map_size, sc.map_size, sc.levels)
    monkeypatch.delenv("HSM_ASYNC_UPDATE")
    dut = capi.MapRepMultiMap(sc.resolution, sc.map_size, sc.map_size, sc.levels)
    for m in (ref, dut):
        m.setUpdateFactorFree(0.4)
        m.setUpdateFactorOccupied(0.9)
        m.set_parity(mode)
    return ref, dut


def _same_maps(sc, a, b):
    for lvl in range(sc.levels):
        la, lb = a.download_level(lvl), b.download_level(lvl)
        assert np.array_equal(bits(la[0]), bits(lb[0])) and np.array_equal(la[1], lb[1]), lvl


@pytest.mark.parametrize("mode", ["auto", "fast"])
def test_e_queued_updates_are_ordered_across_a_capture(capi, pyramid_scene, monkeypatch, mode):
    """updates queued without a synchronize, a match loop captured on a fresh stream right behind them (no device sync at the
    capture), replayed; one eager match on that stream; another queued update and another eager match: each result the one of
    a context that blocks in every update"""
    import torch
    from hector_slam_amd import synth
    sc = pyramid_scene
    ref, dut = _pair(capi, sc, monkeypatch, modes(capi)[mode])
    dev = torch.device("cuda", 0)
    n = 256
    full = sc.query_scans[0]
    init = np.repeat(sc.query_init[0:1], n, 0) + np.random.default_rng(3).uniform(-0.03, 0.03, (n, 3)).astype(np.float32) * np.float32([1, 1, 0.2])
    d_init = torch.from_numpy(init).to(dev)
    d_pts = torch.from_numpy(np.ascontiguousarray(full)).to(dev)
    rng = np.random.default_rng(8)
    sfac = float(np.float32(1.0) / np.float32(sc.resolution))
    dense = [synth.make_scan(sc.world, sc.build_poses[t], 16384, sfac, rng) for t in range(24)]  # long-running updates
    res = {}
    for name, m in (("ref", ref), ("dut", dut)):
        s = torch.cuda.Stream(device=dev)
        out = Out(n)

        def launch():
            m.match_batch_device(n, d_init.data_ptr(), d_pts.data_ptr(), 0, full.shape[0], out.pose.data_ptr(), out.cov.data_ptr(),
                                 s.cuda_stream)
        for t in range(20):
            m.updateByScan(dense[t], sc.build_poses[t])  # queued (dut) / blocking (ref)
        graph = torch.cuda.CUDAGraph()
        out.nan(s)
        with torch.cuda.stream(s):
            graph.capture_begin()
            try:
                for _ in range(3):
                    launch()
            finally:
                graph.capture_end()
        with torch.cuda.stream(s):
            graph.replay()
        s.synchronize()
        r = [out.host()]
        out.nan(s)
        launch()
        s.synchronize()
        r.append(out.host())
        m.updateByScan(dense[20], sc.build_poses[20])
        out.nan(s)
        launch()
        s.synchronize()
        r.append(out.host())
        m.updateByScan(dense[21], sc.build_poses[21])  # behind the eager matches, before a replay the caller orders itself
        m.synchronize()
        with torch.cuda.stream(s):
            out.pose.fill_(float("nan"))
            out.cov.fill_(float("nan"))
            graph.replay()
        s.synchronize()
        r.append(out.host())
        res[name] = r
        del graph
    for k, (a, b) in enumerate(zip(res["ref"], res["dut"])):
        check(f"step {k}", b, a)
    _same_maps(sc, ref, dut)
    ref.close()
    dut.close()


@pytest.mark.parametrize("mode", ["auto", "fast"])
def test_f_an_update_while_a_caller_stream_captures_is_refused(capi, pyramid_scene, monkeypatch, mode):
    """an update issued while a stream that this context matches on is being captured fails with HSM_ERR_INVALID and enqueues
    nothing; the capture ends cleanly, its replay and the map are the blocking context's; after the capture the update runs"""
    import torch
    sc = pyramid_scene
    ref, dut = _pair(capi, sc, monkeypatch, modes(capi)[mode])
    dev = torch.device("cuda", 0)
    n = 256
    full = sc.query_scans[1]
    init = np.repeat(sc.query_init[1:2], n, 0) + np.random.default_rng(4).uniform(-0.03, 0.03, (n, 3)).astype(np.float32) * np.float32([1, 1, 0.2])
    d_init = torch.from_numpy(init).to(dev)
    d_pts = torch.from_numpy(np.ascontiguousarray(full)).to(dev)
    res = {}
    for name, m in (("ref", ref), ("dut", dut)):
        s = torch.cuda.Stream(device=dev)
        out = Out(n)

        def launch():
            m.match_batch_device(n, d_init.data_ptr(), d_pts.data_ptr(), 0, full.shape[0], out.pose.data_ptr(), out.cov.data_ptr(),
                                 s.cuda_stream)
        for t in range(10):
            m.updateByScan(sc.build_scans[t], sc.build_poses[t])
        launch()  # an eager match first: the stream has pending work when the capture starts
        graph = torch.cuda.CUDAGraph()
        idx = m.getUpdateIndex(0)
        with torch.cuda.graph(graph, stream=s):
            launch()
            with pytest.raises(capi.HsmError) as e:
                m.updateByScan(sc.build_scans[10], sc.build_poses[10])
            assert f"({HSM_ERR_INVALID})" in str(e.value) and "captur" in str(e.value), str(e.value)
            launch()
        assert m.getUpdateIndex(0) == idx  # (the refused update changed nothing)
        out.nan()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        r = [out.host()]
        m.updateByScan(sc.build_scans[10], sc.build_poses[10])  # the capture has ended: accepted
        out.nan(s)
        launch()
        s.synchronize()
        r.append(out.host())
        res[name] = r
        del graph
    for k, (a, b) in enumerate(zip(res["ref"], res["dut"])):
        check(f"step {k}", b, a)
    _same_maps(sc, ref, dut)
    ref.close()
    dut.close()


# ---- speculative scratch (HSM_EXACT_SPEC=1, default mode) --------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dense_case(capi, oracle_mod, pyramid_scene):
    """hypotheses of ONE 16384-beam scan, and the reference's pose for each"""
    from hector_slam_amd import synth
    sc = pyramid_scene
    rng = np.random.default_rng(31)
    pts = synth.make_scan(sc.world, sc.query_truth[2], 16384, sc.scale_to_map, rng, pad_to_full=True)
    hyp = np.repeat(sc.query_init[2:3], 12, 0) + rng.uniform(-0.05, 0.05, (12, 3)).astype(np.float32) * np.float32([1, 1, 0.2])
    o = make_oracle(oracle_mod, KIND, sc)
    want = np.stack([o.match(h, pts)[0] for h in hyp])
    return sc, pts, hyp, want


def _spec_ctx(capi, sc, monkeypatch):
    monkeypatch.setenv("HSM_EXACT_SPEC", "1")
    g = capi.MapRepMultiMap(sc.resolution, sc.map_size, sc.map_size, sc.levels)
    monkeypatch.delenv("HSM_EXACT_SPEC")
    g.setUpdateFactorFree(0.4)
    g.setUpdateFactorOccupied(0.9)
    g.build_map(sc.build_poses, sc.build_scans)
    g.synchronize()
    return g


def test_g_two_streams_do_not_share_speculative_scratch(capi, dense_case, monkeypatch):
    """two caller streams each launch 6 hypotheses of one 16k-beam scan, back to back, no sync between: both the reference's bits"""
    import torch
    sc, pts, hyp, want = dense_case
    g = _spec_ctx(capi, sc, monkeypatch)
    d_pts = torch.from_numpy(np.ascontiguousarray(pts)).to("cuda:0")
    d_hyp = torch.from_numpy(hyp).to("cuda:0")
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [Out(6), Out(6)]
    for rep in range(3):
        for k in range(2):
            outs[k].nan(streams[k])
        for k in range(2):
            g.match_batch_device(6, d_hyp[6 * k:].data_ptr(), d_pts.data_ptr(), 0, pts.shape[0], outs[k].pose.data_ptr(),
                                 outs[k].cov.data_ptr(), streams[k].cuda_stream)
            assert g.last_launch_config()["kernel"] == "gn_match_spec_kernel", g.last_launch_config()
        torch.cuda.synchronize()
        for k in range(2):
            pose, cov = outs[k].host()
            assert not np.isnan(pose).any() and not np.isnan(cov).any(), (rep, k)
            d = (bits(pose) != bits(want[6 * k:6 * k + 6])).any(1)
            assert not d.any(), f"round {rep}, stream {k}: {int(d.sum())} of 6 poses differ from the reference"
    g.close()


def test_h_first_speculative_launch_inside_a_capture(capi, dense_case, monkeypatch):
    """the context's first speculative launch is captured: no scratch is allocated under capture, the launch takes the literal
    dense form (the same bits); the replay is the reference's, and the eager launch after it takes the speculative form"""
    import torch
    sc, pts, hyp, want = dense_case
    g = _spec_ctx(capi, sc, monkeypatch)
    d_pts = torch.from_numpy(np.ascontiguousarray(pts)).to("cuda:0")
    d_hyp = torch.from_numpy(hyp).to("cuda:0")
    s = torch.cuda.Stream()
    out = Out(12)

    def launch():
        g.match_batch_device(12, d_hyp.data_ptr(), d_pts.data_ptr(), 0, pts.shape[0], out.pose.data_ptr(), out.cov.data_ptr(),
                             s.cuda_stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        launch()
    assert g.last_launch_config()["kernel"] == "gn_match_exact_dense_kernel", g.last_launch_config()
    out.nan()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    pose_g, cov_g = out.host()
    assert not np.isnan(cov_g).any()
    assert np.array_equal(bits(pose_g), bits(want))
    out.nan(s)
    launch()
    assert g.last_launch_config()["kernel"] == "gn_match_spec_kernel", g.last_launch_config()
    s.synchronize()
    check("eager speculative launch after the capture", out.host(), (pose_g, cov_g), want)
    del graph
    g.close()


# ---- the sort kernel, directly (hsm_debug_batch_order) --------------------------------------------------------------------------

def _part1by1_6(v):
    v = v & 0x3F
    v = (v | (v << 4)) & 0x30F
    v = (v | (v << 2)) & 0x333
    v = (v | (v << 1)) & 0x555
    return v


def key_candidates(g, begin):
    """per scan the tile keys the sort kernel may give it: float64 map coordinates with the kernel's clamping; a coordinate
    within 1e-3 cells of a tile border may fall on either side (the device's fp32 affine, possibly contracted)"""
    sx, sy, _, s = g.level_info(0)
    shift = 0
    while (64 << shift) < max(sx, sy):
        shift += 1
    t = g.getMapCoordsPose(0, np.zeros(3, np.float32)).astype(np.float64)  # (t0, t1): the affine's translation
    b = np.asarray(begin, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        # affine_apply: t + (l00 x + l01 y), l01 = l10 = 0 -- 0 * inf is NaN, as on the device
        m = np.stack([t[0] + (np.float64(s) * b[:, 0] + 0.0 * b[:, 1]), t[1] + (0.0 * b[:, 0] + np.float64(s) * b[:, 1])], 1)
    T = float(1 << shift)

    def tiles(c):
        out = []
        for d in (0.0, -1e-3, 1e-3):
            v = c + d
            cc = 0 if np.isnan(v) else int(min(max(v, 0.0), 1.0e6))
            out.append(min(cc >> shift, 63))
        return set(out)
    keys = []
    for mx, my in m:
        keys.append(sorted({_part1by1_6(tx) | (_part1by1_6(ty) << 1) for tx in tiles(mx) for ty in tiles(my)}))
    return keys, T


def assert_sorted_permutation(g, begin, perm):
    n = begin.shape[0]
    assert perm.shape == (n,)
    assert np.array_equal(np.sort(perm), np.arange(n)), "not a permutation of [0, batch)"
    keys, _ = key_candidates(g, begin)
    cur = -1
    for slot, i in enumerate(perm):
        ok = [k for k in keys[i] if k >= cur]
        assert ok, f"slot {slot}: scan {i} keys {keys[i]} after key {cur}"
        cur = min(ok)


def run_order(g, begin):
    import torch
    d_b = torch.from_numpy(np.ascontiguousarray(begin, np.float32)).to("cuda:0")
    d_p = torch.full((begin.shape[0],), -1, dtype=torch.int32, device="cuda:0")
    s = torch.cuda.Stream()
    g.debug_batch_order(begin.shape[0], d_b.data_ptr(), d_p.data_ptr(), s.cuda_stream)
    s.synchronize()
    return d_p.cpu().numpy()


@pytest.fixture(scope="module")
def order_ctx(capi):
    g = capi.MapRepMultiMap(0.05, 1024, 1024, 1)
    g.set_batch_order(capi.ORDER_MORTON)
    yield g
    g.close()


@pytest.mark.parametrize("n", [1024, 8191, 8192, 8193, 20000])
def test_sort_kernel_random_batches(capi, order_ctx, n):
    rng = np.random.default_rng(n)
    begin = np.zeros((n, 3), np.float32)
    begin[:, :2] = rng.uniform(-27.0, 27.0, (n, 2))  # (the 1024^2 map at 5 cm spans +-25.6 m: some starts off the map)
    begin[:, 2] = rng.uniform(-3, 3, n)
    perm = run_order(order_ctx, begin)
    assert_sorted_permutation(order_ctx, begin, perm)


@pytest.mark.parametrize("n", [1000, 1024, 8193])
def test_sort_kernel_one_tile(capi, order_ctx, n):
    """every scan in one tile: the one-key path of bin_take (a last wavefront part-filled for 1000 and 8193)"""
    rng = np.random.default_rng(n + 1)
    begin = np.zeros((n, 3), np.float32)
    begin[:, :2] = np.float32([3.31, -7.53]) + rng.uniform(0.0, 0.2, (n, 2)).astype(np.float32)  # inside one 16-cell tile
    keys, _ = key_candidates(order_ctx, begin)
    assert len({tuple(k) for k in keys}) == 1 and len(keys[0]) == 1
    perm = run_order(order_ctx, begin)
    assert_sorted_permutation(order_ctx, begin, perm)


def test_sort_kernel_nan_inf_and_far_starts(capi, order_ctx):
    rng = np.random.default_rng(11)
    n = 3000
    begin = np.zeros((n, 3), np.float32)
    begin[:, :2] = rng.uniform(-25.0, 25.0, (n, 2))
    special = [np.nan, np.inf, -np.inf, 1e30, -1e30, 3e5, -3e5]
    idx = rng.choice(n, 600, replace=False)
    for j, i in enumerate(idx):
        begin[i, j % 2] = special[j % len(special)]
        if j % 5 == 0:
            begin[i, 1 - j % 2] = special[(j // 5) % len(special)]
    perm = run_order(order_ctx, begin)
    assert_sorted_permutation(order_ctx, begin, perm)


def test_sort_kernel_auto_keeps_a_batch_in_map_order(capi):
    """HSM_ORDER_AUTO on a 4096^2 level 0: a batch that follows the map already gets the identity; one that does not, a sort"""
    g = capi.MapRepMultiMap(0.05, 4096, 4096, 1)
    assert g.batch_order() == capi.ORDER_AUTO
    rng = np.random.default_rng(5)
    n = 8192
    begin = np.zeros((n, 3), np.float32)
    begin[:, :2] = rng.uniform(-100.0, 100.0, (n, 2))
    keys, _ = key_candidates(g, begin)
    k = np.array([ks[0] for ks in keys])
    begin = begin[np.argsort(k, kind="stable")]
    perm = run_order(g, begin)
    assert np.array_equal(perm, np.arange(n))
    # a batch in few tiles (about 7 x 7 of 64 x 64 cells), shuffled: many more tile changes than tiles -- sorted
    shuffled = begin.copy()
    shuffled[:, :2] = rng.uniform(-10.0, 10.0, (n, 2))
    perm = run_order(g, shuffled)
    assert not np.array_equal(perm, np.arange(n))
    assert_sorted_permutation(g, shuffled, perm)
    g.close()
