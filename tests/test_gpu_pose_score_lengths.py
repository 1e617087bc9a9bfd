"""Every scoring entry at the scan lengths where the shared residual walks of csrc/pose_score.h change path, on the MI355X.

The walks: a wavefront's rounds of 64 beams with a padded last round, a wavefront's lane-strided tree sum, and a lane's chain
unrolled by four with a tail.  The lengths: none, below the unroll (1, 3), the unroll (4), one beyond it (5), and one below, at
and one beyond one and two rounds (63, 64, 65, 128, 129).  The window has three poses, so the lane form's wavefront has 61
lanes behind the last hypothesis.

For every length the likelihood and the residual have the same bits -- compared as uint32, so that the NaN likelihood of the
empty scan takes part -- from hsm_score_window_device and hsm_score_windows_batch_device (all ten scans as one CSR batch), each
in lane and in wave form, from hsm_score_batch_device on the three window poses and, the likelihood, from
hsm_covariance_batch_device's out_lh; and those are the CPU reference's bits (the call test_gpu_window.py makes).  In
HSM_PARITY_FAST the batched score has the bits of the single-scan probe entry (hsm_likelihood_states / hsm_residual_states) and
the window entries keep the reference's.  Every output buffer is filled with a sentinel before a launch.

The likelihood of the empty scan is 1 - 0/0.  The sign of an invalid operation's NaN is the processor's choice: the reference,
compiled for x86-64, returns 0xffc00000 and the device's own arithmetic 0x7fc00000, so csrc/pose_score.h (scan_likelihood)
gives the empty scan the reference's bits.
"""
import numpy as np
import pytest

import window_cases
from conftest import bits, make_oracle, oracle_kinds
from support import capi, dev, layout_of, pack, stream_ptr
from test_gpu_relocalize_batch import KERNEL as BATCH_KERNEL, score_windows_batch
from test_gpu_window import KERNEL, SENTINEL, forced, gpu_for, oracle_window, score_batch, score_window

pytestmark = pytest.mark.gpu

LENS = (0, 1, 3, 4, 5, 63, 64, 65, 128, 129)
HALF, STEP = (1, 0, 0), window_cases.STEP  # 3 x 1 x 1
FORMS = ("lane", "wave")
LAYOUTS = ("quad", "plane")

_CASE = {}
_GOT = {}


def case(oracle_mod, sc):
    """centre, the three poses, the ten scans, a checker per kind and per kind the reference's (likelihood, residual) per length:
    computed once, shared by every test, never changed"""
    if not _CASE:
        centre = (sc.query_truth[0].astype(np.float32) + np.float32([0.03, -0.02, 0.01])).astype(np.float32)
        poses = window_cases.window_poses(centre, STEP, HALF)
        scans = [np.ascontiguousarray(sc.query_scans[0][:n], np.float32) for n in LENS]
        assert [len(s) for s in scans] == list(LENS)
        oracles = {kind: make_oracle(oracle_mod, kind, sc) for kind in oracle_kinds()}
        refs = {kind: [oracle_window(o, 0, poses, s) for s in scans] for kind, o in oracles.items()}
        _CASE.update(centre=centre, poses=poses, scans=scans, oracles=oracles, refs=refs)
    return _CASE


def covariance_lh(g, d_poses, pts):
    """out_lh of hsm_covariance_batch_device for the poses against one shared scan"""
    import torch
    d_pts = dev(np.asarray(pts, np.float32).reshape(-1, 2))
    out = torch.full((d_poses.shape[0],), SENTINEL, dtype=torch.float32, device="cuda:0")
    g.covariance_batch_device(0, d_poses.shape[0], d_poses.data_ptr(), d_pts.data_ptr() if len(pts) else 0, 0, len(pts), 0, 0, 0,
                              out.data_ptr(), stream_ptr())
    return out.cpu().numpy()


def device_scores(capi, monkeypatch, oracle_mod, sc, layout, parity):
    """entry -> per length (likelihood [3], residual [3] or None) in one layout and parity mode: launched once per (layout,
    parity), shared by the tests"""
    if (layout, parity) in _GOT:
        return _GOT[layout, parity]
    c = case(oracle_mod, sc)
    o = c["oracles"][oracle_kinds()[-1]]
    lib = capi.load_library()
    got = {}
    for form in FORMS:
        forced(monkeypatch, form)
        g = gpu_for(capi, sc, o, layout=layout_of(capi, layout))
        if parity is not None:
            g.set_parity(parity)
        got[f"window, {form}"] = []
        for scan in c["scans"]:
            got[f"window, {form}"].append(score_window(g, 0, c["centre"], STEP, HALF, scan))
            assert lib.hsm_last_launch_kernel(g._h) == KERNEL[form] and lib.hsm_last_launch_parity(g._h) == capi.PARITY_EXACT
        pts, offs = pack(c["scans"])
        lh, res = score_windows_batch(g, 0, np.tile(c["centre"], (len(LENS), 1)), STEP, HALF, pts, offs)
        assert lib.hsm_last_launch_kernel(g._h) == BATCH_KERNEL[form] and lib.hsm_last_launch_parity(g._h) == capi.PARITY_EXACT
        got[f"batched windows, {form}"] = [(lh[b], res[b]) for b in range(len(LENS))]
        if form == "wave":  # the entries that no window form reaches
            d_poses = dev(c["poses"])
            states = np.stack([o.map_coords_pose(0, p) for p in c["poses"]]).astype(np.float32)
            got["batched score"] = [score_batch(g, 0, d_poses, scan) for scan in c["scans"]]
            got["batched covariance"] = [(covariance_lh(g, d_poses, scan), None) for scan in c["scans"]]
            got["probe"] = [(g.likelihood_states(0, states, scan), g.residual_states(0, states, scan)) for scan in c["scans"]]
        g.close()
    for name, rows in got.items():
        for n, row in zip(LENS, rows):
            for v in row:
                if v is not None:
                    print(layout, parity, name, n, [hex(x) for x in bits(v)])
                    assert v.shape == (3,) and not (v == SENTINEL).any(), f"{name}, {n} beams: rows never written"
    _GOT[layout, parity] = got
    return got


def differing(got, names, anchor):
    """(entry, beams, output) wherever an entry's bits are not the anchor entry's"""
    bad = []
    for name in names:
        for n, row, want in zip(LENS, got[name], got[anchor]):
            for k, what in enumerate(("likelihood", "residual")):
                if row[k] is not None and not np.array_equal(bits(row[k]), bits(want[k])):
                    bad.append((name, n, what, [hex(x) for x in bits(row[k])], [hex(x) for x in bits(want[k])]))
    return bad


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_entry_gives_the_same_bits(capi, oracle_mod, small_scene, monkeypatch, layout):
    got = device_scores(capi, monkeypatch, oracle_mod, small_scene, layout, None)
    names = ("window, wave", "batched windows, lane", "batched windows, wave", "batched score", "batched covariance", "probe")
    bad = differing(got, names, "window, lane")
    assert not bad, bad
    assert len({tuple(bits(row[1])) for row in got["window, lane"]}) == len(LENS)  # the lengths do differ in their sums


@pytest.mark.parametrize("n", LENS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_entries_have_the_reference_bits(capi, oracle_mod, small_scene, monkeypatch, layout, n):
    """the lane form of the single window against the checkers; the other entries: test_every_entry_gives_the_same_bits"""
    got = device_scores(capi, monkeypatch, oracle_mod, small_scene, layout, None)["window, lane"][LENS.index(n)]
    for kind, refs in case(oracle_mod, small_scene)["refs"].items():
        ref = refs[LENS.index(n)]
        assert np.array_equal(bits(got[1]), bits(ref[1])), (kind, "residual", got[1], ref[1])
        assert np.array_equal(bits(got[0]), bits(ref[0])), (kind, "likelihood", [hex(x) for x in bits(got[0])],
                                                            [hex(x) for x in bits(ref[0])])
    if n == 0:
        assert (bits(got[1]) == 0).all()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_fast_parity_keeps_the_probes_tree_bits_and_the_windows_order(capi, oracle_mod, small_scene, monkeypatch, layout):
    exact = device_scores(capi, monkeypatch, oracle_mod, small_scene, layout, None)
    fast = device_scores(capi, monkeypatch, oracle_mod, small_scene, layout, capi.PARITY_FAST)
    bad = differing(fast, ("batched score",), "probe")
    assert not bad, bad
    windows = ("window, lane", "window, wave", "batched windows, lane", "batched windows, wave")
    bad = differing({**{name: fast[name] for name in windows}, "reference order": exact["window, lane"]}, windows, "reference order")
    assert not bad, bad
