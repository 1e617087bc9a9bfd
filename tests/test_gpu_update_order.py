"""Every form of the map update on scans whose result depends on the ORDER of the beams (tests/order_cases.py), against the
sequential reference (OccGridMapBase.h:121-260) bit for bit.

The kernels rebuild the reference's beam order from atomicMax keys: a cell that a beam ends in is reverted first (lo + f - f)
iff a beam of LOWER index crossed it -- `(kBeamMask - kf) < (kBeamMask - ko)` in apply_box and in update_apply_dense_kernel
(map_update.h) -- and the end-cell passes combine runs of lanes before their atomics.  In fp32 the revert shows only where
lo + f leaves lo's binade, so these tests first put a disc of cells just above -2 (4 free-only updates) or -4 (9), then end
beams in cells that other beams of the same scan cross, in given, reversed and permuted order: the reference's own maps differ
between the orders in 112 .. 627 cells (pinned in tests/test_update_order_reference.py), so a kernel that reverts always, never,
by the wrong key or by the wrong beam of a run cannot match all of them.  `saturate` drives the same cells through the
`lo < 50.0f` clamp of every apply pass (23 occupied updates; 30 are run).

Forms: the keyed single-scan form (< 4096 beams) on rows of 128 and of 120 cells; the byte-map single-scan form (>= 4096 beams)
in both layouts, again with HSM_DENSE_BITS=0 and on rows of 120 cells; hsm_update_by_scans_device with the whole sequence in one
call (CSR, and the shared-scan form for the clear_fan run); hsm_update_by_scans_device_gated with every scan forced.

After EVERY update of the single-scan forms and after every call of the others: log-odds bits, update index and probability
plane of all levels equal to both CPU checkers, no mark left behind, the update counter right; at the end one exact-mode
matchData on a quad-layout context, pose and covariance bits equal to the checkers' (the texels)."""
import numpy as np
import pytest

import order_cases as oc
from conftest import bits, oracle_kinds
from support import capi, dev, new_context, single_update

pytestmark = pytest.mark.gpu

MIN_CELLS = 100


@pytest.fixture(scope="module")
def reference(oracle_mod):
    """(map, case, prior | "saturate", order) -> {checker kind: (the checker, its planes after every update)}; computed once
    per module and shared.  The checkers' maps are not changed afterwards (a match only refreshes the retained containers)."""
    cache = {}

    def get(map_name, case, prior, order="given"):
        key = (map_name, case, prior, order)
        if key not in cache:
            cell, scans = oc.saturate_sequence(case) if prior == "saturate" else oc.order_sequence(case, prior, order)
            cache[key] = {kind: oc.run_reference(oracle_mod, kind, map_name, cell, scans) for kind in oracle_kinds()}
        return cache[key]

    return get


def new_ctx(capi, map_name, layout="quad"):
    sx, sy = oc.MAPS[map_name]
    g = new_context(capi, oc.RES, sx, sy, oc.LEVELS, layout=layout, factors=(oc.FACTOR_FREE, oc.FACTOR_OCC))
    g.map_name = map_name
    return g


def device_update(g, pose, scans, shared=False, gated=False):
    """hsm_update_by_scans_device(_gated) on torch buffers: `scans` in ONE call from `pose` -- CSR, or (shared) the one scan
    scans[0] len(scans) times; gated: every scan forced.  Returns the buffers, which must outlive the update."""
    import torch
    s = torch.cuda.current_stream()
    n = len(scans)
    keep = [dev(np.repeat(np.asarray(pose, np.float32)[None, :], n, 0))]
    if shared:
        keep += [dev(scans[0]), None]
        d_offs, shared_n = 0, len(scans[0])
    else:
        offs = np.zeros(n + 1, np.int32)
        offs[1:] = np.cumsum([len(x) for x in scans])
        keep += [dev(np.concatenate(scans)), dev(offs)]
        d_offs, shared_n = keep[2].data_ptr(), 0
    max_beams = max(len(x) for x in scans)
    if gated:
        keep += [dev(np.ones(n, np.uint8)), torch.full((n,), -7, dtype=torch.int32, device="cuda:0")]
        g.update_by_scans_device_gated(n, keep[0].data_ptr(), keep[1].data_ptr(), d_offs, shared_n, max_beams, None, keep[3].data_ptr(),
                                       keep[4].data_ptr(), s.cuda_stream)
        g.synchronize()
        assert keep[4].cpu().numpy().tolist() == [1] * n, "a forced scan was not integrated"
    else:
        g.update_by_scans_device(n, keep[0].data_ptr(), keep[1].data_ptr(), d_offs, shared_n, max_beams, None, s.cuda_stream)
        g.synchronize()
    return keep


def planes(g):
    return [g.download_level(lvl) + (g.download_prob(lvl),) for lvl in range(oc.LEVELS)]


def assert_same_as_reference(oracle_mod, g, ref, n_updates, what):
    """g after n_updates updates against both checkers' planes after as many"""
    got = planes(g)
    for kind, (_, snaps) in ref.items():
        for lvl, (lo_g, ui_g, prob_g) in enumerate(got):
            lo_o, ui_o = snaps[n_updates - 1][lvl]
            assert np.array_equal(ui_g, ui_o), (what, n_updates, kind, lvl, "update index", int((ui_g != ui_o).sum()))
            assert np.array_equal(bits(lo_g), bits(lo_o)), (what, n_updates, kind, lvl, "log odds", int((bits(lo_g) != bits(lo_o)).sum()))
            _, prob = oracle_mod.libm_expf(lo_o.reshape(-1), kind)
            assert np.array_equal(bits(prob_g).reshape(-1), bits(prob)), (what, n_updates, kind, lvl, "probability")
    for lvl in range(oc.LEVELS):
        assert g.debug_marks_nonzero(lvl) == (0, 0), (what, n_updates, lvl)
        assert g.getUpdateIndex(lvl) == n_updates - 1, (what, lvl, g.getUpdateIndex(lvl))  # lastUpdateIndex starts at -1
    return got


def assert_same_planes(a, b, what):
    for lvl, (pa, pb) in enumerate(zip(a, b)):
        assert np.array_equal(pa[1], pb[1]) and np.array_equal(bits(pa[0]), bits(pb[0])) and np.array_equal(bits(pa[2]), bits(pb[2])), (what, lvl)


def assert_same_match(g, ref, cell, what, others=()):
    """one exact-mode matchData from next to the sensor: pose and covariance bits equal to the checkers' -- the matcher reads
    the texels the updates wrote.  `others`: contexts that must give the same bits."""
    pose = oc.sensor_pose(g.map_name, cell) + np.float32([0.02, -0.015, 0.01])
    pts = oc.mixed_subsample()
    pg, cg = g.matchData(pose, pts)
    assert np.isfinite(pg).all() and not np.array_equal(bits(pg), bits(pose)), (what, "the match did not move: it reads no texel", pg)
    for kind, (o, _) in ref.items():
        po, co = o.match(pose, pts)
        assert np.array_equal(bits(pg), bits(po)) and np.array_equal(bits(cg), bits(co)), (what, kind, pg, po)
    for h in others:
        ph, ch = h.matchData(pose, pts)
        assert np.array_equal(bits(pg), bits(ph)) and np.array_equal(bits(cg), bits(ch)), (what, "between contexts", pg, ph)


def assert_reference_has_teeth(reference, case, prior):
    """the reference's own maps differ between the orders (else every kernel that ignores the order would pass)"""
    last = {order: reference("main", case, prior, order)["ho"][1][-1] for order in oc.ORDERS}
    for order in oc.ORDERS[1:]:
        assert oc.cells_that_differ(last["given"], last[order]) >= MIN_CELLS, (case, prior, order)


def run_single_scan_forms(capi, oracle_mod, monkeypatch, reference, case, prior, order, what):
    """the sequence, scan by scan, through hsm_update_by_scan on: rows of 128 cells in both layouts, the same with the byte-map
    form switched off (scans of >= 4096 beams then take the keyed form), rows of 120 cells in both layouts.  Which form the
    library takes follows from the scan's length: the cases of >= 4096 beams take the byte-map form, the others the keyed one."""
    cell, scans = oc.saturate_sequence(case) if prior == "saturate" else oc.order_sequence(case, prior, order)
    ctxs = [new_ctx(capi, "main", "quad"), new_ctx(capi, "main", "plane")]
    monkeypatch.setenv("HSM_DENSE_BITS", "0")
    ctxs.append(new_ctx(capi, "main", "quad"))
    monkeypatch.delenv("HSM_DENSE_BITS")
    ctxs += [new_ctx(capi, "narrow", "quad"), new_ctx(capi, "narrow", "plane")]
    refs = {m: reference(m, case, prior, order) for m in oc.MAPS}
    for k, pts in enumerate(scans):
        got = []
        for i, g in enumerate(ctxs):
            single_update(capi, g, oc.sensor_pose(g.map_name, cell), pts)
            got.append(assert_same_as_reference(oracle_mod, g, refs[g.map_name], k + 1, (what, case, prior, order, "context", i)))
        assert_same_planes(got[0], got[1], (what, "quad / plane", k))
        assert_same_planes(got[0], got[2], (what, "byte-map form on / off", k))
        assert_same_planes(got[3], got[4], (what, "rows of 120 cells, quad / plane", k))
    assert_same_match(ctxs[0], refs["main"], cell, what, others=[ctxs[2]])
    assert_same_match(ctxs[3], refs["narrow"], cell, what)
    for g in ctxs:
        g.close()
    return refs


# ---- the order cases ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", oc.ORDERS)
@pytest.mark.parametrize("prior", oc.PRIORS)
@pytest.mark.parametrize("case", oc.KEYED_CASES)
def test_keyed_single_scan_form_keeps_the_beam_order(capi, oracle_mod, monkeypatch, reference, case, prior, order):
    assert len(oc.scan_of(case, order)) < oc.DENSE_MIN
    assert_reference_has_teeth(reference, case, prior)
    run_single_scan_forms(capi, oracle_mod, monkeypatch, reference, case, prior, order, "keyed")


@pytest.mark.parametrize("order", oc.ORDERS)
@pytest.mark.parametrize("prior", oc.PRIORS)
@pytest.mark.parametrize("case", oc.DENSE_CASES)
def test_dense_single_scan_forms_keep_the_beam_order(capi, oracle_mod, monkeypatch, reference, case, prior, order):
    assert len(oc.scan_of(case, order)) >= oc.DENSE_MIN
    assert_reference_has_teeth(reference, case, prior)
    run_single_scan_forms(capi, oracle_mod, monkeypatch, reference, case, prior, order, "dense")


@pytest.mark.parametrize("order", oc.ORDERS)
@pytest.mark.parametrize("prior", oc.PRIORS)
@pytest.mark.parametrize("case", oc.DENSE_CASES)
def test_scans_device_forms_keep_the_beam_order(capi, oracle_mod, reference, case, prior, order):
    """the whole sequence -- `prior` clear_fan scans, then the scan under test -- in ONE hsm_update_by_scans_device call (CSR);
    the clear_fan run as one shared-scan call and the scan under test behind it; the gated entry with every scan forced"""
    assert_reference_has_teeth(reference, case, prior)
    cell, scans = oc.order_sequence(case, prior, order)
    ref = reference("main", case, prior, order)
    what = ("scans_device", case, prior, order)
    csr, shared, gated = new_ctx(capi, "main"), new_ctx(capi, "main"), new_ctx(capi, "main")
    pose = oc.sensor_pose("main", cell)
    keep = [device_update(csr, pose, scans)]
    p_csr = assert_same_as_reference(oracle_mod, csr, ref, prior + 1, what + ("one CSR call",))
    keep.append(device_update(shared, pose, scans[:prior], shared=True))
    assert_same_as_reference(oracle_mod, shared, ref, prior, what + ("shared clear_fan run",))
    keep.append(device_update(shared, pose, scans[prior:]))
    p_shared = assert_same_as_reference(oracle_mod, shared, ref, prior + 1, what + ("shared run, then the scan",))
    keep.append(device_update(gated, pose, scans, gated=True))
    p_gated = assert_same_as_reference(oracle_mod, gated, ref, prior + 1, what + ("gated, every scan forced",))
    assert_same_planes(p_csr, p_shared, what + ("CSR / shared",))
    assert_same_planes(p_csr, p_gated, what + ("ungated / gated",))
    assert_same_match(csr, ref, cell, what, others=[shared, gated])
    del keep
    for g in (csr, shared, gated):
        g.close()


# ---- the 50.0 clamp -----------------------------------------------------------------------------------------------------------------
def assert_reference_reaches_the_clamp(ref):
    for kind, (_, snaps) in ref.items():
        assert len(snaps) == oc.N_SATURATE
        assert int((snaps[-1][0][0] >= 50.0).sum()) >= MIN_CELLS and int((snaps[21][0][0] >= 50.0).sum()) == 0, kind


@pytest.mark.parametrize("case", oc.DENSE_CASES + oc.KEYED_CASES)
def test_single_scan_forms_saturate_at_the_clamp(capi, oracle_mod, monkeypatch, reference, case):
    """the scan and its reverse in turn, 30 updates: every apply pass meets cells at and above 50.0 from the 23rd on"""
    refs = run_single_scan_forms(capi, oracle_mod, monkeypatch, reference, case, "saturate", "given", "saturate")
    for ref in refs.values():
        assert_reference_reaches_the_clamp(ref)


@pytest.mark.parametrize("case", oc.DENSE_CASES)
def test_scans_device_forms_saturate_at_the_clamp(capi, oracle_mod, reference, case):
    """the 30 updates as ONE hsm_update_by_scans_device call (update_apply_scan_kernel's clamp), ungated and gated"""
    cell, scans = oc.saturate_sequence(case)
    ref = reference("main", case, "saturate")
    assert_reference_reaches_the_clamp(ref)
    what = ("scans_device saturate", case)
    csr, gated = new_ctx(capi, "main"), new_ctx(capi, "main")
    pose = oc.sensor_pose("main", cell)
    keep = [device_update(csr, pose, scans), device_update(gated, pose, scans, gated=True)]
    p_csr = assert_same_as_reference(oracle_mod, csr, ref, oc.N_SATURATE, what + ("ungated",))
    p_gated = assert_same_as_reference(oracle_mod, gated, ref, oc.N_SATURATE, what + ("gated",))
    assert_same_planes(p_csr, p_gated, what)
    assert int((p_csr[0][0] >= 50.0).sum()) >= MIN_CELLS
    assert_same_match(csr, ref, cell, what, others=[gated])
    del keep
    for g in (csr, gated):
        g.close()
