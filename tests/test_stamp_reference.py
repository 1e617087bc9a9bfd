"""CPU pin of tests/stamp_cases.py, the inputs of tests/test_gpu_restored_stamps.py: levels restored with stamps at or ahead of
the update counter, then integrated.

  * the restatement ("ho") equals the reference headers compiled unmodified ("hr") bit for bit, log-odds and stamps, on every
    geometry, level, counter, case and beam order, after every scan; and stamp_cases' numpy statement of the reference's rule
    equals both (so the classes counted below are the reference's);
  * the inputs are not vacuous: per geometry, level and counter every class holds at least 8 cells that the scans touch --
    frozen (1 << 20), a stored free mark on a cell a beam ends in, a stored free mark on a cell that is only crossed, a stored
    occupied mark, cells that thaw inside the batch, cells at the 50.0 clamp with a stored free mark under an end;
  * the stamp-BLIND rule (map_update.h's header comment with the stored stamp ignored: what the apply passes did before they
    read the stamp) differs from the reference in at least one cell of every class, so the GPU tests cannot pass on kernels
    that ignore the stamp;
  * the same-context restore is exact (W scans, download, upload into the same checker, W more == 2 W scans), and the same
    planes uploaded into a fresh checker are NOT: the restored stamps lie ahead of its counter, which the upload leaves alone.

Measured here, level 0 / level 1 of both geometries: the blind rule differs from the reference in 277 / 89 .. 90 of the 319 /
106 .. 107 cells the single scan touches, and in 301 .. 304 / 102 .. 103 cells over the batch of 8; the smallest class (frozen,
stored occupied mark, stored free mark only crossed on level 1) holds 10 touched cells."""
import numpy as np
import pytest

import stamp_cases as sc
from conftest import bits

MIN_CELLS = 8
CASES = sc.SINGLE_CASES + ("batch",)


def both_kinds(oracle_mod):
    if not oracle_mod.available("hr"):
        pytest.skip("oracle/_ref not built")
    return ("ho", "hr")


def model_run(geom, U, lvl, poses_shifts, scans, blind):
    """stamp_cases' numpy update over the scans on one level -> ([(log-odds, stamps) after every scan], [touched masks])"""
    f, o = sc.log_odds_steps()
    lo, ui = sc.planes(geom, U)[lvl]
    snaps, touched = [], []
    for k, (shift, pts) in enumerate(zip(poses_shifts, scans)):
        ff, fo = sc.touches(geom, lvl, sc.map_pose(geom, lvl, shift), pts * np.float32(1.0 / 2 ** lvl))
        lo, ui = sc.model_update(lo, ui, ff, fo, len(pts), U + 3 * k + 1, f, o, blind)
        snaps.append((lo, ui))
        touched.append((ff < len(pts), fo < len(pts)))
    return snaps, touched


def differs(a, b):
    return (bits(a[0]) != bits(b[0])) | (a[1] != b[1])


def test_log_odds_steps_and_map_poses_are_the_checkers(oracle_mod):
    f, o = sc.log_odds_steps()
    for geom in sc.GEOMETRIES:
        c = sc.new_checker(oracle_mod, "ho", geom)
        sc.checker_update(c, sc.sensor_pose(geom), np.float32([[5.2, 0.1]]))
        lo = c.download_level(0)[0]
        assert set(bits(lo).ravel().tolist()) == {0, bits(f).item(), bits(o).item()}
        for lvl in range(sc.LEVELS):
            for shift in sc.BATCH_SHIFTS:
                got = c.map_coords_pose(lvl, sc.sensor_pose(geom, shift))
                assert np.array_equal(bits(got), bits(sc.map_pose(geom, lvl, shift))), (geom, lvl, shift, got)


@pytest.mark.parametrize("U", sc.COUNTERS)
@pytest.mark.parametrize("geom", sc.GEOMETRIES, ids=sc.gid)
def test_restatement_reference_and_numpy_rule_agree_after_every_scan(oracle_mod, geom, U):
    kinds = both_kinds(oracle_mod)
    for case in CASES:
        for order in sc.ORDERS:
            poses, scans = sc.case_scans(geom, case, order)
            snaps = {k: sc.run_checker(oracle_mod, k, geom, U, poses, scans)[1] for k in kinds}
            for lvl in range(sc.LEVELS):
                model = model_run(geom, U, lvl, sc.BATCH_SHIFTS, scans, blind=False)[0]
                for k in range(len(scans)):
                    for kind in kinds:
                        lo, ui = snaps[kind][k][lvl]
                        what = (sc.gid(geom), U, case, order, lvl, k, kind)
                        assert np.array_equal(ui, model[k][1]), what + ("stamps", int((ui != model[k][1]).sum()))
                        assert np.array_equal(bits(lo), bits(model[k][0])), what + ("log odds", int((bits(lo) != bits(model[k][0])).sum()))


@pytest.mark.parametrize("U", sc.COUNTERS)
@pytest.mark.parametrize("geom", sc.GEOMETRIES, ids=sc.gid)
def test_every_class_is_touched_and_the_stamp_blind_rule_misses_it(geom, U):
    """(the numpy rule is the reference's: the test above)"""
    for lvl in range(sc.LEVELS):
        lo0, ui0 = sc.planes(geom, U)[lvl]
        for order in sc.ORDERS:
            _, one = sc.case_scans(geom, "keyed", order)
            ref, touched = model_run(geom, U, lvl, sc.BATCH_SHIFTS, one, blind=False)
            blind, _ = model_run(geom, U, lvl, sc.BATCH_SHIFTS, one, blind=True)
            crossed, ended = touched[0]
            hit = crossed | ended
            classes = {
                "frozen": (ui0 == sc.FAR) & hit,
                "stored free mark, ended": (ui0 == U + 1) & ended,
                "stored free mark, only crossed": (ui0 == U + 1) & crossed & ~ended,
                "stored occupied mark": (ui0 == U + 2) & hit,
                "at the clamp, stored free mark, ended": (ui0 == U + 1) & ended & (lo0 >= np.float32(49.6)),
            }
            d = differs(ref[0], blind[0])
            _, many = sc.case_scans(geom, "batch", order)
            bref, btouched = model_run(geom, U, lvl, sc.BATCH_SHIFTS, many, blind=False)
            bblind, _ = model_run(geom, U, lvl, sc.BATCH_SHIFTS, many, blind=True)
            late = np.zeros_like(hit)
            for k in range(sc.M_THAW + 1, sc.BATCH):  # scans whose marks lie past the thaw stamps
                late |= btouched[k][0] | btouched[k][1]
            thaw = ((ui0 == U + 3 * sc.M_THAW + 1) | (ui0 == U + 3 * sc.M_THAW + 2)) & late
            thawed = thaw & (bref[-1][1] > U + 3 * sc.M_THAW + 2)  # ... and which one of them then wrote
            classes["thawing mid-batch"] = thawed
            dd = np.zeros_like(hit)
            for k in range(sc.BATCH):
                dd |= differs(bref[k], bblind[k])
            counts = {name: int(m.sum()) for name, m in classes.items()}
            print(sc.gid(geom), U, "level", lvl, order, counts, "blind differs:", int(d.sum()), "of", int(hit.sum()), "/ batch", int(dd.sum()))
            for name, m in classes.items():
                assert counts[name] >= MIN_CELLS, (sc.gid(geom), U, lvl, order, name, counts)
                miss = int((m & (dd if name == "thawing mid-batch" else d)).sum())
                assert miss >= 1, (sc.gid(geom), U, lvl, order, name, "the stamp-blind rule gives the reference's cells")
            # the stored-stamp unsetFree does not depend on the beam order; the in-scan revert does
            assert int(d.sum()) >= 8 * MIN_CELLS


@pytest.mark.parametrize("geom", sc.GEOMETRIES, ids=sc.gid)
def test_both_orders_tell_the_stored_unset_free_from_the_in_scan_revert(oracle_mod, geom):
    """cells with a stored free mark under an end give the same bits in both beam orders (unsetFree whatever came first); among
    the cells below the marks the orders differ somewhere (the in-scan revert next to -2, -4, -8)"""
    U = 0
    last = {order: sc.run_checker(oracle_mod, "ho", geom, U, *sc.case_scans(geom, "keyed", order))[1][-1] for order in sc.ORDERS}
    lo0, ui0 = sc.planes(geom, U)[0]
    d = bits(last["given"][0][0]) != bits(last["reversed"][0][0])
    assert not (d & (ui0 == U + 1)).any()
    assert (d & (ui0 < U + 1)).any()


@pytest.mark.parametrize("geom", sc.GEOMETRIES, ids=sc.gid)
def test_same_context_restore_is_exact_and_cross_context_restore_is_not(oracle_mod, geom):
    kinds = ["ho"] + (["hr"] if oracle_mod.available("hr") else [])
    poses, scans = sc.batch(geom)
    W = sc.BATCH // 2
    for kind in kinds:
        whole = sc.new_checker(oracle_mod, kind, geom)
        for k in range(2 * W):
            sc.checker_update(whole, poses[k], scans[k])
        half = sc.new_checker(oracle_mod, kind, geom)
        for k in range(W):
            sc.checker_update(half, poses[k], scans[k])
        saved = sc.snapshot(half)
        fresh = sc.new_checker(oracle_mod, kind, geom)
        for o in (half, fresh):
            for lvl, (lo, ui) in enumerate(saved):
                o.upload_level(lvl, lo, ui)
            for k in range(W, 2 * W):
                sc.checker_update(o, poses[k], scans[k])
        for lvl in range(sc.LEVELS):
            w, h, fr = whole.download_level(lvl), half.download_level(lvl), fresh.download_level(lvl)
            assert np.array_equal(bits(w[0]), bits(h[0])) and np.array_equal(w[1], h[1]), (kind, lvl, "same-context restore")
            # the fresh checker's counter is 0: the restored stamps (up to 3 W - 1) lie ahead of its marks
            assert int(saved[lvl][1].max()) == 3 * (W - 1) + 2
            assert differs(w, fr).sum() >= MIN_CELLS, (kind, lvl, "a cross-context restore equals the uninterrupted run")
