"""The CPU pin of the moved-entry cases (tests/moved_entry_cases.py): what makes the GPU comparison of
tests/test_gpu_moved_entries.py meaningful.  With both checkers (the restatement and, where it is built, the reference's own
headers):

* the composed loop -- match on the hint, Gate.walk, update_by_scan where the gate says so -- gives the bits of the reference's
  own HectorSlamProcessor::update x 8 on a checker that does not move: poses, covariances, decisions, planes.  The checker has
  no setter for lastMapUpdatePose, so proc_update cannot be carried over a move; this is what licenses the composed loop;
* the conditions of every case hold (moved_entry_cases.case_conditions asserts them) and both checkers agree on every case;
* the move matters: for every reader family the moved checker's answers differ from those of a checker at the OLD start with
  the UNSHIFTED planes -- a context whose move silently did nothing would fail the GPU test;
* for the device-side update the box of the second half's cells in new coordinates differs from the same cells' box in old
  coordinates and from its union with the first half's box -- a stale device box would show.
"""
import numpy as np
import pytest

import moved_entry_cases as mc
from conftest import bits, oracle_kinds
from support import same
from test_gpu_slam_scans_device import Gate

F = np.float32
KINDS = oracle_kinds()
MAPS = pytest.mark.parametrize("m", mc.MAPS, ids=[m.id for m in mc.MAPS])


def same_planes(a, b):
    return all(same(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))


FORMS = [(m, og) for m in mc.MAPS for og in (False, True)] + [(mc.M96, mc.RAW)]
FORM_IDS = ["%s-%s" % (m.id, {False: "origo_zero", True: "origo_per_scan", mc.RAW: "raw_log"}[og]) for m, og in FORMS]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m,origos", FORMS, ids=FORM_IDS)
def test_composed_loop_is_the_references_own_loop(oracle_mod, m, kind, origos):
    """raw_log: on the containers and origos the checker's own tf conversion makes of the raw scans"""
    t = mc.raw_trajectory(oracle_mod, kind, m) if origos == mc.RAW else mc.trajectory(oracle_mod, m)
    r = mc.run_case(oracle_mod, kind, m, None, origos)
    o = mc.old_checker(oracle_mod, kind, m)
    o.proc_set_thresholds(*t.thresholds)
    gate = Gate(o, t.thresholds)
    pose = t.world[0].copy()
    for k in range(mc.N_SCANS):
        hint = (pose + t.deltas[k]).astype(F)
        for c in dict.fromkeys((o.guard, o.o)):
            c.proc_update(t.scans[k], hint, t.origos[k] if origos else mc.ZERO2, False)
        pose, cov = o.proc_last_pose()
        assert same(pose, r["poses"][k]) and same(cov, r["covs"][k]), (m.id, kind, k, pose, r["poses"][k])
        assert bool(gate.walk(pose[None, :])[0]) == bool(r["flags"][k]), (m.id, kind, k)
    assert o.guard.undefined_reads() == 0
    assert same_planes(mc.levels_of(o, m.levels), r["ends"][-1]), (m.id, kind, "planes")
    assert same(gate.last, r["gate_last"]) and gate.count == r["gate_count"]
    o.close()


MOVED_FORMS = [(m, og, name) for m, og in FORMS for name in mc.moves_of(m)]
MOVED = [(m, name) for m in mc.MAPS for name in mc.moves_of(m)]


@pytest.mark.parametrize("m,origos,name", MOVED_FORMS, ids=["%s-%s" % (i, f[2]) for i, f in zip(np.repeat(FORM_IDS, [len(mc.moves_of(m)) for m, _ in FORMS]), MOVED_FORMS)])
def test_conditions_hold_and_the_checkers_agree(oracle_mod, m, origos, name):
    res = [mc.run_case(oracle_mod, kind, m, name, origos) for kind in KINDS]   # asserts the conditions of the case
    for other in res[1:]:
        assert same(other["poses"], res[0]["poses"]) and same(other["covs"], res[0]["covs"]), (m.id, name)
        assert np.array_equal(other["flags"], res[0]["flags"]), (m.id, name)
        assert all(same_planes(a, b) for a, b in zip(other["ends"], res[0]["ends"])), (m.id, name)
    if origos:   # an origo per scan is seen: by the update's cells
        assert not same_planes(res[0]["ends"][0], mc.run_case(oracle_mod, KINDS[0], m, name, False)["ends"][0]), (m.id, name)
    assert len(res[0]["ends"]) == 2 and not same_planes(res[0]["ends"][0], mc.sc.old_planes(oracle_mod, m))


def test_raw_log_converts_alike_and_every_scan_has_a_mount_of_its_own(oracle_mod):
    """the containers of the raw log: both checkers (and the reference's node source, where it is built) give the same end
    points and origos; beams are dropped, most are kept, no two scans share an origo, and the origo moves the begin cell"""
    m = mc.M96
    raw = mc.raw_log(oracle_mod, m)
    ts = [mc.raw_trajectory(oracle_mod, kind, m) for kind in KINDS]
    for other in ts[1:]:
        assert all(same(a, b) for a, b in zip(other.scans, ts[0].scans)) and same(other.origos, ts[0].origos)
    t = ts[0]
    counts = [len(c) for c in t.scans]
    assert all(mc.MAX_BEAMS // 2 <= c < mc.MAX_BEAMS for c in counts) and counts[3] < min(counts[:3]), counts
    assert len({tuple(bits(o)) for o in t.origos}) == mc.N_SCANS
    assert len({tuple(np.floor(o + F(0.5))) for o in t.origos}) >= 3
    plain = mc.trajectory(oracle_mod, m)
    assert all(len(a) != len(b) or not same(a, b) for a, b in zip(t.scans, plain.scans))
    if oracle_mod.available("node"):
        node = oracle_mod.NodeRef(*raw["node_gates"])
        assert (float(F(node.sqr_min)), float(F(node.sqr_max))) == raw["gates"][:2]
        scale = m.checker(oracle_mod, "ho").scale_to_map()
        for k in range(mc.N_SCANS):
            pts, origo, _ = node.project_and_convert(raw["ranges"][k], raw["a0"], raw["inc"], *raw["lim"], raw["rows"][k], scale)
            assert same(pts, t.scans[k]) and same(origo, t.origos[k]), k
        node.close()


@pytest.mark.parametrize("gated", (False, True), ids=("plain", "gated"))
@pytest.mark.parametrize("m,name", MOVED, ids=["%s-%s" % (m.id, name) for m, name in MOVED])
def test_given_pose_updates_agree_and_old_and_new_boxes_differ(oracle_mod, m, name, gated):
    res = [mc.posed_case(oracle_mod, kind, m, name, gated) for kind in KINDS]
    for other in res[1:]:
        assert same_planes(other["end"], res[0]["end"]) and same_planes(other["before"], res[0]["before"]), (m.id, name)
        assert np.array_equal(other["flags"], res[0]["flags"])
    r = res[0]
    new, old, first = r["box_new"][0], r["box_old"][0], r["box_first"][0]
    whole = [0, 0, m.dims(0)[0] - 1, m.dims(0)[1] - 1]
    assert new[2] >= new[0] and new != whole, (m.id, name, new)
    assert new != old, (m.id, name, "the update's box is the same in old and in new coordinates", new)
    assert new != mc.union_box(first, new), (m.id, name, "the first half's box lies inside the second half's", first, new)
    assert new != mc.union_box(first, old) and first[2] >= first[0]


@pytest.mark.parametrize("name", mc.READER_MOVES)
@MAPS
def test_readers_agree_and_the_move_matters(oracle_mod, m, name):
    res = [mc.expected_readers(oracle_mod, kind, m, name) for kind in KINDS]
    for other in res[1:]:
        for lvl in range(m.levels):
            for key in ("score", "states", "rays"):
                assert all(same_or_nan(a, b) for a, b in zip(other[key][lvl], res[0][key][lvl])), (m.id, name, key, lvl)
            assert all(same_or_nan(a, b) for a, b in zip(other["cov"][lvl], res[0]["cov"][lvl])), (m.id, name, "cov", lvl)
            for n in mc.WINDOW_LENS:
                assert all(same_or_nan(a, b) for a, b in zip(other["window"][lvl][n], res[0]["window"][lvl][n])), (m.id, name, lvl, n)
        assert np.array_equal(other["counts"], res[0]["counts"])
        assert all(same(a[0], b[0]) and same(a[1], b[1]) for a, b in zip(other["ranges_match"], res[0]["ranges_match"]))
        for key in ("scores", "index", "cand", "cov", "lh0", "best_pose"):
            assert same_or_nan(other["reloc"][key], res[0]["reloc"][key]), (m.id, name, "reloc", key)
    # the move matters: a checker at the OLD start with the UNSHIFTED planes answers otherwise, in every family, on level 0
    still = mc.expected_readers(oracle_mod, KINDS[0], m, name, o=mc.unmoved_checker(oracle_mod, KINDS[0], m), tag="unmoved")
    r = res[0]
    differs = {"window scores": not same_or_nan(r["window"][0][200][0], still["window"][0][200][0]),
               "score batch": not same_or_nan(r["score"][0][0], still["score"][0][0]),
               "likelihood states": not same_or_nan(r["states"][0][0], still["states"][0][0]),
               "residual states": not same_or_nan(r["states"][0][1], still["states"][0][1]),
               "ray distances": not same_or_nan(r["rays"][0][0], still["rays"][0][0])}
    if name == "one_left":   # one coarsest cell of the map is left: rays hit nothing and the states around the scan's pose read
        assert differs["score batch"] or differs["window scores"], (m.id, name, differs)   # cleared cells in either window
    else:
        assert all(differs.values()), (m.id, name, differs)
        # ... and on every coarser level at least entry_geometry_cases.MIN_SIDE cells high (on the 20 x 5 and 10 x 2 levels of the
        # deep map the scan's beams end off the level in either window): a stale transform there is one the readers see
        for lvl in [l for l in range(1, m.levels) if min(m.dims(l)) >= mc.egc.MIN_SIDE]:
            fam = {"score batch": (r["score"][lvl], still["score"][lvl]), "window scores": (r["window"][lvl][200], still["window"][lvl][200]),
                   "states": (r["states"][lvl], still["states"][lvl])}
            seen = {k: any(not same_or_nan(x, y) for x, y in zip(a, b)) for k, (a, b) in fam.items()}
            assert all(seen.values()) if lvl == 1 else any(seen.values()), (m.id, name, lvl, seen)


def same_or_nan(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != np.float32:
        return np.array_equal(a, b)
    return bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())
