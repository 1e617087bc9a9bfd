"""tests/group_cases.py holds what it says: every sequence contains the transition it is named for, every shard table sums to its
total, and nothing exceeds the size cap (a call gathers at most 64 scans, a sequence has at most 8 calls, a group 3 replicas).
No GPU: a later edit of the tables cannot quietly empty a sequence that tests/test_gpu_group_sequences.py runs."""
import numpy as np
import pytest

import group_cases as gc


def calls(name):
    return gc.SEQUENCES[name]["calls"]


def totals(name):
    return [sum(c.counts) for c in calls(name)]


def pairs(name):
    cs = calls(name)
    return list(zip(cs, cs[1:]))


def test_the_issue_s_sequences_are_all_there():
    assert sorted(gc.SEQUENCES) == sorted(["totals", "cov toggles", "root moves", "empty first", "shared scan", "mode switches", "empty scans"])
    assert gc.SEQUENCES_OF[gc.DIRECT] == list(gc.SEQUENCES) == gc.SEQUENCES_OF[gc.PEER]
    assert gc.SEQUENCES_OF[gc.RCCL] == ["totals", "cov toggles"]


@pytest.mark.parametrize("name", list(gc.SEQUENCES))
def test_size_cap_and_shard_tables(name):
    seq = gc.SEQUENCES[name]
    assert gc.REPLICAS == 3 and gc.MAX_ROWS == 64 and gc.MAX_CALLS == 8
    assert 1 <= len(seq["calls"]) <= gc.MAX_CALLS
    assert seq["form"] in ("csr", "shared", "holes")
    for k, c in enumerate(seq["calls"]):
        assert len(c.counts) == gc.REPLICAS and all(n >= 0 for n in c.counts), (name, k)
        assert 0 <= c.root < gc.REPLICAS and c.mode in (None, gc.DIRECT, gc.PEER), (name, k)
        first = gc.first_rows(c.counts)
        total = sum(c.counts)
        assert total <= gc.MAX_ROWS and first[-1] == total and np.array_equal(np.diff(first), c.counts), (name, k)
        idx, wrap = gc.call_rows(name, k)
        assert len(idx) == total and len({(i, w) for i, w in zip(idx, wrap)}) == total, (name, k, "two rows of a call alike")
        for world in (1, 2, 3, 4, 8):
            r = gc.reshard(c, world)
            assert len(r.counts) == world and sum(r.counts) == total and 0 <= r.root < world, (name, k, world)
            assert max(r.counts) - min(r.counts) <= 1 or world == gc.REPLICAS, (name, k, world)
        assert gc.reshard(c, gc.REPLICAS) is c


@pytest.mark.parametrize("name", list(gc.SEQUENCES))
def test_consecutive_calls_expect_other_rows(name):
    """a row that kept the previous call's value is not what this call expects there: over the rows both calls gather, the
    tables point at other entries"""
    for k in range(len(calls(name)) - 1):
        (a, wa), (b, wb) = gc.call_rows(name, k), gc.call_rows(name, k + 1)
        n = min(len(a), len(b))
        assert all((a[i], wa[i]) != (b[i], wb[i]) for i in range(n)), (name, k)


def test_totals_change_in_both_directions_and_reach_zero():
    t = totals("totals")
    assert t == [16, 48, 1, 0, 16, 64]
    assert any(b > a > 0 for a, b in zip(t, t[1:])) and any(0 < b < a for a, b in zip(t, t[1:]))  # blocks grow; exchanges remade smaller
    assert 0 in t and t[t.index(0) + 1] > 0                                                        # the early-out, and a call after it
    assert t[-1] == gc.MAX_ROWS and max(c.counts[r] for c in calls("totals") for r in range(3)) == 22
    assert all(c.root == 2 and c.want_cov for c in calls("totals"))
    # a replica whose shard grows past what an earlier gather left in its result block
    per = np.array([c.counts for c in calls("totals")])
    assert all((np.maximum.accumulate(per[:, r])[:-1] < per[1:, r]).any() for r in range(3))


def test_cov_toggles_make_drop_and_remake_the_covariance_exchange():
    cs = calls("cov toggles")
    assert [c.want_cov for c in cs] == [True, False, True, False, True, True]
    t = totals("cov toggles")
    assert t == [16, 16, 16, 21, 21, 16]
    # off and on again at one total (the exchange is kept); a total that changes WITHOUT a covariance (the pose exchange alone is
    # remade, the covariance one goes); the covariance back at the new total (made late); a total that changes with one
    assert any(not a.want_cov and b.want_cov and sum(a.counts) == sum(b.counts) for a, b in pairs("cov toggles"))
    assert any(not b.want_cov and sum(a.counts) != sum(b.counts) for a, b in pairs("cov toggles"))
    k = next(k for k, (a, b) in enumerate(pairs("cov toggles")) if not b.want_cov and sum(a.counts) != sum(b.counts))
    assert cs[k + 2].want_cov and t[k + 2] == t[k + 1]
    assert any(a.want_cov and b.want_cov and sum(a.counts) != sum(b.counts) for a, b in pairs("cov toggles"))


def test_root_moves_to_every_replica_and_back():
    cs = calls("root moves")
    assert [c.root for c in cs] == [2, 0, 1, 2, 1, 0]
    assert {c.root for c in cs} == {0, 1, 2}
    assert all(a.root != b.root for a, b in pairs("root moves"))
    assert len(set(totals("root moves"))) == 1            # the exchanges stay: only the root moves ...
    assert len({c.counts for c in cs}) == 2               # ... and once the shard offsets under it
    # every replica is the root first and a receiver of the all-gather afterwards
    for r in range(3):
        k = [c.root for c in cs].index(r)
        assert any(c.root != r for c in cs[k + 1:]), r


def test_empty_first_starts_with_an_empty_root_shard():
    cs = calls("empty first")
    assert cs[0].counts[cs[0].root] == 0 and sum(cs[0].counts) > 0
    assert [c.counts for c in cs] == [(0, 4, 0), (4, 0, 0), (0, 0, 4)] and [c.root for c in cs] == [0, 2, 2]
    # every replica matches for the first time in a call of its own, and is empty in another
    for r in range(3):
        assert sum(c.counts[r] > 0 for c in cs) == 1


def test_shared_scan_has_no_offsets_and_empty_shards():
    seq = gc.SEQUENCES["shared scan"]
    assert seq["form"] == "shared" and [c.counts for c in seq["calls"]] == [(7, 0, 9), (16, 0, 0), (5, 5, 6)]
    assert all(sum(c.counts) == 16 for c in seq["calls"])
    assert all(gc.SEQUENCES[n]["form"] != "shared" for n in gc.SEQUENCES if n != "shared scan")


def test_mode_switches_go_both_ways():
    cs = calls("mode switches")
    assert [(c.mode, sum(c.counts)) for c in cs] == [(gc.DIRECT, 16), (gc.PEER, 48), (gc.DIRECT, 48), (gc.DIRECT, 16), (gc.PEER, 16)]
    assert all(c.mode is None for n in gc.SEQUENCES if n != "mode switches" for c in calls(n))
    # back in direct mode at a total the exchanges were never shaped for: peer mode gathered it in between
    assert cs[1].mode == gc.PEER and cs[2].mode == gc.DIRECT and sum(cs[2].counts) != sum(cs[0].counts)


def test_empty_scans_sit_at_shard_edges_and_fill_one_shard():
    seq = gc.SEQUENCES["empty scans"]
    assert seq["form"] == "holes" and len(gc.HOLES["empty scans"]) == len(seq["calls"])
    for c, holes in zip(seq["calls"], gc.HOLES["empty scans"]):
        assert c.counts == (5, 5, 6)
        assert any(set(h) == set(range(n)) for h, n in zip(holes, c.counts))                       # a shard of empty scans only
        assert all(h and (0 in h or n - 1 in h) and max(h) < n for h, n in zip(holes, c.counts))  # first or last of every shard
        assert any(set(h) == {0} for h in holes) and any(set(h) == {n - 1} for h, n in zip(holes, c.counts))


def test_batches_are_what_the_tables_say():
    """call_batch on the scene: row counts, the wrap's other start estimate, the holes where HOLES puts them, one scan when shared"""
    sc = gc.make_scene()
    assert len(sc.query_scans) == gc.N_QUERY and sc.map_size == gc.MAP_SIZE and sc.levels == gc.LEVELS
    assert min(len(s) for s in sc.query_scans) > 0 and max(len(s) for s in sc.query_scans) <= gc.N_BEAMS
    for name, seq in gc.SEQUENCES.items():
        for k, c in enumerate(seq["calls"]):
            init, scans = gc.call_batch(sc, name, k)
            total = sum(c.counts)
            assert init.shape == (total, 3) and init.dtype == np.float32, (name, k)
            assert len({tuple(p) for p in init.tolist()}) == total, (name, k, "two rows start alike")
            if seq["form"] == "shared":
                assert scans is sc.query_scans[gc.SHARED_SCAN] and len(scans) == gc.N_BEAMS == 360  # shared_n, as the GPU test passes it
                continue
            assert len(scans) == total
            empty = {i for i, s in enumerate(scans) if len(s) == 0}
            if seq["form"] == "holes":
                first = gc.first_rows(c.counts)
                assert empty == {first[r] + j for r, rows in enumerate(gc.HOLES[name][k]) for j in rows}, (name, k)
            else:
                assert not empty, (name, k)


def test_slam_scene_has_the_scans_the_steps_need():
    world, poses, scans = gc.slam_scene()
    assert (gc.SLAM_SX, gc.SLAM_SY, gc.SLAM_LEVELS, gc.SLAM_START) == (320, 192, 4, (0.3, 0.6))
    assert len(scans) == len(poses) == gc.SLAM_STEPS >= 10 + 1 + 1 + 4 + 5
    assert min(len(s) for s in scans) > 100 and max(len(s) for s in scans) <= gc.N_BEAMS
