"""The movement gate of HectorSlamProcessor::update (hector_slam_amd/csrc/update_gate.h: util::poseDifferenceLargerThan in the
reference's fp32 / fp64 mix, and the sequential walk over a log of poses that the device's gate kernel runs in one lane) on the
CPU: tests/cpp/update_gate_model.cpp compiles the header with the host compiler alone, and every decision is compared with
`Oracle.pose_difference_larger_than` of both checker kinds ("hr": the unmodified UtilFunctions.h, where its library is present).
Decisions are booleans: equal or not, no tolerance."""
import subprocess

import numpy as np
import pytest

from conftest import oracle_kinds
from support import build_check

FLT_MAX = np.finfo(np.float32).max
DEFAULTS = (0.4, 0.13)  # HectorSlamProcessor.h:62-63


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return build_check(tmp_path_factory.mktemp("gate"), "update_gate_model.cpp")


@pytest.fixture(scope="module")
def checkers(oracle_mod):
    refs = {kind: oracle_mod.Oracle(kind, 0.05, 64, 64, 1) for kind in oracle_kinds()}
    yield refs
    for o in refs.values():
        o.close()


def run_pred(model, tmp_path, cases):
    cases = np.ascontiguousarray(cases, np.float32).reshape(-1, 8)
    src, dst = tmp_path / "cases.bin", tmp_path / "out.bin"
    cases.tofile(src)
    subprocess.run([str(model), "pred", str(src), str(dst)], check=True)
    out = np.fromfile(dst, np.uint8)
    assert out.size == len(cases)
    return out.astype(bool)


def run_walk(model, tmp_path, thresholds, poses, force):
    poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 3)
    rec = np.zeros(len(poses), np.dtype([("pose", np.float32, 3), ("force", np.int32)]))
    rec["pose"], rec["force"] = poses, np.asarray(force, np.int32)
    src, dst = tmp_path / "walk.bin", tmp_path / "walk_out.bin"
    with open(src, "wb") as f:
        f.write(np.float32(thresholds).tobytes())
        f.write(rec.tobytes())
    subprocess.run([str(model), "walk", str(src), str(dst)], check=True)
    raw = open(dst, "rb").read()
    n = len(poses)
    assert len(raw) == 8 * n + 16
    steps = np.frombuffer(raw[:8 * n], np.int32).reshape(n, 2)
    return steps[:, 0].astype(bool), steps[:, 1], np.frombuffer(raw[8 * n:8 * n + 12], np.float32), int(np.frombuffer(raw[8 * n + 12:], np.int32)[0])


def check_cases(model, tmp_path, checkers, cases, what):
    cases = np.ascontiguousarray(cases, np.float32).reshape(-1, 8)
    got = run_pred(model, tmp_path, cases)
    for kind, o in checkers.items():
        want = np.array([o.pose_difference_larger_than(c[:3], c[3:6], float(c[6]), float(c[7])) for c in cases])
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (what, kind, bad.size, cases[bad[:5]].tolist())
    return got


def case(p1, p2=(0, 0, 0), thr=DEFAULTS):
    return list(p1) + list(p2) + list(thr)


def test_the_cases_the_reference_was_queried_on(model, tmp_path, checkers):
    table = [(0.1, False), (0.5, True), (-0.5, True), (1.2, True), (3.0, True), (6.2, False), (-6.2, False)]
    got = check_cases(model, tmp_path, checkers, [case((0, 0, a)) for a, _ in table], "table")
    assert got.tolist() == [w for _, w in table]
    nan = np.nan
    others = [(case((0.3, 0.3, 0)), True),
              (case((1.5, -2.0, 0.3), (FLT_MAX, FLT_MAX, FLT_MAX)), True),   # the squared distance overflows to infinity
              (case((0, 0, 0), (FLT_MAX, FLT_MAX, FLT_MAX)), True),
              (case((nan, 0, 0)), False), (case((0, 0, nan)), False),          # a NaN compares false: that test never fires ...
              (case((nan, nan, nan), (FLT_MAX, FLT_MAX, FLT_MAX)), False),      # ... so an all-NaN pose is never "larger",
              (case((nan, 0, 0), (FLT_MAX, FLT_MAX, FLT_MAX)), True), (case((5.0, 5.0, nan), (0, 0, 0)), True),  # the OTHER test still can
              (case((0, nan, 3.0)), True), (case((0, 0, 0), (0, 0, nan)), False)]
    got = check_cases(model, tmp_path, checkers, [c for c, _ in others], "further cases")
    assert got.tolist() == [w for _, w in others]


def test_wrap_boundaries_and_thresholds(model, tmp_path, checkers):
    pi = np.float32(np.pi)
    around = []
    for centre in (pi, -pi, np.float32(2 * np.pi), np.float32(-2 * np.pi), np.float32(0.13), np.float32(-0.13), np.float32(0.4)):
        lo, hi = np.nextafter(centre, np.float32(-np.inf)), np.nextafter(centre, np.float32(np.inf))
        around += [lo, centre, hi, np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))]
    thresholds = [(0.0, 0.0), DEFAULTS, (1.0, 0.3), (0.4, np.float32(2 * np.pi) - pi), (np.inf, np.inf), (-1.0, -1.0)]
    cases = []
    for thr in thresholds:
        for a in around:
            cases += [case((0, 0, a), thr=thr), case((0, 0, 0), (0, 0, a), thr), case((0, 0, a), (0, 0, -a), thr),
                      case((a, 0, 0), thr=thr), case((0, a, 0), (0, 0, 0), thr), case((1, 1, a + np.float32(1.0)), (1, 1, 1.0), thr)]
        # distances at the threshold: 3-4-5 triangles scaled so that the norm lands on it, and one ulp either side
        d = np.float32(thr[0]) if np.isfinite(thr[0]) and thr[0] > 0 else np.float32(0.4)
        for s in (np.nextafter(d, np.float32(0)), d, np.nextafter(d, np.float32(9))):
            cases += [case((np.float32(0.6) * s, np.float32(0.8) * s, 0), thr=thr), case((s, 0, 0), thr=thr), case((0, -s, 0), thr=thr)]
        cases += [case((0, 0, 0), thr=thr), case((1e-30, 1e-30, 0), thr=thr), case((1e-23, 0, 0), thr=thr),  # products that underflow
                  case((1e20, 1e20, 0), thr=thr), case((np.inf, 0, 0), thr=thr), case((np.inf, 0, 0), (np.inf, 0, 0), thr),
                  case((0, 0, np.inf), thr=thr), case((0, 0, -np.inf), thr=thr), case((0, 0, 100.0), thr=thr)]
    got = check_cases(model, tmp_path, checkers, cases, "boundaries")
    assert got.any() and not got.all()


def test_ten_thousand_seeded_pairs(model, tmp_path, checkers):
    rng = np.random.default_rng(20261017)
    n = 10000
    p2 = np.concatenate([rng.normal(0, 3, (n, 2)), rng.uniform(-7, 7, (n, 1))], axis=1).astype(np.float32)
    # differences on the scale of the thresholds (half of them), and anywhere (the other half)
    near = np.concatenate([rng.normal(0, 0.3, (n, 2)), rng.normal(0, 0.15, (n, 1))], axis=1)
    far = np.concatenate([rng.normal(0, 2, (n, 2)), rng.uniform(-14, 14, (n, 1))], axis=1)
    diff = np.where((np.arange(n) % 2 == 0)[:, None], near, far)
    wrap = (rng.integers(0, 4, n) == 0) * rng.choice([-2 * np.pi, 2 * np.pi], n)  # a quarter wrapped by a turn
    diff[:, 2] += wrap
    p1 = (p2 + diff).astype(np.float32)
    thr = np.float32([(0.0, 0.0), DEFAULTS, (1.0, 0.3), (0.05, 3.0)])[rng.integers(0, 4, n)]
    got = check_cases(model, tmp_path, checkers, np.concatenate([p1, p2, thr], axis=1), "random pairs")
    assert 0.2 < got.mean() < 0.95, got.mean()  # both outcomes are well represented


@pytest.mark.parametrize("thresholds", [DEFAULTS, (1.0, 0.3), (0.0, 0.0)])
def test_sequential_walk_against_a_loop_over_the_checkers_predicate(model, tmp_path, checkers, thresholds):
    rng = np.random.default_rng(7)
    n = 2000
    steps = np.concatenate([rng.normal(0.05, 0.08, (n, 2)), rng.normal(0.0, 0.04, (n, 1))], axis=1)
    poses = np.cumsum(steps, axis=0).astype(np.float32)
    poses[:, 2] = ((poses[:, 2] * 8 + np.pi) % (2 * np.pi) - np.pi).astype(np.float32)  # headings that cross +-pi
    poses[100] = [np.nan, np.nan, np.nan]
    poses[101, 2] = np.nan
    poses[300] = [np.inf, 1.0, 0.5]
    poses[301] = poses[299]
    force = (rng.integers(0, 25, n) == 0).astype(np.int32)
    force[[0, 100, 300]] = 0
    force[700] = 1
    poses[700] = [np.nan, np.nan, np.nan]  # forced: integrated, and lastMapUpdatePose becomes NaN -- nothing passes until the next forced scan
    flags, ranks, last, applied = run_walk(model, tmp_path, thresholds, poses, force)
    for kind, o in checkers.items():
        state, count = np.float32([FLT_MAX] * 3), 0
        for k in range(n):
            go = o.pose_difference_larger_than(poses[k], state, thresholds[0], thresholds[1]) or bool(force[k])
            assert ranks[k] == count and bool(flags[k]) == go, (kind, k, poses[k], state, ranks[k], count)
            if go:
                state, count = poses[k].copy(), count + 1
        assert count == applied and np.array_equal(last.view(np.uint32), state.view(np.uint32)), (kind, applied, count)
    assert flags[0] and not flags[100] and flags[700] and not flags[701:].all()
    if thresholds != (0.0, 0.0):
        assert 0.05 < flags.mean() < 0.95
