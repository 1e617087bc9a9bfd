"""The driver parses the LAST stdout line of `bench.py`; round 4's line (24.6 KB) did not parse.  These tests pin the
formatter: a canned full record (round 4's own driver-like run, tests/golden/bench_record_r04.json) must come out as ONE
JSON object below 4 KB that round-trips and carries the contract keys, `roofline` and `cpu_baseline`."""
import io
import json
import os
import subprocess
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config", "roofline", "cpu_baseline", "details")


def canned():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "bench_record_r04.json")))


def test_compact_line_is_small_and_round_trips():
    rec = canned()
    assert len(json.dumps(rec)) > 20000  # the record that broke the driver's parser
    line = bench.compact_line(rec, "gpurun_out/bench_details.json")
    assert "\n" not in line and len(line) < 4096
    got = json.loads(line)
    for k in CONTRACT:
        assert k in got, k
    assert got["value"] == rec["value"] and got["ms_per_step"] == rec["ms_per_step"]
    assert got["config"]["workload"].startswith("configs[2]")
    for k in ("kernel", "kernel_ms", "bound", "achieved", "peak", "frac", "traffic"):
        assert k in got["roofline"], k
    assert abs(got["roofline"]["frac"] - got["roofline"]["achieved"] / got["roofline"]["peak"]) < 1e-9
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in got["cpu_baseline"], k


def test_compact_line_survives_oversized_fields():
    rec = canned()
    rec["config"]["workload"] = "w" * 5000
    rec["cpu_baseline"]["sample"] = "s" * 5000
    rec["roofline"]["counter_source"] = "c" * 5000
    rec["n_gpus"] = 2
    rec["ranks"] = {"per_rank_kernel_ms": [0.1] * 512}
    line = bench.compact_line(rec, "gpurun_out/bench_details_n2.json")
    assert len(line) < 4096
    got = json.loads(line)
    assert got["n_gpus"] == 2 and "ranks" not in got and got["details"].endswith("_n2.json")


def test_emit_prints_the_compact_line_last_and_writes_details(tmp_path, monkeypatch):
    rec = canned()
    det = tmp_path / "d" / "bench_details.json"
    monkeypatch.setenv("HSM_BENCH_DETAILS", str(det))
    monkeypatch.delenv("HSM_BENCH_CHILD", raising=False)
    buf = io.StringIO()
    with redirect_stdout(buf):
        print("noise before the line")
        bench.emit(rec)
    last = buf.getvalue().strip().splitlines()[-1]
    assert len(last) < 4096 and json.loads(last)["value"] == rec["value"]
    full = json.load(open(det))
    assert full["configs"] == rec["configs"] and full["roofline"]["valu"] == rec["roofline"]["valu"]  # nothing is lost, only moved


def test_child_legs_keep_the_full_record(monkeypatch):
    rec = canned()
    monkeypatch.setenv("HSM_BENCH_CHILD", "1")
    buf = io.StringIO()
    with redirect_stdout(buf):
        bench.emit(rec)
    assert json.loads(buf.getvalue().strip().splitlines()[-1]) == rec


def test_deferred_emit_holds_the_line_back(monkeypatch, tmp_path):
    """N > 1: the line of an extra workload is held until the process group is destroyed and the other ranks have exited
    (RCCL's printf banner would otherwise land behind it); emit() then prints it"""
    rec = canned()
    monkeypatch.setenv("HSM_BENCH_DETAILS", str(tmp_path / "d.json"))
    monkeypatch.delenv("HSM_BENCH_CHILD", raising=False)
    from hsm_bench import common
    common.defer_emit(True)
    buf = io.StringIO()
    try:
        with redirect_stdout(buf):
            bench.emit(rec)
        assert buf.getvalue() == "" and common._PENDING and common._PENDING[-1] is rec
    finally:
        common.defer_emit(False)
    with redirect_stdout(buf):
        common.emit_pending()
    assert not common._PENDING
    assert json.loads(buf.getvalue().strip().splitlines()[-1])["value"] == rec["value"]


def test_driver_entry_is_small():
    """bench.py is the driver's entry point and nothing else: arguments, self-launch of --gpus N, dispatch into hsm_bench/"""
    n = len(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py")).read().splitlines())
    assert n < 300, n


def test_plain_record_line_and_no_details_file(tmp_path, monkeypatch):
    """a plain run's record (no roofline, no CPU leg) still gives the contract keys; without --full no details file is written"""
    rec = {k: v for k, v in canned().items() if k not in ("roofline", "cpu_baseline", "fast_mode", "sustained", "configs")}
    monkeypatch.delenv("HSM_BENCH_DETAILS", raising=False)
    monkeypatch.delenv("HSM_BENCH_CHILD", raising=False)
    monkeypatch.chdir(tmp_path)
    from hsm_bench import common
    monkeypatch.setattr(common, "details_file", lambda out: str(tmp_path / "should_not_exist.json"))
    buf = io.StringIO()
    with redirect_stdout(buf):
        bench.emit(rec, details=False)
    got = json.loads(buf.getvalue().strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "ms_per_step", "higher_is_better", "dtype", "steps", "warmup"):
        assert got[k] == rec[k], k
    assert got["details"] is None and "roofline" not in got and "cpu_baseline" not in got
    assert not (tmp_path / "should_not_exist.json").exists()


def test_dump_outputs_writes_float_arrays(tmp_path):
    from hsm_bench.common import dump_outputs
    pose = np.arange(30, dtype=np.float32).reshape(10, 3)
    cov = np.arange(90, dtype=np.float32).reshape(10, 9)
    dump_outputs(str(tmp_path / "out"), pose=pose, covariance=cov)
    assert np.array_equal(np.load(tmp_path / "out" / "pose.npy"), pose)
    c = np.load(tmp_path / "out" / "covariance.npy")
    assert c.dtype == np.float32 and np.array_equal(c, cov)
    assert not (tmp_path / "out" / "sample_rows.npy").exists()


def test_dump_outputs_samples_the_same_rows_above_the_limit(tmp_path, monkeypatch):
    from hsm_bench import common
    monkeypatch.setattr(common, "DUMP_LIMIT", 4800)
    pose = np.random.default_rng(1).standard_normal((1000, 3)).astype(np.float32)
    cov = np.random.default_rng(2).standard_normal((1000, 9)).astype(np.float32)
    for d in ("a", "b"):
        common.dump_outputs(str(tmp_path / d), pose=pose, covariance=cov)
    rows = np.load(tmp_path / "a" / "sample_rows.npy").astype(np.int64)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total < 4800 + 3 * 256  # (+ the .npy headers)
    assert np.array_equal(np.load(tmp_path / "a" / "pose.npy"), pose[rows])
    assert np.array_equal(np.load(tmp_path / "a" / "covariance.npy"), cov[rows])
    for f in ("pose.npy", "covariance.npy", "sample_rows.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


@pytest.mark.gpu
def test_plain_run_times_k_steps_and_dumps_the_same_outputs_twice(tmp_path):
    """`bench.py --steps K --warmup W --dump-outputs DIR`: exactly K timed steps, no leg beside the headline, and two runs with the
    same arguments write bit-identical outputs of the last timed step"""
    B = 512
    lines = []
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", str(B),
                            "--dump-outputs", str(tmp_path / d)], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr[-2000:]
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
    for got in lines:
        assert got["steps"] == 3 and got["warmup"] == 1 and got["ms_per_step"] > 0 and got["value"] > 0
        assert "roofline" not in got and "cpu_baseline" not in got and got["details"] is None
    pose = np.load(tmp_path / "a" / "pose.npy")
    cov = np.load(tmp_path / "a" / "covariance.npy")
    assert pose.shape == (B, 3) and pose.dtype == np.float32 and np.isfinite(pose).all()
    assert cov.shape == (B, 9) and cov.dtype == np.float32 and np.isfinite(cov).all()
    assert np.array_equal(pose.view(np.uint32), np.load(tmp_path / "b" / "pose.npy").view(np.uint32))
    assert np.array_equal(cov.view(np.uint32), np.load(tmp_path / "b" / "covariance.npy").view(np.uint32))
    assert sorted(os.listdir(tmp_path)) == ["a", "b"]  # (nothing else written)
