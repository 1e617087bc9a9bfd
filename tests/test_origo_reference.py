"""The reference really depends on the container's origo, on the inputs the device tests of the per-scan origo entries use
(tests/origo_cases.py): with the unmodified reference ("hr") the 24-scan log is run twice through HectorSlamProcessor::update,
once with an origo per scan and once with origo[0] for every scan.  The final log-odds planes differ on every level, and at
both threshold pairs, (0.4, 0.13) and (1.0, 0.3), the gate integrates and rejects at least 6 scans each -- so a device entry
that ignored, mis-scaled or mis-retained an origo could not pass those tests.  The GPU tests call the same asserts.

These tests run the CPU checkers alone: they say something about the INPUTS, not about the library, and pass with or without
the per-scan origo entries.  The entries themselves are covered by tests/test_gpu_update_scans_origos.py,
tests/test_gpu_slam_ranges_tf.py, tests/test_origos_abi.py and tests/test_update_gate_origo_model.py."""
import numpy as np
import pytest

from conftest import oracle_kinds
import origo_cases as oc


@pytest.mark.parametrize("kind", ["hr", "ho"])
def test_planes_differ_on_every_level_and_the_gate_is_exercised(oracle_mod, kind):
    if kind not in oracle_kinds():
        pytest.skip("oracle/_ref not built (no reference tree where the suite was built)")
    r = oc.assert_the_reference_depends_on_the_origo(kind)
    print({k: (v.astype(int).tolist() if isinstance(v, np.ndarray) else v) for k, v in r.items()})


def test_origos_move_the_begin_cell_on_every_level():
    """+-0.3 m of mount translation: the truncated begin cell (int)(T * origo + 0.5) differs between scans on level 2 as well"""
    sc = oc.trajectory()
    assert sc.origos.shape == (oc.N, 2) and np.abs(sc.origos).max() <= 6.0 and np.abs(sc.origos).max() > 4.0
    for lvl in range(oc.LEVELS):
        cells = np.floor(sc.origos * np.float32(0.5 ** lvl) + np.float32(0.5))
        assert len({tuple(c) for c in cells}) >= 4, (lvl, cells)
