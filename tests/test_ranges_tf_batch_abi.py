"""B raw LaserScans and a transform per scan through the node's default tf path (hsm_ingest_batch_ranges_tf_device,
hsm_match_batch_ranges_tf): the C ABI and the numpy statement of the batched conversion (synth.ranges_tf_to_csr) the GPU tests
fall back to.  No compute calls on a device: runs without a GPU."""
import numpy as np
import pytest

from conftest import bits
from support import check_symbols
import ranges_tf_cases as tc

NAMES = ("hsm_ingest_batch_ranges_tf_device", "hsm_match_batch_ranges_tf")
SHAPES = ((1, 1, 20.0), (7, 181, 20.0), (33, 1081, 20.0), (5, 1440, 10.0), (3, 0, 20.0))  # B, n, scale_to_map


def test_names_are_declared_bound_and_exported():
    from hector_slam_amd import capi
    check_symbols(NAMES)
    for method in ("ingest_batch_ranges_tf_device", "match_batch_ranges_tf"):
        assert callable(getattr(capi.MapRepMultiMap, method))


def test_numpy_statement_equals_the_reference_node_tf_path(oracle_mod):
    """synth.ranges_tf_to_csr -- counts, int32 offsets, endpoints and origos of B scans -- is, scan by scan and bit for bit, the
    reference node's projectLaser + rosPointCloudToDataContainer (HectorMappingRos.cpp compiled from its own source): a distinct
    tilted transform per scan and one for all, both cutoffs, both gate settings, inf / NaN / 0 / range-gate values included.
    The set is not vacuous: every drop reason removes a beam somewhere, beams survive, and the origos differ between scans."""
    from hector_slam_amd import synth
    if not oracle_mod.available("node"):
        pytest.skip("oracle/_ref/libhector_node_ref.so not built (no reference tree on this machine)")
    rng = np.random.default_rng(31)
    census = dict.fromkeys(tc.DROP_REASONS, 0)
    kept = 0
    for gates in tc.NODE_GATES:
        node = oracle_mod.NodeRef(*gates)
        ga = tc.gate_args(gates)
        assert (node.sqr_min, node.sqr_max) == (float(ga[0]), float(ga[1]))
        for B, n, scale in SHAPES:
            r, per_scan = tc.batch(rng, B, n)
            for T in (per_scan, tc.rigid_rows(rng)):
                for cutoff in tc.CUTOFFS:
                    rn, ro, rp, rg, clouds = tc.node_reference(node, r, cutoff, T, scale)
                    counts, offs, pts, origos = synth.ranges_tf_to_csr(r, tc.A0, tc.INC, tc.RANGE_MIN, tc.RANGE_MAX, cutoff, T, *ga,
                                                                        scale)
                    what = (gates, B, n, T.ndim, cutoff)
                    assert counts.dtype == np.int32 and offs.dtype == np.int32 and offs.shape == (B + 1,) and offs[0] == 0, what
                    assert pts.dtype == np.float32 and pts.shape == (offs[-1], 2) and origos.dtype == np.float32, what
                    assert np.array_equal(counts, rn) and np.array_equal(offs, ro), what
                    for b in range(B):
                        assert np.array_equal(bits(pts[offs[b]:offs[b + 1]]), bits(rp[ro[b]:ro[b + 1]])), (what, b)
                    assert np.array_equal(bits(origos), bits(rg)), what
                    # non-vacuity, on the oracle's outputs
                    if B > 2 and n:
                        assert rn[tc.NOTHING] == 0 and rn[tc.EVERYTHING] == n, what
                    if B > 1 and T.ndim == 2:
                        assert len({tuple(bits(o)) for o in rg}) == B, what
                    for k, v in tc.drop_census(gates, n, rn, clouds).items():
                        assert v >= 0, (what, k)
                        census[k] += v
                    kept += int(rn.sum())
        node.close()
    print("beams dropped per reason:", census, "kept:", kept)
    assert all(v > 0 for v in census.values()) and kept > 0, (census, kept)
