"""B raw LaserScans in, B poses out (hsm_match_batch_ranges*): the C ABI, the workspace arithmetic and the numpy statement of
the batched conversion the GPU tests hold the device to.  No compute calls on a device: runs without a GPU."""
import numpy as np
import pytest

from conftest import bits
from support import check_symbols

NAMES = ("hsm_match_batch_ranges_device", "hsm_match_batch_ranges_workspace", "hsm_match_batch_ranges")
INT_MAX = 2**31 - 1
GEOM = (np.float32(-2.35619449), np.float32(0.00436332), np.float32(0.4), np.float32(30.0))  # angle_min, increment, range gate


def synthetic_batch(rng, B, n, lo=0.0, hi=35.0):
    """[B, n] ranges with what a driver produces sprinkled in: inf, NaN, 0 and values exactly on both gates"""
    r = rng.uniform(lo, hi, (B, n)).astype(np.float32)
    for b in range(B):
        idx = rng.choice(n, size=max(n // 10, 1), replace=False)
        r[b, idx[0::5]] = np.inf
        r[b, idx[1::5]] = np.nan
        r[b, idx[2::5]] = 0.0
        r[b, idx[3::5]] = GEOM[2]                         # range_min itself: dropped (strict)
        r[b, idx[4::5]] = GEOM[3] - np.float32(0.1)       # range_max - 0.1f itself: dropped (strict)
    return r


def test_names_are_declared_bound_and_exported():
    check_symbols(NAMES, restype=r"(int|size_t)")  # the workspace size is a size_t


def test_workspace_covers_the_csr_container_and_grows_with_the_batch():
    from hector_slam_amd import capi
    ws = capi.match_batch_ranges_workspace
    for B in (0, 1, 5, 257, 4096, 4097):
        for n in (0, 1, 181, 1081, 1440):
            w = ws(B, n)
            assert w >= 8 * B * n + 4 * (B + 1), (B, n, w)
            assert w >= 8, (B, n)  # one endpoint even when every scan is empty
            assert ws(B + 1, n) >= w and ws(B, n + 1) >= w, (B, n)
    assert capi.MapRepMultiMap.match_batch_ranges_workspace(4096, 1081) == ws(4096, 1081)


def test_workspace_is_zero_for_sizes_the_entry_refuses():
    from hector_slam_amd import capi
    ws = capi.match_batch_ranges_workspace
    assert ws(-1, 1081) == 0 and ws(4096, -1) == 0 and ws(-1, -1) == 0
    assert ws(2, INT_MAX // 2 + 1) == 0           # B * n > INT_MAX (int32 CSR offsets)
    assert ws(INT_MAX // 1081 + 1, 1081) == 0
    assert ws(INT_MAX // 1081, 1081) > 0
    assert ws(1, 1048575) > 0 and ws(1, 1048576) == 0  # HSM_MAX_UPDATE_BEAMS


def test_workspace_needs_no_device():
    """pure host arithmetic: the same answer whether or not a device is present (here: none is touched)"""
    from hector_slam_amd import capi
    lib = capi.load_library()
    assert lib.hsm_match_batch_ranges_workspace(4096, 1081) == capi.match_batch_ranges_workspace(4096, 1081)


def test_numpy_csr_statement_equals_the_reference_node_conversion(oracle_mod):
    """synth.ranges_to_csr -- counts, int32 offsets and endpoints of B scans -- is, scan by scan, the reference's
    rosLaserScanToDataContainer (the node compiled from its own source, "hr"), inf / NaN / 0 / both gates included"""
    from hector_slam_amd import synth
    if not oracle_mod.available("hr"):
        pytest.skip("oracle/_ref not built (no reference tree on this machine)")
    o = oracle_mod.Oracle("hr", 0.05, 64, 64, 1)
    rng = np.random.default_rng(11)
    a0, inc, rmin, rmax = GEOM
    for B, n, scale in ((1, 1, 20.0), (7, 181, 20.0), (33, 1081, 20.0), (5, 1440, 10.0), (3, 0, 20.0)):
        r = synthetic_batch(rng, B, n) if n else np.zeros((B, 0), np.float32)
        if B > 2 and n:
            r[1] = np.inf        # a scan that keeps nothing
            r[2] = 10.0          # a scan that keeps everything
        counts, offs, pts = synth.ranges_to_csr(r, a0, inc, rmin, rmax, scale)
        assert counts.dtype == np.int32 and offs.dtype == np.int32 and offs.shape == (B + 1,) and offs[0] == 0
        assert np.array_equal(np.diff(offs), counts) and pts.shape == (offs[-1], 2)
        for b in range(B):
            ref = o.laser_scan_to_container(r[b], a0, inc, rmin, rmax, scale)
            assert counts[b] == ref.shape[0], (B, n, b)
            assert np.array_equal(bits(pts[offs[b]:offs[b + 1]]), bits(ref)), (B, n, b)
        if B > 2 and n:
            assert counts[1] == 0 and counts[2] == n
