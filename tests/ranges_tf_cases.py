"""Inputs and references shared by the tests of the batched tf-path conversion (test_ranges_tf_batch_abi.py on the CPU,
test_gpu_ranges_tf_batch.py on the device): B raw scans of one geometry, a laser -> base transform per scan (or one for all),
and the reference node's own projectLaser + rosPointCloudToDataContainer per scan (`NodeRef.project_and_convert`)."""
import numpy as np

from test_node_rows import NODE_GATES, rigid_rows
from test_ranges_batch_abi import GEOM, synthetic_batch

A0, INC = float(GEOM[0]), float(GEOM[1])
# projectLaser's gate lies below the container's (laser_min_dist 0.4 / 0.25), so that beams reach the squared-distance gates
RANGE_MIN, RANGE_MAX = 0.1, 30.0
CUTOFFS = (30.0, -1.0)
NOTHING, EVERYTHING = 1, 2  # rows of a batch with B > 2: a scan that keeps no beam, a scan that keeps every beam
DROP_REASONS = ("projectLaser", "sqr_min", "sqr_max", "x<0 && d2<0.5", "z")


def batch(rng, B, n):
    """[B, n] ranges (inf, NaN, 0, values on both range gates) and [B, 12] transforms, a distinct tilted one per scan"""
    r = synthetic_batch(rng, B, n) if n else np.zeros((B, 0), np.float32)
    if B > 2 and n:
        r[NOTHING] = np.inf
        r[EVERYTHING] = 1.0  # inside every gate of NODE_GATES under any rigid_rows tilt (|z| <= 0.08, d2 = 1 > 0.5)
    T = np.stack([rigid_rows(rng) for _ in range(B)])
    return r, T


def rows_of(T, b):
    return T if T.ndim == 1 else T[b]


def node_reference(node, ranges, cutoff, T, scale):
    """the reference node per scan -> (counts, offsets, endpoints [total, 2], origos [B, 2], projected clouds)"""
    B, n = ranges.shape
    conts, origos, clouds = [], np.empty((B, 2), np.float32), []
    for b in range(B):
        pts, origos[b], cloud = node.project_and_convert(ranges[b], A0, INC, RANGE_MIN, RANGE_MAX, cutoff, rows_of(T, b), scale)
        conts.append(pts)
        clouds.append(cloud)
    counts = np.array([c.shape[0] for c in conts], np.int32)
    offsets = np.zeros(B + 1, np.int32)
    np.cumsum(counts, out=offsets[1:])
    pts = np.concatenate(conts).reshape(-1, 2) if B else np.zeros((0, 2), np.float32)
    return counts, offsets, pts, origos, clouds


def drop_census(gates, n, counts, clouds):
    """beams each reason removed, read off the oracle's own outputs: the projected cloud (what projectLaser kept) and the
    container (what the conversion kept of it).  The three fp32 gates are evaluated on the cloud's points as :519-526 does;
    whatever else is missing from the container fell to the z gate, the only one left."""
    c = dict.fromkeys(DROP_REASONS, 0)
    sqr_min, sqr_max = gate_args(gates)[:2]
    for cnt, cloud in zip(counts, clouds):
        c["projectLaser"] += n - cloud.shape[0]
        with np.errstate(invalid="ignore", over="ignore"):
            x = cloud[:, 0]
            d2 = x * x + cloud[:, 1] * cloud[:, 1]
            lo, hi = ~(d2 > sqr_min), ~(d2 < sqr_max) & (d2 > sqr_min)
            near = (x < 0) & (d2 < np.float32(0.5)) & ~lo & ~hi
        c["sqr_min"] += int(lo.sum())
        c["sqr_max"] += int(hi.sum())
        c["x<0 && d2<0.5"] += int(near.sum())
        c["z"] += cloud.shape[0] - int(lo.sum() + hi.sum() + near.sum()) - int(cnt)
    return c


def gate_args(gates):
    """(sqr_laser_min_dist, sqr_laser_max_dist, laser_z_min, laser_z_max) as the node makes them of its parameters: the two
    distances squared in double and narrowed to float (HectorMappingRos.cpp:95-100; NodeRef.sqr_min / sqr_max)"""
    return (np.float32(gates[0] * gates[0]), np.float32(gates[1] * gates[1]), gates[2], gates[3])


__all__ = ["NODE_GATES", "rigid_rows", "A0", "INC", "RANGE_MIN", "RANGE_MAX", "CUTOFFS", "NOTHING", "EVERYTHING", "DROP_REASONS",
           "batch", "rows_of", "node_reference", "drop_census", "gate_args"]
