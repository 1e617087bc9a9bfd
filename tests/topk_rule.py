"""The ranking rule of hsm_select_topk_device, restated in numpy: the expected value of tests/test_gpu_window.py, itself tested
on hand-made arrays (tests/test_window_model.py).

The K best entries in rank order: a NaN never takes part; the higher score first; equal scores (compared as floats, so
+0 == -0) the lower index first.  Places that no entry fills are index -1, score NaN.
"""
import numpy as np

MAX_TOPK = 64


def topk(scores, k):
    """-> (index [k] int32, score [k] float32)"""
    s = np.ascontiguousarray(scores, np.float32).reshape(-1)
    keep = np.flatnonzero(~np.isnan(s))
    # a stable sort on -score keeps equal scores (-0.0 == +0.0 too: -(+0) and -(-0) compare equal) in index order
    order = keep[np.argsort(-s[keep].astype(np.float64), kind="stable")][:k]
    index = np.full(k, -1, np.int32)
    score = np.full(k, np.nan, np.float32)
    index[:order.size] = order
    score[:order.size] = s[order]
    return index, score


def topk_cases():
    """(name, scores) pairs: ties, signed zeros, NaNs, short and empty arrays, the sizes around a wavefront and a workgroup, and
    100 000 scores quantised to 16 values (every place decided by the index)"""
    rng = np.random.default_rng(2024)
    nan = np.float32(np.nan)
    yield "ties", np.array([0.5, 0.7, 0.7, 0.1, 0.7, 0.5, 0.9, 0.9], np.float32)
    yield "signed zeros", np.array([-0.0, 0.0, -1.0, 0.0, -0.0, 1.0], np.float32)
    yield "nans", np.array([nan, 0.3, nan, 0.8, 0.3, nan, -np.inf, np.inf], np.float32)
    yield "all nan", np.full(70, nan, np.float32)
    yield "count below k", np.array([0.25, 0.75, 0.5], np.float32)
    yield "empty", np.zeros(0, np.float32)
    for n in (1, 63, 64, 65, 257):
        a = rng.uniform(0, 1, n).astype(np.float32)
        a[rng.integers(0, n, n // 8)] = nan
        a[rng.integers(0, n, n // 4)] = np.float32(0.5)
        yield f"count {n}", a
    big = (rng.integers(0, 16, 100_000) / np.float32(16)).astype(np.float32)
    big[rng.integers(0, 100_000, 700)] = nan
    yield "100000 in 16 values", big
    descending = np.arange(20_000, 0, -1).astype(np.float32)  # the best 64 all in the first slice's first lanes
    yield "descending", descending
    yield "ascending", descending[::-1].copy()
