"""A window of pose hypotheses (hector_slam_amd/csrc/window_grid.h) restated in numpy fp32, the windows the tests use, and the
committed relocalisation case.

Hypothesis w = (k*(2hy+1) + j)*(2hx+1) + i of a window with centre c, steps s and half-extents h, every operation rounded once
to fp32:  x = cx + float(i - hx) * sx,  y = cy + float(j - hy) * sy,  theta = ctheta + float(k - ht) * stheta.
"""
import numpy as np

# (hx, hy, ht): 105 hypotheses (a ragged last wavefront, rows of 7 that straddle lanes), one, a row, a fan of headings
WINDOWS = ((3, 2, 1), (0, 0, 0), (40, 0, 0), (0, 0, 5))
STEP = (0.05, 0.07, 0.013)


def window_count(half):
    hx, hy, ht = half
    return (2 * hx + 1) * (2 * hy + 1) * (2 * ht + 1)


def window_ijk(half, w):
    hx, hy, ht = half
    w = np.asarray(w, np.int64)
    nx, ny = 2 * hx + 1, 2 * hy + 1
    return w % nx, (w // nx) % ny, w // (nx * ny)


def window_poses(center, step, half, index=None):
    """[count, 3] float32 world poses of the window indices `index` (None: the whole window); NaN rows for indices outside"""
    c = np.asarray(center, np.float32)
    s = np.asarray(step, np.float32)
    W = window_count(half)
    w = np.arange(W) if index is None else np.asarray(index, np.int64)
    ok = (w >= 0) & (w < W)
    ijk = window_ijk(half, np.where(ok, w, 0))
    out = np.empty((w.size, 3), np.float32)
    for a in range(3):
        d = (ijk[a] - half[a]).astype(np.float32)
        out[:, a] = c[a] + d * s[a]  # float32 * float32 and float32 + float32: one rounding each
    out[~ok] = np.nan
    return out


# ---- the committed relocalisation case (tests/test_window_model.py chooses nothing at run time: it checks these) ----------------
# conftest.pyramid_scene, query scan RELOC_QUERY from its true pose; the window's centre is the truth displaced by RELOC_OFFSET,
# beyond the matcher's basin: the reference's match from the centre ends more than 0.2 m or 0.1 rad from the truth, the reference
# composition over the window (coarsest level, K = 8) ends within one level-0 cell and 0.02 rad of it -- and its winner is the
# seventh candidate of the coarse level, not the first.
RELOC_QUERY = 3
RELOC_OFFSET = (-1.0, 0.6, 0.45)
RELOC_STEP = (0.2, 0.2, 0.05)   # the coarsest level's cell (0.05 m * 4) and about three degrees
RELOC_HALF = (7, 7, 12)          # +-1.4 m, +-0.6 rad: 15 * 15 * 25 = 5625 hypotheses
RELOC_K = 8


def reloc_case(scene):
    """(truth, centre, scan) of the committed case on `scene`"""
    truth = np.asarray(scene.query_truth[RELOC_QUERY], np.float32)
    centre = (truth + np.asarray(RELOC_OFFSET, np.float32)).astype(np.float32)
    return truth, centre, np.asarray(scene.query_scans[RELOC_QUERY], np.float32)
