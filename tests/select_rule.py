"""The ranking rule of hsm_select_best_device, restated in numpy: the expected value of the GPU tests (tests/test_gpu_score_batch.py),
itself tested on hand-made arrays (tests/test_score_batch_abi.py).

Per group the index, into the whole score array, of the highest score.  A NaN never wins; among equal scores (compared as
floats, so +0 == -0) the LOWEST index wins; a group that is empty or all NaN gives -1.
"""
import numpy as np


def group_bounds(n_scores, groups=None, group_size=None, group_offsets=None):
    """[G+1] offsets of either form: CSR ``group_offsets``, or ``groups`` groups of ``group_size`` consecutive entries"""
    if group_offsets is not None:
        offs = np.asarray(group_offsets, np.int64)
        assert offs.ndim == 1 and offs.size >= 1 and np.all(np.diff(offs) >= 0) and offs[0] >= 0 and offs[-1] <= n_scores
        return offs
    offs = np.arange(groups + 1, dtype=np.int64) * group_size
    assert offs[-1] <= n_scores
    return offs


def select_best(scores, groups=None, group_size=None, group_offsets=None):
    """-> (index [G] int32, score [G] float32 -- NaN where index is -1)"""
    s = np.ascontiguousarray(scores, np.float32).reshape(-1)
    offs = group_bounds(s.size, groups, group_size, group_offsets)
    G = offs.size - 1
    index = np.full(G, -1, np.int32)
    score = np.full(G, np.nan, np.float32)
    for g in range(G):
        best = -1
        for k in range(int(offs[g]), int(offs[g + 1])):  # ascending: only a strictly greater score replaces the holder
            v = s[k]
            if v != v:
                continue
            if best < 0 or v > s[best]:
                best = k
        index[g] = best
        if best >= 0:
            score[g] = s[best]
    return index, score


def winner_poses(index, poses_world, before):
    """what d_out_pose_world holds afterwards: the winner's pose bit for bit, `before` where a group has none"""
    out = np.array(before, np.float32, copy=True).reshape(-1, 3)
    p = np.ascontiguousarray(poses_world, np.float32).reshape(-1, 3)
    for g, i in enumerate(index):
        if i >= 0:
            out[g] = p[i]
    return out
