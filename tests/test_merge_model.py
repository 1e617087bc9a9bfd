"""The host model of a merge of two pyramids (tests/merge_cases.py: merge_model, merge_box) against what the rule of
include/hector_mi355/capi.h implies, without a GPU.  The GPU tests hold hsm_merge_map to this model bit for bit; these hold the
model to properties that do not depend on it.  Comparisons are exact."""
import math

import numpy as np
import pytest

import merge_cases as mc

F = np.float32


def planes_of(pair):
    geom_dst, geom_src = mc.PAIRS[pair]
    return geom_dst, geom_src, mc.synthetic_planes(geom_dst, 11), mc.synthetic_planes(geom_src, 23)


def test_identity_into_an_empty_map_of_the_same_geometry_gives_src_cut_at_50():
    geom = mc.DST_GEOM
    src = mc.synthetic_planes(geom, 23)
    assert any((lo > 50).any() for lo in src) and any((lo < -50).any() for lo in src)
    for lvl in range(geom[3]):
        sx, sy = mc.level_size(geom, lvl)
        got, box = mc.merge_model(np.zeros((sy, sx), F), src[lvl], geom, geom, lvl, F([0, 0, 0]))
        assert box == (0, 0, sx - 1, sy - 1), (lvl, box)
        assert np.array_equal(got, np.minimum(src[lvl], F(50.0))), lvl   # (-0.0 == 0.0: an unknown cell either way)
        assert not np.signbit(got[0, 0]), "a cell whose sample is -0.0 is not written"


@pytest.mark.parametrize("theta,t,k", [(math.pi / 2, (-1, 0), -1), (-math.pi / 2, (0, -1), 1)])
def test_quarter_turn_on_a_square_centred_map_is_rot90(theta, t, k):
    """A map of N x N cells with centre start coordinates holds the world origin at map coordinates (N/2, N/2), half a cell off
    the centre of its cells 0..N-1, so a quarter turn about the origin carries the grid onto itself moved by one cell; with that
    cell taken back by the translation the merge is numpy.rot90 of the plane (rows are y)."""
    N, res = 32, 0.1
    geom = (res, N, N, 1, (0.5, 0.5))
    src = np.minimum(mc.synthetic_planes(geom, 5)[0], F(50.0))
    src[src == 0] = F(0.0)
    tr = F([t[0] * float(F(res)), t[1] * float(F(res)), theta])
    got, box = mc.merge_model(np.zeros((N, N), F), src, geom, geom, 0, tr)
    assert box == (0, 0, N - 1, N - 1)
    assert np.array_equal(got, np.rot90(src, k))
    assert not np.array_equal(got, np.rot90(src, -k))


@pytest.mark.parametrize("pair,name,t", mc.CASES, ids=mc.CASE_IDS)
def test_box_contains_every_cell_the_rule_changes(pair, name, t):
    geom_dst, geom_src, dst, src = planes_of(pair)
    some = False
    for lvl in range(geom_dst[3]):
        sx, sy = mc.level_size(geom_dst, lvl)
        whole, box = mc.merge_model(dst[lvl], src[lvl], geom_dst, geom_src, lvl, t, visit=(0, 0, sx - 1, sy - 1))
        boxed, box2 = mc.merge_model(dst[lvl], src[lvl], geom_dst, geom_src, lvl, t)
        assert box == box2 and (box == mc.EMPTY or (0 <= box[0] <= box[2] < sx and 0 <= box[1] <= box[3] < sy)), (lvl, box)
        assert np.array_equal(whole.view(np.uint32), boxed.view(np.uint32)), (lvl, box)
        # every src cell a visited cell reads lies in the box the staged route copies
        if box != mc.EMPTY:
            some = True
            _, ix, iy, inside = mc.sampled(src[lvl], geom_dst, geom_src, lvl, t, box)
            sb = mc.merge_src_box(geom_dst, geom_src, lvl, t)
            assert inside.any(), (lvl, "a box that is not empty reads src somewhere")
            assert (ix[inside] >= sb[0]).all() and (ix[inside] <= sb[2]).all(), (lvl, sb)
            assert (iy[inside] >= sb[1]).all() and (iy[inside] <= sb[3]).all(), (lvl, sb)
    assert some == (name != "misses")


def test_half_outside_case_is_cut_by_the_level_and_the_miss_is_empty():
    geom_dst, geom_src = mc.PAIRS["local"]
    t = dict(mc.TRANSFORMS)
    for lvl in range(mc.LEVELS):
        sx, _ = mc.level_size(geom_dst, lvl)
        box = mc.merge_box(geom_dst, geom_src, lvl, F(t["half_outside"]))
        assert box[2] == sx - 1 and box[0] > sx // 2, (lvl, box)
        assert mc.merge_box(geom_dst, geom_src, lvl, F(t["misses"])) == mc.EMPTY


@pytest.mark.parametrize("pair,name,t", mc.CASES, ids=mc.CASE_IDS)
def test_positive_evidence_never_passes_50_and_never_lowers_a_cell(pair, name, t):
    geom_dst, geom_src, dst, src = planes_of(pair)
    for lvl in range(geom_dst[3]):
        new, box = mc.merge_model(dst[lvl], src[lvl], geom_dst, geom_src, lvl, t)
        if box == mc.EMPTY:
            assert np.array_equal(new.view(np.uint32), dst[lvl].view(np.uint32))
            continue
        x0, y0, x1, y1 = box
        v, _, _, _ = mc.sampled(src[lvl], geom_dst, geom_src, lvl, t, box)
        old, got = dst[lvl][y0:y1 + 1, x0:x1 + 1], new[y0:y1 + 1, x0:x1 + 1]
        up = v > 0
        assert (got[up] >= old[up]).all() and (got[up] <= np.maximum(old[up], F(50.0))).all(), lvl
        assert np.array_equal(got[up & (old >= 50)], old[up & (old >= 50)]), (lvl, "the reference's gate")
        down = v < 0
        assert np.array_equal(got[down], (old[down] + v[down]).astype(F)), lvl
        assert np.array_equal(got[v == 0].view(np.uint32), old[v == 0].view(np.uint32)), (lvl, "v == 0 is not written")
        assert np.isfinite(new).all()
