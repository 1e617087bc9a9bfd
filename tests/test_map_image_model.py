"""The rules of hsm_map_extents*, hsm_map_image* and hsm_map_tiles* without a GPU: the numpy statements of tests/image_cases.py,
which the GPU tests hold the entries to, against plain double-loop transcriptions of the reference loops they restate
(GridMapBase.h:334-383, HectorMapTools.h:241-290, map_to_image_node.cpp:98-140 and :143-235), and against a grid the reference's
node published.  Bytes and boxes are compared for equality: there is no tolerance."""
import numpy as np
import pytest

import image_cases as ic
import merge_cases as mc

PLANES = ic.planes()
_, SX, SY, _, _ = ic.BIG_GEOM
META = ic.metadata(ic.BIG_GEOM, 0)


@pytest.fixture(scope="module")
def pyramid(oracle_mod):
    return ic.pyramid_planes(oracle_mod)


def test_byte_rule_on_the_special_values():
    lo = np.float32([-1.0, 1.0, 0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, -1e-45])
    assert ic.published(lo).tolist() == [0, 100, -1, -1, -1, 100, 0, 100, 0]
    assert ic.image_bytes(lo).tolist() == [255, 0, 127, 127, 127, 0, 255, 0, 255]


@pytest.mark.parametrize("name", sorted(PLANES))
def test_extents_rule_equals_both_reference_loops(name):
    lo = PLANES[name]
    want = ic.extents_model(lo)
    found, top_left, bottom_right = ic.extents_loop_map_tools(ic.published(lo))
    assert (found, top_left + bottom_right) == (True, (want[0], want[1], want[2] + 1, want[3] + 1)) if want != ic.EMPTY else not found
    g_found, x_max, y_max, x_min, y_min = ic.extents_loop_grid_map_base(lo)
    if name in ic.NAN_FREE:  # the two conventions agree: GridMapBase's box is the inclusive one
        assert (g_found, (x_min, y_min, x_max, y_max)) == (True, want) if want != ic.EMPTY else not g_found
    if name in ("all_zero", "all_nan"):
        assert want == ic.EMPTY
    if name == "all_known":
        assert want == (0, 0, SX - 1, SY - 1)


def test_a_nan_cell_is_unknown_here_and_known_to_grid_map_base():
    """the documented difference: the published grid says -1 for a NaN, `getValue() != 0.0f` is true for it"""
    lo = np.zeros((9, 11), np.float32)
    lo[4, 5] = -0.4
    lo[7, 9] = np.nan
    assert ic.extents_model(lo) == (5, 4, 5, 4)
    assert ic.extents_loop_map_tools(ic.published(lo)) == (True, (5, 4), (6, 5))
    assert ic.extents_loop_grid_map_base(lo) == (True, 9, 7, 5, 4)
    assert ic.extents_loop_grid_map_base(PLANES["all_nan"][:8, :8])[0] and ic.extents_model(PLANES["all_nan"]) == ic.EMPTY


@pytest.mark.parametrize("name", sorted(PLANES))
def test_image_rule_equals_the_reference_loop(name):
    lo = PLANES[name]
    full = ic.image_model(lo)
    assert full.shape == (SY, SX) and np.array_equal(full, ic.image_loop_full(ic.published(lo)))
    for crop in ((13, 9, 270, 190), (-5, -3, 40, 21), (250, 180, 400, 300), (17, 23, 17, 23), ic.extents_model(lo)):
        x0, y0, x1, y1 = ic.pc.clamp_box(crop, SX, SY)
        got = ic.image_model(lo, crop)
        if x1 < x0:
            assert got.shape == (0, 0)
        else:
            assert np.array_equal(got, full[SY - 1 - y1:SY - y0, x0:x1 + 1]), crop
    assert ic.image_model(lo, (400, 0, 500, 10)).shape == (0, 0)


@pytest.mark.parametrize("size", ic.tile_sizes(SX, SY), ids=lambda s: "%dx%d" % s)
def test_tile_rule_equals_the_reference_loop(size):
    lo = PLANES["random_1"]
    grid = ic.published(lo)
    poses = ic.poses(META, SX, SY)
    if size == (SX, SY):
        poses = poses[[0, 1, 9, 22, 26, 30]]  # (every pose gives the whole level: the loop is slow and says nothing new)
    tiles, boxes = ic.tiles_model(lo, META, poses, *size)
    for b, pose in enumerate(poses):
        tile, box = ic.tile_loop(grid, META, pose, *size)
        assert np.array_equal(tiles[b], tile) and tuple(boxes[b]) == tuple(box), (b, pose, box)
    finite = np.isfinite(poses[:, :2]).all(1)
    assert (boxes[~finite] == ic.EMPTY).all() and (tiles[~finite] == 127).all() and (~finite).sum() >= 2
    assert (boxes[finite, 0] >= 0).all() and (boxes[finite, 2] < SX).all() and (boxes[finite, 3] < SY).all()


def test_truncation_toward_zero_and_the_far_poses():
    boxes = ic.tiles_model(PLANES["random_1"], META, ic.poses(META, SX, SY), 1, 1)[1]
    assert tuple(boxes[17]) == (0, 40, 0, 40) and tuple(boxes[18]) == (40, 0, 40, 0) and tuple(boxes[19]) == (0, 0, 0, 0)
    assert tuple(boxes[22]) == (SX - 1, boxes[22][1], SX - 1, boxes[22][3]) and boxes[23][1] == 0
    assert tuple(boxes[24]) == (0, SY - 1, 0, SY - 1) and tuple(boxes[25]) == (SX - 1, 0, SX - 1, 0)


@pytest.mark.parametrize("name", ["random_1", "random_2", "cell_last"])
def test_a_64_window_equals_the_same_window_of_the_full_image(name):
    lo = PLANES[name]
    full = ic.image_model(lo)
    tiles, boxes = ic.tiles_model(lo, META, ic.poses(META, SX, SY), 64, 64)
    for tile, (x0, y0, x1, y1) in zip(tiles, boxes):
        if x1 >= x0:
            assert (x1 - x0, y1 - y0) == (63, 63)
            assert np.array_equal(tile, full[SY - 1 - y1:SY - y0, x0:x1 + 1])


def test_full_image_equals_the_byte_map_of_the_published_grid_flipped(oracle_mod, pyramid):
    byte_of = np.full(256, 77, np.uint8)
    byte_of[[255, 0, 100]] = [127, 255, 0]  # (-1 as a byte, 0, 100)
    for lvl, lo in enumerate(pyramid):
        assert lo.shape == mc.level_size(ic.PYRAMID_GEOM, lvl)[::-1]
        grid = ic.node_published(oracle_mod, lo)
        assert np.array_equal(grid, ic.published(lo)) and {-1, 0, 100} == set(np.unique(grid).tolist())
        assert np.array_equal(ic.image_model(lo), byte_of[grid.view(np.uint8)][::-1]), lvl
        assert np.array_equal(ic.image_model(lo), ic.image_loop_full(grid)), lvl
        found, top_left, bottom_right = ic.extents_loop_map_tools(grid)
        want = ic.extents_model(lo)
        assert found and top_left + bottom_right == (want[0], want[1], want[2] + 1, want[3] + 1)
        assert ic.extents_loop_grid_map_base(lo) == (True, want[2], want[3], want[0], want[1])
        meta = ic.metadata(ic.PYRAMID_GEOM, lvl)
        sy, sx = lo.shape
        for size in ic.tile_sizes(sx, sy):
            poses = ic.poses(meta, sx, sy)
            tiles, boxes = ic.tiles_model(lo, meta, poses, *size)
            for b in range(0, len(poses), 3):
                tile, box = ic.tile_loop(grid, meta, poses[b], *size)
                assert np.array_equal(tiles[b], tile) and tuple(boxes[b]) == tuple(box), (lvl, size, b)
