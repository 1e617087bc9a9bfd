"""updateByScan with DENSE scans (>= 4096 beams: update_mark_occ_dense_kernel / update_mark_free_dense_kernel /
update_apply_dense_kernel, map_update.h) where Bresenham and the block-owned apply pass are delicate
(reference: OccGridMapBase.h:121-260):

  * end points 1.5 .. 6 cells OUTSIDE each of the four borders (the whole beam is skipped, :176-188) mixed with end points
    on the border cells themselves, so the update boxes touch x = 0, x = sx - 1, y = 0 and y = sy - 1;
  * the begin cell off the map at level 0 but valid at level 1 / 2 (low edges: (int) truncates towards zero), off the map on
    the high side, in the corners;
  * maps whose rows are 64, 128, 192 cells and whose HEIGHT is not a multiple of 4 (the apply pass owns 64 x 4-cell blocks:
    the last block row straddles y >= sy), and pyramids in which a coarse level falls back to the keyed form;
  * both layouts (the quad layout writes the edge-replicated texels of the last column / row from the apply pass).

After EVERY update: all levels bit-identical to the CPU checker, and the two mark planes that carry no generation tag --
the crossed-cell byte map and the end-cell bitmap -- all zero again (hsm_debug_marks_nonzero)."""
import numpy as np
import pytest

from conftest import bits
from support import capi, kind, layout_of

pytestmark = pytest.mark.gpu


from edge_cases import GEOMETRIES, begin_cells, border_fan, probe_coords, world_pose_of_cell  # noqa: E402


@pytest.mark.parametrize("layout", ["quad", "plane"])
@pytest.mark.parametrize("geom", GEOMETRIES, ids=lambda g: "%dx%d_L%d_n%d" % g)
def test_dense_update_on_and_beyond_the_four_borders_is_bit_exact(capi, oracle_mod, kind, geom, layout):
    sx, sy, levels, n = geom
    res = 0.05
    g = capi.MapRepMultiMap(res, sx, sy, levels, layout=layout_of(capi, layout))
    o = oracle_mod.Oracle(kind, res, sx, sy, levels)
    for m_ in (g.setUpdateFactorFree, o.set_update_factor_free):
        m_(0.4)
    for m_ in (g.setUpdateFactorOccupied, o.set_update_factor_occupied):
        m_(0.9)
    rng = np.random.default_rng(sx * 1000 + sy)
    origo = np.zeros(2, np.float32)
    touched = np.zeros(levels, np.int64)
    for k, (cx, cy) in enumerate(begin_cells(sx, sy)):
        th = float(rng.uniform(-np.pi, np.pi)) if k % 3 else 0.0
        pose = world_pose_of_cell(res, sx, sy, cx, cy, th)
        pts = border_fan(rng, sx, sy, cx, cy, th, n)
        og = origo if k % 4 else np.array([0.3, -0.2], np.float32)  # a laser origin off the robot's centre now and then
        o.match(pose, pts, og)  # retains the coarse containers (MapRepMultiMap.h:127,143)
        g.matchData(pose, pts, None, og)
        o.update_by_scan(pose, pts, og)
        g.updateByScan(pts, pose, og)
        o.on_map_updated()
        for lvl in range(levels):
            (lo_g, ui_g), (lo_o, ui_o) = g.download_level(lvl), o.download_level(lvl)
            assert np.array_equal(ui_g, ui_o), (geom, layout, k, lvl, int((ui_g != ui_o).sum()))
            assert np.array_equal(bits(lo_g), bits(lo_o)), (geom, layout, k, lvl, int((bits(lo_g) != bits(lo_o)).sum()))
            assert g.debug_marks_nonzero(lvl) == (0, 0), (geom, layout, k, lvl)
            touched[lvl] = int((ui_o >= 0).sum())
    # the scans did reach all four borders of level 0
    _, ui = o.download_level(0)
    assert (ui[0] >= 0).any() and (ui[-1] >= 0).any() and (ui[:, 0] >= 0).any() and (ui[:, -1] >= 0).any(), geom
    assert (touched > 20).all(), touched
    # the matcher's view: probability plane everywhere, sampled footprints along the borders (the quad layout's texels of the
    # last column / row are edge replicated by the apply pass)
    for lvl in range(levels):
        lo_o, _ = o.download_level(lvl)
        _, prob = oracle_mod.libm_expf(lo_o.reshape(-1), o.kind)
        assert np.array_equal(bits(g.download_prob(lvl)).reshape(-1), bits(prob)), (geom, layout, lvl)
        lsx, lsy = sx >> lvl, sy >> lvl
        if lsx >= 4 and lsy >= 4:
            pc = probe_coords(lsx, lsy, rng)
            got = g.eval_beams(lvl, np.zeros(3, np.float32), pc)
            assert np.array_equal(bits(got[:, :3]), bits(o.interp(lvl, pc))), (geom, layout, lvl)
    g.close()


def test_dense_update_with_no_end_point_inside_the_map_leaves_no_marks(capi, oracle_mod, kind):
    """a dense scan whose end points ALL lie outside the map (or whose begin cell does): nothing is marked, nothing applied,
    the counters advance (OccGridMapBase.h:123-124,167) -- and the next ordinary scan gives the reference's map"""
    sx = sy = 256
    res = 0.05
    g = capi.MapRepMultiMap(res, sx, sy, 2)
    o = oracle_mod.Oracle(kind, res, sx, sy, 2)
    rng = np.random.default_rng(3)
    a = np.linspace(-np.pi, np.pi, 5000, endpoint=False)
    far = np.stack([np.cos(a), np.sin(a)], 1).astype(np.float32) * np.float32(400.0)  # 400 cells out: all outside
    near = np.stack([np.cos(a), np.sin(a)], 1).astype(np.float32) * rng.uniform(20, 90, a.size).astype(np.float32)[:, None]
    centre = world_pose_of_cell(res, sx, sy, 128.0, 128.0, 0.1)
    outside = world_pose_of_cell(res, sx, sy, 300.0, 128.0, 0.0)
    for pose, pts in ((centre, far), (outside, near), (centre, near), (outside, far), (centre, near)):
        o.match(pose, pts)
        g.matchData(pose, pts)
        o.update_by_scan(pose, pts)
        g.updateByScan(pts, pose)
        o.on_map_updated()
        for lvl in range(2):
            (lo_g, ui_g), (lo_o, ui_o) = g.download_level(lvl), o.download_level(lvl)
            assert np.array_equal(ui_g, ui_o) and np.array_equal(bits(lo_g), bits(lo_o)), lvl
            assert g.debug_marks_nonzero(lvl) == (0, 0), lvl
    g.close()


def test_sparse_update_leaves_the_end_cell_bitmap_clear(capi, oracle_mod, kind, pyramid_scene):
    """the keyed form's end-cell bitmap obeys the same all-zero-between-updates invariant (1081-beam scans)"""
    sc = pyramid_scene
    g = capi.MapRepMultiMap(sc.resolution, sc.map_size, sc.map_size, sc.levels)
    for t in range(12):
        g.matchData(sc.build_poses[t], sc.build_scans[t])
        g.updateByScan(sc.build_scans[t], sc.build_poses[t])
        for lvl in range(sc.levels):
            assert g.debug_marks_nonzero(lvl) == (0, 0), (t, lvl)
    g.close()
