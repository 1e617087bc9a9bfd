"""A level's occupied cells as a point set (hsm_occupied_points_device, hsm_occupied_points) on the MI355X, against the numpy
model of tests/points_cases.py bit for bit: no tolerance and no excluded case anywhere in this file.

The planes are written with hsm_upload_level, so the test controls every cell: a single-level 300 x 210 map of random log-odds
(about 15 % positive, NaN, +0, -0, negatives, infinities, denormals) that spans 16 tiles of the extraction with a ragged last one,
an all-zero and an all-occupied plane; and the three levels of a 70 x 52 pyramid built by the product's own updates.  Every
device run gets an exact-size workspace full of garbage and sentinel floats behind the last point it may write.  Both layouts.

At the parent commit every test of this file fails: the entries do not exist."""
import ctypes as C

import numpy as np
import pytest

import merge_cases as mc
import points_cases as pc
from conftest import bits
from support import capi, dev, new_context, single_update, stream_ptr

pytestmark = pytest.mark.gpu

HSM_ERR_INVALID = -1
F = np.float32
SENTINEL = -777.0
GUARD = 16   # floats behind the points, ints behind the workspace
LAYOUTS = pytest.mark.parametrize("layout", ("quad", "plane"))
BIG = pc.random_plane(pc.BIG_GEOM[1], pc.BIG_GEOM[2], 11)


def new_ctx(capi, geom, layout):
    return new_context(capi, geom[0], geom[1], geom[2], geom[3], geom[4], layout)


def uploaded(capi, geom, layout, planes):
    g = new_ctx(capi, geom, layout)
    for lvl, lo in enumerate(planes):
        g.upload_level(lvl, lo, np.full(lo.shape, -1, np.int32))
    return g


class DeviceRun:
    """hsm_occupied_points_device on torch buffers: the points [max_points + guard], the counts, the workspace of exactly
    hsm_occupied_points_workspace(cells of the clamped box) bytes with garbage in and behind it"""

    def __init__(self, capi, g, level, bbox, every, max_points):
        import torch
        sx, sy, _, _ = g.level_info(level)
        self.args = (level, bbox, every, max_points)
        self.max_points = max_points
        self.ws_bytes = capi.MapRepMultiMap.occupied_points_workspace(pc.box_cells(pc.clamp_box(bbox, sx, sy)))
        assert self.ws_bytes > 0 and self.ws_bytes % 8 == 0
        self.garbage = np.random.default_rng(max_points + every).integers(0, 2 ** 32, self.ws_bytes // 4 + GUARD, dtype=np.uint32)
        self.ws = dev(self.garbage.view(np.int32))
        self.pts = torch.full((max_points + GUARD // 2, 2), SENTINEL, dtype=torch.float32, device="cuda:0")
        self.count = torch.full((2,), -9, dtype=torch.int32, device="cuda:0")
        self.g = g

    def launch(self, stream):
        level, bbox, every, max_points = self.args
        self.g.occupied_points_device(level, bbox, every, max_points, self.pts.data_ptr(), self.count.data_ptr(), self.ws.data_ptr(),
                                      self.ws_bytes, stream)

    def result(self):
        """-> (points [written, 2], counts); the floats behind the written points and the ints behind the workspace are intact"""
        count = self.count.cpu().numpy()
        pts = self.pts.cpu().numpy()
        assert 0 <= count[0] <= self.max_points and count[0] <= count[1], count
        assert (pts[count[0]:] == SENTINEL).all(), "wrote behind the last point"
        assert np.array_equal(self.ws.cpu().numpy().view(np.uint32)[self.ws_bytes // 4:], self.garbage[self.ws_bytes // 4:]), \
            "wrote behind the workspace"
        return pts[:count[0]], count


def extract(capi, g, level, bbox, every, max_points):
    import torch
    run = DeviceRun(capi, g, level, bbox, every, max_points)
    torch.cuda.synchronize()
    run.launch(stream_ptr())
    torch.cuda.synchronize()
    return run.result()


def assert_model(what, got, lo, bbox, every, max_points, affine, scale):
    pts, count = got
    want, want_count = pc.occupied_points_model(lo, bbox, every, max_points, affine, scale)
    print(what, "counts", count.tolist(), "model", want_count, "points that differ",
          int((bits(pts) != bits(want)).any(axis=1).sum()) if pts.shape == want.shape else "shape")
    assert tuple(count.tolist()) == want_count, (what, count, want_count)
    assert pts.shape == want.shape and np.array_equal(bits(pts), bits(want)), what


@pytest.fixture(scope="module")
def big(capi):
    made = {}

    def get(layout):
        if layout not in made:
            made[layout] = uploaded(capi, pc.BIG_GEOM, layout, [BIG])
        return made[layout]
    yield get
    for g in made.values():
        g.close()


def big_frame(g):
    """the model's transform is the context's: hsm_world_coords_pose of three cells, and the scale"""
    affine, scale = pc.world_from_map(pc.BIG_GEOM, 0), pc.scale_to_map(pc.BIG_GEOM)
    assert bits(F(g.getScaleToMap())) == bits(scale)
    cells = np.array([[0, 0], [299, 0], [0, 209], [123, 77]], np.int64)
    host = np.stack([g.getWorldCoordsPose(0, F([x, y, 0]))[:2] * scale for x, y in cells]).astype(F)
    assert np.array_equal(bits(pc.cell_points(cells, affine, scale)), bits(host))
    return affine, scale


# ---- 1. the random plane: thinning and the cap -------------------------------------------------------------------------------
def test_the_big_plane_spans_three_tiles_and_more_with_a_ragged_last_one(capi):
    cells = BIG.size
    assert cells == 63000 and cells > 2 * capi.POINTS_TILE and cells % capi.POINTS_TILE != 0
    with np.errstate(invalid="ignore"):
        share = float((BIG > 0).mean())
    assert 0.12 < share < 0.20 and np.isnan(BIG).any() and (bits(BIG) == 0x80000000).any() and (BIG < 0).any()


@LAYOUTS
@pytest.mark.parametrize("every", (1, 3, 7))
def test_random_plane_every_and_caps(capi, big, layout, every):
    g = big(layout)
    affine, scale = big_frame(g)
    kept = len(pc.kept_cells(BIG, None, every))
    assert kept > 1000
    for cap in (0, 1, kept - 1, kept, kept + 5):
        got = extract(capi, g, 0, None, every, cap)
        assert_model(f"{layout} every {every} cap {cap}", got, BIG, None, every, cap, affine, scale)
        assert got[1][1] == kept
        pts, count = g.occupied_points(0, None, every, cap)   # the host entry
        assert np.array_equal(count, got[1]) and np.array_equal(bits(pts), bits(got[0])), ("host entry", every, cap)


# ---- 2. boxes ------------------------------------------------------------------------------------------------------------------
@LAYOUTS
@pytest.mark.parametrize("name,box", pc.BOXES, ids=[n for n, _ in pc.BOXES])
def test_boxes(capi, big, layout, name, box):
    g = big(layout)
    affine, scale = big_frame(g)
    for every in (1, 3):
        got = extract(capi, g, 0, box, every, 5000)
        assert_model(f"{layout} {name} every {every}", got, BIG, box, every, 5000, affine, scale)
        pts, count = g.occupied_points(0, box, every, 5000)
        assert np.array_equal(count, got[1]) and np.array_equal(bits(pts), bits(got[0])), ("host entry", name)
    nothing = pc.clamp_box(box, 300, 210) == pc.EMPTY
    assert nothing == name.startswith(("misses", "empty"))
    if nothing:
        assert got[1].tolist() == [0, 0]
    elif name != "single_cell":
        assert got[1][0] > 0


@LAYOUTS
def test_a_step_beyond_every_rank_keeps_rank_zero_alone(capi, big, layout):
    """every up to INT_MAX: ceil(occupied / every) must not be formed through occupied + every - 1"""
    g = big(layout)
    affine, scale = big_frame(g)
    occupied = len(pc.kept_cells(BIG, None, 1))
    for every in (occupied - 1, occupied, occupied + 1, 2 ** 31 - 4096, 2 ** 31 - 1):
        got = extract(capi, g, 0, None, every, 8)
        assert_model(f"{layout} every {every}", got, BIG, None, every, 8, affine, scale)
        assert got[1].tolist() == ([2, 2] if every < occupied else [1, 1])
        pts, count = g.occupied_points(0, None, every, 8)
        assert np.array_equal(count, got[1]) and np.array_equal(bits(pts), bits(got[0]))


def test_a_single_cell_either_way(capi, big):
    g = big("quad")
    with np.errstate(invalid="ignore"):
        occ = np.argwhere(BIG > 0)[5]
        free = np.argwhere(~(BIG > 0))[5]
    for (y, x), want in ((occ, 1), (free, 0)):
        pts, count = extract(capi, g, 0, (x, y, x, y), 1, 3)
        assert count.tolist() == [want, want]
        if want:
            host = (g.getWorldCoordsPose(0, F([x, y, 0]))[:2] * F(g.getScaleToMap())).astype(F)
            assert np.array_equal(bits(pts[0]), bits(host))


# ---- 3. nothing and everything ---------------------------------------------------------------------------------------------------
@LAYOUTS
def test_all_zero_and_all_occupied_planes(capi, layout):
    geom = (0.1, 64, 64, 1, (0.5, 0.5))
    affine, scale = pc.world_from_map(geom, 0), pc.scale_to_map(geom)
    for name, lo in (("zeros", np.zeros((64, 64), F)), ("occupied", np.full((64, 64), 1.5, F))):
        g = uploaded(capi, geom, layout, [lo])
        for every, cap in ((1, 5000), (5, 5000), (1, 100)):
            got = extract(capi, g, 0, None, every, cap)
            assert_model(f"{layout} {name} every {every} cap {cap}", got, lo, None, every, cap, affine, scale)
        assert got[1].tolist() == ([0, 0] if name == "zeros" else [100, 4096])
        g.close()


def test_more_tiles_than_workgroups(capi):
    """2900 x 2970 cells are 2103 tiles, the grid is capped at 2048 workgroups: some take a second tile, and the scan of the tile
    counts a third round of 1024; a box narrower than the level takes the dividing form over the same trips"""
    geom = (0.05, 2900, 2970, 1, (0.5, 0.5))
    assert 2048 < -(-2900 * 2970 // capi.POINTS_TILE) and 2048 < -(-2890 * 2970 // capi.POINTS_TILE)
    lo = pc.random_plane(2900, 2970, 5)
    g = uploaded(capi, geom, "plane", [lo])
    affine, scale = pc.world_from_map(geom, 0), pc.scale_to_map(geom)
    for box, every in ((None, 1), (None, 9), ((3, 0, 2892, 2969), 9)):
        kept = len(pc.kept_cells(lo, box, every))
        for cap in (kept + 3, 20000):
            assert_model(f"large plane box {box} every {every} cap {cap}", extract(capi, g, 0, box, every, cap), lo, box, every, cap,
                         affine, scale)
    g.close()


# ---- 4. a pyramid built by the product's own updates --------------------------------------------------------------------------------
@LAYOUTS
def test_levels_of_a_built_pyramid_give_world_coords_pose_times_the_scale(capi, layout):
    geom = mc.DST_GEOM
    g = new_ctx(capi, geom, layout)
    for pose, pts in mc.build_scans(77, n_scans=5):
        single_update(capi, g, pose, pts)
    scale = F(g.getScaleToMap())
    for lvl in (2, 1, 0):
        lo, _ = g.download_level(lvl)
        for every in (1, 4):
            cells = pc.kept_cells(lo, None, every)
            assert len(cells) > (3 if lvl == 2 else 20), (lvl, len(cells))
            want = np.stack([(g.getWorldCoordsPose(lvl, F([x, y, 0]))[:2] * scale).astype(F) for x, y in cells])
            pts, count = extract(capi, g, lvl, None, every, len(cells) + 3)
            assert count.tolist() == [len(cells)] * 2 and np.array_equal(bits(pts), bits(want)), (lvl, every)
            assert_model(f"{layout} level {lvl} every {every}", (pts, count), lo, None, every, len(cells) + 3,
                         pc.world_from_map(geom, lvl), pc.scale_to_map(geom))
    g.close()


# ---- 5. ordering and capture ---------------------------------------------------------------------------------------------------------
def test_queued_updates_are_seen_and_a_captured_extraction_replays_on_the_new_map(capi):
    import torch
    geom = mc.DST_GEOM
    scans = mc.build_scans(77, n_scans=5)
    g, twin = new_ctx(capi, geom, "quad"), new_ctx(capi, geom, "quad")
    affine, scale = pc.world_from_map(geom, 0), pc.scale_to_map(geom)
    s = torch.cuda.Stream()
    run = DeviceRun(capi, g, 0, None, 2, 3000)
    torch.cuda.synchronize()
    for pose, pts in scans[:3]:
        single_update(capi, g, pose, pts)      # queued on the context, not waited for
        single_update(capi, twin, pose, pts)
    run.launch(s.cuda_stream)                  # on a caller's stream: behind the three updates
    single_update(capi, g, *scans[3])          # behind the read
    s.synchronize()
    before = twin.download_level(0)[0]
    assert_model("behind three queued updates", run.result(), before, None, 2, 3000, affine, scale)
    single_update(capi, twin, *scans[3])
    g.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        run.launch(s.cuda_stream)
    with torch.cuda.stream(s):
        run.pts.fill_(SENTINEL)
        graph.replay()
    s.synchronize()
    four = twin.download_level(0)[0]
    assert_model("replay", run.result(), four, None, 2, 3000, affine, scale)
    single_update(capi, g, *scans[4])
    single_update(capi, twin, *scans[4])
    g.synchronize()                            # (the caller orders replays against updates)
    with torch.cuda.stream(s):
        run.pts.fill_(SENTINEL)
        graph.replay()
    s.synchronize()
    five = twin.download_level(0)[0]
    assert not np.array_equal(pc.kept_cells(four, None, 2), pc.kept_cells(five, None, 2)), "the update changes the point set"
    assert_model("replay after an update", run.result(), five, None, 2, 3000, affine, scale)
    del graph
    assert np.array_equal(bits(g.download_level(0)[0]), bits(five))
    g.close()
    twin.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_queue_nothing_and_leave_the_outputs(capi, big):
    import torch
    g = big("quad")
    lib = g._lib
    pts = torch.full((64,), SENTINEL, dtype=torch.float32, device="cuda:0")
    cnt = torch.full((2,), -9, dtype=torch.int32, device="cuda:0")
    ws = torch.full((1024,), -5, dtype=torch.int32, device="cuda:0")
    need = lib.hsm_occupied_points_workspace(63000)
    assert need <= 4096
    box = (C.c_int * 4)(0, 0, 299, 209)
    ok = dict(h=g._h, level=0, box=box, every=1, cap=8, pts=pts.data_ptr(), cnt=cnt.data_ptr(), ws=ws.data_ptr(), wsb=need)
    bad = []
    for change in (dict(h=None), dict(level=-1), dict(level=1), dict(every=0), dict(every=-3), dict(cap=-1), dict(cnt=None),
                   dict(pts=None), dict(ws=None), dict(ws=ws.data_ptr() + 4), dict(wsb=need - 1), dict(wsb=0)):
        a = dict(ok, **change)
        bad.append(lib.hsm_occupied_points_device(a["h"], a["level"], a["box"], a["every"], a["cap"], a["pts"], a["cnt"], a["ws"],
                                                  a["wsb"], None))
    h_pts, h_cnt = np.full(16, SENTINEL, F), np.full(2, -9, np.int32)
    for change in (dict(h=None), dict(level=1), dict(every=0), dict(cap=-1), dict(cnt=None), dict(pts=None)):
        a = dict(ok, pts=h_pts.ctypes.data, cnt=h_cnt.ctypes.data)
        a.update(change)
        bad.append(lib.hsm_occupied_points(a["h"], a["level"], a["box"], a["every"], a["cap"], a["pts"], a["cnt"]))
    assert bad and all(rc == HSM_ERR_INVALID for rc in bad), bad
    torch.cuda.synchronize()
    assert cnt.cpu().numpy().tolist() == [-9, -9] and (ws == -5).all() and (pts == SENTINEL).all(), "a refused call queued something"
    # a smaller box needs a smaller workspace; NULL points are fine where nothing can be written
    small = (C.c_int * 4)(0, 0, 9, 9)
    assert lib.hsm_occupied_points_device(g._h, 0, small, 1, 0, None, cnt.data_ptr(), ws.data_ptr(),
                                          lib.hsm_occupied_points_workspace(100), None) == 0
    torch.cuda.synchronize()
    assert (pts == SENTINEL).all() and (h_pts == SENTINEL).all() and h_cnt.tolist() == [-9, -9]
    with np.errstate(invalid="ignore"):
        assert cnt.cpu().numpy().tolist() == [0, int((BIG[:10, :10] > 0).sum())]
