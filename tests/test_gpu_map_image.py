"""hsm_map_extents*, hsm_map_image* and hsm_map_tiles* on the MI355X, held to the numpy rules of tests/image_cases.py (which
tests/test_map_image_model.py holds to the reference's loops) byte for byte and box for box: no tolerance anywhere.

Every device output lies between two runs of the guard byte 165 (no image byte has that value) and starts at an odd address, at
an even one that is no multiple of 4, and at a multiple of 4: the guards stay intact and every byte between them is the model's.
Shapes: one level of 300 x 210 cells (no multiple of 4 or 64 either way), the 70 x 52 / 35 x 26 / 17 x 13 pyramid built by the
product's own updates, and a 2101 x 1101 level, on which the extents launch reaches its cap and strides.

Nothing here provokes a device fault."""
import numpy as np
import pytest

import image_cases as ic
import merge_cases as mc
import support
from support import capi, dev, stream_ptr

pytestmark = pytest.mark.gpu

HSM_ERR_INVALID = -1
GUARD = 165
PLANES = ic.planes()
_, SX, SY, _, _ = ic.BIG_GEOM
META = ic.metadata(ic.BIG_GEOM, 0)
POSES = ic.poses(META, SX, SY)
CROPS = [None, (13, 9, 270, 190), (-5, -3, 40, 21), (250, 180, 400, 300), (17, 23, 17, 23), (0, 101, 299, 101), (299, 0, 299, 209),
         (31, 7, 33, 9)]


@pytest.fixture(scope="module", params=["quad", "plane"])
def layout(request):
    return request.param


@pytest.fixture(scope="module")
def big(capi, layout):
    g = support.new_context(capi, *ic.BIG_GEOM[:4], start=ic.BIG_GEOM[4], layout=layout)
    yield g
    g.close()


# ---- guarded device outputs -----------------------------------------------------------------------------------------------------
class Guarded:
    """`nbytes` bytes of device memory that start `pad` bytes into a block filled with the guard byte"""

    def __init__(self, nbytes, pad=67):
        import torch
        self.n, self.pad = nbytes, pad
        self.buf = torch.full((pad + nbytes + 64,), GUARD, dtype=torch.uint8, device="cuda:0")
        self.ptr = self.buf.data_ptr() + pad
        assert self.buf.data_ptr() % 256 == 0

    def take(self):
        """the payload, once the guards have been seen intact"""
        a = self.buf.cpu().numpy()
        assert (a[:self.pad] == GUARD).all() and (a[self.pad + self.n:] == GUARD).all(), "a byte outside the output was written"
        return a[self.pad:self.pad + self.n]

    def untouched(self):
        return bool((self.buf.cpu().numpy() == GUARD).all())


class GuardedBoxes:
    def __init__(self, count):
        import torch
        self.count = count
        self.buf = torch.full((4 + 4 * count + 4,), -9, dtype=torch.int32, device="cuda:0")
        self.ptr = self.buf.data_ptr() + 16

    def take(self):
        a = self.buf.cpu().numpy()
        assert (a[:4] == -9).all() and (a[4 + 4 * self.count:] == -9).all(), "an int outside the boxes was written"
        return a[4:4 + 4 * self.count].reshape(self.count, 4)

    def untouched(self):
        return bool((self.buf.cpu().numpy() == -9).all())


def device_extents(g, lvl=0, stream=0):
    out = GuardedBoxes(1)
    g.map_extents_device(lvl, out.ptr, stream)
    return tuple(int(v) for v in out.take()[0])


def device_image(g, lvl, crop, shape, pad=67, stream=0):
    out = Guarded(shape[0] * shape[1], pad)
    g.map_image_device(lvl, crop, out.ptr, stream)
    return out.take().reshape(shape)


def device_tiles(g, lvl, poses, tw, th, pad=67, stream=0, want_boxes=True):
    p = dev(np.ascontiguousarray(poses, np.float32).reshape(-1, 3))
    out, boxes = Guarded(len(poses) * tw * th, pad), GuardedBoxes(len(poses))
    g.map_tiles_device(lvl, len(poses), p.data_ptr(), tw, th, out.ptr, boxes.ptr if want_boxes else 0, stream)
    tiles = out.take().reshape(len(poses), th, tw)
    if not want_boxes:
        assert boxes.untouched()
    return tiles, boxes.take()


def check_level(g, lvl, lo, meta, poses, sizes, crops):
    """every entry, device and host form, against the model on the level `lvl` that holds the log-odds `lo`"""
    sy, sx = lo.shape
    want = ic.extents_model(lo)
    assert device_extents(g, lvl) == want
    assert tuple(int(v) for v in g.map_extents(lvl)) == want
    half_open = g.map_extents(lvl, half_open=True)
    assert half_open is None if want == ic.EMPTY else tuple(int(v) for v in half_open) == (want[0], want[1], want[2] + 1, want[3] + 1)
    for crop in crops + [want]:
        model = ic.image_model(lo, crop)
        assert np.array_equal(g.map_image(lvl, crop), model), crop
        for pad in (67, 66, 64):
            assert np.array_equal(device_image(g, lvl, crop, model.shape, pad), model), (crop, pad)
    for tw, th in sizes:
        tiles, boxes = ic.tiles_model(lo, meta, poses, tw, th)
        host_tiles, host_boxes = g.map_tiles(lvl, poses, tw, th)
        assert np.array_equal(host_tiles, tiles) and np.array_equal(host_boxes, boxes), (tw, th)
        for pad in (67, 64):
            got, got_boxes = device_tiles(g, lvl, poses, tw, th, pad)
            assert np.array_equal(got_boxes, boxes), (tw, th, np.nonzero((got_boxes != boxes).any(1))[0])
            assert np.array_equal(got, tiles), (tw, th, pad, np.nonzero((got != tiles).any((1, 2)))[0])
        assert np.array_equal(device_tiles(g, lvl, poses, tw, th, 65, want_boxes=False)[0], tiles), (tw, th)


# ---- 1: exactness and bounds ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PLANES))
def test_every_entry_equals_the_model_on_the_300_by_210_planes(big, name):
    lo = PLANES[name]
    big.upload_level(0, lo)
    assert support.same(big.download_level(0)[0], lo)
    sizes = ic.tile_sizes(SX, SY)
    check_level(big, 0, lo, META, POSES, sizes if name.startswith("random") else sizes[:2] + sizes[-1:], CROPS)
    assert big.map_image(0, (400, 0, 500, 10)).shape == (0, 0) and big.map_image(0, (0, -9, 299, -1)).shape == (0, 0)


@pytest.fixture(scope="module")
def pyramid(capi, layout):
    """PYRAMID_GEOM built by the product's own updates"""
    g = support.new_context(capi, *ic.PYRAMID_GEOM[:4], start=ic.PYRAMID_GEOM[4], layout=layout)
    for pose, pts in ic.pyramid_scans():
        support.single_update(capi, g, pose, pts)
    yield g
    g.close()


def test_every_entry_equals_the_model_on_a_pyramid_the_product_built(pyramid, oracle_mod):
    g = pyramid
    byte_of = np.full(256, 77, np.uint8)
    byte_of[[255, 0, 100]] = [127, 255, 0]  # (-1 as a byte, 0, 100)
    for lvl, ref_lo in enumerate(ic.pyramid_planes(oracle_mod)):
        lo = g.download_level(lvl)[0]
        assert support.same(lo, ref_lo), lvl
        sy, sx = lo.shape
        meta = ic.metadata(ic.PYRAMID_GEOM, lvl)
        assert tuple(np.float32(v) for v in g.map_metadata(lvl)) == tuple(meta)
        check_level(g, lvl, lo, meta, ic.poses(meta, sx, sy), ic.tile_sizes(sx, sy), [None, (3, 2, sx - 4, sy - 3), (-2, 5, 9, 99)])
        grid = ic.node_published(oracle_mod, lo)  # the grid the reference's node publishes for this level
        assert np.array_equal(g.map_image(lvl), byte_of[grid.view(np.uint8)][::-1]), lvl
        assert np.array_equal(g.occupancy_grid(lvl), grid)
        found, top_left, bottom_right = ic.extents_loop_map_tools(grid)
        assert found and tuple(int(v) for v in g.map_extents(lvl, half_open=True)) == top_left + bottom_right


# ---- 2: batching and shape independence -----------------------------------------------------------------------------------------------
def test_a_batch_of_257_equals_257_single_calls(big):
    import torch
    lo = PLANES["random_2"]
    big.upload_level(0, lo)
    rng = np.random.default_rng(5)
    poses = np.concatenate([POSES, np.zeros((257 - len(POSES), 3), np.float32)])
    far = rng.uniform(-60.0, 360.0, (257 - len(POSES), 2))
    poses[len(POSES):, :2] = [ic.world_of(META, x, y) for x, y in far]
    poses = poses.astype(np.float32)
    s = torch.cuda.Stream()
    for tw, th in ((64, 64), (5, 3)):
        want, want_boxes = ic.tiles_model(lo, META, poses, tw, th)
        with torch.cuda.stream(s):  # a caller's stream: the tiles are complete where it stands behind the call
            got, got_boxes = device_tiles(big, 0, poses, tw, th, stream=s.cuda_stream)
        assert np.array_equal(got, want) and np.array_equal(got_boxes, want_boxes), (tw, th)
        p = dev(poses)
        singles, single_boxes = Guarded(257 * tw * th, 64), GuardedBoxes(257)
        for b in range(257):
            big.map_tiles_device(0, 1, p[b].data_ptr(), tw, th, singles.ptr + b * tw * th, single_boxes.ptr + 16 * b, stream_ptr())
        assert np.array_equal(singles.take().reshape(257, th, tw), want) and np.array_equal(single_boxes.take(), want_boxes)
        one, one_box = device_tiles(big, 0, poses[40:41], tw, th)
        assert np.array_equal(one[0], want[40]) and np.array_equal(one_box[0], want_boxes[40])


def test_extents_and_image_do_not_depend_on_the_launch_shape(capi, layout):
    """the same known cells on levels of 70 x 52 (4 workgroups), 300 x 210 (62) and 2101 x 1101 (the cap of 2048, strided, and a
    last cell outside the 4-cell groups): one box; then a cell in that last position"""
    rng = np.random.default_rng(9)
    patch = np.where(rng.random((40, 60)) < 0.05, np.float32(0.8472979), np.float32(0.0)).astype(np.float32)
    patch[3, 2] = patch[38, 57] = np.float32(-0.4054651)
    want = ic.extents_model(np.pad(patch, ((5, 0), (7, 0))))
    assert want[0] >= 7 and want[1] >= 5 and (want[2], want[3]) >= (64, 43)
    for sx, sy in ((70, 52), (300, 210), (2101, 1101)):
        g = support.new_context(capi, 0.05, sx, sy, 1, layout=layout)
        lo = np.zeros((sy, sx), np.float32)
        lo[5:45, 7:67] = patch
        g.upload_level(0, lo)
        assert device_extents(g) == want and tuple(int(v) for v in g.map_extents(0)) == want, (sx, sy)
        assert device_extents(g) == want  # the accumulators were left as they were found
        assert np.array_equal(device_image(g, 0, None, (sy, sx)), ic.image_model(lo)), (sx, sy)
        if sx == 2101:
            assert (sx * sy) % 4 == 1
            lo[sy - 1, sx - 1] = np.float32(0.8472979)
            lo[sy - 1, 0] = np.float32(np.nan)
            g.upload_level(0, lo)
            assert device_extents(g) == (want[0], want[1], sx - 1, sy - 1) == ic.extents_model(lo)
            meta = ic.metadata((0.05, sx, sy, 1, (0.5, 0.5)), 0)
            poses = ic.poses(meta, sx, sy)[:13]
            tiles, boxes = device_tiles(g, 0, poses, 64, 64)
            want_tiles, want_boxes = ic.tiles_model(lo, meta, poses, 64, 64)
            assert np.array_equal(tiles, want_tiles) and np.array_equal(boxes, want_boxes)
        g.close()


# ---- 3: map state ------------------------------------------------------------------------------------------------------------------------
def test_shift_then_update_and_the_boxes_of_the_other_consumers(capi, layout):
    geom = ic.PYRAMID_GEOM
    g, twin = (support.new_context(capi, *geom[:4], start=geom[4], layout=layout) for _ in range(2))
    scans = ic.pyramid_scans()
    for c in (g, twin):
        for pose, pts in scans[:-1]:
            support.single_update(capi, c, pose, pts)
    sx, sy = mc.level_size(geom, 0)
    meta0 = ic.metadata(geom, 0)
    poses = ic.poses(meta0, sx, sy)
    before = ic.tiles_model(g.download_level(0)[0], meta0, poses, 5, 3)
    # tiles after a window move use the moved origin
    for c in (g, twin):
        assert c.shift_map(c.start_for_shift(1, -1)) != (0, 0)
    moved = (geom[0], sx, sy, geom[3], tuple(float(v) for v in g.map_start()))
    for lvl in range(geom[3]):
        meta = ic.metadata(moved, lvl)
        assert tuple(np.float32(v) for v in g.map_metadata(lvl)) == tuple(meta) and (lvl > 0 or tuple(meta) != tuple(meta0))
        lo = g.download_level(lvl)[0]
        lsx, lsy = mc.level_size(geom, lvl)
        want = ic.tiles_model(lo, meta, poses, 5, 3)
        got = device_tiles(g, lvl, poses, 5, 3)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), lvl
        if lvl == 0:
            assert not np.array_equal(want[1], before[1])  # the windows did move with the origin
        assert device_extents(g, lvl) == ic.extents_model(lo)
        assert np.array_equal(device_image(g, lvl, None, (lsy, lsx)), ic.image_model(lo))
    # both consumers' boxes are emptied; then one further update on each context
    for c in (g, twin):
        for lvl in range(geom[3]):
            c.take_dirty_bbox(lvl)
            c.occupancy_changes(lvl, np.zeros(mc.level_size(geom, lvl)[::-1], np.int8))
    old_lo = g.download_level(0)[0]
    old_extents, old_image = device_extents(g), device_image(g, 0, None, (sy, sx))
    for c in (g, twin):
        support.single_update(capi, c, *scans[-1])
    lo = g.download_level(0)[0]
    assert not np.array_equal(ic.published(lo), ic.published(old_lo))  # the update changed cells of the published grid
    # ... after which every entry runs on g, and none on the twin
    for lvl in range(geom[3]):
        level_lo = g.download_level(lvl)[0]
        lsx, lsy = mc.level_size(geom, lvl)
        assert device_extents(g, lvl) == ic.extents_model(level_lo) == tuple(int(v) for v in g.map_extents(lvl))
        assert np.array_equal(device_image(g, lvl, None, (lsy, lsx)), ic.image_model(level_lo))
        assert np.array_equal(g.map_image(lvl, (1, 1, 9, 7)), ic.image_model(level_lo, (1, 1, 9, 7)))
        meta = ic.metadata(moved, lvl)
        assert np.array_equal(device_tiles(g, lvl, poses, 5, 3)[0], ic.tiles_model(level_lo, meta, poses, 5, 3)[0])
        assert np.array_equal(g.map_tiles(lvl, poses, 1, 1)[0], ic.tiles_model(level_lo, meta, poses, 1, 1)[0])
    assert not np.array_equal(device_image(g, 0, None, (sy, sx)), old_image)  # the image changed with the update
    assert old_extents == ic.extents_model(old_lo)
    for lvl in range(geom[3]):
        shape = mc.level_size(geom, lvl)[::-1]
        assert g.occupancy_changes(lvl, np.zeros(shape, np.int8)).tolist() == twin.occupancy_changes(lvl, np.zeros(shape, np.int8)).tolist()
        assert g.take_dirty_bbox(lvl).tolist() == twin.take_dirty_bbox(lvl).tolist() != list(ic.EMPTY)
        assert support.same(g.download_level(lvl)[0], twin.download_level(lvl)[0])
        assert np.array_equal(g.download_level(lvl)[1], twin.download_level(lvl)[1])  # the stamps
    g.close()
    twin.close()


# ---- 4: refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_return_invalid_and_touch_nothing(big):
    import torch
    big.upload_level(0, PLANES["random_1"])
    lib, h = big._lib, big._h
    img, tiles, boxes, box = Guarded(SX * SY), Guarded(4 * 64 * 64), GuardedBoxes(4), GuardedBoxes(1)
    p = dev(POSES[:4])
    host_img, host_tiles = np.full(SX * SY, GUARD, np.uint8), np.full(4 * 64 * 64, GUARD, np.uint8)
    host_boxes, host_box = np.full((4, 4), -9, np.int32), np.full(4, -9, np.int32)
    hp = np.ascontiguousarray(POSES[:4])
    crop = np.int32([0, 0, 9, 9])

    def tiles_device(batch=4, poses=p.data_ptr(), tw=64, th=64, out=tiles.ptr, lvl=0, ctx=h):
        return lib.hsm_map_tiles_device(ctx, lvl, batch, poses, tw, th, out, boxes.ptr, None)

    def tiles_host(batch=4, poses=hp.ctypes.data, tw=64, th=64, out=host_tiles.ctypes.data, lvl=0, ctx=h):
        return lib.hsm_map_tiles(ctx, lvl, batch, poses, tw, th, out, host_boxes.ctypes.data)

    calls = {
        "extents_device: null context": lambda: lib.hsm_map_extents_device(None, 0, box.ptr, None),
        "extents_device: level -1": lambda: lib.hsm_map_extents_device(h, -1, box.ptr, None),
        "extents_device: level 1": lambda: lib.hsm_map_extents_device(h, 1, box.ptr, None),
        "extents_device: null box": lambda: lib.hsm_map_extents_device(h, 0, None, None),
        "extents: null context": lambda: lib.hsm_map_extents(None, 0, host_box),
        "extents: level 1": lambda: lib.hsm_map_extents(h, 1, host_box),
        "image_device: null context": lambda: lib.hsm_map_image_device(None, 0, None, img.ptr, None),
        "image_device: level 1": lambda: lib.hsm_map_image_device(h, 1, None, img.ptr, None),
        "image_device: null image": lambda: lib.hsm_map_image_device(h, 0, crop.ctypes.data, None, None),
        "image: null context": lambda: lib.hsm_map_image(None, 0, None, host_img.ctypes.data),
        "image: level -1": lambda: lib.hsm_map_image(h, -1, None, host_img.ctypes.data),
        "image: null image": lambda: lib.hsm_map_image(h, 0, None, None),
    }
    for name, call in (("tiles_device", tiles_device), ("tiles", tiles_host)):
        calls.update({
            name + ": null context": lambda call=call: call(ctx=None),
            name + ": level 1": lambda call=call: call(lvl=1),
            name + ": batch -1": lambda call=call: call(batch=-1),
            name + ": null poses": lambda call=call: call(poses=None),
            name + ": null tiles": lambda call=call: call(out=None),
            name + ": tile_w 0": lambda call=call: call(tw=0),
            name + ": tile_h -3": lambda call=call: call(th=-3),
            name + ": tile_w > sx": lambda call=call: call(tw=SX + 1),
            name + ": tile_h > sy": lambda call=call: call(th=SY + 1),
            name + ": more than INT_MAX bytes": lambda call=call: call(batch=2 ** 31 // (SX * SY) + 1, tw=SX, th=SY),
        })
    for what, call in calls.items():
        assert call() == HSM_ERR_INVALID, what
    # degenerate calls that are no refusal: an empty batch (null pointers and all), a crop that misses the level
    assert tiles_device(batch=0, poses=None, out=None) == 0 and tiles_host(batch=0, poses=None, out=None) == 0
    miss = np.int32([400, 0, 500, 10])
    assert lib.hsm_map_image_device(h, 0, miss.ctypes.data, img.ptr, None) == 0
    assert lib.hsm_map_image(h, 0, miss.ctypes.data, host_img.ctypes.data) == 0
    assert lib.hsm_map_image_device(h, 0, miss.ctypes.data, None, None) == 0  # (nothing to write: a null image is no error)
    # `stream` is being captured, and: a stream this context has matched on is being captured
    s, other = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s):
        b = dev(np.zeros((1, 3), np.float32))
        pts = dev(np.float32([[10.0, 0.0], [0.0, 10.0], [7.0, 7.0]]))
        out = torch.zeros((1, 3), device="cuda:0")
        big.match_batch_device(1, b.data_ptr(), pts.data_ptr(), 0, 3, out.data_ptr(), 0, s.cuda_stream)  # s: a stream `big` has matched on
        x = torch.zeros(8, device="cuda:0")
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        x.add_(1.0)
        for st in (s, other):
            for call in (lambda: big.map_extents_device(0, box.ptr, st.cuda_stream),
                         lambda: big.map_image_device(0, None, img.ptr, st.cuda_stream),
                         lambda: big.map_tiles_device(0, 4, p.data_ptr(), 64, 64, tiles.ptr, boxes.ptr, st.cuda_stream)):
                with pytest.raises(big_error(big)) as e:
                    call()
                assert f"({HSM_ERR_INVALID})" in str(e.value) and "captur" in str(e.value), str(e.value)
        x.add_(1.0)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert x.cpu().numpy().tolist() == [2.0] * 8  # the capture ended normally
    # nothing was queued: no byte, no box
    assert img.untouched() and tiles.untouched() and boxes.untouched() and box.untouched()
    assert (host_img == GUARD).all() and (host_tiles == GUARD).all() and (host_boxes == -9).all() and (host_box == -9).all()
    # ... and the entries still work
    assert device_extents(big) == ic.extents_model(PLANES["random_1"])


def big_error(g):
    from hector_slam_amd import capi as m
    return m.HsmError
