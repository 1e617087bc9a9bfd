"""Rectangular maps: geometries whose width and height differ a lot, and the scenes, hypothesis strategy and SLAM loop the
tests run on them.  Every geometry appears with its transpose, so that a kernel or host path that swaps or mixes the two
axes fails on one of the pair, whichever way the mistake goes.  Pure numpy (hypothesis is imported where a strategy is
asked for); shared by the CPU pin (restatement == reference headers, tests/test_oracle_vs_reference.py) and the GPU tests
(tests/test_gpu_rect_maps.py)."""
import numpy as np

RES = 0.05

GEOMETRIES = [  # (sx, sy, levels)
    (640, 192, 3),    # wide: rows a multiple of 64 on every level (the aligned dense apply path), 3:1
    (192, 640, 3),    # tall
    (333, 90, 2),     # sx % 4 != 0: partial quad tiles and the unaligned keyed apply; 45 rows (odd) at level 1
    (90, 333, 2),
    (1000, 24, 3),    # strip: level 2 is 250 x 6 (limy = 4, fewer than 8 rows per 16 x 8 mark tile), most beams off the map
    (24, 1000, 3),
    (8192, 1040, 1),  # more than 2^23 cells: the large-map matcher forms and the automatic sort, tile shift set by sx only
    (1040, 8192, 1),
]
LARGE = [g for g in GEOMETRIES if g[0] * g[1] > (1 << 23)]
SMALL = [g for g in GEOMETRIES if g not in LARGE]


def gid(g):
    return "%dx%d_L%d" % g


def world_for(sx, sy, res, grow, seed):
    """a room `grow` times the map's extent on each axis (grow > 1: many beams end outside the map)"""
    from hector_slam_amd import synth
    w, h = sx * res * grow, sy * res * grow
    room = synth.World.make(w, h, n_boxes=0)
    # boxes sized by the SHORTER side (synth.World.make sizes them by the width), off the loop's ellipse
    rng = np.random.default_rng(seed)
    segs = [room.segments]
    while len(segs) < 5:
        bw, bh = rng.uniform(0.05, 0.15, 2) * min(w, h)
        cx, cy = rng.uniform(-0.45, 0.45) * w, rng.uniform(-0.45, 0.45) * h
        if abs(np.hypot(cx / (0.125 * w), cy / (0.125 * h)) - 1.0) < 0.5:
            continue
        x0, x1, y0, y1 = cx - bw / 2, cx + bw / 2, cy - bh / 2, cy + bh / 2
        segs.append(np.array([(x0, y0, x1, y0), (x1, y0, x1, y1), (x1, y1, x0, y1), (x0, y1, x0, y0)]))
    return synth.World(np.concatenate(segs), w, h)


def scene(sx, sy, steps, beams, seed, res=RES, grow=0.9):
    """(world, ground-truth poses (steps, 3), scans) of a loop inside the room, level-0 cell units"""
    from hector_slam_amd import synth
    world = world_for(sx, sy, res, grow, seed)
    s = float(np.float32(1.0) / np.float32(res))
    poses = synth.loop_trajectory(world, steps, frac=0.25).astype(np.float32)
    noise = np.random.default_rng(seed)
    scans = [synth.make_scan(world, p, beams, s, noise, range_max=min(30.0, max(sx, sy) * res)) for p in poses]
    return world, poses, scans


def levels_for(sx, sy, levels, floor=8):
    while (min(sx, sy) >> (levels - 1)) < floor:
        levels -= 1
    return levels


# the seeded property (hypothesis' @seed, no example database): the CPU pin and the GPU test draw the same examples
RECT_SEED = 20261016
RECT_SIZES = [24, 64, 90, 125, 192, 333, 640]


def rect_geometry():
    """independent size_x and size_y, levels, resolution, start coordinates, update factors, fan, room and laser origin"""
    from hypothesis import strategies as st
    return st.fixed_dictionaries({
        "size_x": st.sampled_from(RECT_SIZES),
        "size_y": st.sampled_from(RECT_SIZES),
        "levels": st.integers(1, 3),
        "res": st.sampled_from([0.05, 0.1]),
        "start": st.tuples(st.floats(0.3, 0.7), st.floats(0.3, 0.7)),
        "free": st.floats(0.3, 0.49),
        "occ": st.floats(0.55, 0.95),
        "beams": st.sampled_from([181, 400, 1081, 4096]),
        "grow": st.sampled_from([0.6, 0.9, 1.15]),
        "seed": st.integers(0, 2 ** 20),
        "origo": st.tuples(st.floats(-2, 2), st.floats(-2, 2)),
    })


def reference_undefined(impl) -> bool:
    """the restatement counts map reads with a NaN coordinate: where the reference would index its grid with (int)NaN and
    crash (tests/test_property_hypothesis.py), so the input has no reference result"""
    o = impl.get("keep")
    return hasattr(o, "undefined_reads") and o.undefined_reads() > 0


def oracle_impl(pyoracle, kind):
    def make(res, sx, sy, levels, start, free, occ):
        o = pyoracle.Oracle(kind, res, sx, sy, levels, start)
        o.set_update_factor_free(free)
        o.set_update_factor_occupied(occ)

        def upd(p, sc, og):
            o.update_by_scan(p, sc, og)
            o.on_map_updated()
        return {"match": lambda h, sc, og: o.match(h, sc, og), "update": upd, "level": o.download_level, "keep": o}
    return make


def run_loop(g, make_a, make_b, steps=6, make_guard=None):
    """the short SLAM loop of a rect_geometry example on two implementations (a match, then an update at the matched pose):
    every pose, covariance and the final maps bit-identical.  make_guard: a restatement stepped ahead of b when b is the
    reference, so that an input on which the reference would crash is discarded (hypothesis.assume)"""
    from hypothesis import assume
    sx, sy, res = g["size_x"], g["size_y"], g["res"]
    levels = levels_for(sx, sy, g["levels"])
    world = world_for(sx, sy, res, g["grow"], g["seed"])
    from hector_slam_amd import synth
    s = float(np.float32(1.0) / np.float32(res))
    poses = synth.loop_trajectory(world, steps + 1, frac=0.25).astype(np.float32)
    noise = np.random.default_rng(g["seed"])
    scans = [synth.make_scan(world, p, g["beams"], s, noise, range_max=min(30.0, max(sx, sy) * res)) for p in poses]
    origo = np.asarray(g["origo"], np.float32)
    args = (res, sx, sy, levels, g["start"], g["free"], g["occ"])
    a, b = make_a(*args), make_b(*args)
    guard = make_guard(*args) if make_guard else None
    pose = poses[0].copy()
    for t in range(steps):
        hint = pose + (poses[t] - poses[max(t - 1, 0)])
        pa, ca = a["match"](hint, scans[t], origo)
        assume(not reference_undefined(a))
        if guard is not None:
            guard["match"](hint, scans[t], origo)
            assume(not reference_undefined(guard))
        pb, cb = b["match"](hint, scans[t], origo)
        assume(not reference_undefined(b))
        if not np.isfinite(pa).all():  # singular H: the reference divides by a zero determinant (NaN payloads not pinned)
            assert np.array_equal(np.isnan(pa), np.isnan(pb))
            return
        assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32)) and np.array_equal(ca.view(np.uint32), cb.view(np.uint32)), \
            (g, t, pa, pb)
        for impl in (a, b) + ((guard,) if guard is not None else ()):
            impl["update"](pa, scans[t], origo)
        for impl in (a, b):
            if "check" in impl:
                impl["check"](g, t)
        pose = pa
    for lvl in range(levels):
        la, lb = a["level"](lvl), b["level"](lvl)
        assert np.array_equal(la[0].view(np.uint32), lb[0].view(np.uint32)) and np.array_equal(la[1], lb[1]), (g, lvl)
