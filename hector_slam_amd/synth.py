"""Deterministic synthetic worlds, laser scans and trajectories.

The reference ships no bag files or fixtures, so every input used by the tests
and by bench.py is generated here from seeds: an axis-aligned room with box
obstacles, analytic ray casting, Gaussian range noise, and the same range
filtering / range->endpoint conversion the ROS node applies before the scan
reaches the matcher (hector_mapping/src/HectorMappingRos.cpp:483-507,
``rosLaserScanToDataContainer``: keep ``range_min < r < range_max - 0.1``,
endpoint = (cos(a) r s, sin(a) r s) with s = scaleToMap, all fp32).

Pure numpy (plus the C library's cosf / sinf for the node's sensor table), no GPU, no oracle: this module only
produces inputs.
"""
from __future__ import annotations

import ctypes
import ctypes.util
import dataclasses
import functools
import math

import numpy as np

# beam fans named in BASELINE.json configs
SCAN_SHAPES = {
    181: (-math.pi / 2, math.pi / 180.0),                    # 180 deg / 1 deg
    1081: (-math.radians(135.0), math.radians(0.25)),        # Hokuyo UTM-30LX 270 deg / 0.25 deg
    16384: (-math.pi, 2.0 * math.pi / 16384.0),              # dense multi-echo / 3D-projected
}


@dataclasses.dataclass
class World:
    """Room + obstacles as a list of wall segments, world frame, metres."""
    segments: np.ndarray  # (M, 4) float64: x0, y0, x1, y1
    width: float
    height: float

    @staticmethod
    def make(width: float = 40.0, height: float = 30.0, n_boxes: int = 12, seed: int = 1234,
             box_min: float = 0.5, box_max: float = 3.0, keep_clear: float = 2.5) -> "World":
        rng = np.random.default_rng(seed)
        hw, hh = width / 2.0, height / 2.0
        segs = [(-hw, -hh, hw, -hh), (hw, -hh, hw, hh), (hw, hh, -hw, hh), (-hw, hh, -hw, -hh)]
        n = 0
        while n < n_boxes:
            bw, bh = rng.uniform(box_min, box_max, size=2) * (width / 40.0)
            cx = rng.uniform(-hw + bw, hw - bw)
            cy = rng.uniform(-hh + bh, hh - bh)
            # keep the trajectory corridor (an ellipse at 55% of the room) free
            if abs(math.hypot(cx / (0.55 * hw), cy / (0.55 * hh)) - 1.0) < keep_clear / min(hw, hh):
                continue
            x0, x1, y0, y1 = cx - bw / 2, cx + bw / 2, cy - bh / 2, cy + bh / 2
            segs += [(x0, y0, x1, y0), (x1, y0, x1, y1), (x1, y1, x0, y1), (x0, y1, x0, y0)]
            n += 1
        return World(np.asarray(segs, dtype=np.float64), width, height)

    def raycast(self, pose, angles: np.ndarray) -> np.ndarray:
        """Exact ranges (float64) for beams at robot-frame ``angles`` from ``pose``=(x,y,theta)."""
        x, y, th = (float(v) for v in pose)
        a = angles.astype(np.float64) + th
        dx, dy = np.cos(a)[:, None], np.sin(a)[:, None]
        sx0, sy0, sx1, sy1 = (self.segments[:, i][None, :] for i in range(4))
        ex, ey = sx1 - sx0, sy1 - sy0
        den = dx * ey - dy * ex
        with np.errstate(divide="ignore", invalid="ignore"):
            t = ((sx0 - x) * ey - (sy0 - y) * ex) / den
            u = ((sx0 - x) * dy - (sy0 - y) * dx) / den
        ok = (np.abs(den) > 1e-12) & (t > 1e-9) & (u >= 0.0) & (u <= 1.0)
        t = np.where(ok, t, np.inf)
        return t.min(axis=1)


_ANGLE_CACHE: dict = {}


def beam_angles(n_beams: int) -> np.ndarray:
    """the fan's beam angles (cached per fan: every scan of a bench batch shares them; callers do not modify the array)"""
    if n_beams in _ANGLE_CACHE:
        return _ANGLE_CACHE[n_beams]
    a0, inc = SCAN_SHAPES[n_beams] if n_beams in SCAN_SHAPES else (-math.pi, 2.0 * math.pi / n_beams)
    # the node accumulates ``angle += angle_increment`` in fp32 (HectorMappingRos.cpp:491,505)
    out = np.empty(n_beams, dtype=np.float32)
    ang = np.float32(a0)
    inc32 = np.float32(inc)
    for i in range(n_beams):
        out[i] = ang
        ang = np.float32(ang + inc32)
    out.setflags(write=False)
    _ANGLE_CACHE[n_beams] = out
    return out


def scan_to_points(ranges: np.ndarray, angles: np.ndarray, scale_to_map: float,
                   range_min: float = 0.4, range_max: float = 30.0) -> np.ndarray:
    """LaserScan ranges -> DataContainer endpoints, fp32, robot frame, level-0 cell units."""
    r = ranges.astype(np.float32)
    keep = (r > np.float32(range_min)) & (r < np.float32(range_max) - np.float32(0.1))
    r = r[keep] * np.float32(scale_to_map)
    a = angles[keep].astype(np.float32)
    pts = np.empty((r.shape[0], 2), dtype=np.float32)
    pts[:, 0] = np.cos(a).astype(np.float32) * r
    pts[:, 1] = np.sin(a).astype(np.float32) * r
    return pts


@functools.lru_cache(maxsize=16)
def _node_trig(n: int, a0_bits: int, inc_bits: int) -> np.ndarray:
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    cosf, sinf = libm.cosf, libm.sinf
    for f in (cosf, sinf):
        f.restype, f.argtypes = ctypes.c_float, [ctypes.c_float]
    inc = np.array([inc_bits], np.uint32).view(np.float32)[0]
    angle = np.array([a0_bits], np.uint32).view(np.float32)[0]
    t = np.empty((n, 2), np.float32)
    for i in range(n):
        t[i] = cosf(float(angle)), sinf(float(angle))
        angle = np.float32(angle + inc)
    t.setflags(write=False)
    return t


def node_scan_trig(n: int, angle_min: float, angle_increment: float) -> np.ndarray:
    """(cos, sin) per beam as the node evaluates them: the C library's float cosf / sinf of the running fp32 angle
    (HectorMappingRos.cpp:487,502,505); [n, 2] float32, read-only"""
    bits = np.array([angle_min, angle_increment], np.float32).view(np.uint32)
    return _node_trig(int(n), int(bits[0]), int(bits[1]))


def ranges_to_csr(ranges: np.ndarray, angle_min: float, angle_increment: float, range_min: float, range_max: float,
                  scale_to_map: float):
    """rosLaserScanToDataContainer (HectorMappingRos.cpp:483-507) for B scans of one geometry, ranges [B, n], laid out as
    the batched matcher's CSR input: (counts [B] int32, offsets [B + 1] int32, endpoints [total, 2] float32, level-0 cell
    units, each scan's kept beams in beam order).  fp32 throughout: keep iff range_min < r < range_max - 0.1f (NaN and
    +-inf fail both), then r * scale_to_map, then (cos * r, sin * r)."""
    r = np.ascontiguousarray(ranges, np.float32)
    B, n = r.shape
    with np.errstate(invalid="ignore"):
        keep = (r > np.float32(range_min)) & (r < np.float32(np.float32(range_max) - np.float32(0.1)))
    counts = keep.sum(1).astype(np.int32)
    offsets = np.zeros(B + 1, np.int32)
    np.cumsum(counts, out=offsets[1:])
    t = node_scan_trig(n, angle_min, angle_increment)
    rows, beams = np.nonzero(keep)  # row-major: scan by scan, beams in order
    d = r[rows, beams] * np.float32(scale_to_map)
    pts = np.empty((d.shape[0], 2), np.float32)
    pts[:, 0] = t[beams, 0] * d
    pts[:, 1] = t[beams, 1] * d
    return counts, offsets, pts


@functools.lru_cache(maxsize=16)
def _laser_units(n: int, a0_bits: int, inc_bits: int) -> np.ndarray:
    a0, inc = (float(v) for v in np.array([a0_bits, inc_bits], np.uint32).view(np.float32))  # float -> double is exact
    t = np.empty((n, 2), np.float64)
    for i in range(n):
        a = a0 + float(i) * inc  # fp64: a product, then a sum
        t[i] = math.cos(a), math.sin(a)
    t.setflags(write=False)
    return t


def laser_unit_vectors(n: int, angle_min: float, angle_increment: float) -> np.ndarray:
    """laser_geometry's unit vectors: the C library's double cos / sin of angle_min + (double)i * angle_increment, the float
    geometry widened to double; one math.cos / math.sin call per element (numpy's vectorised ones need not give the same
    bits); [n, 2] float64, read-only"""
    bits = np.array([angle_min, angle_increment], np.float32).view(np.uint32)
    return _laser_units(int(n), int(bits[0]), int(bits[1]))


def ranges_tf_to_csr(ranges: np.ndarray, angle_min: float, angle_increment: float, range_min: float, range_max: float,
                     range_cutoff: float, tf_rows: np.ndarray, sqr_laser_min_dist: float, sqr_laser_max_dist: float,
                     laser_z_min: float, laser_z_max: float, scale_to_map: float):
    """The node's default ingestion (projectLaser, the laser -> base transform, rosPointCloudToDataContainer,
    HectorMappingRos.cpp:257-282,509-542) for B scans of one geometry, ranges [B, n]; tf_rows [B, 12] float64 rows [R | t] per
    scan, or [12] for every scan.  Returns (counts [B] int32, offsets [B + 1] int32, endpoints [total, 2] float32 in level-0
    cell units, each scan's kept beams in beam order, origos [B, 2] float32).  Per beam, with the types the node has:
      point   = float32(float64(range) * unit)               z = 0
      valid   = float64(range) < cutoff and range >= range_min          (cutoff < 0 means range_max)
      dist2   = x * x + y * y in float32, kept in (sqr_min, sqr_max) and not (x < 0 and dist2 < 0.5)
      base    = (T0 * x + T1 * y + T2 * z) + T3 per row in float64, every product and sum rounded on its own
      z gate  = float32(base_z - T11) in (z_min, z_max)
      out     = float32(base_x) * scale, float32(base_y) * scale;   origo = float32(T3) * scale, float32(T7) * scale"""
    f32, f64 = np.float32, np.float64
    r = np.ascontiguousarray(ranges, f32)
    B, n = r.shape
    T = np.ascontiguousarray(tf_rows, f64)
    T = np.broadcast_to(T, (B, 12)) if T.ndim == 1 else T.reshape(B, 12)
    cutoff = f64(range_max if range_cutoff < 0 else range_cutoff)
    u = laser_unit_vectors(n, angle_min, angle_increment)
    scale = f32(scale_to_map)
    with np.errstate(invalid="ignore", over="ignore"):
        rd = r.astype(f64)
        x, y = (rd * u[:, 0]).astype(f32), (rd * u[:, 1]).astype(f32)
        keep = (rd < cutoff) & (r >= f32(range_min))
        d2 = x * x + y * y
        keep &= (d2 > f32(sqr_laser_min_dist)) & (d2 < f32(sqr_laser_max_dist)) & ~((x < f32(0)) & (d2 < f32(0.5)))
        vx, vy, vz = x.astype(f64), y.astype(f64), np.zeros((B, n), f64)
        t = [T[:, k:k + 1] for k in range(12)]
        bx = ((t[0] * vx + t[1] * vy) + t[2] * vz) + t[3]
        by = ((t[4] * vx + t[5] * vy) + t[6] * vz) + t[7]
        bz = ((t[8] * vx + t[9] * vy) + t[10] * vz) + t[11]
        zl = (bz - t[11]).astype(f32)
        keep &= (zl > f32(laser_z_min)) & (zl < f32(laser_z_max))
        ex, ey = bx.astype(f32) * scale, by.astype(f32) * scale
    counts = keep.sum(1).astype(np.int32)
    offsets = np.zeros(B + 1, np.int32)
    np.cumsum(counts, out=offsets[1:])
    rows, beams = np.nonzero(keep)  # row-major: scan by scan, beams in order
    pts = np.stack([ex[rows, beams], ey[rows, beams]], 1).astype(f32).reshape(-1, 2)
    origos = np.stack([T[:, 3].astype(f32) * scale, T[:, 7].astype(f32) * scale], 1)
    return counts, offsets, pts, origos


def make_scan(world: World, pose, n_beams: int, scale_to_map: float, rng: np.random.Generator | None,
              noise_sigma: float = 0.01, range_max: float = 30.0, pad_to_full: bool = False) -> np.ndarray:
    """One scan taken at ground-truth ``pose``; returns (n_valid, 2) fp32 endpoints.

    With ``pad_to_full`` invalid returns are clamped into range instead of dropped so
    every scan has exactly ``n_beams`` endpoints (fixed-shape batches for the bench).
    """
    ang = beam_angles(n_beams)
    r = world.raycast(pose, ang)
    if rng is not None and noise_sigma > 0:
        r = r + rng.normal(0.0, noise_sigma, size=r.shape)
    if pad_to_full:
        r = np.clip(r, 0.45, range_max - 0.2)
    return scan_to_points(r, ang, scale_to_map, range_max=range_max)


def loop_trajectory(world: World, n_poses: int, frac: float = 0.55, phase: float = 0.0) -> np.ndarray:
    """Elliptic loop inside the room, heading tangent to the path; (n, 3) float64."""
    t = phase + np.linspace(0.0, 2.0 * math.pi, n_poses, endpoint=False)
    x = frac * world.width / 2.0 * np.cos(t)
    y = frac * world.height / 2.0 * np.sin(t)
    th = np.arctan2(frac * world.height / 2.0 * np.cos(t), -frac * world.width / 2.0 * np.sin(t))
    return np.stack([x, y, th], axis=1)


def perturb_poses(poses: np.ndarray, rng: np.random.Generator, d_xy: float = 0.15,
                  d_th: float = 0.05) -> np.ndarray:
    """Initial estimates = truth + U[-d_xy, d_xy] m, U[-d_th, d_th] rad (inside the GN basin)."""
    out = poses.astype(np.float64).copy()
    out[:, :2] += rng.uniform(-d_xy, d_xy, size=(poses.shape[0], 2))
    out[:, 2] += rng.uniform(-d_th, d_th, size=poses.shape[0])
    return out.astype(np.float32)


@dataclasses.dataclass
class Scene:
    """Everything needed to exercise the path: map-building scans and query scans."""
    world: World
    resolution: float
    map_size: int
    levels: int
    n_beams: int
    build_poses: np.ndarray          # (T, 3) float32 ground-truth poses used to build the map
    build_scans: list                # T arrays (n_i, 2) float32
    query_truth: np.ndarray          # (B, 3) float32
    query_init: np.ndarray           # (B, 3) float32 perturbed start estimates
    query_scans: list                # B arrays (n_i, 2) float32

    @property
    def scale_to_map(self) -> float:
        return float(np.float32(1.0) / np.float32(self.resolution))


def make_scene(n_beams: int = 1081, map_size: int = 2048, levels: int = 3, resolution: float = 0.05,
               n_build: int = 200, n_query: int = 64, room=(40.0, 30.0), seed: int = 1234,
               pad_to_full: bool = False, range_max: float = 30.0) -> Scene:
    world = World.make(room[0], room[1], seed=seed)
    s = float(np.float32(1.0) / np.float32(resolution))
    rng_noise = np.random.default_rng(seed + 1)
    rng_init = np.random.default_rng(seed + 2)
    build_poses = loop_trajectory(world, n_build).astype(np.float32)
    build_scans = [make_scan(world, p, n_beams, s, rng_noise, range_max=range_max) for p in build_poses]
    query_truth = loop_trajectory(world, n_query, phase=0.37 * 2 * math.pi / max(n_build, 1)).astype(np.float32)
    query_scans = [make_scan(world, p, n_beams, s, rng_noise, pad_to_full=pad_to_full, range_max=range_max)
                   for p in query_truth]
    query_init = perturb_poses(query_truth, rng_init)
    return Scene(world, resolution, map_size, levels, n_beams, build_poses, build_scans,
                 query_truth, query_init, query_scans)


def pack_scans(scans) -> tuple[np.ndarray, np.ndarray]:
    """CSR packing used by the batched C ABI: (total, 2) fp32 points + (B+1,) int32 offsets."""
    offs = np.zeros(len(scans) + 1, dtype=np.int32)
    for i, s in enumerate(scans):
        offs[i + 1] = offs[i] + s.shape[0]
    pts = np.concatenate(scans, axis=0).astype(np.float32) if scans else np.zeros((0, 2), np.float32)
    return np.ascontiguousarray(pts), offs
