"""Float64 reference of ONE Gauss-Newton evaluation (getCompleteHessianDerivs, OccGridMapUtil.h:64-104) and the rounding
bound a tree-summed fp32 kernel must meet against it.  A test helper, not a conftest: the fast-mode tests of
test_gpu_parity.py check every kernel form's H and dTr with it, test_gn_f64_reference.py checks the helper itself.

Per beam the float32 factors are the reference's bits, built exactly as test_per_beam_terms_bit_exact builds them: the
oracle's `interp` (M, gx, gy) at the fp32 transform t + (c*x + (-s)*y), sin/cos from the host libm, rotDeriv as the
source's fp32 expression, funVal = 1 - M in fp32.  The nine products and their sums are then formed in float64.

The bound.  A kernel multiplies two fp32 factors (one rounding, relative error <= u = 2^-24) and adds each product into
a sum through at most `d` fp32 additions.  With p_i the exact products, the computed sum s satisfies
    |s - sum p_i| <= gamma(d + 1) * sum |p_i|,      gamma(k) = k u / (1 - k u)
(Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., 4.2: every term carries at most d + 1 factors
(1 + delta)).  d is the longest chain of additions a single beam's product passes through, read off the kernel source
(hector_slam_amd/csrc/: gn_match_teams.h, gn_match_cached.h, gn_match_dense.h, probe_kernels.h; the reductions: gn_step.h):

  gn_match_kernel<W, SPB, L, BPL>  (team forms, T = 64 W lanes per scan): lane j adds the beams j, j + T, j + 2T, ...
      into its own accumulator (BPL register-resident beams, padding slots add exact zeros, beams beyond T * BPL stream
      in the same per-lane order) -> ceil(n / T) additions; then wave_allreduce9: six butterfly levels (permlane32,
      permlane16, row_mirror, row_half_mirror, quad_perm x2) -> 6; then team_allreduce9: lane t adds the W wave
      partials in wave order, a sequential chain -> W - 1.
          d = ceil(n / T) + 6 + (W - 1)
  gn_match_cached_kernel<SPB, BPL, L, 1, RELAXED>  (one wave per scan, SPB scans per workgroup that never mix):
      the BPL cached beams of a lane in order, then the streamed tail in the same per-lane order, then
      wave_allreduce9 -> d = ceil(n / 64) + 6.  RELAXED contracts the accumulation into v_fma_f32 (the product is
      not rounded on its own: the bound above still holds) but also evaluates the per-beam factors with contracted
      multiply-adds, so its factors are not the reference's bits; its cases take the factors of relaxed_factors(),
      the same expressions with an exact fma, instead.
  gn_match_coop_kernel  (K <= 64 workgroups of 256 lanes, one scan): lane g adds beams g, g + 256 K, ... ->
      ceil(n / (256 K)); wave_allreduce9 -> 6; the four wave partials ((r0 + r1) + r2) + r3 -> 3; the K workgroup
      partials through one more wave_allreduce9 (lanes >= K add zeros) -> 6.
          d = ceil(n / (256 K)) + 15
  gn_eval_kernel  (hsm_hessian_derivs in the fast mode; 1024 lanes): ceil(n / 1024) + 6 + 15.
  the oracle's hessian_derivs (one sequential chain per term): d = n.

Subnormal terms.  The relative bound assumes that a product rounds with a relative error of u, which holds only while the
product is a normal fp32 number.  A product that underflows is rounded to a multiple of the smallest subnormal, s = 2^-149:
an absolute error of up to s / 2 however small the product (sums of subnormals are exact, so the additions add nothing).  With
n beams the sum is off by at most n s / 2 more; bound() adds the floor n s -- one subnormal ulp per addition -- to every entry
that has a non-zero term.  On maps of young cells the floor is some 1e-42 next to bounds of 1e-6: it changes no verdict there.
On aged maps (tests/aged_cases.py: probabilities of 1e-38 and below) it is the whole bound.

The GPU tests compare H entry by entry with bound(); a kernel that loses or double-counts beam i moves an entry by
|p_i|, which a test sees where |p_i| > 2 * bound (the bound is the rounding allowance on both sides).  beam_margin()
is that ratio, and the test scans are chosen (gn_cases.make_scan) so that it exceeds 1 for every non-zero beam.
"""
from __future__ import annotations

import math

import numpy as np

U = 2.0 ** -24
SUBNORMAL_ULP = 2.0 ** -149  # the spacing of fp32 below 2^-126

# entry order of the 12 sums: H as a row-major 3x3 (9, symmetric), then dTr (3)
H_IDX = [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2)]


def gamma(k: int) -> float:
    return k * U / (1.0 - k * U)


def depth_team(n: int, wps: int) -> int:
    """gn_match_kernel<W, ...> and gn_match_cached_kernel (W = 1)"""
    return -(-n // (64 * wps)) + 6 + (wps - 1)


def depth_coop(n: int, k: int) -> int:
    return -(-n // (256 * k)) + 15


def depth_eval(n: int) -> int:
    return -(-n // 1024) + 6 + 15


def coop_workgroups(n: int) -> int:
    """K of gn_match_coop_kernel: one workgroup per 256 beams, at most 64 (what last_launch_config()['grid'] reports)"""
    return min((n + 255) // 256, 64)


def _fma(a, b, c):
    """fp32 fma: the product of two fp32 values is exact in float64, the sum rounds once more (a double rounding that
    can differ from the fused operation only where the float64 sum lies exactly half-way between two fp32 values)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def relaxed_factors(prob, pm, pts, s, c):
    """(M, gx, gy, rotDeriv) as gn_match_cached_kernel<.., RELAXED = true> computes them (gn_match_cached.h, `locate` and
    `consume`): the rotation, the bilinear blend as two lerps, the gradient blends and rotDeriv as contracted
    multiply-adds.  Its endpoint positions differ from the reference's in the last bit, so a beam within an ulp of a cell
    border may sample the neighbouring cell, whose source-literal gradient is another one: the reference's factors are
    no model of this form there, these are.  prob: the level's probability plane [sy, sx]; off-map beams sample zeros."""
    f = np.float32
    x, y = pts[:, 0], pts[:, 1]
    rx = _fma(c, x, -(f(s) * y))
    ry = _fma(s, x, f(c) * y)
    tx = (f(pm[0]) + f(0.0) + rx).astype(f)
    ty = (f(pm[1]) + f(0.0) + ry).astype(f)
    sy, sx = prob.shape
    oob = ~((tx >= 0) & (ty >= 0) & (tx <= f(sx - 2)) & (ty <= f(sy - 2)))  # (NaN and huge values: out)
    ix = np.where(oob, 0, np.nan_to_num(tx)).astype(np.int64)
    iy = np.where(oob, 0, np.nan_to_num(ty)).astype(np.int64)
    fx = np.where(oob, f(0), tx - ix.astype(f)).astype(f)
    fy = np.where(oob, f(0), ty - iy.astype(f)).astype(f)
    z = f(0)
    i0 = np.where(oob, z, prob[iy, ix])
    i1 = np.where(oob, z, prob[iy, np.minimum(ix + 1, sx - 1)])
    i2 = np.where(oob, z, prob[np.minimum(iy + 1, sy - 1), ix])
    i3 = np.where(oob, z, prob[np.minimum(iy + 1, sy - 1), np.minimum(ix + 1, sx - 1)])
    xi, yi = (f(1) - fx).astype(f), (f(1) - fy).astype(f)
    dx1, dx2, dy1, dy2 = (i0 - i1).astype(f), (i2 - i3).astype(f), (i0 - i2).astype(f), (i1 - i3).astype(f)
    t0, t1 = _fma(-fx, dx1, i0), _fma(-fx, dx2, i2)
    M = _fma(fy, (t1 - t0).astype(f), t0)
    Gx = _fma(dx2, fx, (dx1 * xi).astype(f))
    Gy = _fma(dy2, fy, (dy1 * yi).astype(f))
    rot = _fma(ry, Gx, -(rx * Gy).astype(f))
    return M, (-Gx).astype(f), (-Gy).astype(f), rot


class Eval64:
    """One evaluation at `pose_map` (map frame of `level`) over level-scaled points `pts`.

    Attributes: fac (n, 5) float32 [M, gx, gy, rotDeriv, funVal]; terms (n, 12) float64 per-beam contributions in the
    order H_IDX then dTr; H (3, 3), dTr (3,) float64 sums; absH (3, 3), absd (3,) the sums of |contribution|."""

    def __init__(self, oracle, level: int, pose_map, pts, kind: str = "ho", relaxed_prob=None):
        """relaxed_prob: the level's probability plane -- the factors are then those of the RELAXED kernel
        (relaxed_factors) instead of the reference's"""
        from oracle import pyoracle
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
        pm = np.asarray(pose_map, np.float32)
        s, c = (v[0] for v in pyoracle.libm_sincosf(pm[2:3], kind))
        x, y = pts[:, 0], pts[:, 1]
        with np.errstate(over="ignore", invalid="ignore"):
            tx = pm[0] + (c * x + (-s) * y)
            ty = pm[1] + (s * x + c * y)
            self.coords = np.stack([tx, ty], 1).astype(np.float32)
            if relaxed_prob is not None:
                M, gx, gy, rot = relaxed_factors(relaxed_prob, pm, pts, s, c)
            else:
                ref = oracle.interp(level, self.coords) if pts.shape[0] else np.zeros((0, 3), np.float32)
                M, gx, gy = ref[:, 0], ref[:, 1], ref[:, 2]
                rot = ((-s * x - c * y) * gx + (c * x - s * y) * gy).astype(np.float32)
        fun = (np.float32(1.0) - M).astype(np.float32)
        self.fac = np.stack([M, gx, gy, rot, fun], 1)
        g = [gx.astype(np.float64), gy.astype(np.float64), rot.astype(np.float64)]
        f = fun.astype(np.float64)
        t = np.empty((pts.shape[0], 12), np.float64)
        for k, (r, cc) in enumerate(H_IDX):
            t[:, k] = g[r] * g[cc]
        for r in range(3):
            t[:, 9 + r] = g[r] * f
        self.terms = t
        self.H = t[:, :9].sum(0).reshape(3, 3)
        self.dTr = t[:, 9:].sum(0)
        a = np.abs(t).sum(0)
        self.absH = a[:9].reshape(3, 3)
        self.absd = a[9:]

    @property
    def n(self) -> int:
        return self.terms.shape[0]

    def bound(self, d: int):
        """(H bound (3, 3), dTr bound (3,)) of an fp32 form with addition depth d"""
        gm = gamma(d + 1)
        floor = self.n * SUBNORMAL_ULP  # products that underflow: see "Subnormal terms" above
        return gm * self.absH + np.where(self.absH > 0, floor, 0.0), gm * self.absd + np.where(self.absd > 0, floor, 0.0)

    def beam_margin(self, d: int):
        """per beam: max over the 12 entries of |p_ie| / (2 * allowance_e); inf-free, 0 for beams whose terms are all
        zero.  A dropped or doubled beam i is seen by an entry-wise check at that allowance where this exceeds 1."""
        bh, bd = self.bound(d)
        b = np.concatenate([bh.reshape(-1), bd])
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(b > 0, np.abs(self.terms) / (2.0 * np.where(b > 0, b, 1.0)), np.where(self.terms != 0, np.inf, 0.0))
        return r.max(1)

    def nonzero(self):
        return np.any(self.terms != 0.0, axis=1)


def check_H(Hg, ev: Eval64, d: int, what: str):
    """entry by entry |H_gpu - H64| <= bound; H_gpu bitwise symmetric.  Returns the worst used fraction."""
    Hg = np.asarray(Hg, np.float32).reshape(3, 3)
    assert np.array_equal(Hg.view(np.uint32), Hg.T.view(np.uint32)), f"{what}: H not bitwise symmetric\n{Hg}"
    bh, _ = ev.bound(d)
    err = np.abs(Hg.astype(np.float64) - ev.H)
    assert (err <= bh).all(), f"{what}: |H - H64| beyond the bound (d={d})\nerr=\n{err}\nbound=\n{bh}\nH64=\n{ev.H}\nH=\n{Hg}"
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.nanmax(np.where(bh > 0, err / np.where(bh > 0, bh, 1.0), 0.0)))


def check_dtr(dg, ev: Eval64, d: int, what: str):
    _, bd = ev.bound(d)
    err = np.abs(np.asarray(dg, np.float64) - ev.dTr)
    assert (err <= bd).all(), f"{what}: |dTr - dTr64| beyond the bound (d={d}) err={err} bound={bd} dTr64={ev.dTr}"


def solve32(H, b):
    """the kernel's step, gn_solve_and_step (gn_step.h; Eigen's cofactor inverse, ScanMatcher.h:201-217) in numpy fp32 with
    the same operations in the same order: (s0, s1, s2 clamped to +-0.2) and |inverse| (3, 3) float64"""
    f = np.float32
    H = np.asarray(H, np.float32).reshape(3, 3)
    b = np.asarray(b, np.float32)
    m00, m01, m02, m11, m12, m22 = H[0, 0], H[0, 1], H[0, 2], H[1, 1], H[1, 2], H[2, 2]
    m10, m20, m21 = m01, m02, m12
    c00 = f(f(m11 * m22) - f(m12 * m21))
    c10 = f(f(m21 * m02) - f(m22 * m01))
    c20 = f(f(m01 * m12) - f(m02 * m11))
    det = f(f(c00 * m00) + f(f(c10 * m10) + f(c20 * m20)))
    invdet = f(f(1.0) / det)
    inv = np.array([[c00 * invdet, c10 * invdet, c20 * invdet],
                    [f(f(m12 * m20) - f(m10 * m22)) * invdet, f(f(m22 * m00) - f(m20 * m02)) * invdet, f(f(m02 * m10) - f(m00 * m12)) * invdet],
                    [f(f(m10 * m21) - f(m11 * m20)) * invdet, f(f(m20 * m01) - f(m21 * m00)) * invdet, f(f(m00 * m11) - f(m01 * m10)) * invdet]],
                   np.float32)
    s = np.array([f(inv[r, 0] * b[0]) + f(f(inv[r, 1] * b[1]) + f(inv[r, 2] * b[2])) for r in range(3)], np.float32)
    s[2] = min(max(s[2], f(-0.2)), f(0.2))
    return s, np.abs(inv.astype(np.float64))


def check_step(Hg, start_map, end_map, ev: Eval64, d: int, what: str) -> bool:
    """One GN step taken by the kernel: end = start + clamp(H^-1 dTr) in the map frame.  The kernel's own fp32 solve is
    replayed on the kernel's H (solve32) with dTr64 in place of the kernel's dTr; the two steps may differ by what the
    dTr allowance moves through the fp32 inverse, |inv| (bound + ulp of dTr), plus the last roundings of the step's three
    products and two sums in either solve (8 u |inv| |dTr|), plus the pose's own roundings: end = fl(start + s) and the returned world pose
    taken back to the map frame in fp32 (2 ulps of each coordinate), and normalize_angle, which rounds the angle through
    2 pi + angle in fp32 (2 ulps of 2 pi).  A rotation clamped to +-0.2 rad is compared as such.
    Returns True (checked)."""
    e0 = np.asarray(start_map, np.float32).astype(np.float64)
    e1 = np.asarray(end_map, np.float32)
    step = e1.astype(np.float64) - e0
    _, bd = ev.bound(d)
    s_ref, ainv = solve32(Hg, ev.dTr.astype(np.float32))
    ad = np.abs(ev.dTr)
    tol = ainv @ (bd + U * ad) + 8 * U * (ainv @ ad) + 2.0 * np.spacing(np.abs(e1)).astype(np.float64) + np.spacing(np.abs(e0).astype(np.float32)).astype(np.float64)
    tol[2] += 2.0 * float(np.spacing(np.float32(2 * np.pi)))  # normalize_angle: fmod + 2 pi, cast to fp32, - 2 pi
    err = np.abs(step - s_ref.astype(np.float64))
    assert (err <= tol).all(), f"{what}: step {step} vs the fp32 step from dTr64 {s_ref}: err={err} tol={tol} dTr64={ev.dTr}"
    return True


def min_margin(ev: Eval64, d: int) -> float:
    nz = ev.nonzero()
    if not nz.any():
        return math.inf
    return float(ev.beam_margin(d)[nz].min())
