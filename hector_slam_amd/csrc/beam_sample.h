// beam_sample.h -- the sampler: the device primitives that take a beam's end point to its map cell and the cell's four
// probabilities.  The workgroup -> XCD mapping, the lane index, the texel address, the affine transforms, the reference's sinf /
// cosf / normalize_angle, a level's fields in registers, and the two stages of the bilinear sample (fetch, finish).  Included by
// every kernel header that samples a level or maps coordinates; what a matcher form builds a Gauss-Newton step from on top of
// it is in gn_step.h.  No kernel is defined here.
#pragma once
#include <hip/hip_runtime.h>

#include "libm_exact.h"
#include "match_types.h"

namespace hsm {

// Workgroup b runs on XCD b % 8 (observed, MI355X_MICROARCH.md; used for speed only -- any placement is
// correct), and every XCD has its own 4 MiB L2.  A batch is usually spatially ordered (consecutive scans of a
// trajectory, hypotheses around one pose).  Two mappings, chosen per launch by the host (MatchParams::xcd_chunk):
//   contiguous (xcd_chunk == 0): each XCD takes one CONTIGUOUS eighth of the batch, so the map region its L2 has to hold
//     is eight times smaller than with the hardware's round robin -- the mapping for maps whose touched region
//     outgrows the L2s (4096^2 pyramid: 135 vs 138 us, exact form 308 vs 319 us);
//   chunked cyclic (xcd_chunk == c): XCD x takes chunks x, x + 8, x + 16, ... of c consecutive workgroups.  How long a
//     scan takes depends on where it was taken (per-wave time stamps: 37.6 .. 44.1 us between sixteenths of the bench
//     batch), so contiguous eighths leave whole XCDs with the slow stretches; chunks keep an XCD's working set
//     compact (16 workgroups = 64 consecutive scans) and give every XCD a sample of the whole batch (2048^2 headline:
//     49.2 vs 50.5 us).
// Bijective for any grid.
__device__ __forceinline__ int xcd_block(int b, int nblocks, int chunk) {
  int base = 0;
  if (chunk > 0) {
    const int main_blocks = nblocks / (8 * chunk) * (8 * chunk);
    if (b < main_blocks) {
      const int xcd = b & 7, j = b >> 3;
      return ((j / chunk) * 8 + xcd) * chunk + j % chunk;
    }
    base = main_blocks;  // the remainder of the grid: contiguous
  }
  const int rb = b - base, rn = nblocks - base;
  const int xcd = rb & 7, idx = rb >> 3, q = rn >> 3, r = rn & 7;
  return base + xcd * q + (xcd < r ? xcd : r) + idx;
}

// The lane index, recomputed where it is used (two v_mbcnt) instead of being carried in a VGPR from the top of a
// kernel that has none to spare: the volatile asm is neither hoisted nor merged with the threadIdx-derived value.
__device__ __forceinline__ int lane_id_now() {
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l;
}

// Texel address of cell (x, y) in the quad plane: row major, index = y*sizeX + x like the reference's grid -- one
// v_mad_u32_u24 per beam.  (Measured against 4x2-cell Morton tiles, which cut the cache-line requests of a gather along a
// wall by about a third but cost five more integer VALU ops per beam: the matcher is VALU-issue bound and both run at
// the same speed, profiles/r01/kernel_ab_tile.jsonl.)
__host__ __device__ __forceinline__ unsigned quad_index(unsigned x, unsigned y, int tiles_x, int sx) {
  (void)tiles_x;
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul24(y, (unsigned)sx) + x;
#else
  return y * (unsigned)sx + x;
#endif
}

// Transform<Affine> * Vector2f = t + (l(i,0)*x + l(i,1)*y)   (Eigen Transform.h)
__device__ __forceinline__ void affine_apply(const Affine2& a, float x, float y, float& ox, float& oy) {
  ox = a.t0 + (a.l00 * x + a.l01 * y);
  oy = a.t1 + (a.l10 * x + a.l11 * y);
}

// sinf/cosf of the reference (float overloads; OccGridMapUtil.h:70-71 compile to one
// sincosf call): glibc's algorithm operation for operation (libm_exact.h) -- identical bits for every
// argument, ~20 fp64 operations, no table on the |theta| < 120 path the matcher lives on.
// PIN: the texel-cache forms pin the binary64 constants to their use (libm_exact.h at_use: they have no register to hoist
// them into); the latency forms let the optimiser hoist them out of the 14-step chain
template <bool PIN = false>
__device__ __forceinline__ void sincos_f32(float th, float& s, float& c) {
  libm::sincosf_glibc<PIN>(th, s, c);
}

// util::normalize_angle (HSL/util/UtilFunctions.h:37-49): double fmod, float result
template <bool PIN = false>
__device__ __forceinline__ float normalize_angle(float angle) {
  const double two_pi = libm::at_use<PIN>(2.0 * 3.14159265358979323846);  // PIN: materialised here, not hoisted over the GN loops
  float a = (float)fmod(fmod((double)angle, two_pi) + two_pi, two_pi);
  if ((double)a > libm::at_use<PIN>(3.14159265358979323846)) {
    a = (float)((double)a - two_pi);
  }
  return a;
}

// The LevelView fields the beam loop reads, pulled into registers ONCE per level (the kernel
// argument block lives in memory; re-reading it per beam costs a scalar load + wait each time).
struct LevelRegs {
  const float4* quad;
  const float* prob;
  int sx;
  int tiles_x;
  float limx, limy;
  int zero_index;  // index of the all-zero texel / pad cells behind the plane (see sample_fetch)
};

template <int LAYOUT>
__device__ __forceinline__ LevelRegs level_regs(const LevelView& L) {
  LevelRegs R;
  R.quad = L.quad;
  R.prob = L.prob;
  R.sx = L.sx;
  R.tiles_x = L.tiles_x;
  R.limx = L.limx;
  R.limy = L.limy;
  R.zero_index = LAYOUT == kLayoutQuad ? L.quad_texels : L.sx * L.sy;
  return R;
}

// a1, split in two so that a lane can ISSUE the texel gathers of several beams back to back
// (stage 1) before it CONSUMES any of them (stage 2): memory latency is hidden by
// instruction-level parallelism inside the wavefront, not only by occupancy.
// Two fp32 values kept together (storage only).  Measured on MI355X (tools/microbench/valu_rate.hip,
// profiles/r01/valu_rate.txt): v_mul/v_add/v_fma_f32 issue every ~2.5 cycles per wave64, while
// v_pk_mul/v_pk_add_f32 -- and v_med3, v_fract, v_cvt, v_mad_u32_u24 -- take ~4: a packed op is
// worth 1.6 scalar ones, which the v_mov shuffles needed to form pairs eat up again.  So the
// arithmetic below is plain scalar fp32 and the library is built with -fno-slp-vectorize.
typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4v __attribute__((ext_vector_type(4)));  // a native 128-bit register tuple (inline-asm operand)

struct BeamSample {
  f2 lo, hi;  // (P(ix,iy), P(ix+1,iy)), (P(ix,iy+1), P(ix+1,iy+1))
  f2 X, Y;    // (xFacInv, fx), (yFacInv, fy)  -- OccGridMapUtil.h:298,338-339
};

// stage 1: bounds test, cell index, fractions, and the (asynchronous) gather.
//
// Out-of-map beams (MapDimensionProperties::pointOutOfMapBounds, MapDimensionProperties.h:65-68)
// must contribute EXACT zeros, like the (0,0,0) the reference returns at OccGridMapUtil.h:290-292.
// They are pointed at an all-zero texel stored behind the plane: P00=P10=P01=P11=0 gives
// dM/dx = dM/dy = -0 and M = 0, so every product added to H and dTr is +-0 and the running fp32
// sums are unchanged bit for bit -- the same outcome as the reference's explicit zeros, without a
// branch or three selects per beam.  The matcher is VALU-issue bound (profiles/r01), so the test
// itself is written for instruction count.  A beam is outside when x < 0 or x > dims-2, as in the
// reference; a NaN coordinate counts as outside too (the reference would index the map with (int)NaN
// there and crash).  v_fract_f32(x) == x - (float)(int)x exactly for 0 <= x < 2^23.
// Bounds test of one map coordinate pair: 0 <= x <= lim on the BIT PATTERNS -- for
// x >= +0 the unsigned pattern of an fp32 value is monotonic in the value, every negative value (sign bit set) and
// every NaN compares above any non-negative limit, so `bits(x) <= bits(lim)` is the whole test in ONE v_cmp_le_u32
// per axis (a clamp with v_med3 costs that + v_cmp_neq per axis).  The one value the pattern test would judge
// differently is -0.0 (inside for the reference: -0.0 < 0 is false); c = e + r is -0.0 only if e AND r are -0.0,
// and the callers pass e + 0.0f (wave-uniform, once per GN step; changes no other sum), so it cannot occur.
// Outside beams keep their raw coordinate: v_cvt_i32_f32 saturates and v_fract_f32 of a finite value is finite,
// which is all the all-zero texel needs to yield +-0 products.  (A coordinate is inf or NaN only when the estimate is: the
// whole evaluation is then put right once, in gn_solve_and_step.)
// the estimate's map coordinates as the beam loop adds them to the rotated endpoints: -0.0 -> +0.0 (see above; for
// every other value x + 0.0f == x, and (+0.0) + r == (-0.0) + r unless r is -0.0 too)
__device__ __forceinline__ f2 step_origin(float ex, float ey) {
  return f2{ex + 0.0f, ey + 0.0f};
}

struct CellCoord {
  unsigned ix, iy;
  float fx, fy;
  bool oob;
};

__device__ __forceinline__ CellCoord cell_coord(const LevelRegs& L, f2 c) {
  CellCoord q;
  q.oob = (int)(__float_as_uint(c.x) > __float_as_uint(L.limx)) | (int)(__float_as_uint(c.y) > __float_as_uint(L.limy));
  const float sx_ = c.x, sy_ = c.y;
  // truncation, OccGridMapUtil.h:295.  The instruction itself (saturating, defined for every input) rather than a
  // C++ cast, whose result is undefined for the raw coordinate of an outside beam.
  asm("v_cvt_i32_f32 %0, %1" : "=v"(q.ix) : "v"(sx_));
  asm("v_cvt_i32_f32 %0, %1" : "=v"(q.iy) : "v"(sy_));
  q.fx = __builtin_amdgcn_fractf(sx_);  // :298
  q.fy = __builtin_amdgcn_fractf(sy_);
  return q;
}

template <int LAYOUT>
__device__ __forceinline__ BeamSample sample_fetch(const LevelRegs& L, f2 c) {
  BeamSample b;
  const CellCoord q = cell_coord(L, c);
  const bool oob = q.oob;
  const unsigned ix = q.ix, iy = q.iy;
  b.X.y = q.fx;
  b.Y.y = q.fy;
  b.X.x = 1.0f - b.X.y;  // :338-339
  b.Y.x = 1.0f - b.Y.y;
  if (LAYOUT == kLayoutQuad) {
    const unsigned index = oob ? (unsigned)L.zero_index : quad_index(ix, iy, L.tiles_x, L.sx);
    // 32-bit byte offset on a uniform base: one global_load_dwordx4 with an SGPR base address
    const float4 q = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(L.quad) + (size_t)(index << 4));
    b.lo = f2{q.x, q.y};
    b.hi = f2{q.z, q.w};
  } else {
    // indices index, index+1, index+sizeX, index+sizeX+1 (:302-330); the plane is followed by
    // sizeX+2 zero cells so that the zero_index footprint is all zeros too
    const unsigned index = oob ? (unsigned)L.zero_index : __umul24(iy, (unsigned)L.sx) + ix;
    const float* p = reinterpret_cast<const float*>(reinterpret_cast<const char*>(L.prob) + (size_t)(index << 2));
    b.lo = f2{p[0], p[1]};
    b.hi = f2{p[L.sx], p[L.sx + 1]};
  }
  return b;
}

// stage 2: the interpolation and the source-literal "derivatives" (:332-346):
//   M  = ((P00*xFacInv + P10*fx) * yFacInv) + ((P01*xFacInv + P11*fx) * fy)
//   gx = -((P00-P10)*xFacInv + (P01-P11)*fx)      gy = -((P00-P01)*yFacInv + (P10-P11)*fy)
// (x-differences blended with the x fractions, as the source does -- SURVEY.md row a1).
// Returned as M and G = (-gx, -gy): the two negations of the source are exact sign flips, and
// every consumer (gn_step.h) absorbs them into an operand-negate modifier or a product of two of them.
struct BeamTerms {
  float M;
  f2 G;  // (-dM/dx, -dM/dy) as the source defines them
};

__device__ __forceinline__ BeamTerms sample_finish(const BeamSample& b) {
  const float xFacInv = b.X.x, fx = b.X.y, yFacInv = b.Y.x, fy = b.Y.y;
  const float i0 = b.lo.x, i1 = b.lo.y, i2 = b.hi.x, i3 = b.hi.y;
  const float dx1 = i0 - i1;  // :332-336
  const float dx2 = i2 - i3;
  const float dy1 = i0 - i2;
  const float dy2 = i1 - i3;
  BeamTerms r;
  r.M = ((i0 * xFacInv + i1 * fx) * (yFacInv)) + ((i2 * xFacInv + i3 * fx) * (fy));  // :341-344
  r.G.x = ((dx1 * xFacInv) + (dx2 * fx));  // -gx  :345
  r.G.y = ((dy1 * yFacInv) + (dy2 * fy));  // -gy  :346
  return r;
}

// The rotated endpoint R(theta) * p, shared by the transform and by rotDeriv:
//   transform * currPoint   = t + [c -s; s c] p = (ex + (c*px + (-s)*py), ey + (s*px + c*py))   (:80)
//   rotDeriv (:87)          = (-s*px - c*py) * gx + (c*px - s*py) * gy
// In IEEE arithmetic (-s)*py == -(s*py) and a + (-b) == a - b exactly, and round-to-nearest is
// symmetric, so  c*px + (-s)*py == c*px - s*py == rx  and  -s*px - c*py == -(s*px + c*py) == -ry
// BIT FOR BIT, but for the sign of an exact zero (s*px = +0, c*py = -0: -(+0) against -0 - (-0) = +0), which only an end point
// with a -0.0 component produces and which no sum shows: every chain and partial sum starts at +0, and x + (+-0) == x.
// The two products/one sum per component are computed once and reused.
struct BeamRot {
  f2 r;  // (rx, ry)
};

// cs = (cos, sin), sc = (sin, cos) of the current estimate; e = (ex, ey); p = endpoint
template <int LAYOUT>
__device__ __forceinline__ BeamSample beam_fetch(const LevelRegs& L, f2 e, f2 cs, f2 sc, f2 p, BeamRot& r) {
  r.r.x = cs.x * p.x - sc.x * p.y;  // c*px - s*py
  r.r.y = cs.y * p.x + sc.y * p.y;  // s*px + c*py
  return sample_fetch<LAYOUT>(L, f2{e.x + r.r.x, e.y + r.r.y});
}

}  // namespace hsm
