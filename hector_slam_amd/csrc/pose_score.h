// pose_score.h -- the likelihood of one scan at one pose, stated once for every scoring kernel (probe_kernels.h, score_kernels.h,
// window_kernels.h): OccGridMapUtil::getLikelihoodForState / getResidualForState (OccGridMapUtil.h:184-221), residual =
// sum_i (1 - M_i) with M from interpMapValue (:233-285) -- the matcher's bilinear sample without the gradient, taken by
// beam_fetch (beam_sample.h): same texel gather, and an out-of-map beam reads the all-zero texel, M = 0, funval = 1, exactly the
// reference's `return 0.0f`.  A pose is held as a frame; a residual is one of three walks over (frame, scan), two of which sum in
// the reference's beam order and give its bits.  The kernels decide who a wavefront or a lane is, make the frame, call one walk
// and store; that every one of them returns the same bits for the same (pose, scan) is what this header states.
// No kernel is defined here.
#pragma once
#include <hip/hip_runtime.h>

#include "beam_sample.h"
#include "gn_step.h"

namespace hsm {

// funval = 1 - M of one sample, M with interpMapValue's parenthesisation (the scorers' ONE spelling of it; the matcher forms M
// together with the gradient, beam_sample.h sample_finish)
__device__ __forceinline__ float beam_funval(const BeamSample& s) {
  const float M = ((s.lo.x * s.X.x + s.lo.y * s.X.y) * (s.Y.x)) + ((s.hi.x * s.X.x + s.hi.y * s.X.y) * (s.Y.y));
  return 1.0f - M;
}

// likelihood = 1 - residual / size (getLikelihoodForState, :184-203), the one spelling of it.  A scan of 0 beams: 0 / 0, an
// invalid operation, whose NaN is the processor's choice -- and the reference's processor is x86-64, whose default NaN has the
// sign bit set (0xffc00000; 1 - NaN keeps it), where the device returns 0x7fc00000 for 1 - 0 / 0.  No other operand of this
// division is invalid (n is finite, and a NaN residual passes through), so the empty scan alone is given the reference's bits
__device__ __forceinline__ float scan_likelihood(float residual, int n) {
  return n == 0 ? __uint_as_float(0xffc00000u) : 1 - (residual / (float)n);
}

// scan b of a CSR batch (offsets in points) or, offsets == nullptr, the one scan of shared_n beams that every b shares.  b is
// wave-uniform, so the two offsets are scalar loads
__device__ __forceinline__ const float2* batch_scan(const float2* __restrict__ pts_all, const int* __restrict__ offsets,
                                                    int shared_n, int b, int& n) {
  int beg = 0;
  n = shared_n;
  if (offsets) {
    beg = offsets[b];
    n = offsets[b + 1] - beg;
  }
  return pts_all + beg;
}

// ---- a pose, as the beam loop wants it ------------------------------------------------------------------------------------------
// the level's fields in registers, the pose's origin (step_origin), (cos, sin) and (sin, cos), and the factor that takes an end
// point from level-0 units to the level's (DataContainer::setFrom)
struct PoseFrame {
  LevelRegs R;
  f2 e2, cs, sc;
  float pt_scale;
};

// from a state in the level's MAP frame; the caller names the end points' scale
template <int LAYOUT>
__device__ __forceinline__ PoseFrame pose_frame_map(const LevelView& L, float ex, float ey, float eth, float pt_scale) {
  float sinRot, cosRot;
  sincos_f32(eth, sinRot, cosRot);
  PoseFrame F;
  F.R = level_regs<LAYOUT>(L);
  F.e2 = step_origin(ex, ey), F.cs = f2{cosRot, sinRot}, F.sc = f2{sinRot, cosRot};
  F.pt_scale = pt_scale;
  return F;
}

// from a WORLD pose: getMapCoordsPose (GridMapBase.h:235-239, the matchers' own first step), end points scaled by the level's
// 2^-level
template <int LAYOUT>
__device__ __forceinline__ PoseFrame pose_frame_world(const LevelView& L, float x, float y, float th) {
  float ex, ey;
  affine_apply(L.mapTworld, x, y, ex, ey);
  return pose_frame_map<LAYOUT>(L, ex, ey, th, L.pt_scale);
}

template <int LAYOUT>
__device__ __forceinline__ BeamSample frame_fetch(const PoseFrame& F, float2 p) {
  BeamRot r;
  return beam_fetch<LAYOUT>(F.R, F.e2, F.cs, F.sc, f2{p.x * F.pt_scale, p.y * F.pt_scale}, r);
}

// ---- the residual of scan (pts, n) at frame F: three walks -----------------------------------------------------------------------
// A WAVEFRONT, the reference's order: 64 beams a round, one per lane, through the wavefront's LDS row (gn_step.h
// exact_residual_round); the sum is meaningful in lane 0 only.  The one loop that pads: the lanes beyond the scan's end
// contribute funval = +0, and M is only ever 0 .. 1, so no sum is -0 and +0 changes nothing.  n == 0: +0.
template <int LAYOUT>
__device__ __forceinline__ float residual_reference_order(const PoseFrame& F, const float2* __restrict__ pts, int n,
                                                          float* __restrict__ row, int lane) {
  float residual = 0.0f;
  for (int base = 0; base < n; base += 64) {  // wave-uniform trip count
    const int i = base + lane;
    float funval = 0.0f;
    if (i < n) funval = beam_funval(frame_fetch<LAYOUT>(F, pts[i]));
    residual = exact_residual_round(funval, row, lane, residual);
  }
  return residual;
}

// A WAVEFRONT, the tree order (HSM_PARITY_FAST): lane-strided partial sums and a wave_allreduce; every lane returns the sum
template <int LAYOUT>
__device__ __forceinline__ float residual_tree_order(const PoseFrame& F, const float2* __restrict__ pts, int n, int lane) {
  float residual = 0.0f;
  for (int i = lane; i < n; i += 64) residual += beam_funval(frame_fetch<LAYOUT>(F, pts[i]));
  return wave_allreduce(residual);
}

// A LANE, the reference's order: the lane walks beams 0 .. n-1 itself, so its running sum IS getResidualForState's chain -- no LDS
// hand-over, no idle lanes.  With a wave-uniform scan the beam index is wave-uniform too and an end point is one scalar load that
// the wavefront's 64 poses share (no LDS copy of the scan: the scalar cache serves it, and the workgroup needs no barrier).
// kWindowUnroll texel gathers are issued before the first is used.
constexpr int kWindowUnroll = 4;

template <int LAYOUT>
__device__ __forceinline__ float residual_lane_chain(const PoseFrame& F, const float2* __restrict__ pts, int n) {
  float residual = 0.0f;
  int i = 0;
  for (; i + kWindowUnroll <= n; i += kWindowUnroll) {
    BeamSample s[kWindowUnroll];
#pragma unroll
    for (int u = 0; u < kWindowUnroll; ++u) s[u] = frame_fetch<LAYOUT>(F, pts[i + u]);
#pragma unroll
    for (int u = 0; u < kWindowUnroll; ++u) residual += beam_funval(s[u]);
  }
  for (; i < n; ++i) residual += beam_funval(frame_fetch<LAYOUT>(F, pts[i]));
  return residual;
}

}  // namespace hsm
