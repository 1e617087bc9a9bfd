// probe_kernels.h -- the kernels that only the probes and test hooks launch (probes.hip): the test hooks of the map planes and of
// libm_exact.h, one evaluation of the matcher's sums at a given pose, and the likelihood and covariance of map-frame poses (the
// likelihood itself: pose_score.h).  Some are not templates, so exactly one translation unit may include this header.
#pragma once
#include <hip/hip_runtime.h>

#include "beam_sample.h"
#include "gn_step.h"
#include "libm_exact.h"
#include "map_cells.h"
#include "match_types.h"
#include "pose_score.h"

namespace hsm {

// test hook (hsm_debug_marks_nonzero): the dense update's byte map and the keyed update's end-cell bitmap must be ALL ZERO
// between updates (each apply pass clears what its mark passes set; map_update.h "dense scans"): count the non-zero words
__global__ void __launch_bounds__(256) count_nonzero_words_kernel(const unsigned int* __restrict__ words, size_t n,
                                                                  unsigned long long* __restrict__ out) {
  unsigned int local = 0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    local += words[i] != 0u ? 1u : 0u;
  const unsigned long long m = __ballot(local != 0u);
  if (m == 0ull) return;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) local += (unsigned int)__shfl_down((int)local, d);
  if ((threadIdx.x & 63) == 0) atomicAdd(out, (unsigned long long)local);
}

// rectangle (x0,y0,w,h) of the two SoA planes -> the reference's AoS LogOddsCell {float, int}
__global__ void pack_cells_kernel(LevelRW L, int x0, int y0, int w, int h, int2* __restrict__ out) {
  const size_t n = (size_t)w * h;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int x = x0 + (int)(i % (size_t)w), y = y0 + (int)(i / (size_t)w);
    const size_t c = (size_t)y * L.sx + x;
    out[i] = make_int2(__float_as_int(L.logodds[c]), L.update_index[c]);
  }
}

// device expf / getGridProbability sweep for the parity tests
__global__ void expf_debug_kernel(const float* __restrict__ x, int n, float* __restrict__ e, float* __restrict__ p) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  e[i] = libm::expf_glibc(x[i]);
  p[i] = grid_probability(x[i]);
}

// device sin/cos sweep for the parity tests
__global__ void sincos_debug_kernel(const float* __restrict__ x, int n, float* __restrict__ s,
                                    float* __restrict__ c) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  sincos_f32(x[i], s[i], c[i]);
}

// ---- parity / debug kernels: one evaluation at a given map-frame pose ------------
// H, dTr of one getCompleteHessianDerivs call (same device functions as the matcher)
template <int LAYOUT, bool EXACT = false>
__global__ void __launch_bounds__(1024) gn_eval_kernel(const LevelView L, const float2* __restrict__ pts,
                                                      int n, float ex, float ey, float eth,
                                                      float* out12 /* H[9] col-major, dTr[3] */) {
  __shared__ __attribute__((aligned(16))) float red[2][9][16];
  __shared__ float stage[EXACT ? 9 * (1024 + kExactPad) : 1];
  const int lane = threadIdx.x & 63;
  const int wit = threadIdx.x >> 6;
  float sinRot, cosRot;
  sincos_f32(eth, sinRot, cosRot);
  Acc9 acc;
  acc.zero();
  const LevelRegs R = level_regs<LAYOUT>(L);
  if (EXACT) {
    const f2 e2 = step_origin(ex, ey), cs = f2{cosRot, sinRot}, sc = f2{sinRot, cosRot};
    float run = 0.0f;
    for (int base = 0; base < n; base += 1024) {
      const int i = base + (int)threadIdx.x;
      const float2 p = i < n ? pts[i] : make_float2(1.0e30f, 1.0e30f);
      BeamRot r;
      const BeamSample b = beam_fetch<LAYOUT>(R, e2, cs, sc, f2{p.x, p.y}, r);
      float pr[9];
      beam_products(b, r, pr);
      run = exact_round<1024>(pr, stage, (int)threadIdx.x, run, min(1024, n - base));
    }
    float* const redf = &red[0][0][0];
    if (threadIdx.x < 9) redf[threadIdx.x] = run;
    __syncthreads();
    acc.d01 = f2{redf[0], redf[1]}; acc.d2 = redf[2];
    acc.hd = f2{redf[3], redf[4]}; acc.h22 = redf[5];
    acc.h01 = redf[6]; acc.hr = f2{redf[7], redf[8]};
  } else {
    for (int i = threadIdx.x; i < n; i += 1024) {
      const float2 p = pts[i];
      beam_accumulate<LAYOUT>(R, ex, ey, sinRot, cosRot, p.x, p.y, acc);
    }
    team_allreduce9<16>(acc, red, 0, wit, lane);
  }
  if (threadIdx.x == 0) {
    out12[0] = acc.hd.x; out12[1] = acc.h01; out12[2] = acc.hr.x;
    out12[3] = acc.h01; out12[4] = acc.hd.y; out12[5] = acc.hr.y;
    out12[6] = acc.hr.x; out12[7] = acc.hr.y; out12[8] = acc.h22;
    out12[9] = acc.d01.x; out12[10] = acc.d01.y; out12[11] = acc.d2;
  }
}

// per-beam M, dM/dx, dM/dy, rotDeriv
template <int LAYOUT>
__global__ void gn_beam_terms_kernel(const LevelView L, const float2* __restrict__ pts, int n, float ex,
                                     float ey, float eth, float4* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float sinRot, cosRot;
  sincos_f32(eth, sinRot, cosRot);
  Acc9 acc;
  acc.zero();
  BeamTerms t;
  const float2 p = pts[i];
  const LevelRegs R = level_regs<LAYOUT>(L);
  float rd = beam_accumulate<LAYOUT>(R, ex, ey, sinRot, cosRot, p.x, p.y, acc, &t);
  // out-of-map beams: the matcher's zero-texel trick yields dM = -0 where the reference returns
  // literal +0 (same sums, different sign bit); report the reference's literal values here
  const float cx = ex + (cosRot * p.x - sinRot * p.y), cy = ey + (sinRot * p.x + cosRot * p.y);
  float gx = -t.G.x, gy = -t.G.y;
  if ((cx < 0.0f) | (cx > R.limx) | (cy < 0.0f) | (cy > R.limy)) {
    t.M = gx = gy = 0.0f;
    rd = ((-sinRot * p.x - cosRot * p.y) * gx + (cosRot * p.x - sinRot * p.y) * gy);
  }
  // a rotDeriv of exactly zero: the shared rotation (BeamRot) may give it the other SIGN than the source's expression (an end
  // point with a -0.0 component: -(0 + -0) is -0, -0 - (-0) is +0).  No sum can show it, this hook can: report the source's
  if (rd == 0.0f) rd = ((-sinRot * p.x - cosRot * p.y) * gx + (cosRot * p.x - sinRot * p.y) * gy);
  out[i] = make_float4(t.M, gx, gy, rd);
}

// ---- f3: pose likelihood for a batch of map-frame states against ONE scan --------
// OccGridMapUtil::getLikelihoodForState (OccGridMapUtil.h:184-214): residual = sum_i (1 - M_i), likelihood = 1 - residual / size.
// One wavefront per state; sampler, padding and the two summation orders (EXACT: the reference's) are pose_score.h's.

template <int LAYOUT, bool EXACT = false>
__global__ void __launch_bounds__(256) likelihood_kernel(const LevelView L, const float* __restrict__ states,
                                                         int batch, const float2* __restrict__ pts, int n,
                                                         float pt_scale, float* __restrict__ out_lh,
                                                         float* __restrict__ out_residual) {
  __shared__ float rows[EXACT ? 4 : 1][EXACT ? 64 : 1];
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (b >= batch) return;
  const PoseFrame F = pose_frame_map<LAYOUT>(L, states[3 * b], states[3 * b + 1], states[3 * b + 2], pt_scale);
  float residual;
  if (EXACT) residual = residual_reference_order<LAYOUT>(F, pts, n, rows[(threadIdx.x >> 6) & 3], lane);
  else residual = residual_tree_order<LAYOUT>(F, pts, n, lane);
  if (lane == 0) {
    if (out_lh) out_lh[b] = scan_likelihood(residual, n);
    if (out_residual) out_residual[b] = residual;  // getResidualForState (:205-221)
  }
}

// OccGridMapUtil::getCovarianceForPose (HSL/map/OccGridMapUtil.h:106-160) + getCovMatrixWorldCoords
// (:162-188): 7 sigma points around a MAP-frame pose (+-1.5 cells, +-0.05 rad, the pose itself), their
// likelihoods weight a sample mean and a 3x3 sample covariance.  One workgroup per pose, wave w scores
// sigma point w (same sampler as above), thread 0 does the 7-term statistics in the source's order.
template <int LAYOUT, bool EXACT = false>
__global__ void __launch_bounds__(448) pose_covariance_kernel(const LevelView L, const float* __restrict__ poses,
                                                              int batch, const float2* __restrict__ pts, int n,
                                                              float pt_scale, float cell_length,
                                                              float* __restrict__ out_cov_map,
                                                              float* __restrict__ out_cov_world,
                                                              float* __restrict__ out_lh7) {
  __shared__ float lh[7];
  __shared__ float rows[EXACT ? 7 : 1][EXACT ? 64 : 1];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.x;
  const float x = poses[3 * b], y = poses[3 * b + 1], ang = poses[3 * b + 2];
  float sp[7][3];
  sigma_points(x, y, ang, sp);
  {
    float ex = sp[0][0], ey = sp[0][1], ea = sp[0][2];
#pragma unroll
    for (int k = 1; k < 7; ++k)
      if (w == k) ex = sp[k][0], ey = sp[k][1], ea = sp[k][2];
    const PoseFrame F = pose_frame_map<LAYOUT>(L, ex, ey, ea, pt_scale);
    float residual;
    if (EXACT) residual = residual_reference_order<LAYOUT>(F, pts, n, rows[w], lane);
    else residual = residual_tree_order<LAYOUT>(F, pts, n, lane);
    if (lane == 0) lh[w] = scan_likelihood(residual, n);
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  // the 7-term statistics in the source's order (gn_step.h)
  sigma_point_statistics(sp, lh, cell_length, out_lh7 ? out_lh7 + 7 * b : nullptr, out_cov_map ? out_cov_map + 9 * b : nullptr,
                         out_cov_world ? out_cov_world + 9 * b : nullptr);
}

}  // namespace hsm
