// window_kernels.h -- the kernels of window.hip: the likelihood of ONE scan at every pose of a window that never exists in memory
// (two forms with the same bits), window indices turned into poses, and the K best of an array of scores.
#pragma once
#include <hip/hip_runtime.h>

#include "beam_sample.h"
#include "gn_step.h"
#include "match_types.h"
#include "window_grid.h"

namespace hsm {

struct WindowParams {
  WindowGrid grid;
  const float* center;  // [3] world pose, DEVICE memory
  int count;            // W
  const float2* pts;    // one scan, level-0 units
  int n;
  float* out_lh;        // [W] or null
  float* out_residual;  // [W] or null
};

__device__ __forceinline__ float window_beam_funval(const BeamSample& s) {
  const float M = ((s.lo.x * s.X.x + s.lo.y * s.X.y) * (s.Y.x)) + ((s.hi.x * s.X.x + s.hi.y * s.X.y) * (s.Y.y));
  return 1.0f - M;
}

// ---- one LANE per hypothesis ------------------------------------------------------------------------------------------------
// Every lane walks beams 0 .. n-1 itself, so its running sum IS getResidualForState's chain: no LDS hand-over, no idle lanes.
// The beam index is wave-uniform, so an end point is one scalar load that all 64 hypotheses share (no LDS copy of the scan: the
// scalar cache serves it, and the workgroup needs no barrier).  kWindowUnroll texel gathers are issued before the first is used.
// Lanes that are neighbours in x sample neighbouring texels.  The lanes behind the last hypothesis redo the last one (no
// divergent exit; they write nothing).  Sampler, bounds and zero-texel treatment are beam_fetch's.
constexpr int kWindowUnroll = 4;

template <int LAYOUT>
__global__ void __launch_bounds__(256) score_window_lane_kernel(const LevelView L, const WindowParams P) {
  const long long wl = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool live = wl < P.count;
  const int w = live ? (int)wl : P.count - 1;
  float x, y, th;
  window_pose(P.grid, P.center[0], P.center[1], P.center[2], w, x, y, th);
  float ex, ey;
  affine_apply(L.mapTworld, x, y, ex, ey);  // getMapCoordsPose
  float sinRot, cosRot;
  sincos_f32(th, sinRot, cosRot);
  const float pt_scale = L.pt_scale;
  const LevelRegs R = level_regs<LAYOUT>(L);
  const f2 e2 = step_origin(ex, ey), cs = f2{cosRot, sinRot}, sc = f2{sinRot, cosRot};
  const float2* __restrict__ pts = P.pts;
  const int n = P.n;
  float residual = 0.0f;
  int i = 0;
  for (; i + kWindowUnroll <= n; i += kWindowUnroll) {
    BeamSample s[kWindowUnroll];
#pragma unroll
    for (int u = 0; u < kWindowUnroll; ++u) {
      const float2 p = pts[i + u];
      BeamRot r;
      s[u] = beam_fetch<LAYOUT>(R, e2, cs, sc, f2{p.x * pt_scale, p.y * pt_scale}, r);
    }
#pragma unroll
    for (int u = 0; u < kWindowUnroll; ++u) residual += window_beam_funval(s[u]);
  }
  for (; i < n; ++i) {
    const float2 p = pts[i];
    BeamRot r;
    const BeamSample s = beam_fetch<LAYOUT>(R, e2, cs, sc, f2{p.x * pt_scale, p.y * pt_scale}, r);
    residual += window_beam_funval(s);
  }
  if (!live) return;
  if (P.out_lh) P.out_lh[w] = 1 - (residual / (float)n);  // getLikelihoodForState (:184-203); n == 0: NaN
  if (P.out_residual) P.out_residual[w] = residual;       // getResidualForState (:205-221)
}

// ---- one WAVEFRONT per hypothesis: score_batch_kernel<LAYOUT, true> with the pose generated from w ----------------------------
template <int LAYOUT>
__global__ void __launch_bounds__(256) score_window_wave_kernel(const LevelView L, const WindowParams P) {
  __shared__ float rows[4][64];
  const int lane = threadIdx.x & 63;
  const long long wl = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wl >= P.count) return;  // (a whole wavefront)
  const int w = __builtin_amdgcn_readfirstlane((int)wl);
  float x, y, th;
  window_pose(P.grid, P.center[0], P.center[1], P.center[2], w, x, y, th);
  float ex, ey;
  affine_apply(L.mapTworld, x, y, ex, ey);
  float sinRot, cosRot;
  sincos_f32(th, sinRot, cosRot);
  const float pt_scale = L.pt_scale;
  const LevelRegs R = level_regs<LAYOUT>(L);
  const f2 e2 = step_origin(ex, ey), cs = f2{cosRot, sinRot}, sc = f2{sinRot, cosRot};
  const float2* __restrict__ pts = P.pts;
  const int n = P.n;
  float residual = 0.0f;
  float* row = rows[(threadIdx.x >> 6) & 3];
  for (int base = 0; base < n; base += 64) {  // wave-uniform trip count
    const int i = base + lane;
    float funval = 0.0f;  // padding beyond the scan: +0 changes no sum (see likelihood_kernel)
    if (i < n) {
      const float2 p = pts[i];
      BeamRot r;
      funval = window_beam_funval(beam_fetch<LAYOUT>(R, e2, cs, sc, f2{p.x * pt_scale, p.y * pt_scale}, r));
    }
    residual = exact_residual_round(funval, row, lane, residual);
  }
  if (lane == 0) {
    if (P.out_lh) P.out_lh[w] = 1 - (residual / (float)n);
    if (P.out_residual) P.out_residual[w] = residual;
  }
}

// ---- window indices -> poses ------------------------------------------------------------------------------------------------
// index == nullptr: indices 0 .. count-1.  An index outside [0, W): three quiet NaNs.
__global__ void __launch_bounds__(256) window_poses_kernel(const WindowGrid g, int W, const float* __restrict__ center,
                                                           const int* __restrict__ index, int count,
                                                           float* __restrict__ out_pose) {
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  if (c >= count) return;
  const int w = index ? index[c] : (int)c;
  const float qnan = __uint_as_float(0x7fc00000u);
  float x = qnan, y = qnan, t = qnan;
  if (w >= 0 && w < W) window_pose(g, center[0], center[1], center[2], w, x, y, t);
  out_pose[3 * c + 0] = x;
  out_pose[3 * c + 1] = y;
  out_pose[3 * c + 2] = t;
}

// ---- the K best of an array of scores, in rank order ---------------------------------------------------------------------------
// The strict total order of best_beats on (score, index): K rounds, each finds the best entry that the winner of the round
// before beats ("retired" entries are the ones that do not lose to it), so no entry is ever marked.  Stage 1 (CANDIDATES =
// false): every wavefront takes the strided slice {slice * 64 + lane + m * slices * 64} of the scores and leaves its K best as
// (score, index) pairs.  Stage 2 (CANDIDATES = true): ONE workgroup runs the same rounds over all the pairs.  The K best of the
// whole array are among the K best of the slices, and the order is total, so the result does not depend on the slicing.
template <bool CANDIDATES>
__device__ __forceinline__ void topk_scan(const float* __restrict__ score, const int* __restrict__ index, long long first,
                                          long long stride, long long count, bool have, float bs, int bi, float& s, int& i) {
  s = 0.0f;
  i = -1;
  for (long long e = first; e < count; e += stride) {
    const float v = score[e];
    const int id = CANDIDATES ? index[e] : (int)e;
    if (id < 0 || v != v) continue;
    if (have && !best_beats(bs, bi, v, id)) continue;  // retired in an earlier round
    if (best_beats(v, id, s, i)) s = v, i = id;
  }
}

__global__ void __launch_bounds__(256) topk_slice_kernel(const float* __restrict__ scores, int count, int k, int slices,
                                                         float* __restrict__ cand_score, int* __restrict__ cand_index) {
  const int lane = threadIdx.x & 63;
  const int slice = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
  if (slice >= slices) return;  // (a whole wavefront)
  bool have = false, none = false;
  float bs = 0.0f;
  int bi = -1;
  for (int r = 0; r < k; ++r) {
    float s = 0.0f;
    int i = -1;
    if (!none) {
      topk_scan<false>(scores, nullptr, (long long)slice * 64 + lane, (long long)slices * 64, count, have, bs, bi, s, i);
      wave_best(s, i);
    }
    none = i < 0;
    have = true, bs = s, bi = i;
    if (lane == 0) {
      cand_score[slice * k + r] = i >= 0 ? s : __uint_as_float(0x7fc00000u);
      cand_index[slice * k + r] = i;
    }
  }
}

__global__ void __launch_bounds__(256) topk_merge_kernel(const float* __restrict__ cand_score, const int* __restrict__ cand_index,
                                                         int cands, int k, int* __restrict__ out_index,
                                                         float* __restrict__ out_score) {
  __shared__ float ws[2][4];
  __shared__ int wi[2][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  bool have = false, none = false;
  float bs = 0.0f;
  int bi = -1;
  for (int r = 0; r < k; ++r) {  // (k and `none` are uniform over the workgroup: every thread reaches every barrier)
    float s = 0.0f;
    int i = -1;
    if (!none) {
      topk_scan<true>(cand_score, cand_index, threadIdx.x, 256, cands, have, bs, bi, s, i);
      wave_best(s, i);
      if (lane == 0) ws[r & 1][wave] = s, wi[r & 1][wave] = i;  // (two rows: round r+1 writes while a slow wave still reads r)
      __syncthreads();
      s = ws[r & 1][lane & 3];
      i = wi[r & 1][lane & 3];
#pragma unroll
      for (int off = 2; off > 0; off >>= 1) {
        const float so = __shfl_xor(s, off, 64);
        const int io = __shfl_xor(i, off, 64);
        if (best_beats(so, io, s, i)) s = so, i = io;
      }
    }
    none = i < 0;
    have = true, bs = s, bi = i;
    if (threadIdx.x == 0) {
      out_index[r] = i;
      if (out_score) out_score[r] = i >= 0 ? s : __uint_as_float(0x7fc00000u);
    }
  }
}

// the winner among the K candidates -> the window index its start came from (in place)
__global__ void window_best_index_kernel(const int* __restrict__ cand_window_index, int k, int* __restrict__ io_index) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int c = io_index[0];
  io_index[0] = c >= 0 && c < k ? cand_window_index[c] : -1;
}

}  // namespace hsm
