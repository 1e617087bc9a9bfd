// window_kernels.h -- the kernels of window.hip: the likelihood of ONE scan at every pose of a window that never exists in memory
// (two forms with the same bits), window indices turned into poses, and the K best of an array of scores; each with a batch
// dimension too -- B scans in B windows of one shape, the K best of every group -- and the copy that lays a CSR batch of scans out
// K times for the matcher.
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

// ---- B windows of one shape, window b around centre b against scan b, in ONE launch -------------------------------------------
// The two forms above with a batch dimension, and the same bits as B launches of them: a hypothesis' chain is its own whatever
// else the launch holds.  The scans are a CSR batch or (offsets == nullptr) one scan of shared_n beams for every window.
struct WindowBatchParams {
  WindowGrid grid;
  const float* centers;  // [batch * 3] world poses, DEVICE memory
  int batch, count;      // B, W: batch * count <= INT_MAX
  const float2* pts;     // level-0 units
  const int* offsets;    // [batch + 1] or null
  int shared_n;
  float* out_lh;        // [batch * W] or null, window b at [b * W, (b + 1) * W)
  float* out_residual;  // [batch * W] or null
};

// scan b of the batch; b wave-uniform, so the two offsets are scalar loads
__device__ __forceinline__ const float2* window_batch_scan(const WindowBatchParams& P, int b, int& n) {
  int beg = 0;
  n = P.shared_n;
  if (P.offsets) {
    beg = P.offsets[b];
    n = P.offsets[b + 1] - beg;
  }
  return P.pts + beg;
}

// A LANE per hypothesis.  Every window is padded to whole wavefronts, so a wavefront's 64 lanes walk ONE scan: the beam index and
// the scan's base stay wave-uniform and an end point stays a scalar load.  The lanes behind a window's last hypothesis redo it and
// write nothing.  A workgroup's four wavefronts may belong to different scans (no LDS, no barrier).
template <int LAYOUT>
__global__ void __launch_bounds__(256) score_windows_batch_lane_kernel(const LevelView L, const WindowBatchParams P) {
  const int waves_per_window = (P.count + 63) >> 6;
  const long long gw = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (gw >= (long long)P.batch * waves_per_window) return;  // (a whole wavefront)
  const int b = __builtin_amdgcn_readfirstlane((int)(gw / waves_per_window));
  const int wv = __builtin_amdgcn_readfirstlane((int)(gw - (long long)b * waves_per_window));
  const int wl = wv * 64 + (int)(threadIdx.x & 63);
  const bool live = wl < P.count;
  const int w = live ? wl : P.count - 1;
  const float* __restrict__ center = P.centers + 3 * (size_t)b;
  float x, y, th;
  window_pose(P.grid, center[0], center[1], center[2], w, x, y, th);
  float ex, ey;
  affine_apply(L.mapTworld, x, y, ex, ey);  // getMapCoordsPose
  float sinRot, cosRot;
  sincos_f32(th, sinRot, cosRot);
  const float pt_scale = L.pt_scale;
  const LevelRegs R = level_regs<LAYOUT>(L);
  const f2 e2 = step_origin(ex, ey), cs = f2{cosRot, sinRot}, sc = f2{sinRot, cosRot};
  int n;
  const float2* __restrict__ pts = window_batch_scan(P, b, n);
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
  const size_t o = (size_t)b * (size_t)P.count + (size_t)w;
  if (P.out_lh) P.out_lh[o] = 1 - (residual / (float)n);  // n == 0: NaN
  if (P.out_residual) P.out_residual[o] = residual;
}

// A WAVEFRONT per hypothesis g = b * W + w; a workgroup's four wavefronts may belong to different scans.
template <int LAYOUT>
__global__ void __launch_bounds__(256) score_windows_batch_wave_kernel(const LevelView L, const WindowBatchParams P) {
  __shared__ float rows[4][64];
  const int lane = threadIdx.x & 63;
  const long long gl = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (gl >= (long long)P.batch * P.count) return;  // (a whole wavefront)
  const int g = __builtin_amdgcn_readfirstlane((int)gl);
  const int b = g / P.count, w = g - b * P.count;
  const float* __restrict__ center = P.centers + 3 * (size_t)b;
  float x, y, th;
  window_pose(P.grid, center[0], center[1], center[2], w, x, y, th);
  float ex, ey;
  affine_apply(L.mapTworld, x, y, ex, ey);
  float sinRot, cosRot;
  sincos_f32(th, sinRot, cosRot);
  const float pt_scale = L.pt_scale;
  const LevelRegs R = level_regs<LAYOUT>(L);
  const f2 e2 = step_origin(ex, ey), cs = f2{cosRot, sinRot}, sc = f2{sinRot, cosRot};
  int n;
  const float2* __restrict__ pts = window_batch_scan(P, b, n);
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
    if (P.out_lh) P.out_lh[g] = 1 - (residual / (float)n);
    if (P.out_residual) P.out_residual[g] = residual;
  }
}

// ---- window indices -> poses ------------------------------------------------------------------------------------------------
// index == nullptr: indices 0 .. count-1.  An index outside [0, W): three quiet NaNs.  Entry c belongs to window c / per_window,
// whose centre is center[3 * (c / per_window) ..]; one window: per_window = count.
__global__ void __launch_bounds__(256) window_poses_kernel(const WindowGrid g, int W, const float* __restrict__ centers,
                                                           const int* __restrict__ index, int count, int per_window,
                                                           float* __restrict__ out_pose) {
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  if (c >= count) return;
  const int w = index ? index[c] : (int)c;
  const float* __restrict__ center = centers + 3 * (size_t)(c / per_window);
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

// Groups: `groups` runs of `count` scores, one after the other, each sliced and merged on its own -- the wavefronts of stage 1
// are numbered group * slices + slice, stage 2 runs ONE workgroup per group, indices are relative to the group.  Two launches
// however many groups.
__global__ void __launch_bounds__(256) topk_slice_kernel(const float* __restrict__ scores, int count, int k, int slices, int groups,
                                                         float* __restrict__ cand_score, int* __restrict__ cand_index) {
  const int lane = threadIdx.x & 63;
  const long long gs = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (gs >= (long long)groups * slices) return;  // (a whole wavefront)
  const int group = __builtin_amdgcn_readfirstlane((int)(gs / slices));
  const int slice = __builtin_amdgcn_readfirstlane((int)(gs - (long long)group * slices));
  scores += (size_t)group * (size_t)count;
  cand_score += (size_t)group * (size_t)slices * (size_t)k;
  cand_index += (size_t)group * (size_t)slices * (size_t)k;
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
  cand_score += (size_t)blockIdx.x * (size_t)cands;  // blockIdx.x: the group
  cand_index += (size_t)blockIdx.x * (size_t)cands;
  out_index += (size_t)blockIdx.x * (size_t)k;
  if (out_score) out_score += (size_t)blockIdx.x * (size_t)k;
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

// the winner among the K candidates of every group -> the window index its start came from (in place).  io_index[g]: the winner's
// place among all the cands = groups * K candidates, as select_best_kernel leaves it, or -1
__global__ void __launch_bounds__(256) window_best_index_kernel(const int* __restrict__ cand_window_index, int cands, int groups,
                                                                int* __restrict__ io_index) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= groups) return;
  const int c = io_index[g];
  io_index[g] = c >= 0 && c < cands ? cand_window_index[c] : -1;
}

// ---- a CSR batch of scans laid out K times: the scans of hsm_relocalize_batch_device's B * K matches ---------------------------
// The batch matcher takes one scan per pair and cannot name a scan twice, so candidate c = b * K + r gets a copy of scan b.  Scan
// b is [lo, hi) with both ends clamped into [0, total_points] (an end before its beginning: an empty scan); its K copies fill
// [K * lo, K * hi) of the output, copy r at K * lo + r * (hi - lo).  K * hi <= K * total_points, so nothing is written beyond
// the region whatever the offsets hold, and with offsets that start at 0 and do not decrease the copies tile it.  One workgroup
// per candidate; out_offsets [B * K + 1].
__global__ void __launch_bounds__(256) replicate_scans_kernel(const float2* __restrict__ pts, const int* __restrict__ offsets,
                                                              int batch, int k, int total_points, float2* __restrict__ out_pts,
                                                              int* __restrict__ out_offsets) {
  const int c = (int)blockIdx.x;  // < batch * k
  const int b = c / k, r = c - b * k;
  const auto clamped = [total_points](int v) { return v < 0 ? 0 : (v > total_points ? total_points : v); };
  const int lo = clamped(offsets[b]), hi = clamped(offsets[b + 1]);
  const int n = hi > lo ? hi - lo : 0;
  const int at = k * lo + r * n;  // <= k * total_points <= INT_MAX
  if (threadIdx.x == 0) {
    out_offsets[c] = at;
    if (c == batch * k - 1) out_offsets[c + 1] = at + n;
  }
  for (int i = threadIdx.x; i < n; i += 256) out_pts[at + i] = pts[lo + i];
}

}  // namespace hsm
