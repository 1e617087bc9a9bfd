// window_kernels.h -- the kernels of window.hip: the likelihood of ONE scan at every pose of a window that never exists in memory
// (two forms with the same bits), window indices turned into poses, and the K best of an array of scores; each with a batch
// dimension too -- B scans in B windows of one shape, the K best of every group -- and the copy that lays a CSR batch of scans out
// K times for the matcher.  The score of one hypothesis is pose_score.h's: a window kernel only says which hypothesis a lane or
// a wavefront is and where its centre, its scan and its output slot are.
#pragma once
#include <hip/hip_runtime.h>

#include "match_types.h"
#include "pose_score.h"
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

// B windows of one shape, window b around centre b against scan b, in ONE launch: the same bits as B launches of the single
// kernels -- a hypothesis' chain is its own whatever else the launch holds.  The scans are a CSR batch or (offsets == nullptr) one
// scan of shared_n beams for every window.
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

// hypothesis w of the window around `center`, as a frame
template <int LAYOUT>
__device__ __forceinline__ PoseFrame window_frame(const LevelView& L, const WindowGrid& grid, const float* center, int w) {
  float x, y, th;
  window_pose(grid, center[0], center[1], center[2], w, x, y, th);
  return pose_frame_world<LAYOUT>(L, x, y, th);
}

// likelihood and residual of one hypothesis into slot `o` of the outputs that exist
__device__ __forceinline__ void window_store(float* out_lh, float* out_residual, size_t o, float residual, int n) {
  if (out_lh) out_lh[o] = scan_likelihood(residual, n);
  if (out_residual) out_residual[o] = residual;       // getResidualForState (:205-221)
}

// ---- one LANE per hypothesis (pose_score.h residual_lane_chain) -----------------------------------------------------------------
// Lane wl of a window's wavefronts takes hypothesis wl; the lanes behind the last hypothesis redo the last one (no divergent
// exit; they write nothing).  Lanes that are neighbours in x sample neighbouring texels.  `slot`: where the window's scores begin.
template <int LAYOUT>
__device__ __forceinline__ void score_window_lane(const LevelView& L, const WindowGrid& grid, const float* center, int count,
                                                  long long wl, const float2* __restrict__ pts, int n, float* out_lh,
                                                  float* out_residual, size_t slot) {
  const bool live = wl < count;
  const int w = live ? (int)wl : count - 1;
  const PoseFrame F = window_frame<LAYOUT>(L, grid, center, w);
  const float residual = residual_lane_chain<LAYOUT>(F, pts, n);
  if (live) window_store(out_lh, out_residual, slot + (size_t)w, residual, n);
}

template <int LAYOUT>
__global__ void __launch_bounds__(256) score_window_lane_kernel(const LevelView L, const WindowParams P) {
  score_window_lane<LAYOUT>(L, P.grid, P.center, P.count, (long long)blockIdx.x * 256 + threadIdx.x, P.pts, P.n, P.out_lh,
                            P.out_residual, 0);
}

// Every window is padded to whole wavefronts, so a wavefront's 64 lanes walk ONE scan: the beam index and the scan's base stay
// wave-uniform and an end point stays a scalar load.  A workgroup's four wavefronts may belong to different scans (no LDS, no
// barrier).
template <int LAYOUT>
__global__ void __launch_bounds__(256) score_windows_batch_lane_kernel(const LevelView L, const WindowBatchParams P) {
  const int waves_per_window = (P.count + 63) >> 6;
  const long long gw = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (gw >= (long long)P.batch * waves_per_window) return;  // (a whole wavefront)
  const int b = __builtin_amdgcn_readfirstlane((int)(gw / waves_per_window));
  const int wv = __builtin_amdgcn_readfirstlane((int)(gw - (long long)b * waves_per_window));
  int n;
  const float2* pts = batch_scan(P.pts, P.offsets, P.shared_n, b, n);
  score_window_lane<LAYOUT>(L, P.grid, P.centers + 3 * (size_t)b, P.count, wv * 64 + (int)(threadIdx.x & 63), pts, n, P.out_lh,
                            P.out_residual, (size_t)b * (size_t)P.count);
}

// ---- one WAVEFRONT per hypothesis (pose_score.h residual_reference_order): score_batch_kernel<LAYOUT, true> with the pose
// generated from w; lane 0 stores ----------------------------------------------------------------------------------------------
template <int LAYOUT>
__device__ __forceinline__ void score_window_wave(const LevelView& L, const WindowGrid& grid, const float* center, int w,
                                                  const float2* __restrict__ pts, int n, float* __restrict__ row, float* out_lh,
                                                  float* out_residual, size_t o) {
  const int lane = threadIdx.x & 63;
  const PoseFrame F = window_frame<LAYOUT>(L, grid, center, w);
  const float residual = residual_reference_order<LAYOUT>(F, pts, n, row, lane);
  if (lane == 0) window_store(out_lh, out_residual, o, residual, n);
}

template <int LAYOUT>
__global__ void __launch_bounds__(256) score_window_wave_kernel(const LevelView L, const WindowParams P) {
  __shared__ float rows[4][64];
  const long long wl = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wl >= P.count) return;  // (a whole wavefront)
  const int w = __builtin_amdgcn_readfirstlane((int)wl);
  score_window_wave<LAYOUT>(L, P.grid, P.center, w, P.pts, P.n, rows[(threadIdx.x >> 6) & 3], P.out_lh, P.out_residual, (size_t)w);
}

// hypothesis g = b * W + w; a workgroup's four wavefronts may belong to different scans
template <int LAYOUT>
__global__ void __launch_bounds__(256) score_windows_batch_wave_kernel(const LevelView L, const WindowBatchParams P) {
  __shared__ float rows[4][64];
  const long long gl = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (gl >= (long long)P.batch * P.count) return;  // (a whole wavefront)
  const int g = __builtin_amdgcn_readfirstlane((int)gl);
  const int b = g / P.count, w = g - b * P.count;
  int n;
  const float2* pts = batch_scan(P.pts, P.offsets, P.shared_n, b, n);
  score_window_wave<LAYOUT>(L, P.grid, P.centers + 3 * (size_t)b, w, pts, n, rows[(threadIdx.x >> 6) & 3], P.out_lh, P.out_residual,
                            (size_t)g);
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
