// score_kernels.h -- the weighting, the covariance estimate and the ranking of batches of pose hypotheses (score_batch_kernel,
// covariance_batch_kernel, select_best_kernel), launched by match.hip only.  The likelihood of a scan at a pose -- frame, funval,
// the two summation orders, scan b of a batch: pose_score.h; the sigma-point statistics and the (score, index) order: gn_step.h.
#pragma once
#include <hip/hip_runtime.h>

#include "match_types.h"
#include "pose_score.h"

namespace hsm {

// ---- the weighting step of a batch of pose hypotheses, for what hsm_match_batch_device returns ---------------------------------
// B (WORLD pose, scan) pairs in one launch: the scans a CSR batch (offsets in points) or one shared scan, the poses converted to
// the level's map frame and the endpoints scaled by the level's 2^-level in the frame (pose_score.h pose_frame_world).  One
// wavefront per hypothesis, four per workgroup; pose and CSR offsets are read once per wavefront through the scalar unit.  EXACT:
// the reference's summation order, else the tree order.  A scan of 0 beams: residual +0, likelihood 1 - 0/0 = NaN, as the
// reference computes it.  Reads the map, the poses and the scans; writes its two outputs; keeps no other state.
template <int LAYOUT, bool EXACT>
__global__ void __launch_bounds__(256) score_batch_kernel(const LevelView L, const float* __restrict__ poses_world, int batch,
                                                          const float2* __restrict__ pts_all,
                                                          const int* __restrict__ offsets, int shared_n,
                                                          float* __restrict__ out_lh, float* __restrict__ out_residual) {
  __shared__ float rows[EXACT ? 4 : 1][EXACT ? 64 : 1];
  const int lane = threadIdx.x & 63;
  const int b = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));  // wave-uniform
  if (b >= batch) return;
  int n;
  const float2* __restrict__ pts = batch_scan(pts_all, offsets, shared_n, b, n);
  const PoseFrame F = pose_frame_world<LAYOUT>(L, poses_world[3 * b], poses_world[3 * b + 1], poses_world[3 * b + 2]);
  float residual;
  if (EXACT) residual = residual_reference_order<LAYOUT>(F, pts, n, rows[(threadIdx.x >> 6) & 3], lane);
  else residual = residual_tree_order<LAYOUT>(F, pts, n, lane);
  if (lane == 0) {
    if (out_lh) out_lh[b] = scan_likelihood(residual, n);
    if (out_residual) out_residual[b] = residual;       // getResidualForState (:205-221)
  }
}

// ---- the covariance estimate of a batch of pose hypotheses: pose_covariance_kernel for what hsm_match_batch_device returns ------
// getCovarianceForPose (OccGridMapUtil.h:106-160) + getCovMatrixWorldCoords (:162-188) for B (WORLD pose, scan) pairs in one
// launch, on score_batch_kernel's conventions (CSR or shared scan, getMapCoordsPose and pt_scale applied here, one wavefront per
// hypothesis, four per workgroup, pose and offsets read once per wavefront through the scalar unit).  A wavefront scores all
// seven sigma points of its hypothesis: a round of 64 beams loads and scales an end point once, the five sigma points that
// differ from the pose by a translation share one sincos_f32 and one rotated end point, the two angle sigma points have their own.
//
// Sharing the rotated end point leaves every bit as it was: the reference applies Translation * Rotation to the point, which is
// t + (R p) with R p evaluated first (beam_sample.h BeamRot), so R p does not depend on t; beam_fetch forms e + r from the same two
// operations, and the funval of the sample is pose_score.h's beam_funval.  Sigma point 6 is the pose: its likelihood is
// score_batch_kernel's, bit for bit.
//
// EXACT: the seven residuals are summed in the reference's beam order.  A round writes seven LDS rows of 64 funvals and lanes
// 0 .. 6 each add their own row left to right, so one pass of 64 dependent additions advances all seven chains.  Row k is stored
// rotated by 4 k floats, which keeps its float4s whole and puts the seven lanes' reads of one step into distinct banks.  Padding
// beyond the scan contributes +0 (pose_score.h residual_reference_order).  Else: lane-strided partial sums and a wave_allreduce per sigma point, the
// summation shape of pose_covariance_kernel<_, false>.  LDS: 7 x 64 x 4 B per wavefront (EXACT), none otherwise; no scratch.
// A scan of 0 beams: every likelihood 1 - 0/0 = NaN and with them every covariance, as the reference computes it.
// Lane 0 does the 7-term statistics (gn_step.h sigma_point_statistics, the probe's).  out_lh [B] = sigma point 6, contiguous.
template <int LAYOUT>
__device__ __forceinline__ float sigma_funval(const LevelRegs& R, f2 e, f2 r) {
  return beam_funval(sample_fetch<LAYOUT>(R, f2{e.x + r.x, e.y + r.y}));
}

template <int LAYOUT, bool EXACT>
__global__ void __launch_bounds__(256) covariance_batch_kernel(const LevelView L, const float* __restrict__ poses_world, int batch,
                                                               const float2* __restrict__ pts_all,
                                                               const int* __restrict__ offsets, int shared_n, float cell_length,
                                                               float* __restrict__ out_cov_world, float* __restrict__ out_cov_map,
                                                               float* __restrict__ out_lh7, float* __restrict__ out_lh) {
  __shared__ __attribute__((aligned(16))) float rows[EXACT ? 4 : 1][EXACT ? 7 : 1][EXACT ? 64 : 1];
  const int lane = threadIdx.x & 63;
  const int b = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));  // wave-uniform
  if (b >= batch) return;
  int n;
  const float2* __restrict__ pts = batch_scan(pts_all, offsets, shared_n, b, n);
  float x, y;
  affine_apply(L.mapTworld, poses_world[3 * b], poses_world[3 * b + 1], x, y);  // getMapCoordsPose
  float sp[7][3];
  sigma_points(x, y, poses_world[3 * b + 2], sp);
  // sigma points 0 .. 3 and 6 share the pose's angle, 4 and 5 the pose's origin
  float sinRot, cosRot, sinP, cosP, sinM, cosM;
  sincos_f32(sp[6][2], sinRot, cosRot);
  sincos_f32(sp[4][2], sinP, cosP);
  sincos_f32(sp[5][2], sinM, cosM);
  const float pt_scale = L.pt_scale;
  const LevelRegs R = level_regs<LAYOUT>(L);
  const f2 e0 = step_origin(sp[0][0], sp[0][1]), e1 = step_origin(sp[1][0], sp[1][1]), e2 = step_origin(sp[2][0], sp[2][1]),
           e3 = step_origin(sp[3][0], sp[3][1]), e6 = step_origin(sp[6][0], sp[6][1]);
  // the seven funvals of one beam; r = R(angle) p as beam_fetch forms it
  auto funvals = [&](float2 q, float fv[7]) {
    const f2 p = f2{q.x * pt_scale, q.y * pt_scale};
    const f2 r = f2{cosRot * p.x - sinRot * p.y, sinRot * p.x + cosRot * p.y};
    const f2 rp = f2{cosP * p.x - sinP * p.y, sinP * p.x + cosP * p.y};
    const f2 rm = f2{cosM * p.x - sinM * p.y, sinM * p.x + cosM * p.y};
    fv[0] = sigma_funval<LAYOUT>(R, e0, r);
    fv[1] = sigma_funval<LAYOUT>(R, e1, r);
    fv[2] = sigma_funval<LAYOUT>(R, e2, r);
    fv[3] = sigma_funval<LAYOUT>(R, e3, r);
    fv[4] = sigma_funval<LAYOUT>(R, e6, rp);
    fv[5] = sigma_funval<LAYOUT>(R, e6, rm);
    fv[6] = sigma_funval<LAYOUT>(R, e6, r);
  };
  float lh[7];
  if (EXACT) {
    float(*row)[EXACT ? 64 : 1] = rows[(threadIdx.x >> 6) & 3];
    const float* mine = row[lane < 7 ? lane : 6];  // lanes 0 .. 6: the chain of sigma point `lane`
    float run = 0.0f;
    for (int base = 0; base < n; base += 64) {  // wave-uniform trip count
      const int i = base + lane;
      float fv[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};  // padding beyond the scan: +0 changes no sum
      if (i < n) funvals(pts[i], fv);
#pragma unroll
      for (int k = 0; k < 7; ++k) row[k][(lane + 4 * k) & 63] = fv[k];
      // (one wavefront: its LDS operations execute in program order, no barrier)
      if (lane < 7) {
#pragma unroll 4
        for (int q = 0; q < 64; q += 4) {
          const float4 v = *reinterpret_cast<const float4*>(mine + ((q + 4 * lane) & 63));
          run += v.x;
          run += v.y;
          run += v.z;
          run += v.w;
        }
      }
    }
    const float mine_lh = scan_likelihood(run, n);  // in lane k for sigma point k
#pragma unroll
    for (int k = 0; k < 7; ++k) lh[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine_lh), k));
  } else {
    float res[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int i = lane; i < n; i += 64) {
      float fv[7];
      funvals(pts[i], fv);
#pragma unroll
      for (int k = 0; k < 7; ++k) res[k] += fv[k];
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) lh[k] = scan_likelihood(wave_allreduce(res[k]), n);
  }
  if (lane != 0) return;
  sigma_point_statistics(sp, lh, cell_length, out_lh7 ? out_lh7 + 7 * (size_t)b : nullptr,
                         out_cov_map ? out_cov_map + 9 * (size_t)b : nullptr, out_cov_world ? out_cov_world + 9 * (size_t)b : nullptr);
  if (out_lh) out_lh[b] = lh[6];
}

// WAVE_PER_GROUP: four groups per workgroup, one wavefront each (many small groups); else the whole workgroup takes one group.
// offsets [G+1] index `scores`, or nullptr = groups of `group_size` consecutive entries.  An empty or all-NaN group: index -1,
// score NaN, pose left as it is.
template <bool WAVE_PER_GROUP>
__global__ void __launch_bounds__(256) select_best_kernel(int groups, const int* __restrict__ offsets, int group_size,
                                                          const float* __restrict__ scores,
                                                          const float* __restrict__ poses, int* __restrict__ out_index,
                                                          float* __restrict__ out_score, float* __restrict__ out_pose) {
  __shared__ float ws[4];
  __shared__ int wi[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = __builtin_amdgcn_readfirstlane(WAVE_PER_GROUP ? (int)blockIdx.x * 4 + wave : (int)blockIdx.x);
  if (g >= groups) return;  // (a whole wavefront, and without WAVE_PER_GROUP the whole workgroup, at once)
  const int beg = offsets ? offsets[g] : g * group_size;
  const int end = offsets ? offsets[g + 1] : beg + group_size;
  float s = 0.0f;
  int i = -1;
  for (int k = beg + (WAVE_PER_GROUP ? lane : (int)threadIdx.x); k < end; k += WAVE_PER_GROUP ? 64 : 256) {
    const float v = scores[k];
    if (v == v && (i < 0 || v > s)) s = v, i = k;  // ascending k: an equal score later on never replaces the earlier one
  }
  wave_best(s, i);
  if (!WAVE_PER_GROUP) {
    if (lane == 0) ws[wave] = s, wi[wave] = i;
    __syncthreads();
    if (wave != 0) return;
    s = ws[lane & 3];
    i = wi[lane & 3];
#pragma unroll
    for (int off = 2; off > 0; off >>= 1) {
      const float so = __shfl_xor(s, off, 64);
      const int io = __shfl_xor(i, off, 64);
      if (best_beats(so, io, s, i)) s = so, i = io;
    }
  }
  if (lane != 0) return;
  out_index[g] = i;
  if (out_score) out_score[g] = i >= 0 ? s : __uint_as_float(0x7fc00000u);
  if (out_pose && i >= 0) {
    out_pose[3 * g + 0] = poses[3 * i + 0];
    out_pose[3 * g + 1] = poses[3 * i + 1];
    out_pose[3 * g + 2] = poses[3 * i + 2];
  }
}

}  // namespace hsm
