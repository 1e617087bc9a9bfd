// score_kernels.h -- the weighting and ranking of batches of pose hypotheses (score_batch_kernel, select_best_kernel), launched
// by match.hip only.  Sampler: beam_sample.h; the residual chain and the (score, index) order: gn_step.h.
#pragma once
#include <hip/hip_runtime.h>

#include "beam_sample.h"
#include "gn_step.h"
#include "match_types.h"

namespace hsm {

// ---- the weighting step of a batch of pose hypotheses: likelihood_kernel for what hsm_match_batch_device returns --------------
// B (WORLD pose, scan) pairs in one launch: the scans a CSR batch (offsets in points) or one shared scan, the poses converted to
// the level's map frame here (getMapCoordsPose, GridMapBase.h:235-239 -- the matchers' own first step), the endpoints scaled by
// the level's 2^-level (DataContainer::setFrom).  One wavefront per hypothesis, four per workgroup; pose and CSR offsets are
// read once per wavefront through the scalar unit.  Sampler, zero-texel treatment of out-of-map beams and the two summation
// orders are likelihood_kernel's.  A scan of 0 beams: residual +0, likelihood 1 - 0/0 = NaN, as the reference computes it.
// Reads the map, the poses and the scans; writes its two outputs; keeps no other state.
template <int LAYOUT, bool EXACT>
__global__ void __launch_bounds__(256) score_batch_kernel(const LevelView L, const float* __restrict__ poses_world, int batch,
                                                          const float2* __restrict__ pts_all,
                                                          const int* __restrict__ offsets, int shared_n,
                                                          float* __restrict__ out_lh, float* __restrict__ out_residual) {
  __shared__ float rows[EXACT ? 4 : 1][EXACT ? 64 : 1];
  const int lane = threadIdx.x & 63;
  const int b = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));  // wave-uniform
  if (b >= batch) return;
  int beg = 0, n = shared_n;
  if (offsets) {
    beg = offsets[b];
    n = offsets[b + 1] - beg;
  }
  const float2* __restrict__ pts = pts_all + beg;
  float ex, ey;
  affine_apply(L.mapTworld, poses_world[3 * b], poses_world[3 * b + 1], ex, ey);  // getMapCoordsPose
  float sinRot, cosRot;
  sincos_f32(poses_world[3 * b + 2], sinRot, cosRot);
  const float pt_scale = L.pt_scale;
  const LevelRegs R = level_regs<LAYOUT>(L);
  const f2 e2 = step_origin(ex, ey), cs = f2{cosRot, sinRot}, sc = f2{sinRot, cosRot};
  float residual = 0.0f;
  if (EXACT) {
    float* row = rows[(threadIdx.x >> 6) & 3];
    for (int base = 0; base < n; base += 64) {  // wave-uniform trip count
      const int i = base + lane;
      float funval = 0.0f;  // padding beyond the scan: +0 changes no sum (see likelihood_kernel)
      if (i < n) {
        const float2 p = pts[i];
        BeamRot r;
        const BeamSample s = beam_fetch<LAYOUT>(R, e2, cs, sc, f2{p.x * pt_scale, p.y * pt_scale}, r);
        const float M = ((s.lo.x * s.X.x + s.lo.y * s.X.y) * (s.Y.x)) + ((s.hi.x * s.X.x + s.hi.y * s.X.y) * (s.Y.y));
        funval = 1.0f - M;
      }
      residual = exact_residual_round(funval, row, lane, residual);
    }
  } else {
    for (int i = lane; i < n; i += 64) {
      const float2 p = pts[i];
      BeamRot r;
      const BeamSample s = beam_fetch<LAYOUT>(R, e2, cs, sc, f2{p.x * pt_scale, p.y * pt_scale}, r);
      const float M = ((s.lo.x * s.X.x + s.lo.y * s.X.y) * (s.Y.x)) + ((s.hi.x * s.X.x + s.hi.y * s.X.y) * (s.Y.y));
      residual += 1.0f - M;
    }
    residual = wave_allreduce(residual);
  }
  if (lane == 0) {
    if (out_lh) out_lh[b] = 1 - (residual / (float)n);  // getLikelihoodForState (:184-203)
    if (out_residual) out_residual[b] = residual;       // getResidualForState (:205-221)
  }
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
