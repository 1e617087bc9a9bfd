// gn_step.h -- what every form of the matcher builds a Gauss-Newton step from, on top of the sampler (beam_sample.h): the nine
// per-beam products and their accumulators, the two summation orders (the reference's chains through LDS; wavefront and team
// all-reduces), the 3x3 solve, the residual chain, the sigma-point statistics and the (score, index) order of the scoring kernels, and how a launch says it
// is done or takes part in the pose exchange.  Included by the matcher kernel headers (gn_match_teams.h, gn_match_cached.h,
// gn_match_dense.h, gn_match_exact.h, gn_match_spec.h), by pose_score.h for the scoring kernels and by probe_kernels.h.  No kernel
// is defined here.
#pragma once
#include <hip/hip_runtime.h>

#include "beam_sample.h"
#include "match_types.h"
#include "pose_exchange.h"

namespace hsm {

__device__ __forceinline__ void publish_done(const MatchParams& P) {
  if (P.done_flag) __hip_atomic_store(P.done_flag, P.done_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- a matcher launch that takes part in the pose exchange itself (MatchParams::xp, pose_exchange.h) -------------------------------
// POST: the wavefront that has just finished scan `row` stores its pose -- three 8-byte {value, epoch tag} granules per rank, one
// system-scope store each (global_store_dwordx2 sc0 sc1), lanes 0 .. 3 world - 1 in ONE instruction -- into every rank's mailbox.
__device__ __forceinline__ void exchange_post_pose(const ExchangeFused& X, int row, float x, float y, float th) {
  const int l = (int)(threadIdx.x & 63u);
  if (l < 3 * X.world) {
    const int p = l / 3, c = l - 3 * p;
    const float v = c == 0 ? x : (c == 1 ? y : th);
    uint64_t* dst = X.peer[p] + X.post_off + (size_t)row * 3 + c;
    __hip_atomic_store(dst, ((uint64_t)X.post_tag << 32) | (uint64_t)__float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
// WAIT + unpack: workgroup `wb` of the `X.wait_blocks` extra workgroups behind the matcher's own (they are dispatched as those
// retire, i.e. into the launch's tail, when the epoch they wait for -- one match back -- has long arrived); bounded like the
// stand-alone kernel's wait (pose_exchange.hip)
__device__ __forceinline__ void exchange_wait_unpack(const ExchangeFused& X, int wb) {
  const uint64_t* box = X.peer[X.rank] + X.wait_off;
  unsigned long long t0 = 0;
  for (int i = wb * (int)blockDim.x + (int)threadIdx.x; i < X.total_granules; i += X.wait_blocks * (int)blockDim.x) {
    uint64_t g = __hip_atomic_load(box + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    bool late = false;
    while ((uint32_t)(g >> 32) != X.wait_tag) {
      if (t0 == 0) t0 = wall_clock64() | 1ull;
      __builtin_amdgcn_s_sleep(4);
      g = __hip_atomic_load(box + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      if ((uint32_t)(g >> 32) != X.wait_tag && wall_clock64() - t0 > X.timeout_ticks) {
        late = true;
        break;
      }
    }
    if (late) {
      __hip_atomic_fetch_add(X.status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(X.status + 1, X.wait_tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (X.out) X.out[i] = __uint_as_float(late ? 0x7fc00000u : (uint32_t)g);
  }
}

// per-beam contribution to (dTr, H) -- OccGridMapUtil.h:76-98; paired accumulators
struct Acc9 {
  f2 d01;   // dTr[0], dTr[1]
  f2 hd;    // H(0,0), H(1,1)
  f2 hr;    // H(0,2), H(1,2)
  float d2, h22, h01;
  __device__ __forceinline__ void zero() {
    d01 = hd = hr = f2{0.0f, 0.0f};
    d2 = h22 = h01 = 0.0f;
  }
};

// With g = -G (the source's gx, gy) and rd = rotDeriv, in IEEE arithmetic:
//   rd      = (-ry)*gx + rx*gy = ry*Gx - rx*Gy          (sign flips are exact)
//   dTr    += g*funVal, rd*funVal  ==  dTr -= G*funVal  (a + (-b) == a - b)
//   H      += g*g, gx*gy           ==  G*G, Gx*Gy
//   H(.,2) += g*rd                 ==  H(.,2) -= G*rd
__device__ __forceinline__ float beam_finish(const BeamSample& b, const BeamRot& r, Acc9& a,
                                             BeamTerms* terms_out = nullptr) {
  const BeamTerms t = sample_finish(b);
  const float Gx = t.G.x, Gy = t.G.y;
  const float funVal = 1.0f - t.M;
  const float rotDeriv = r.r.y * Gx - r.r.x * Gy;  // :87
  a.d01.x -= Gx * funVal;
  a.d01.y -= Gy * funVal;
  a.d2 += rotDeriv * funVal;
  a.hd.x += Gx * Gx;
  a.hd.y += Gy * Gy;
  a.h22 += rotDeriv * rotDeriv;
  a.h01 += Gx * Gy;
  a.hr.x -= Gx * rotDeriv;
  a.hr.y -= Gy * rotDeriv;
  if (terms_out) *terms_out = t;
  return rotDeriv;
}

template <int LAYOUT>
__device__ __forceinline__ float beam_accumulate(const LevelRegs& L, float ex, float ey, float sinRot,
                                                 float cosRot, float px, float py, Acc9& a,
                                                 BeamTerms* terms_out = nullptr) {
  BeamRot r;
  const BeamSample b = beam_fetch<LAYOUT>(L, step_origin(ex, ey), f2{cosRot, sinRot}, f2{sinRot, cosRot}, f2{px, py}, r);
  return beam_finish(b, r, a, terms_out);
}

// ---- HSM_PARITY_EXACT: the reference's summation ORDER -------------------------------------------
// getCompleteHessianDerivs (OccGridMapUtil.h:76-98) runs nine independent fp32 chains over the beams,
// acc_t = acc_t + product_t(i) for i = 0 .. n-1.  The products are the same bits in every form of the
// matcher; what the throughput forms change is the order of the additions (lane-strided partial sums +
// tree), which is where the last-bit differences of H and dTr -- and, on scans where Gauss-Newton has
// not settled, the visible pose differences -- come from.  The exact form keeps the reference's order:
// a round of T consecutive beams (one per lane of the team) writes its 9 x T products to LDS, row t =
// term t, and lane t of the team's first wave (t = 0..8) adds row t to its running sum left to right.
// The nine chains run side by side in nine lanes; a round costs 64 dependent v_add_f32 per 64 beams on
// top of the beam arithmetic (about 2.5x the instruction count of the fast form).  Padding lanes and
// out-of-map beams contribute +-0, which leaves a running sum that started at +0 unchanged bit for bit.
constexpr int kExactGroupRounds = 5;  // rounds the exact-order team form fetches, stages and sums together; a scan of at most that
                                      // many rounds keeps its endpoints in registers (xq_resident): it is read from memory ONCE
constexpr int kExactPad = 4;  // row stride T + 4 floats: rows stay 16-byte aligned, the nine chain lanes hit distinct banks

// the nine products with the reference's signs (g = -G): dTr[0..2], H(0,0), H(1,1), H(2,2), H(0,1), H(0,2), H(1,2)
__device__ __forceinline__ void beam_products(const BeamSample& b, const BeamRot& r, float pr[9]) {
  const BeamTerms t = sample_finish(b);
  const float Gx = t.G.x, Gy = t.G.y;
  const float funVal = 1.0f - t.M;
  const float rotDeriv = r.r.y * Gx - r.r.x * Gy;  // :87
  pr[0] = -(Gx * funVal);
  pr[1] = -(Gy * funVal);
  pr[2] = rotDeriv * funVal;
  pr[3] = Gx * Gx;
  pr[4] = Gy * Gy;
  pr[5] = rotDeriv * rotDeriv;
  pr[6] = Gx * Gy;
  pr[7] = -(Gx * rotDeriv);
  pr[8] = -(Gy * rotDeriv);
}

// one round: beams base .. base+T-1 (thread tid holds beam base+tid).  `run` is meaningful in threads
// 0..8 of the team only.  T == 64: one wavefront, whose LDS operations execute in program order -- no
// barrier; T > 64: the team owns its workgroup and synchronises around the chain.
// `count` = beams of this round that exist (the lanes beyond stage +-0 products, which leave a running sum unchanged bit for
// bit, so the chain stops after the last float4 pair that holds a real beam).  The row streams through two 32-byte halves:
// a half is requested again right after its values are consumed, so a dependent addition costs its own latency (8.5 cycles
// on a lone wavefront, tools/ubench_chain.hip) instead of 14.4 with one 16-byte read in flight -- the chain is 1081 x 14
// additions of a single-scan match in exact mode, ~100 of its ~135 us before.
// stage the nine products of the beam at position `pos` of rows of RL beams
template <int RL>
__device__ __forceinline__ void exact_stage(const float pr[9], float* __restrict__ stage, int pos) {
#pragma unroll
  for (int t = 0; t < 9; ++t) stage[t * (RL + kExactPad) + pos] = pr[t];
}

// the chains over the first `count` beams of the staged rows (rows of RL beams; SYNC: the team is wider than one wavefront)
template <int RL, bool SYNC>
__device__ __forceinline__ float exact_chain(float* __restrict__ stage, int tid, float run, int count) {
  if (SYNC) __syncthreads();
  if (tid < 9) {
    const f4v* row = reinterpret_cast<const f4v*>(stage + tid * (RL + kExactPad));
    // 16 beams per iteration, branch-free (loads behind a branch make the compiler wait for all of them): the last
    // iteration's read-ahead is clamped into the row, beams between `count` and the next multiple of 16 add their +-0
    const int nq = ((count + 15) >> 4) << 2;  // float4s, a multiple of 4, <= RL / 4
    f4v a0 = row[0], a1 = row[1], b0 = row[2], b1 = row[3];  // two 32-byte halves in flight
    // (the additions as inline asm: left to itself the compiler keeps the running sum in the registers of the half it is
    // consuming, which postpones that half's refill to the end of the iteration -- one exposed LDS round trip per 16 beams)
    auto add8 = [&](const f4v& u, const f4v& v) {
      asm volatile(
          "v_add_f32 %0, %1, %0\n\tv_add_f32 %0, %2, %0\n\tv_add_f32 %0, %3, %0\n\tv_add_f32 %0, %4, %0\n\t"
          "v_add_f32 %0, %5, %0\n\tv_add_f32 %0, %6, %0\n\tv_add_f32 %0, %7, %0\n\tv_add_f32 %0, %8, %0"
          : "+v"(run)
          : "v"(u.x), "v"(u.y), "v"(u.z), "v"(u.w), "v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w)
          : "memory");
    };
    for (int q = 0; q < nq; q += 4) {
      add8(a0, a1);
      const int qa = min(q + 4, RL / 4 - 4);  // refilled right behind its last use: eight additions to arrive in
      a0 = row[qa], a1 = row[qa + 1];
      add8(b0, b1);
      b0 = row[qa + 2], b1 = row[qa + 3];
    }
  }
  if (SYNC) __syncthreads();
  return run;
}

// one round of T beams: stage, sum
template <int T>
__device__ __forceinline__ float exact_round(const float pr[9], float* __restrict__ stage, int tid, float run, int count = T) {
  exact_stage<T>(pr, stage, tid);
  return exact_chain<T, (T > 64)>(stage, tid, run, count);
}

// Wavefront all-reduce without LDS traffic: four DPP steps inside each row of 16 lanes (the
// cross-lane operand rides on the v_add itself), then the two gfx950 row/half swaps
// (v_permlane16_swap, v_permlane32_swap).  Every lane ends with the same bits.
template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}

__device__ __forceinline__ float wave_allreduce(float v) {
  v += dpp_f32<0xB1>(v);   // quad_perm [1,0,3,2]: lane ^ 1
  v += dpp_f32<0x4E>(v);   // quad_perm [2,3,0,1]: lane ^ 2
  v += dpp_f32<0x141>(v);  // row_half_mirror: the other quad of the 8-lane half row
  v += dpp_f32<0x140>(v);  // row_mirror: the other half of the 16-lane row
  {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_int(v), __float_as_int(v), false, false);
    v = __int_as_float(r[0]) + __int_as_float(r[1]);  // rows 0+1, 2+3
  }
  {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_int(v), __float_as_int(v), false, false);
    v = __int_as_float(r[0]) + __int_as_float(r[1]);  // lower + upper 32 lanes
  }
  return v;
}

// The nine totals at once, "folded": a butterfly level that pairs lanes i and p(i) needs the sum of a value only in
// ONE lane of each pair if the other lane of the pair carries a second value -- so each level halves the number of
// live registers instead of keeping nine.  v_permlane32_swap / v_permlane16_swap do exactly that for two registers
// (swap + add = 2 instructions per PAIR of values instead of mov + swap + add per value), the two row levels do it with
// DPP bank masks (v_add_f32_dpp writes only the enabled banks of its destination), and the last two levels run on
// the single register that is left.  25 instructions + 9 v_readlane_b32 (the totals end up in SGPRs, identical in
// every lane) instead of 90.  Level order 32, 16, row_mirror, row_half_mirror, lane^2, lane^1 -- the same pairing
// tree for all nine values.
__device__ __forceinline__ float fold_swap32(float a, float b) {  // lanes 0..31: a[i] + a[i+32];  32..63: b[i-32] + b[i]
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_int(a), __float_as_int(b), false, false);
  return __int_as_float(r[0]) + __int_as_float(r[1]);
}
__device__ __forceinline__ float fold_swap16(float a, float b) {  // rows 0, 2: a (row + row^1);  rows 1, 3: b
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_int(a), __float_as_int(b), false, false);
  return __int_as_float(r[0]) + __int_as_float(r[1]);
}

__device__ __forceinline__ void wave_allreduce9(Acc9& a) {
  // level 32 and level 16: the totals over the four rows, per column of 16
  const float a0 = fold_swap32(a.d01.x, a.d01.y);  // rows 0,1: dTr0   rows 2,3: dTr1
  const float a1 = fold_swap32(a.d2, a.hd.x);      //           dTr2             H00
  const float a2 = fold_swap32(a.hd.y, a.h22);     //           H11              H22
  const float a3 = fold_swap32(a.h01, a.hr.x);     //           H01              H02
  const float a4 = fold_swap32(a.hr.y, a.hr.y);    // H12 everywhere
  float b0 = fold_swap16(a0, a1);                  // rows: dTr0, dTr2, dTr1, H00
  float b1 = fold_swap16(a2, a3);                  // rows: H11,  H01,  H22,  H02
  float b2 = fold_swap16(a4, a4);                  // H12 in every row
  // row levels.  s_nop: the hazard recogniser does not look into inline asm (a DPP operand needs two wait states
  // after the VALU write of its register)
  asm("s_nop 1\n\t"
      // row_mirror (lane i <-> 15 - i): banks 2,3 of b1 keep b1's sums, banks 0,1 of b1 take b0's; b2 plain
      "v_add_f32_dpp %[b1], %[b1], %[b1] row_mirror row_mask:0xf bank_mask:0xc\n\t"
      "v_add_f32_dpp %[b1], %[b0], %[b0] row_mirror row_mask:0xf bank_mask:0x3\n\t"
      "v_add_f32_dpp %[b2], %[b2], %[b2] row_mirror row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\t"
      // row_half_mirror (i <-> 7 - i inside each half row): banks 1,3 of b2 keep H12, banks 0,2 take b1's
      "v_add_f32_dpp %[b2], %[b2], %[b2] row_half_mirror row_mask:0xf bank_mask:0xa\n\t"
      "v_add_f32_dpp %[b2], %[b1], %[b1] row_half_mirror row_mask:0xf bank_mask:0x5\n\t"
      "s_nop 1\n\t"
      "v_add_f32_dpp %[b2], %[b2], %[b2] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\t"
      "v_add_f32_dpp %[b2], %[b2], %[b2] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1"
      : [b1] "+v"(b1), [b2] "+v"(b2)
      : [b0] "v"(b0));
  // where the totals sit: lane 16 * row + 4 * bank.  bank 0 <- b0's rows, bank 2 <- b1's rows, banks 1, 3 <- H12
  auto lane_value = [&](int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(b2), lane)); };
  a.d01.x = lane_value(0);
  a.d2 = lane_value(16);
  a.d01.y = lane_value(32);
  a.hd.x = lane_value(48);
  a.hd.y = lane_value(8);
  a.h01 = lane_value(24);
  a.h22 = lane_value(40);
  a.hr.x = lane_value(56);
  a.hr.y = lane_value(4);
}

// team-wide totals: wave all-reduce, then (WPS > 1) LDS staging of the per-wave partials; every thread of the team
// returns with identical bits.  The stage is TRANSPOSED, red[buf][term][wave]: after the barrier lane t (t < 9) reads the
// WPS partials of term t as 16-byte rows and adds them in wave order (the same order as ever: w = 0, 1, 2, ...), and nine
// v_readlane hand the totals to every lane as SGPRs -- 1 + 3 + 9 instructions for four waves instead of the 36 LDS reads
// and 27 additions every lane used to do on its own (the exchange sits on the 14-step dependent chain of a single-scan
// match: its cost grows with WPS, which is what held wider teams back).
template <int WPS>
__device__ __forceinline__ void team_allreduce9(Acc9& a, float (*red)[9][WPS < 4 ? 4 : WPS], int buf, int wave_in_team,
                                                int lane) {
  wave_allreduce9(a);
  if (WPS > 1) {
    if (lane == 0) {
      float(*r)[WPS < 4 ? 4 : WPS] = red[buf];
      r[0][wave_in_team] = a.d01.x; r[1][wave_in_team] = a.d01.y; r[2][wave_in_team] = a.d2;
      r[3][wave_in_team] = a.hd.x; r[4][wave_in_team] = a.hd.y; r[5][wave_in_team] = a.h22;
      r[6][wave_in_team] = a.h01; r[7][wave_in_team] = a.hr.x; r[8][wave_in_team] = a.hr.y;
    }
    __syncthreads();
    const float* row = red[buf][lane < 9 ? lane : 8];
    float t = row[0];
#pragma unroll
    for (int w = 1; w < WPS; ++w) t += row[w];
    auto total = [&](int k) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t), k)); };
    a.d01 = f2{total(0), total(1)}; a.d2 = total(2);
    a.hd = f2{total(3), total(4)}; a.h22 = total(5);
    a.h01 = total(6); a.hr = f2{total(7), total(8)};
  }
}

// H.inverse() * dTr as Eigen evaluates it (LU/InverseImpl.h cofactors * invdet, then a
// coefficient-based product; 3-term sums are x0 + (x1 + x2)), ScanMatcher.h:201-217.
//
// A NON-FINITE estimate (a step that divided by a determinant of 0 or overflowed): every beam of the evaluation that filled `a`
// was outside the map -- inf + r is beyond every limit for the reference too, and a NaN coordinate counts as outside
// (cell_coord) -- so each must have contributed the reference's exact zeros for M and both gradients.  The all-zero texel
// delivers them only through finite fractions, and v_fract_f32 of inf or NaN is NaN; instead of two selects per beam the
// totals are put right here, once per step and wave-uniformly: the sums of +-0 products are +0, and the four sums that hold
// rotDeriv are NaN where the angle itself is not finite (sinf / cosf of it are NaN: NaN * 0), +0 otherwise.  H(0,0) == 0 then
// skips the step as the reference's own test does, and `a` (the covariance and the hook trace read it) says what was summed.
__device__ __forceinline__ void gn_solve_and_step(Acc9& a, float& ex, float& ey, float& eth) {
  const float rot_nf = eth - eth;  // +0 for a finite value, NaN for inf and NaN
  if (((ex - ex) + (ey - ey)) + rot_nf != 0.0f) {
    a.d01 = a.hd = f2{0.0f, 0.0f};
    a.h01 = 0.0f;
    a.hr = f2{rot_nf, rot_nf};
    a.d2 = a.h22 = rot_nf;
    return;
  }
  if ((a.hd.x != 0.0f) && (a.hd.y != 0.0f)) {
    // symmetric H: m(r,c)
    const float m00 = a.hd.x, m01 = a.h01, m02 = a.hr.x;
    const float m10 = a.h01, m11 = a.hd.y, m12 = a.hr.y;
    const float m20 = a.hr.x, m21 = a.hr.y, m22 = a.h22;
    // cofactor_3x3<i,j> = m(i1,j1)*m(i2,j2) - m(i1,j2)*m(i2,j1), i1=(i+1)%3 ...
    const float c00 = m11 * m22 - m12 * m21;
    const float c10 = m21 * m02 - m22 * m01;
    const float c20 = m01 * m12 - m02 * m11;
    const float det = c00 * m00 + (c10 * m10 + c20 * m20);
    const float invdet = 1.0f / det;
    const float i00 = c00 * invdet, i01 = c10 * invdet, i02 = c20 * invdet;
    const float i10 = (m12 * m20 - m10 * m22) * invdet;  // cofactor<0,1>
    const float i11 = (m22 * m00 - m20 * m02) * invdet;  // cofactor<1,1>
    const float i12 = (m02 * m10 - m00 * m12) * invdet;  // cofactor<2,1>
    const float i20 = (m10 * m21 - m11 * m20) * invdet;  // cofactor<0,2>
    const float i21 = (m20 * m01 - m21 * m00) * invdet;  // cofactor<1,2>
    const float i22 = (m00 * m11 - m01 * m10) * invdet;  // cofactor<2,2>
    const float s0 = i00 * a.d01.x + (i01 * a.d01.y + i02 * a.d2);
    const float s1 = i10 * a.d01.x + (i11 * a.d01.y + i12 * a.d2);
    float s2 = i20 * a.d01.x + (i21 * a.d01.y + i22 * a.d2);
    if (s2 > 0.2f) {
      s2 = 0.2f;
    } else if (s2 < -0.2f) {
      s2 = -0.2f;
    }
    ex += s0;
    ey += s1;
    eth += s2;
  }
}

// a wave-uniform value moved to an SGPR
__device__ __forceinline__ float uniform_f32(float v) {
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

// One residual chain in the reference's order (getResidualForState: residual += funval, i = 0 .. n-1), the
// HSM_PARITY_EXACT counterpart of wave_allreduce in the likelihood and scoring kernels: a round of 64 beams writes its funvals to the wavefront's
// LDS row and lane 0 adds them left to right (same idea as exact_round, one term instead of nine).  Every lane returns
// the running sum that is only meaningful in lane 0.
__device__ __forceinline__ float exact_residual_round(float funval, float* __restrict__ row, int lane, float run) {
  row[lane] = funval;
  if (lane == 0) {
#pragma unroll 4
    for (int q = 0; q < 64; q += 4) {
      const float4 v = *reinterpret_cast<const float4*>(row + q);
      run += v.x;
      run += v.y;
      run += v.z;
      run += v.w;
    }
  }
  return run;
}

// ---- the sigma-point covariance estimate (OccGridMapUtil::getCovarianceForPose, OccGridMapUtil.h:106-160) ----------------------
// the seven sigma points around a MAP-frame pose, in the source's order (:119-125): x +- 1.5 cells, y +- 1.5 cells, angle +- 0.05,
// the pose itself.  (Host-callable as well: tests/cpp/sigma_stats_check.cpp holds both functions to the numpy restatement.)
__host__ __device__ __forceinline__ void sigma_points(float x, float y, float ang, float sp[7][3]) {
  const float deltaTransX = 1.5f, deltaTransY = 1.5f, deltaAng = 0.05f;
  const float s[7][3] = {{x + deltaTransX, y, ang}, {x - deltaTransX, y, ang}, {x, y + deltaTransY, ang},
                         {x, y - deltaTransY, ang}, {x, y, ang + deltaAng},    {x, y, ang - deltaAng}, {x, y, ang}};
  for (int i = 0; i < 7; ++i)
    for (int r = 0; r < 3; ++r) sp[i][r] = s[i][r];
}

// The 7-term statistics in the source's order (:138-154) and getCovMatrixWorldCoords (:162-188): the seven likelihoods `lh`
// weight a sample mean and a 3x3 sample covariance of the sigma points.  One thread; the three outputs are one pose's rows
// (7, 9 and 9 floats, the matrices column major), each may be null.
__host__ __device__ __forceinline__ void sigma_point_statistics(const float sp[7][3], const float* lh, float cell_length,
                                                                float* out_lh7, float* out_cov_map, float* out_cov_world) {
  // likelihoods.sum(): fixed-size 7-vector, unrolled halves (0..2) + (3..6)
  const float sum = ((lh[0] + (lh[1] + lh[2])) + ((lh[3] + lh[4]) + (lh[5] + lh[6])));
  const float invLhNormalizer = 1 / sum;
  float mean[3] = {0.0f, 0.0f, 0.0f};
  for (int i = 0; i < 7; ++i)
    for (int r = 0; r < 3; ++r) mean[r] += sp[i][r] * lh[i];
  for (int r = 0; r < 3; ++r) mean[r] *= invLhNormalizer;
  float cov[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // column major
  for (int i = 0; i < 7; ++i) {
    const float d[3] = {sp[i][0] - mean[0], sp[i][1] - mean[1], sp[i][2] - mean[2]};
    const float wgt = lh[i] * invLhNormalizer;
    for (int c = 0; c < 3; ++c)
      for (int r = 0; r < 3; ++r) cov[c * 3 + r] += wgt * (d[r] * d[c]);
  }
  if (out_lh7)
    for (int i = 0; i < 7; ++i) out_lh7[i] = lh[i];
  if (out_cov_map)
    for (int i = 0; i < 9; ++i) out_cov_map[i] = cov[i];
  if (out_cov_world) {
    const float scaleTrans = cell_length, scaleTransSq = scaleTrans * scaleTrans;
    float* W = out_cov_world;  // (r,c) at c*3+r
    W[0] = cov[0] * scaleTransSq;
    W[4] = cov[4] * scaleTransSq;
    W[1] = cov[1] * scaleTransSq;  // (1,0)
    W[3] = W[1];
    W[2] = cov[2] * scaleTrans;  // (2,0)
    W[6] = W[2];
    W[5] = cov[5] * scaleTrans;  // (2,1)
    W[7] = W[5];
    W[8] = cov[8];
  }
}

// ---- ranking inside groups of hypotheses ------------------------------------------------------------------------------------
// Per group the entry with the highest score.  The order is on the PAIR (score, index): a NaN never takes part; a beats b when
// its score is greater, or equal (as floats: +0 == -0) with the lower index.  That is a strict total order on the entries that
// take part, so the maximum is unique and every reduction shape finds the same one: no float atomics, no arrival order.
__device__ __forceinline__ bool best_beats(float sa, int ia, float sb, int ib) {
  return ia >= 0 && (ib < 0 || sa > sb || (sa == sb && ia < ib));
}
__device__ __forceinline__ void wave_best(float& s, int& i) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float so = __shfl_xor(s, off, 64);
    const int io = __shfl_xor(i, off, 64);
    if (best_beats(so, io, s, i)) s = so, i = io;
  }
}

}  // namespace hsm
