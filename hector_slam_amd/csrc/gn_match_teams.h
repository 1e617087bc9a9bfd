// gn_match_teams.h -- the scan-to-map Gauss-Newton matcher as CDNA4 (gfx950) HIP kernels: its design, and the team form
// (gn_match_kernel), launched by match_teams.hip only.
//
// What it computes (reference, HSL/ = hector_mapping/include/hector_slam_lib/):
//   per beam   OccGridMapUtil::interpMapValueWithDerivatives   HSL/map/OccGridMapUtil.h:287-347   beam_sample.h
//   per scan   OccGridMapUtil::getCompleteHessianDerivs        HSL/map/OccGridMapUtil.h:64-104    gn_step.h
//   per step   ScanMatcher::estimateTransformationLogLh        HSL/matcher/ScanMatcher.h:194-221  gn_step.h (gn_solve_and_step)
//   per level  ScanMatcher::matchData                          HSL/matcher/ScanMatcher.h:54-190   every kernel's level loop
//   per match  MapRepMultiMap::matchData                       HSL/slam_main/MapRepMultiMap.h:116-132
//
// How it is mapped onto the machine:
//   * one TEAM of WPS wavefronts (64 lanes each) owns one (pose hypothesis, scan) pair for the WHOLE coarse-to-fine schedule
//     (all levels, all GN steps) -- the 14-step dependent chain never leaves the CU, no host round trips;
//   * beams are dealt round-robin to lanes (beam i -> lane i mod 64*WPS), so the float2 endpoint loads of a wavefront are one
//     contiguous 512-byte segment and neighbouring lanes sample neighbouring map cells;
//   * the occupancy pyramid is sampled from a texture-like "quad" plane, ONE 16-byte gather per beam, or (HSM_LAYOUT_PLANE) from
//     the probability plane itself (beam_sample.h sample_fetch);
//   * the 6 unique H terms + 3 dTr terms are lane-local fp32 partial sums, reduced with ONE folded wavefront reduction and, when
//     WPS > 1, staged through LDS (gn_step.h wave_allreduce9, team_allreduce9); every lane ends up with bit-identical totals and
//     solves the 3x3 system redundantly: no broadcast, no divergence;
//   * batches of long scans run the texel-cache form (gn_match_cached.h; in the reference's summation order gn_match_exact.h);
//   * a single DENSE scan (>= 4096 beams): one workgroup whose first wavefront adds while fifteen produce, or with
//     HSM_PARITY_FAST up to 64 workgroups that exchange tagged partial sums (gn_match_dense.h).
//   No MFMA: this is a bilinear gather plus a 9-term reduction, not a contraction.
//   Measured limits (profiles/r02/README.md): VALU issue (61 instructions per beam) and
//   the texture path of the divergent 16-byte gathers -- not HBM.
//
// Numerics: built with -ffp-contract=off.  Every per-beam value (M, dM/dx, dM/dy,
// rotDeriv and the nine products) is the same IEEE fp32 expression, in the same
// order, as the reference.  In the DEFAULT mode (HSM_PARITY_AUTO, and HSM_PARITY_EXACT) the
// nine per-beam products are staged through LDS and summed by nine lanes in beam order,
// i = 0 .. n-1, exactly the reference's fp32 chains: identical bits on every entry point.
// The opt-in HSM_PARITY_FAST changes only the ORDER of the beam summation (strided partial
// sums + tree instead of one sequential chain).  sinf/cosf/expf are glibc's algorithms
// operation for operation (libm_exact.h): identical bits.
#pragma once
#include <hip/hip_runtime.h>

#include "beam_sample.h"
#include "gn_step.h"
#include "match_types.h"

namespace hsm {

// One team (WPS wavefronts) per scan; SPB scans per workgroup (SPB > 1 only when WPS == 1,
// where no barrier is ever executed so the wavefronts of a block are fully independent).
//
// BPL > 0: "beams per lane" register-resident form.  A scan with n <= 64*WPS*BPL beams is loaded
// ONCE (coalesced float2, beam i -> slot i / (64*WPS) of lane i mod 64*WPS) and stays in VGPRs for
// all levels and GN steps; the beam loop is fully unrolled so the BPL texel gathers of a step are
// independent and issue back to back (latency hiding by ILP, not only by occupancy).  The
// per-lane summation order (ascending beam index) is the same as the memory loop's, so both
// forms produce identical bits.  Longer scans (or BPL == 0) take the memory loop.
// Occupancy the kernel is BUILT for (and test_kernel_resources.py asserts): four waves per SIMD, except the exact-order teams
// of two and four wavefronts -- they keep a whole group of rounds alive at once (five endpoints, five texels, five rotated
// points per lane: ~150 VGPRs) and stage it in 23 / 46 KB of LDS, and they are latency launches (one team per scan, chosen only
// when the batch cannot fill the chip), so three waves per SIMD is what they get and what they ask for.
template <int WPS, int SPB, int LAYOUT, int BPL, bool EXACT = false>
__global__ void __launch_bounds__(64 * WPS * SPB, ((EXACT && SPB == 1 && (WPS == 2 || WPS == 4)) ? 3 : 4)) gn_match_kernel(const MatchParams P) {
  static_assert(WPS == 1 || SPB == 1, "barrier-synchronised teams own their workgroup");
  static_assert(!EXACT || BPL == 0, "the exact-order form streams the endpoints");
  constexpr int T = 64 * WPS;  // lanes per team
  __shared__ __attribute__((aligned(16))) float red[2][9][WPS < 4 ? 4 : WPS];
  // exact order: [team][term][beam]; single-scan teams of up to four wavefronts stage a whole GROUP of rounds (kXGroup x T beams,
  // 46 KB at four wavefronts) and sum it in one go, the others round by round
  constexpr int kXGroup = kExactGroupRounds;
  constexpr int kXStaged = (EXACT && SPB == 1 && T <= 256) ? kXGroup : 1;  // rounds staged together
  constexpr int kXRowLen = kXStaged * T;
  __shared__ float stage[EXACT ? SPB * 9 * (kXRowLen + kExactPad) : 1];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int team = wave / WPS;
  const int wit = wave - team * WPS;
  const int scan = __builtin_amdgcn_readfirstlane(xcd_block((int)blockIdx.x, (int)gridDim.x, P.xcd_chunk) * SPB + team);  // wave-uniform
  if (scan >= P.batch) return;  // whole team exits together
#ifdef HSM_TEAM_TIMELINE
  if (EXACT && P.clock_probe != nullptr && scan == 0 && threadIdx.x == 0) P.clock_probe[4] = wall_clock64();
#endif

  int beg = 0, n = P.shared_n;
  if (P.offsets) {
    beg = P.offsets[scan];
    n = P.offsets[scan + 1] - beg;
  }
  float pw0, pw1, pw2;
  if (P.begin_world) {
    pw0 = P.begin_world[3 * scan + 0];
    pw1 = P.begin_world[3 * scan + 1];
    pw2 = P.begin_world[3 * scan + 2];
  } else {  // single-scan host entry: the pose rides in the kernel arguments, no H2D copy
    pw0 = P.begin_inline[0];
    pw1 = P.begin_inline[1];
    pw2 = P.begin_inline[2];
  }
  if (n == 0) {  // ScanMatcher.h:68,189: pose passes through, cov untouched
    if (lane == 0 && wit == 0) {
      P.out_pose[3 * scan + 0] = pw0;
      P.out_pose[3 * scan + 1] = pw1;
      P.out_pose[3 * scan + 2] = pw2;
      if (scan == 0) publish_done(P);
    }
    return;
  }
  const float2* __restrict__ pts = P.pts + beg;
  const int tid_in_team = wit * 64 + lane;
  constexpr int NREG = BPL > 0 ? BPL : 1;
  f2 pt[NREG];
  const bool in_regs = BPL > 0 && n <= T * BPL;  // team-uniform
  if (in_regs) {
#pragma unroll
    for (int k = 0; k < NREG; ++k) {
      const int i = tid_in_team + k * T;
      // padding slots of the last partial row: an endpoint far outside ANY map.  |R(theta) p| =
      // |p| ~ 1.4e30 for every theta, so the transformed point is out of bounds on at least one
      // axis and takes the exact-zero path of sample_fetch; all intermediates stay finite and the
      // per-level power-of-two rescale keeps it huge.
      const float2 q = i < n ? pts[i] : make_float2(1.0e30f, 1.0e30f);
      pt[k] = f2{q.x, q.y};
    }
  }
  // exact order: a scan that is ONE group of rounds keeps its endpoints (unscaled) in registers across all levels and GN steps
  // -- one dependent memory round trip per step, the texel gather, instead of two
  const bool xq_resident = EXACT && n <= kXGroup * T;  // (team-uniform)
  float2 xq[EXACT ? kXGroup : 1];
  if (xq_resident) {
#pragma unroll
    for (int g = 0; g < (EXACT ? kXGroup : 1); ++g) {
      const int i = g * T + tid_in_team;
      xq[g] = i < n ? pts[i] : make_float2(1.0e30f, 1.0e30f);
    }
  }
  Acc9 acc;
  acc.zero();
  int buf = 0;
  int step = 0;
  float reg_scale = 1.0f;  // scale the register-resident endpoints currently carry
  for (int l = P.first_level; l >= P.last_level; --l) {
    const LevelView& L = P.lv[l];
    float ex, ey, eth;
    affine_apply(L.mapTworld, pw0, pw1, ex, ey);  // getMapCoordsPose, GridMapBase.h:235-239
    eth = pw2;
    const float ps = L.pt_scale;
    const int gn_steps = L.gn_steps;
    const LevelRegs R = level_regs<LAYOUT>(L);
    if (in_regs) {
      // DataContainer::setFrom(scan, 2^-level): rescale IN PLACE when the level changes.  All
      // factors are powers of two, so p*2^-a*2^(a-b) == p*2^-b bit for bit, and no second
      // register copy of the scan is kept alive across the GN steps.
      const float ratio = ps / reg_scale;
      reg_scale = ps;
#pragma unroll
      for (int k = 0; k < NREG; ++k) pt[k] *= f2{ratio, ratio};
    }
    for (int it = 0; it < gn_steps; ++it) {
#ifdef HSM_TEAM_TIMELINE  // (variant builds, tools/study/team_phase_probe.py: cycles of a GN step's phases, summed over the steps)
      const unsigned long long tt0 = __builtin_readcyclecounter();
      unsigned long long tt1 = tt0, tt2 = tt0;
#endif
      float sinRot, cosRot;
      sincos_f32(eth, sinRot, cosRot);
      acc.zero();
      const f2 e2 = step_origin(ex, ey), cs = f2{cosRot, sinRot}, sc = f2{sinRot, cosRot};
      if (in_regs) {
        // chunks of kChunk beams: issue all gathers of a chunk, then consume them in beam order
        // (the accumulation order stays k = 0, 1, 2 ... so the bits equal the memory loop's)
        // Throughput launches (one wave per scan, 4 waves per SIMD): one beam at a time is fastest -- the four waves
        // per SIMD already interleave, extra texels in flight only cost registers (372 M it/s; a one-deep software
        // pipeline 358; chunks of 2 / 4 / 6 / 9: 359 / 342 / 340 / 309, profiles/r01/README.md).
        // Latency launches (WPS > 1 is only chosen when the batch cannot fill the chip, typically one wave
        // per SIMD): nobody else hides the L2 latency, so the lane's gathers are issued in chunks before the
        // first is consumed -- all of them up to 5 beams per lane (single 1081-beam scan: kernel 31.5 -> 25 us),
        // else 4 at a time (16k-beam scan on 16 waves: 170 / 155 / 173 us for chunks of 1 / 4 / 9).
        constexpr int kChunk = WPS > 1 ? (NREG <= 5 ? NREG : 4) : 1;
#pragma unroll
        for (int k0 = 0; k0 < NREG; k0 += kChunk) {
          BeamSample smp[kChunk];
          BeamRot rot[kChunk];
#pragma unroll
          for (int u = 0; u < kChunk; ++u) {
            if (k0 + u < NREG)
              smp[u] = beam_fetch<LAYOUT>(R, e2, cs, sc, pt[k0 + u], rot[u]);
          }
#pragma unroll
          for (int u = 0; u < kChunk; ++u) {
            if (k0 + u < NREG) beam_finish(smp[u], rot[u], acc);
          }
          // Pin the chunk: the accumulators must be final here ("+v") and no later gather may be
          // hoisted above this point ("memory").  Without it the compiler issues all BPL gathers
          // first and spills their results; with it at most kChunk texels are in flight per lane.
          asm volatile(""
                       : "+v"(acc.d01), "+v"(acc.d2), "+v"(acc.hd), "+v"(acc.h22), "+v"(acc.h01), "+v"(acc.hr)
                       :
                       : "memory");
        }
      } else if (EXACT) {
        float run = 0.0f;
        float* st = stage + team * 9 * (kXRowLen + kExactPad);
        // Rounds in groups of kXGroup: the endpoints of the whole group are requested together, then its texels, then the
        // rounds are summed one after the other -- two memory round trips per group instead of two per round (a 1081-beam
        // scan on four wavefronts is ONE group per GN step; the dependent loads were ~40 % of the exact single-scan match).
        for (int base0 = 0; base0 < n; base0 += kXGroup * T) {  // team-uniform trip count
          float2 q[kXGroup];
#pragma unroll
          for (int g = 0; g < kXGroup; ++g) {
            if (xq_resident) {  // a scan of one group: its endpoints were loaded once, before the first level
              q[g] = xq[g];
            } else {
              const int i = base0 + g * T + tid_in_team;
              q[g] = i < n ? pts[i] : make_float2(1.0e30f, 1.0e30f);  // padding: exact +-0 products (see above)
            }
          }
          BeamSample b[kXGroup];
          BeamRot r[kXGroup];
#pragma unroll
          for (int g = 0; g < kXGroup; ++g) b[g] = beam_fetch<LAYOUT>(R, e2, cs, sc, f2{q[g].x * ps, q[g].y * ps}, r[g]);
          if (kXStaged == kXGroup) {
            // the whole group behind ONE barrier pair, the chain runs through it without a stop (rounds beyond the scan
            // stage +-0 and are not summed)
#pragma unroll
            for (int g = 0; g < kXGroup; ++g) {
              float pr[9];
              beam_products(b[g], r[g], pr);
              exact_stage<kXRowLen>(pr, st, g * T + tid_in_team);
            }
#ifdef HSM_TEAM_TIMELINE
            tt1 = __builtin_readcyclecounter();
#endif
            run = exact_chain<kXRowLen, (T > 64)>(st, tid_in_team, run, min(kXRowLen, n - base0));
#ifdef HSM_TEAM_TIMELINE
            tt2 = __builtin_readcyclecounter();
#endif
          } else {
#pragma unroll
            for (int g = 0; g < kXGroup; ++g) {
              const int base = base0 + g * T;
              if (base < n) {  // team-uniform
                float pr[9];
                beam_products(b[g], r[g], pr);
                run = exact_round<T>(pr, st, tid_in_team, run, min(T, n - base));
              }
            }
          }
        }
        float t[9];
        if (WPS == 1) {
#pragma unroll
          for (int k = 0; k < 9; ++k) t[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(run), k));
        } else {
          // threads 0..8 publish; the next write of red[] lies behind the >= 2 barriers of the next step's rounds
          if (tid_in_team < 9) (&red[0][0][0])[tid_in_team] = run;
          __syncthreads();
#pragma unroll
          for (int k = 0; k < 9; ++k) t[k] = (&red[0][0][0])[k];
        }
        acc.d01 = f2{t[0], t[1]}; acc.d2 = t[2];
        acc.hd = f2{t[3], t[4]}; acc.h22 = t[5];
        acc.h01 = t[6]; acc.hr = f2{t[7], t[8]};
      } else {
        for (int i = tid_in_team; i < n; i += T) {
          const float2 p = pts[i];
          BeamRot r;
          const BeamSample b = beam_fetch<LAYOUT>(R, e2, cs, sc, f2{p.x * ps, p.y * ps}, r);
          beam_finish(b, r, acc);
        }
      }
      if (!EXACT) {
        team_allreduce9<WPS>(acc, red, buf, wit, lane);
        buf ^= 1;
      }
      gn_solve_and_step(acc, ex, ey, eth);
#ifdef HSM_TEAM_TIMELINE
      if (EXACT && P.clock_probe != nullptr && scan == 0 && tid_in_team == 0) {
        const unsigned long long tt3 = __builtin_readcyclecounter();
        const bool first = l == P.first_level && it == 0;
        if (first) P.clock_probe[8] = P.clock_probe[9] = P.clock_probe[10] = P.clock_probe[11] = 0, P.clock_probe[12] = tt0, P.clock_probe[13] = wall_clock64();
        const int sno = (int)P.clock_probe[11];
        P.clock_probe[8] += tt1 - tt0, P.clock_probe[9] += tt2 - tt1, P.clock_probe[10] += tt3 - tt2, P.clock_probe[11] += 1;
        if (sno < 16) P.clock_probe[16 + sno] = tt1 - tt0, P.clock_probe[32 + sno] = tt2 - tt1, P.clock_probe[48 + sno] = tt3 - tt2;
        P.clock_probe[14] = tt3, P.clock_probe[15] = wall_clock64();
      }
#endif
      if (P.trace) {  // kernel-uniform; only the single-scan hook path sets it
        if (scan == 0 && lane == 0 && wit == 0) {
          float* t = P.trace + 12 * step;
          t[0] = ex; t[1] = ey; t[2] = eth;
          t[3] = acc.hd.x; t[4] = acc.h01; t[5] = acc.hr.x;
          t[6] = acc.h01; t[7] = acc.hd.y; t[8] = acc.hr.y;
          t[9] = acc.hr.x; t[10] = acc.hr.y; t[11] = acc.h22;
        }
        ++step;
      }
    }
    eth = normalize_angle(eth);                     // ScanMatcher.h:170
    affine_apply(L.worldTmap, ex, ey, pw0, pw1);    // getWorldCoordsPose, :186
    pw2 = eth;
  }
  if (lane == 0 && wit == 0) {
    P.out_pose[3 * scan + 0] = pw0;
    P.out_pose[3 * scan + 1] = pw1;
    P.out_pose[3 * scan + 2] = pw2;
    if (P.out_cov) {  // covMatrix = H of the last evaluation (ScanMatcher.h:184), column major
      float* c = P.out_cov + 9 * scan;
      c[0] = acc.hd.x; c[1] = acc.h01; c[2] = acc.hr.x;
      c[3] = acc.h01; c[4] = acc.hd.y; c[5] = acc.hr.y;
      c[6] = acc.hr.x; c[7] = acc.hr.y; c[8] = acc.h22;
    }
#ifdef HSM_TEAM_TIMELINE
    if (EXACT && P.clock_probe != nullptr && scan == 0) P.clock_probe[5] = wall_clock64();
#endif
    if (scan == 0) publish_done(P);
  }
}

}  // namespace hsm
