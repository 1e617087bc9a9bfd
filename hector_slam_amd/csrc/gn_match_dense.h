// gn_match_dense.h -- the two forms of the matcher for ONE dense scan, launched by match.hip only: the producers-ahead
// form in the reference's summation order (gn_match_exact_dense_kernel) and the multi-workgroup form of HSM_PARITY_FAST
// (gn_match_coop_kernel).  The design of the matcher as a whole: gn_match_teams.h.
#pragma once
#include <hip/hip_runtime.h>

#include "beam_sample.h"
#include "gn_step.h"
#include "match_types.h"

namespace hsm {

// ---- one DENSE scan in the reference's summation order: producers ahead of the chain (round 5) ---------------------------------
// The exact-order team form (gn_match_teams.h) runs a 16 k-beam scan as rounds of 1024 beams on 16 wavefronts: all of them compute a round's
// products, then fifteen and a half of them wait while nine lanes add 1024 x 9 values (8.5 cycles per dependent v_add_f32: 3.6 us),
// then everybody gathers the next round's texels (~1-2 us with nothing else to do) -- 90 us per Gauss-Newton step on configs[4],
// of which the nine chains themselves are 16 384 x 8.5 cycles = 58 us.  This form takes the chain out of the team: wavefront 0
// only adds, wavefronts 1..15 only produce, one round AHEAD of it (two stage buffers, one workgroup barrier per round), so a
// round costs max(chain, production) = the chain.  Same products, same order of the additions: identical bits.  What is left
// per step is the floor of the literal chain -- n x 8.5 cycles -- plus one round of production before the first addition.
// (The block-scan form that would have removed the dependent chain itself is a measured negative: tools/study/exact_scan.h,
// profiles/r05/README.md.)
constexpr int kDenseProducers = 15;                  // wavefronts
constexpr int kDenseRound = 64 * kDenseProducers;    // beams per round: one per producer lane

template <int LAYOUT>
__global__ void __launch_bounds__(1024) gn_match_exact_dense_kernel(const MatchParams P) {
  constexpr int RL = kDenseRound;  // staged row length (a multiple of 16: exact_chain reads whole float4 groups)
  __shared__ __attribute__((aligned(16))) float stage[2][9 * (RL + kExactPad)];
  __shared__ float totals[9];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const bool chain_wave = wave == 0;
  const int ptid = (int)threadIdx.x - 64;  // producer lane 0 .. RL-1 (negative in the chain wavefront)
  const int scan = (int)blockIdx.x;
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
  } else {
    pw0 = P.begin_inline[0];
    pw1 = P.begin_inline[1];
    pw2 = P.begin_inline[2];
  }
  if (n == 0) {  // ScanMatcher.h:68,189
    if (threadIdx.x == 0) {
      P.out_pose[3 * scan + 0] = pw0;
      P.out_pose[3 * scan + 1] = pw1;
      P.out_pose[3 * scan + 2] = pw2;
      if (scan == 0) publish_done(P);
    }
    return;
  }
  const float2* __restrict__ pts = P.pts + beg;
  const int rounds = (n + RL - 1) / RL;
  // the chain is the critical path of every round: its wavefront issues ahead of the three producers that share its SIMD
  if (chain_wave) __builtin_amdgcn_s_setprio(3);
  auto endpoint_load = [&](int r) -> float2 {  // padding: an endpoint outside any map -> exact +-0 products (gn_match_kernel)
    const int i = r * RL + ptid;
    return (ptid >= 0 && i < n) ? pts[i] : make_float2(1.0e30f, 1.0e30f);
  };
  // a scan of one or two rounds (the node's 1081 beams) keeps its endpoints in registers across all levels and GN steps: one
  // dependent memory round trip per step -- the texel gather -- before the chain can start, instead of two
  const bool resident = rounds <= 2;  // (workgroup-uniform)
  float xq0x = 1.0e30f, xq0y = 1.0e30f, xq1x = 1.0e30f, xq1y = 1.0e30f;  // (scalars: a float2 selected through a lambda went to scratch)
  if (resident) {
    const float2 a = endpoint_load(0);
    xq0x = a.x, xq0y = a.y;
    if (rounds > 1) {
      const float2 b = endpoint_load(1);
      xq1x = b.x, xq1y = b.y;
    }
  }
  auto endpoint_of = [&](int r) -> float2 {
    if (!resident) return endpoint_load(r);
    return make_float2(r == 0 ? xq0x : xq1x, r == 0 ? xq0y : xq1y);
  };
  Acc9 acc;
  acc.zero();
  int step = 0;
  for (int l = P.first_level; l >= P.last_level; --l) {
    const LevelView& L = P.lv[l];
    float ex, ey, eth;
    affine_apply(L.mapTworld, pw0, pw1, ex, ey);
    eth = pw2;
    const float ps = L.pt_scale;
    const int gn_steps = L.gn_steps;
    const LevelRegs R = level_regs<LAYOUT>(L);
    for (int it = 0; it < gn_steps; ++it) {
      float sinRot, cosRot;
      sincos_f32(eth, sinRot, cosRot);
      const f2 e2 = step_origin(ex, ey), cs = f2{cosRot, sinRot}, sc = f2{sinRot, cosRot};
      // producers: the products of round r into stage[r & 1]; the endpoint of the round after it is requested meanwhile
      float2 q_next = endpoint_of(0);
      auto produce = [&](int r) {
        const float2 q = q_next;
        if (r + 1 < rounds) q_next = endpoint_of(r + 1);
        BeamRot rot;
        const BeamSample b = beam_fetch<LAYOUT>(R, e2, cs, sc, f2{q.x * ps, q.y * ps}, rot);
        float pr[9];
        beam_products(b, rot, pr);
        exact_stage<RL>(pr, stage[r & 1], ptid);
      };
      if (!chain_wave) produce(0);
      float run = 0.0f;
      for (int r = 0; r < rounds; ++r) {  // workgroup-uniform trip count
        __syncthreads();  // round r is staged; the chain has left the other buffer
        if (chain_wave) {
          run = exact_chain<RL, false>(stage[r & 1], lane, run, min(RL, n - r * RL));
        } else if (r + 1 < rounds) {
          produce(r + 1);
        }
      }
      if (chain_wave && lane < 9) totals[lane] = run;
      __syncthreads();
      acc.d01 = f2{totals[0], totals[1]}; acc.d2 = totals[2];
      acc.hd = f2{totals[3], totals[4]}; acc.h22 = totals[5];
      acc.h01 = totals[6]; acc.hr = f2{totals[7], totals[8]};
      gn_solve_and_step(acc, ex, ey, eth);
      if (P.trace) {  // kernel-uniform; only the single-scan hook path sets it
        if (scan == 0 && threadIdx.x == 0) {
          float* t = P.trace + 12 * step;
          t[0] = ex; t[1] = ey; t[2] = eth;
          t[3] = acc.hd.x; t[4] = acc.h01; t[5] = acc.hr.x;
          t[6] = acc.h01; t[7] = acc.hd.y; t[8] = acc.hr.y;
          t[9] = acc.hr.x; t[10] = acc.hr.y; t[11] = acc.h22;
        }
        ++step;
      }
      // (the next step's first write of totals[] lies behind its rounds' barriers; stage[0] is rewritten by produce(0) of the
      // next step only after every wavefront has passed the barrier above, and the chain read it last in an earlier round)
    }
    eth = normalize_angle(eth);
    affine_apply(L.worldTmap, ex, ey, pw0, pw1);
    pw2 = eth;
  }
  if (threadIdx.x == 0) {
    P.out_pose[3 * scan + 0] = pw0;
    P.out_pose[3 * scan + 1] = pw1;
    P.out_pose[3 * scan + 2] = pw2;
    if (P.out_cov) {  // covMatrix = H of the last evaluation (ScanMatcher.h:184), column major
      float* c = P.out_cov + 9 * scan;
      c[0] = acc.hd.x; c[1] = acc.h01; c[2] = acc.hr.x;
      c[3] = acc.h01; c[4] = acc.hd.y; c[5] = acc.hr.y;
      c[6] = acc.hr.x; c[7] = acc.hr.y; c[8] = acc.h22;
    }
    if (scan == 0) publish_done(P);
  }
}

// ---- one DENSE scan on many CUs --------------------------------------------------------------------
// gn_match_kernel keeps a scan inside one workgroup (<= 16 waves on ONE CU): right for batches, but a
// single 16k-beam scan then uses 1/256 of the chip (11 us per GN step).  This variant spreads the beams of
// ONE scan over K <= 64 workgroups of 256 lanes and keeps the 14-step chain inside one cooperative launch:
// per GN step every workgroup reduces its beams to 9 partials, publishes them, the grid synchronises
// (cooperative groups: all K workgroups are co-resident by construction, the runtime refuses the launch
// otherwise), and every workgroup sums the K partials in the same fixed order -- wave 0, lane l takes
// workgroup l, then the DPP/permlane tree -- so all of them take the identical GN step.  Partials are double
// buffered by step parity: one grid sync per step.
// Grid barrier of the cooperative matcher: one monotonically increasing device-memory counter (the host passes
// its value at launch, so it is never reset), one agent-scope release increment per workgroup and an acquire
// spin by thread 0 -- 2-3 us per GN step cheaper than cooperative_groups' grid.sync().  All K workgroups are co-resident:
// the launch is still a cooperative launch.
// TAGGED (default since round 3; env HSM_COOP_TAGGED=0 selects the counter barrier at run time): no grid barrier at all --
// tagged 16-byte records, see the kernel.  That exchange relies on a 16-byte sc0 sc1 store being observed untorn, which is
// documented behaviour of gfx942 / gfx950 only:
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__) && !defined(__gfx942__)
#error "gn_match_coop_kernel's tagged exchange is written for gfx942 / gfx950"
#endif
__device__ __forceinline__ void coop_barrier(unsigned* counter, unsigned target) {
  __syncthreads();  // the workgroup's partials are written
  if (threadIdx.x == 0) {
    __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    // relaxed polls (each acquire load would invalidate the caches), ONE acquire fence once everybody arrived
    while ((int)(__hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - target) < 0)
      __builtin_amdgcn_s_sleep(1);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  }
  __syncthreads();
}

template <int LAYOUT, bool TAGGED = true>
__global__ void __launch_bounds__(256) gn_match_coop_kernel(const MatchParams P, float* __restrict__ partials,
                                                            unsigned* __restrict__ bar_counter, unsigned bar_base) {
  __shared__ float red[4][9];
  __shared__ float tot[9];
  __shared__ int gave_up;  // the exchange timed out in this workgroup: leave (ordered by the barriers of the step)
  if (threadIdx.x == 0) gave_up = 0;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int K = (int)gridDim.x;
  const int n = P.shared_n;
  const float2* __restrict__ pts = P.pts;
  float pw0 = P.begin_inline[0], pw1 = P.begin_inline[1], pw2 = P.begin_inline[2];
  const int g0 = blockIdx.x * 256 + threadIdx.x, stride = K * 256;
  Acc9 acc;
  acc.zero();
  int step = 0;
  for (int l = P.first_level; l >= P.last_level; --l) {
    const LevelView& L = P.lv[l];
    float ex, ey, eth;
    affine_apply(L.mapTworld, pw0, pw1, ex, ey);
    eth = pw2;
    const float ps = L.pt_scale;
    const int gn_steps = L.gn_steps;
    const LevelRegs R = level_regs<LAYOUT>(L);
    for (int it = 0; it < gn_steps; ++it, ++step) {
      float sinRot, cosRot;
      sincos_f32(eth, sinRot, cosRot);
      acc.zero();
      const f2 e2 = step_origin(ex, ey), cs = f2{cosRot, sinRot}, sc = f2{sinRot, cosRot};
      for (int i = g0; i < n; i += stride) {
        const float2 p = pts[i];
        BeamRot r;
        const BeamSample b = beam_fetch<LAYOUT>(R, e2, cs, sc, f2{p.x * ps, p.y * ps}, r);
        beam_finish(b, r, acc);
      }
      // workgroup partial: wave all-reduce, 4 waves through LDS (fixed order)
      wave_allreduce9(acc);
      if (lane == 0) {
        float* r = red[wave];
        r[0] = acc.d01.x; r[1] = acc.d01.y; r[2] = acc.d2;
        r[3] = acc.hd.x; r[4] = acc.hd.y; r[5] = acc.h22;
        r[6] = acc.h01; r[7] = acc.hr.x; r[8] = acc.hr.y;
      }
      __syncthreads();
      if constexpr (TAGGED) {
      // Exchange WITHOUT a barrier: every workgroup publishes its nine partials as three self-describing 16-byte granules
      // {p, p, p, tag} (tag = the step's global sequence number) with device-coherent stores, and every workgroup polls the K
      // records of the step until all their granules carry the tag.  A 16-byte sc0 sc1 store is observed untorn, sc1 loads are
      // served by memory-side coherent L2 -- no release write-back, no acquire invalidate (1.7 us each on this machine), no
      // counter round trip.  Two record buffers by step parity: a workgroup overwrites buffer s & 1 for step s + 2 only after
      // it has read every workgroup's step-(s + 1) record, which that workgroup published after it finished reading step s.
      const unsigned tag = bar_base + (unsigned)step + 1u;
      f4v* const recs = reinterpret_cast<f4v*>(partials) + (size_t)(step & 1) * 64 * 3;
      if (threadIdx.x < 3 && P.coop_mute_block != (int)blockIdx.x + 1) {
        const int t0 = 3 * (int)threadIdx.x;
        f4v g;
        g.x = ((red[0][t0] + red[1][t0]) + red[2][t0]) + red[3][t0];
        g.y = ((red[0][t0 + 1] + red[1][t0 + 1]) + red[2][t0 + 1]) + red[3][t0 + 1];
        g.z = ((red[0][t0 + 2] + red[1][t0 + 2]) + red[2][t0 + 2]) + red[3][t0 + 2];
        g.w = __uint_as_float(tag);
        f4v* dst = recs + 3 * blockIdx.x + threadIdx.x;
        asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" : : "v"(dst), "v"(g) : "memory");
      }
      if (wave == 0) {
        Acc9 t;
        t.zero();
        const f4v* src = recs + 3 * (lane < K ? lane : 0);
        f4v g0, g1, g2;
        for (int spin = 0;; ++spin) {
          asm volatile("global_load_dwordx4 %0, %3, off sc0 sc1\n\t"
                       "global_load_dwordx4 %1, %3, off offset:16 sc0 sc1\n\t"
                       "global_load_dwordx4 %2, %3, off offset:32 sc0 sc1\n\t"
                       "s_waitcnt vmcnt(0)"
                       : "=&v"(g0), "=&v"(g1), "=&v"(g2) : "v"(src) : "memory");
          const bool ok = lane >= K || (__float_as_uint(g0.w) == tag && __float_as_uint(g1.w) == tag && __float_as_uint(g2.w) == tag);
          if (__ballot(!ok) == 0ull) break;
          if (spin > (1 << 22)) {
            // bounded: a lost workgroup must not hang the device.  The records are then stale or partial, and so is every
            // step from here on: say so where the host looks (match_single turns it into an error return) -- ordered
            // before this workgroup's next record, so that whoever consumes the wrong sums also finds the word
            if (lane == 0 && P.err_flag) {
              __hip_atomic_store(P.err_flag, P.done_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
              __threadfence_system();
            }
            // ... and leave: every other workgroup times out on this one's missing records in turn, so the launch ends after
            // ONE bounded wait instead of one per remaining GN step (the host re-runs the scan on the one-workgroup matcher)
            if (lane == 0) gave_up = 1;
            break;
          }
          __builtin_amdgcn_s_sleep(1);
        }
        if (lane < K) {
          t.d01 = f2{g0.x, g0.y}; t.d2 = g0.z;
          t.hd = f2{g1.x, g1.y}; t.h22 = g1.z;
          t.h01 = g2.x; t.hr = f2{g2.y, g2.z};
        }
        wave_allreduce9(t);
        if (lane == 0) {
          tot[0] = t.d01.x; tot[1] = t.d01.y; tot[2] = t.d2;
          tot[3] = t.hd.x; tot[4] = t.hd.y; tot[5] = t.h22;
          tot[6] = t.h01; tot[7] = t.hr.x; tot[8] = t.hr.y;
        }
      }
      } else {
      float* mine = partials + ((size_t)(step & 1) * K + blockIdx.x) * 9;
      if (threadIdx.x < 9) mine[threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
      coop_barrier(bar_counter, bar_base + (unsigned)K * (unsigned)(step + 1));
      // every workgroup: the same K partials in the same order
      if (wave == 0) {
        const float* src = partials + ((size_t)(step & 1) * K + lane) * 9;
        Acc9 t;
        t.zero();
        if (lane < K) {
          t.d01 = f2{src[0], src[1]}; t.d2 = src[2];
          t.hd = f2{src[3], src[4]}; t.h22 = src[5];
          t.h01 = src[6]; t.hr = f2{src[7], src[8]};
        }
        wave_allreduce9(t);
        if (lane == 0) {
          tot[0] = t.d01.x; tot[1] = t.d01.y; tot[2] = t.d2;
          tot[3] = t.hd.x; tot[4] = t.hd.y; tot[5] = t.h22;
          tot[6] = t.h01; tot[7] = t.hr.x; tot[8] = t.hr.y;
        }
      }
      }
      __syncthreads();
      if (TAGGED && gave_up) return;  // (workgroup-uniform)
      acc.d01 = f2{tot[0], tot[1]}; acc.d2 = tot[2];
      acc.hd = f2{tot[3], tot[4]}; acc.h22 = tot[5];
      acc.h01 = tot[6]; acc.hr = f2{tot[7], tot[8]};
      gn_solve_and_step(acc, ex, ey, eth);
      if (P.trace && blockIdx.x == 0 && threadIdx.x == 0) {
        float* t = P.trace + 12 * step;
        t[0] = ex; t[1] = ey; t[2] = eth;
        t[3] = acc.hd.x; t[4] = acc.h01; t[5] = acc.hr.x;
        t[6] = acc.h01; t[7] = acc.hd.y; t[8] = acc.hr.y;
        t[9] = acc.hr.x; t[10] = acc.hr.y; t[11] = acc.h22;
      }
      __syncthreads();  // tot[] / red[] are rewritten in the next step
    }
    eth = normalize_angle(eth);
    affine_apply(L.worldTmap, ex, ey, pw0, pw1);
    pw2 = eth;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    P.out_pose[0] = pw0;
    P.out_pose[1] = pw1;
    P.out_pose[2] = pw2;
    if (P.out_cov) {
      float* c = P.out_cov;
      c[0] = acc.hd.x; c[1] = acc.h01; c[2] = acc.hr.x;
      c[3] = acc.h01; c[4] = acc.hd.y; c[5] = acc.hr.y;
      c[6] = acc.hr.x; c[7] = acc.hr.y; c[8] = acc.h22;
    }
    publish_done(P);
  }
}

}  // namespace hsm
