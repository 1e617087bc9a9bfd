// gn_match_cached.h -- the fast texel-cache form of the matcher (gn_match_cached_kernel), launched by match_teams.hip only.  The
// design of the matcher as a whole: gn_match_teams.h.
#pragma once
#include <type_traits>
#include <hip/hip_runtime.h>

#include "beam_sample.h"
#include "gn_step.h"
#include "match_types.h"
#include "texel_cache.h"

namespace hsm {

// The SIMD's issue arbiter favours its oldest wavefront.  In a throughput launch -- one wavefront per scan, four per
// SIMD, all started within 2 us -- the four therefore finish one after another (time stamps of a headline launch:
// ~33 / 42 / 50 / 52 us) and the last ones run with too few neighbours to cover their gathers.  Rotating the priority
// from GN step to GN step (slot id of the wave + step counter, two SALU instructions) keeps them in step: headline
// 57.1 -> 55.4 us, 3-level pyramid 118.7 -> 110 us, 4096^2 pyramid 150 -> 142 us (profiles/r02/README.md).  Used by the
// texel-cache form only: the form that gathers every beam in every step loses 4 % with it (67 -> 69.5 us).
__device__ __forceinline__ void rotate_wave_priority(int step) {
  unsigned hwid;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));  // bits 3:0 = wave slot on its SIMD
  switch (((hwid & 0xFu) + (unsigned)step) & 3u) {
    case 0: __builtin_amdgcn_s_setprio(0); break;
    case 1: __builtin_amdgcn_s_setprio(1); break;
    case 2: __builtin_amdgcn_s_setprio(2); break;
    default: __builtin_amdgcn_s_setprio(3); break;
  }
}

// ---- throughput form with a per-beam texel cache --------------------------------------------------
// From the third GN step on the estimate moves by a fraction of a cell, so most beams fall into the SAME
// map cell as in the step before (bench workload: 77 / 46 / 14 / 2 / 0.2 % of the lanes change cell in steps
// 2..6) and would gather the texel they already hold.  The gather, not the arithmetic, is what the texture
// path charges for -- one lane-request per cycle, whatever the pattern (profiles/r01/README.md) -- so this
// form keeps every beam's last texel and its byte offset in VGPRs (5 registers per beam) and gathers only in
// the lanes whose offset changed (exec-masked load; skipped by the whole wave when no lane changed).  To stay
// at 4 waves per SIMD (<= 128 VGPRs) the endpoints move from VGPRs to LDS: slot [wave][k][lane], written and
// read by the same lane only, so no barrier is ever needed (SPB * BPL * 512 B per workgroup).  Same
// arithmetic on the same texel values in the same order as gn_match_kernel: identical bits.
// One wave per scan, no trace.  The gathers run ONE beam ahead of their use (measured, profiles/r02/README.md: one
// ahead 57.1 us on the headline workload, two ahead 58.3 at 128 VGPRs, chunks of 3 without a pipeline 58.4).
// What the kernel does on top of that, each measured against the form without it in profiles/r02/README.md: counted waits
// for the masked texel gathers (see locate()), the endpoint of beam k+2 read from LDS while beam k is consumed, the zero
// texel's offset pinned in a VGPR, the first GN step taking the endpoints from their load registers.

// WPS: one wavefront per scan is the only form (the parameter stays for the kernels' names; two wavefronts per scan were
// measured in profiles/r02/README.md).
//
// RELAXED (HSM_PARITY_RELAXED, opt-in): the same expressions with their multiply-add pairs CONTRACTED -- the rotation, the
// bilinear blend written as two lerps on the differences the gradient needs anyway, the blends of the differences, rotDeriv
// and the nine accumulations become v_fma_f32: 32 instead of 51 fp32 operations per beam (42 instead of 61 VALU
// instructions).  Per-beam values then differ from the reference's in the last bit or two (one rounding instead of two
// per pair); the mode's bar is north_star's tolerance (1e-4 m / 1e-4 rad on the pose), measured at full size against the
// reference (tests/test_gpu_full_size.py, bench.py), not bit-exactness of the terms.
template <int SPB, int BPL, int LAYOUT = kLayoutQuad, int WPS = 1, bool RELAXED = false>
__global__ void __launch_bounds__(64 * SPB, 4) gn_match_cached_kernel(const MatchParams P) {
  static_assert(WPS == 1, "one wavefront per scan");
  static_assert(!RELAXED || LAYOUT == kLayoutQuad, "the tolerance mode exists for the throughput form only");
  constexpr int T = 64;  // lanes per scan
  __shared__ f2 lds_pts[SPB][BPL][64];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  // wave-uniform: kept in an SGPR (and with it the pose / covariance addresses, which live across the whole kernel)
  const int slot = __builtin_amdgcn_readfirstlane(xcd_block((int)blockIdx.x, (int)gridDim.x, P.xcd_chunk) * SPB + wave);
  if (slot >= P.batch) return;
  // (MatchParams::perm: the batch in Morton order of its start poses -- neighbours in the launch are neighbours in the map)
  const int scan = P.perm != nullptr ? __builtin_amdgcn_readfirstlane(P.perm[slot]) : slot;

  int beg = 0, n = P.shared_n;
  if (P.offsets) {
    beg = P.offsets[scan];
    n = P.offsets[scan + 1] - beg;
  }
  float pw0 = P.begin_world[3 * scan + 0], pw1 = P.begin_world[3 * scan + 1], pw2 = P.begin_world[3 * scan + 2];
  if (n == 0) {
    if (lane == 0) {
      P.out_pose[3 * scan + 0] = pw0;
      P.out_pose[3 * scan + 1] = pw1;
      P.out_pose[3 * scan + 2] = pw2;
    }
    return;
  }
  const float2* __restrict__ pts = P.pts + beg;
  f2(*mine)[64] = lds_pts[wave];
  // Endpoint staging.  Every wave of a launch starts at the same time and needs its 8.6 KB of endpoints first: 35 MB for
  // 4096 scans, 6.5 us during which no wave has anything to compute if all endpoints are staged before the first GN
  // step (measured with per-wave time stamps, profiles/r02/README.md).  So the FIRST GN step of the first level
  // is peeled (kPeel): its beam k takes its endpoint straight from the register of a load issued kEpAhead beams
  // earlier and writes it to LDS for the later steps, so the arithmetic and the texel gathers of step one run while
  // the endpoints are still streaming in.  All loads of that step -- endpoints and (unmasked: every lane gathers in a
  // level's first step) texels -- are inline asm with counted waits: loads return in order, and peel_schedule() gives
  // the position of every load in the wave's issue order, hence how many younger loads may still be in flight when a
  // given one is needed.  Out-of-range lanes read the scan's last endpoint (exec stays full, so every load is issued
  // and the counts are static) and are replaced by the padding value.
  constexpr bool kPeel = LAYOUT == kLayoutQuad;
  constexpr int kEpAhead = HSM_EP_AHEAD < BPL ? HSM_EP_AHEAD : BPL - 1;
  static_assert(BPL <= 31, "PeelSchedule holds 32 positions per load kind");
  constexpr PeelSchedule kSched = peel_schedule(BPL, kEpAhead);
  static_assert(kSched.total <= 2 * BPL, "one endpoint load and one gather per beam");
  const bool peel = kPeel && P.lv[P.first_level].gn_steps > 0;  // wave-uniform
  if (!peel) {
#pragma unroll
    for (int k = 0; k < BPL; ++k) {
      const int i = lane + k * T;
      const float2 q = i < n ? pts[i] : make_float2(1.0e30f, 1.0e30f);  // padding: see gn_match_kernel
      mine[k][lane] = f2{q.x, q.y};
    }
  }
  f4v tq[BPL];
  unsigned toff[BPL];
  Acc9 acc;
  acc.zero();
  float reg_scale = 1.0f;
  for (int l = P.first_level; l >= P.last_level; --l) {
    const LevelView& L = P.lv[l];
    float ex, ey, eth;
    affine_apply(L.mapTworld, pw0, pw1, ex, ey);
    eth = pw2;
    const float ps = L.pt_scale;
    const int gn_steps = L.gn_steps;
    const LevelRegs R = level_regs<LAYOUT>(L);
    const float ratio = ps / reg_scale;  // powers of two: exact (see gn_match_kernel)
    reg_scale = ps;
    const bool peel_here = peel && l == P.first_level;  // the peeled step stages the endpoints, scaled for this level
#pragma unroll
    for (int k = 0; k < BPL; ++k) {
      if (!peel_here && ratio != 1.0f) mine[k][lane] *= f2{ratio, ratio};
      toff[k] = 0xffffffffu;  // never a texel offset (not a multiple of 16): every beam gathers in the first step
    }
    // byte offset of the all-zero texel, pinned in a VGPR (as an SGPR it costs a v_mov per beam in front of the select)
    unsigned zero_off = (unsigned)R.zero_index << (LAYOUT == kLayoutQuad ? 4 : 2);
    asm volatile("" : "+v"(zero_off));
    // one GN step; FIRST = the peeled step (compile-time)
    const bool wg_sync = __builtin_amdgcn_readfirstlane(P.wg_sync) != 0;
    auto gn_step = [&](auto FIRST, int it) {
      constexpr bool kFirst = decltype(FIRST)::value;
      // peeled step: the endpoint registers live only here.  The byte offset is made opaque so that its computation
      // stays at the load (hoisted out of the level loop, 17 offsets would sit in VGPRs for the whole kernel).
      f2 pq[kFirst ? BPL : 1];
      auto endpoint_issue = [&](int k) {
        int i = min((int)lane_id_now() + T * k, n - 1);
        asm volatile("" : "+v"(i));
        const unsigned byte_off = (unsigned)i << 3;
        asm volatile("global_load_dwordx2 %0, %1, %2" : "=v"(pq[kFirst ? k : 0]) : "v"(byte_off), "s"(pts) : "memory");
      };
      if (kFirst) {
        // clock probe, begin stamps (see the end of the kernel): here, at the top of the peeled step, no texel is live
        // yet -- the same block at the kernel's entry made the register allocator spill
        if (P.clock_probe != nullptr && scan == 0 && lane_id_now() == 0) {
          P.clock_probe[0] = __builtin_readcyclecounter();
          P.clock_probe[1] = wall_clock64();
        }
#pragma unroll
        for (int k = 0; k <= kEpAhead; ++k) endpoint_issue(k);
      }
      rotate_wave_priority(it + l);
      float sinRot, cosRot;
      // (the tolerance mode keeps glibc's sincosf: with v_sin_f32 / v_cos_f32 or a 1-ulp fp32 polynomial it is 15-20 % instead of
      // 10-18 % faster than the fast mode, but one scan of the 32 768-scan sweep then lands 1.07e-4 m from the reference and
      // the worst case of the 3-level batch grows from 7.6e-6 to 9.5e-5 m -- profiles/r03/README.md)
      sincos_f32<true>(eth, sinRot, cosRot);
      acc.zero();
      // the step's pose and rotation are wave-uniform: held in SGPRs (4 VGPRs less in a kernel that has none to spare)
      const f2 o2 = step_origin(ex, ey);
      const f2 e2 = f2{uniform_f32(o2.x), uniform_f32(o2.y)};
      const f2 cs = f2{uniform_f32(cosRot), uniform_f32(sinRot)}, sc = f2{cs.y, cs.x};
      // "locate" a beam: rotate, bounds test, cell offset, fractions, and -- only in the lanes whose cell changed since
      // the previous step -- the gather of its texel straight into the beam's cache registers
      auto locate = [&](int k, f2 p, BeamRot& r, float& fx, float& fy) -> unsigned long long {
        if (RELAXED) {
          r.r.x = __builtin_fmaf(cs.x, p.x, -(sc.x * p.y));
          r.r.y = __builtin_fmaf(cs.y, p.x, sc.y * p.y);
        } else {
          r.r.x = cs.x * p.x - sc.x * p.y;
          r.r.y = cs.y * p.x + sc.y * p.y;
        }
        const CellCoord q = cell_coord(R, f2{e2.x + r.r.x, e2.y + r.r.y});
        fx = q.fx;
        fy = q.fy;
        unsigned idx = LAYOUT == kLayoutQuad ? quad_index(q.ix, q.iy, R.tiles_x, R.sx) : __umul24(q.iy, (unsigned)R.sx) + q.ix;
        asm volatile("" : "+v"(idx));  // computed unconditionally: a select below, not a branch
        const unsigned off = q.oob ? zero_off : idx << (LAYOUT == kLayoutQuad ? 4 : 2);
        if (kFirst) {  // a level's first step: every lane gathers (toff[] holds no offset yet)
          asm volatile("global_load_dwordx4 %[t], %[o], %[b]" : [t] "=v"(tq[k]) : [o] "v"(off), [b] "s"(R.quad) : "memory");
          toff[k] = off;
          return ~0ull;
        }
        if (LAYOUT == kLayoutQuad) {
          // The masked gather as ONE instruction sequence under the wave's own control.  The compiler's form of
          // `if (off != toff[k]) load` waits with vmcnt(0) before the PREVIOUS beam is consumed -- it cannot count
          // loads that sit behind a branch -- which puts the gather just issued on the critical path and defeats the
          // software pipeline below.  Here the wave records whether the gather was issued (the mask of the lanes that
          // moved, wave-uniform) and texel_ready() waits for exactly the load it needs.  No C++ control flow: the
          // compiler sees straight-line code and keeps tq[k] where it is (it does not know about the asynchronous
          // write; texel_ready(k) is ordered before every read of tq[k] through its "+v" operand).
          // (Letting lane 0 re-read its texel at every beam, so that the load and wait counts are static and both branches
          // go, measured neutral here: 49.5 / 95.7 / 133 us either way, profiles/r02/README.md.)
          unsigned long long moved, saved;
          asm volatile(
              "v_cmp_ne_u32 vcc, %[o], %[to]\n\t"
              "s_mov_b64 %[mv], vcc\n\t"
              "s_and_saveexec_b64 %[sv], vcc\n\t"
              "s_cbranch_execz 1f\n\t"
              "global_load_dwordx4 %[t], %[o], %[b]\n\t"
              "v_mov_b32 %[to], %[o]\n\t"
              "1:\n\t"
              "s_mov_b64 exec, %[sv]"
              : [t] "+v"(tq[k]), [to] "+v"(toff[k]), [sv] "=&s"(saved), [mv] "=&s"(moved)
              : [o] "v"(off), [b] "s"(R.quad)
              : "vcc", "scc", "memory");
          return moved;
        }
        if (off != toff[k]) {
          if (LAYOUT == kLayoutQuad) {
            tq[k] = *reinterpret_cast<const f4v*>(reinterpret_cast<const char*>(R.quad) + (size_t)off);
          } else {
            // the probability plane itself (4 B per cell: a quarter of the texel plane's footprint, so far more of
            // a map that outgrows the L2 stays in it): rows iy and iy + 1, two cells each
            const char* row = reinterpret_cast<const char*>(R.prob) + (size_t)off;
            const CellPair lo = *reinterpret_cast<const CellPair*>(row);
            const CellPair hi = *reinterpret_cast<const CellPair*>(row + ((size_t)R.sx << 2));
            tq[k] = f4v{lo.a, lo.b, hi.a, hi.b};
          }
          toff[k] = off;
        }
        return 0ull;
      };
      // beam k's texel has landed.  `next_moved` = the mask returned by the locate() of the only gather that may have
      // been issued after beam k's (wave-uniform): loads return in order, so with it in flight vmcnt(1) is enough.
      auto texel_ready = [&](int k, unsigned long long next_moved, bool has_next) {
        if (LAYOUT != kLayoutQuad) return;
        if (kFirst) {  // static schedule: everything issued after beam k's gather may still be in flight
          wait_vmcnt((has_next ? kSched.posG[k + 1] + 1 : kSched.total) - kSched.posG[k] - 1, tq[k]);
        } else if (has_next) {
          asm volatile(
              "s_cmp_eq_u64 %[m], 0\n\t"
              "s_cbranch_scc1 1f\n\t"
              "s_waitcnt vmcnt(1)\n\t"
              "s_branch 2f\n\t"
              "1:\n\t"
              "s_waitcnt vmcnt(0)\n\t"
              "2:"
              : "+v"(tq[k])
              : [m] "s"(next_moved)
              : "scc", "memory");
        } else {
          asm volatile("s_waitcnt vmcnt(0)" : "+v"(tq[k]) : : "memory");
        }
      };
      // peeled step: endpoint k from its load register (padding lanes replaced), scaled for this level, into LDS
      auto endpoint_take = [&](int k) -> f2 {
        wait_vmcnt(kSched.posG[k] - kSched.posE[k] - 1, pq[k]);  // beam k's gather is the next load in issue order
        const bool pad = (int)lane_id_now() + T * k >= n;
        const f2 p = f2{(pad ? 1.0e30f : pq[k].x) * ps, (pad ? 1.0e30f : pq[k].y) * ps};
        mine[k][lane] = p;
        return p;
      };
      auto consume = [&](int k, const BeamRot& r, float fx, float fy) {
        if (RELAXED) {
          // OccGridMapUtil.h:332-346 and :80-97 with contracted multiply-adds: the blend as two lerps on the x differences
          // (i0*(1-fx) + i1*fx == i0 - fx*(i0-i1)), then one on the rows; accumulations as v_fma_f32
          const float i0 = tq[k].x, i1 = tq[k].y, i2 = tq[k].z, i3 = tq[k].w;
          const float xFacInv = 1.0f - fx, yFacInv = 1.0f - fy;
          const float dx1 = i0 - i1, dx2 = i2 - i3, dy1 = i0 - i2, dy2 = i1 - i3;
          const float t0 = __builtin_fmaf(-fx, dx1, i0), t1 = __builtin_fmaf(-fx, dx2, i2);
          const float M = __builtin_fmaf(fy, t1 - t0, t0);
          const float Gx = __builtin_fmaf(dx2, fx, dx1 * xFacInv);  // -gx
          const float Gy = __builtin_fmaf(dy2, fy, dy1 * yFacInv);  // -gy
          const float funVal = 1.0f - M;
          const float rotDeriv = __builtin_fmaf(r.r.y, Gx, -(r.r.x * Gy));
          acc.d01.x = __builtin_fmaf(-Gx, funVal, acc.d01.x);
          acc.d01.y = __builtin_fmaf(-Gy, funVal, acc.d01.y);
          acc.d2 = __builtin_fmaf(rotDeriv, funVal, acc.d2);
          acc.hd.x = __builtin_fmaf(Gx, Gx, acc.hd.x);
          acc.hd.y = __builtin_fmaf(Gy, Gy, acc.hd.y);
          acc.h22 = __builtin_fmaf(rotDeriv, rotDeriv, acc.h22);
          acc.h01 = __builtin_fmaf(Gx, Gy, acc.h01);
          acc.hr.x = __builtin_fmaf(-Gx, rotDeriv, acc.hr.x);
          acc.hr.y = __builtin_fmaf(-Gy, rotDeriv, acc.hr.y);
          return;
        }
        BeamSample b;
        b.X = f2{1.0f - fx, fx};
        b.Y = f2{1.0f - fy, fy};
        b.lo = f2{tq[k].x, tq[k].y};
        b.hi = f2{tq[k].z, tq[k].w};
        beam_finish(b, r, acc);
      };
      // Software pipeline: the texel gather of beam k+1 is ISSUED before beam k is consumed, so a gather has the
      // arithmetic of a whole beam (and the other waves' share of the SIMD) to land in.  The gathers write the beams'
      // own cache registers, so the only extra state in flight is the next beam's (rot, fx, fy); the endpoint of beam
      // k+2 is read from LDS before beam k+1 is located, so the LDS latency is off the chain too.
      // Same arithmetic in the same beam order: identical bits.
      {
        BeamRot rc, rn;
        float fxc, fyc, fxn = 0.0f, fyn = 0.0f;
        f2 p_next = f2{0.0f, 0.0f};
        unsigned long long next_moved = 0ull;
        if (kFirst) {
          locate(0, endpoint_take(0), rc, fxc, fyc);
        } else {
          p_next = mine[BPL > 1 ? 1 : 0][lane];
          locate(0, mine[0][lane], rc, fxc, fyc);
        }
#pragma unroll
        for (int k = 0; k < BPL; ++k) {
          if (kFirst) {
            if (k + 1 + kEpAhead < BPL) endpoint_issue(k + 1 + kEpAhead);
            if (k + 1 < BPL) next_moved = locate(k + 1, endpoint_take(k + 1), rn, fxn, fyn);
          } else {
            const f2 p_cur = p_next;
            if (k + 2 < BPL) p_next = mine[k + 2][lane];
            if (k + 1 < BPL) next_moved = locate(k + 1, p_cur, rn, fxn, fyn);
          }
          // large maps (MatchParams::wg_sync): the four waves of a workgroup -- consecutive scans, whose beam k ends in
          // the same or neighbouring cells -- locate beam k together, so the texel lines one of them pulls in are still
          // in the CU's L1 when the others ask (4096^2 pyramid: 137 -> 133 us; nothing on maps whose touched region the
          // L2s hold).  Waves that have left the kernel (empty scan, batch tail) do not count at s_barrier.
          if (wg_sync) asm volatile("s_barrier" ::: "memory");
          texel_ready(k, next_moved, k + 1 < BPL);
          consume(k, rc, fxc, fyc);
          asm volatile(""
                       : "+v"(acc.d01), "+v"(acc.d2), "+v"(acc.hd), "+v"(acc.h22), "+v"(acc.h01), "+v"(acc.hr)
                       :
                       : "memory");
          rc = rn;
          fxc = fxn;
          fyc = fyn;
        }
      }
      // a scan longer than the 64 * BPL cached beams (BPL comes from a host-side length HINT): the rest streams
      // from memory like gn_match_kernel's loop, in the same per-lane order (wave-uniform trip count)
      for (int i = T * BPL + (n > T * BPL ? lane_id_now() : 0); i < n; i += T) {
        const float2 p = pts[i];
        BeamRot r;
        const BeamSample b = beam_fetch<LAYOUT>(R, e2, cs, sc, f2{p.x * ps, p.y * ps}, r);
        beam_finish(b, r, acc);
      }
      wave_allreduce9(acc);
      gn_solve_and_step(acc, ex, ey, eth);
    };
    int it = 0;
    if (kPeel && peel_here) {
      gn_step(std::true_type{}, 0);
      it = 1;
    }
    for (; it < gn_steps; ++it) gn_step(std::false_type{}, it);
    eth = normalize_angle<true>(eth);
    affine_apply(L.worldTmap, ex, ey, pw0, pw1);
    pw2 = eth;
  }
  if (lane_id_now() == 0) {
    P.out_pose[3 * scan + 0] = pw0;
    P.out_pose[3 * scan + 1] = pw1;
    P.out_pose[3 * scan + 2] = pw2;
    if (P.out_cov) {
      float* c = P.out_cov + 9 * scan;
      c[0] = acc.hd.x; c[1] = acc.h01; c[2] = acc.hr.x;
      c[3] = acc.h01; c[4] = acc.hd.y; c[5] = acc.hr.y;
      c[6] = acc.hr.x; c[7] = acc.hr.y; c[8] = acc.h22;
    }
  }
  // clock probe (bench.py: what clock does the kernel actually get?): the wave of scan 0 stamps the shader-clock counter
  // (s_memtime) and the 100 MHz wall clock at the top of its first GN step and here, as its last act; the ratio of the
  // two differences is the clock it ran at.  (Stamps of different launches cannot be compared: the wave lands on
  // different CUs, whose shader-clock counters are not aligned.)
  if (P.clock_probe != nullptr && scan == 0 && lane_id_now() == 0) {
    P.clock_probe[2] = __builtin_readcyclecounter();
    P.clock_probe[3] = wall_clock64();
  }
}

}  // namespace hsm
