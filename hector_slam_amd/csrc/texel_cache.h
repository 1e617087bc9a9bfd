// texel_cache.h -- the pieces the two texel-cache forms share: gn_match_cached_kernel (gn_match_cached.h, match_teams.hip) and
// the exact-order forms of gn_match_exact.h (match_exact_cached.hip).  The issue order of the peeled first step's loads, the
// counted wait for them, and the 8-byte load of two neighbouring cells.  A header of its own so that an edit of either kernel
// does not rebuild the other's unit.  No kernel is defined here.
#pragma once
#include <hip/hip_runtime.h>

namespace hsm {

#ifndef HSM_EP_AHEAD     // endpoint loads in flight ahead of the beam being located in the peeled step
#define HSM_EP_AHEAD 4
#endif

// Issue order of the loads of the peeled first step: endpoints E_0 .. E_d up front, the gather G_0, then per beam j
// the endpoint E_{j+1+d} and the gather G_{j+1}.  pos*[k] = index in that order; total = number of loads.
struct PeelSchedule {
  int posE[32], posG[32], total;
};
constexpr PeelSchedule peel_schedule(int bpl, int d) {
  PeelSchedule s{};
  int c = 0;
  for (int k = 0; k <= d && k < bpl; ++k) s.posE[k] = c++;
  s.posG[0] = c++;
  for (int j = 0; j < bpl; ++j) {
    if (j + 1 + d < bpl) s.posE[j + 1 + d] = c++;
    if (j + 1 < bpl) s.posG[j + 1] = c++;
  }
  s.total = c;
  return s;
}

// s_waitcnt vmcnt(n) for the inline-asm loads, ordered before every later use of `x` (the register the awaited load
// writes).  n is a compile-time constant after unrolling; anything above the cases waits for everything.
template <class T>
__device__ __forceinline__ void wait_vmcnt(int n, T& x) {
  switch (n) {
    case 1: asm volatile("s_waitcnt vmcnt(1)" : "+v"(x) : : "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(2)" : "+v"(x) : : "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(3)" : "+v"(x) : : "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(4)" : "+v"(x) : : "memory"); break;
    case 5: asm volatile("s_waitcnt vmcnt(5)" : "+v"(x) : : "memory"); break;
    case 6: asm volatile("s_waitcnt vmcnt(6)" : "+v"(x) : : "memory"); break;
    case 7: asm volatile("s_waitcnt vmcnt(7)" : "+v"(x) : : "memory"); break;
    case 8: asm volatile("s_waitcnt vmcnt(8)" : "+v"(x) : : "memory"); break;
    case 9: asm volatile("s_waitcnt vmcnt(9)" : "+v"(x) : : "memory"); break;
    case 10: asm volatile("s_waitcnt vmcnt(10)" : "+v"(x) : : "memory"); break;
    case 11: asm volatile("s_waitcnt vmcnt(11)" : "+v"(x) : : "memory"); break;
    case 12: asm volatile("s_waitcnt vmcnt(12)" : "+v"(x) : : "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(0)" : "+v"(x) : : "memory"); break;
  }
}

// 8-byte load from a 4-byte aligned address (two neighbouring cells of a row of the probability plane): one
// global_load_dwordx2 -- the hardware handles dword-aligned wide loads
struct __attribute__((packed, aligned(4))) CellPair {
  float a, b;
};

}  // namespace hsm
