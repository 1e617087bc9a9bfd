// CPU check for the device-side update preparation (map_update_scans.h update_prep_kernel): the host path of updateByScan calls
// glibc's sinf and cosf SEPARATELY (prepare_level), the device evaluates libm_exact.h's sincosf_glibc once.  Both must be the
// same pair of floats for every argument.  Swept: every `stride`-th float bit pattern (all exponents, both signs, denormals,
// inf / NaN), and every bit pattern within 4096 of the boundaries of sincosf_glibc's argument ranges (2^-12, pi/4, 120, inf)
// and of the first multiples of pi/2, both signs.  sinf / cosf are called through volatile pointers: the compiler must not
// merge the two calls into one sincosf.  Prints one JSON line; exit code 1 on any mismatch.
// Build: g++ -O2 -ffp-contract=off -pthread sincos_pair_check.cpp -lm
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <thread>
#include <vector>

#include "../../hector_slam_amd/csrc/libm_exact.h"

static float (*volatile host_sinf)(float) = sinf;
static float (*volatile host_cosf)(float) = cosf;

static inline bool same(float a, float b) {
  const uint32_t x = hsm::libm::f32_bits(a), y = hsm::libm::f32_bits(b);
  if (x == y) return true;
  return (a != a) && (b != b);  // any NaN equals any NaN (payload / sign of invalid results not pinned)
}

static inline bool pair_ok(uint32_t u) {
  const float x = hsm::libm::bits_f32(u);
  float s, c;
  hsm::libm::sincosf_glibc<false>(x, s, c);
  return same(host_sinf(x), s) && same(host_cosf(x), c);
}

int main(int argc, char** argv) {
  const uint64_t stride = argc > 1 ? strtoull(argv[1], nullptr, 10) : 257;
  const int T = argc > 2 ? atoi(argv[2]) : (int)std::thread::hardware_concurrency();
  std::atomic<uint64_t> bad{0}, n{0};
  std::atomic<uint32_t> first{0};
  std::vector<std::thread> th;
  const uint64_t total = (1ULL << 32);
  for (int t = 0; t < T; ++t)
    th.emplace_back([&, t]() {
      uint64_t lb = 0, ln = 0;
      for (uint64_t u = (uint64_t)t * stride; u < total; u += stride * (uint64_t)T) {
        if (!pair_ok((uint32_t)u) && !lb++) first.store((uint32_t)u);
        ++ln;
      }
      bad += lb;
      n += ln;
    });
  for (auto& x : th) x.join();
  // the range boundaries of sincosf_glibc (top 12 bits 0x398, 0x3f4, 0x42f, 0x7f8) and k * pi/2, k = 1 .. 8
  std::vector<uint32_t> centres = {0x39800000u, 0x3f400000u, 0x42f00000u, 0x7f800000u, 0x00800000u, 0u};
  for (int k = 1; k <= 8; ++k) centres.push_back(hsm::libm::f32_bits((float)(k * 1.5707963267948966)));
  uint64_t nb = 0, bad_b = 0;
  for (uint32_t c : centres)
    for (int sign = 0; sign < 2; ++sign)
      for (int64_t d = -4096; d <= 4096; ++d) {
        const int64_t m = (int64_t)c + d;
        if (m < 0 || m > 0x7fffffff) continue;
        const uint32_t u = (uint32_t)m | (sign ? 0x80000000u : 0u);
        if (!pair_ok(u) && !bad_b++ && !bad.load()) first.store(u);
        ++nb;
      }
  printf("{\"checked\": %llu, \"stride\": %llu, \"boundary_checked\": %llu, \"mismatches\": %llu, \"first_bad_bits\": \"0x%08x\"}\n",
         (unsigned long long)n.load(), (unsigned long long)stride, (unsigned long long)nb,
         (unsigned long long)(bad.load() + bad_b), first.load());
  return (bad.load() || bad_b) ? 1 : 0;
}
