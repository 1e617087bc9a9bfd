// match_plan_check.cpp -- hector_slam_amd/csrc/match_plan.h on the CPU (tests/test_match_plan.py).
//   sites    reads launch sites from stdin, one per line (the MatchSite fields in the order of read_site), and prints the plan of each:
//            family, the five hsm_last_launch_config values, parity, cached rows, probe, tail batch | kernel name
//   cases    what the launch record cannot show (cached rows, the probe instantiation), written out from gn_match_exact.h's constants
//   staging  reads_scan_once against the function the host runtime had before the plan existed, restated literally, over a grid
// `cases` and `staging` print one JSON line {"cases": N, "mismatches": M} and return M != 0.
#include <cstdio>
#include <cstring>

#include "match_plan.h"

using namespace hsm_plan;

static bool read_site(MatchSite& s) {
  int f[25];
  unsigned long long cells = 0;
  for (int i = 0; i < 25; ++i) {
    if (i == 11) {
      if (scanf("%llu", &cells) != 1) return false;
      continue;
    }
    if (scanf("%d", &f[i]) != 1) return false;
  }
  s = MatchSite();
  s.batch = f[0], s.max_n = f[1], s.n_bound = f[2], s.exact = f[3], s.relaxed = f[4], s.layout = f[5], s.batched = f[6];
  s.trace = f[7], s.clock_probe = f[8], s.capturing = f[9], s.compute_units = f[10], s.level0_cells = (size_t)cells;
  s.wps_override = f[12], s.bpl_override = f[13], s.texel_cache = f[14], s.exact_cached = f[15], s.exact_chain_wave = f[16];
  s.exact_split_tail = f[17], s.exact_dense = f[18], s.exact_dense_min = f[19], s.exact_spec = f[20], s.exact_spec1 = f[21];
  s.spb_large = f[22], s.coop_min_beams = f[23], s.coop_skip = f[24];
  return true;
}

static int run_sites() {
  MatchSite s;
  while (read_site(s)) {
    const MatchPlan p = plan_match(s);
    printf("%d %d %d %d %d %d %d %d %d %d|%s\n", (int)p.family, p.record[0], p.record[1], p.record[2], p.record[3],
           p.record[5] ? -p.record[4] : p.record[4], p.parity, p.bpc, (int)p.probe, p.tail_batch, p.name);
  }
  return 0;
}

static int g_cases = 0, g_bad = 0;
static void expect(bool ok, const char* what) {
  ++g_cases;
  if (!ok) {
    ++g_bad;
    fprintf(stderr, "mismatch: %s\n", what);
  }
}

static MatchSite exact_batch(int batch, int n, size_t cells) {
  MatchSite s;
  s.batch = batch, s.max_n = n, s.n_bound = n, s.exact = true, s.batched = true, s.level0_cells = cells;
  return s;
}

static int run_cases() {
  const int CU = 256;
  const size_t within = (size_t)2048 * 2048, beyond = (size_t)4096 * 2304;
  // gn_match_exact.h: HSM_XBPC 15, HSM_XBPC_MAIN 13, HSM_XBPC_CW 6
  MatchPlan p = plan_match(exact_batch(16 * CU, 1081, within));
  expect(p.family == Family::kExactCached && p.bpl == 17 && p.bpc == 13 && !p.probe && p.block == 256, "17 rows, 13 cached at four workgroups per CU");
  p = plan_match(exact_batch(16 * CU, 1081, beyond));
  expect(p.family == Family::kExactCached && p.bpl == 17 && p.bpc == 15 && !p.probe, "17 rows, 15 cached beyond the L2s");
  p = plan_match(exact_batch(8 * CU, 1081, within));
  expect(p.family == Family::kExactCachedCw && p.bpl == 17 && p.bpc == 15 && p.block == 320, "chain wavefront, 15 cached up to 2 CU groups");
  p = plan_match(exact_batch(8 * CU, 1081, beyond));
  expect(p.family == Family::kExactCachedCw && p.bpl == 17 && p.bpc == 15, "chain wavefront, 15 cached up to 2 CU groups beyond the L2s");
  p = plan_match(exact_batch(8 * CU + 4, 1081, within));
  expect(p.family == Family::kExactCachedCw && p.bpl == 17 && p.bpc == 6, "chain wavefront, 6 cached up to 3 CU groups");
  p = plan_match(exact_batch(12 * CU, 1081, within));
  expect(p.family == Family::kExactCachedCw && p.bpl == 17 && p.bpc == 6, "chain wavefront, 6 cached at 3 CU groups");
  p = plan_match(exact_batch(12 * CU, 1081, beyond));
  expect(p.family == Family::kExactCached && p.bpl == 17 && p.bpc == 15, "no chain wavefront at 3 CU groups beyond the L2s");
  p = plan_match(exact_batch(12 * CU + 4, 1081, within));
  expect(p.family == Family::kExactCached && p.bpc == 13, "no chain wavefront beyond 3 CU groups");
  p = plan_match(exact_batch(12 * CU, 720, within));
  expect(p.family == Family::kExactCachedCw && p.bpl == 13 && p.bpc == 7, "13 rows, chain wavefront with 7 cached");
  p = plan_match(exact_batch(8 * CU, 720, within));
  expect(p.family == Family::kExactCachedCw && p.bpl == 13 && p.bpc == 13, "13 rows, chain wavefront with all cached");
  p = plan_match(exact_batch(16 * CU, 720, within));
  expect(p.family == Family::kExactCached && p.bpl == 13 && p.bpc == 13, "13 rows at four workgroups per CU");
  p = plan_match(exact_batch(16 * CU, 320, within));
  expect(p.family == Family::kExactCached && p.bpl == 5 && p.bpc == 5, "5 rows");
  p = plan_match(exact_batch(16, 576, within));
  expect(p.family == Family::kExactCachedCw && p.bpl == 9 && p.bpc == 9, "9 rows, chain wavefront");
  // the probe instantiation: the 13-cached-row headline form with a clock probe, and nothing else
  for (int probe = 0; probe < 2; ++probe) {
    MatchSite s = exact_batch(16 * CU, 1081, within);
    s.clock_probe = probe;
    expect(plan_match(s).probe == (probe != 0), "probe on the headline form iff a clock probe is set");
    s.level0_cells = beyond;
    expect(!plan_match(s).probe, "no probe instantiation with 15 cached rows");
    s = exact_batch(8 * CU, 1081, within), s.clock_probe = probe;
    expect(!plan_match(s).probe, "no probe instantiation of the chain-wavefront forms");
    s = exact_batch(16 * CU, 720, within), s.clock_probe = probe;
    expect(!plan_match(s).probe, "no probe instantiation of the 13-row form");
    s = exact_batch(16 * CU + 4, 1081, within), s.clock_probe = probe;  // split: the probe belongs to the first launch
    const MatchPlan sp = plan_match(s);
    expect(sp.tail_batch == 4 && sp.probe == (probe != 0) && sp.bpc == 13, "split launch: first part carries the probe");
  }
  // the exchange rides on the forms without a chain wavefront only, and its workgroups count in the grid
  {
    MatchSite s = exact_batch(16 * CU, 1081, within);
    s.exchange = true, s.exchange_wait_blocks = 3;
    p = plan_match(s);
    expect(p.carries_exchange && p.grid == 4 * CU + 3 && p.record[3] == 4 * CU + 3, "exchange carried by the headline form");
    s.batch = 8 * CU;
    p = plan_match(s);
    expect(!p.carries_exchange && p.grid == 2 * CU, "exchange not carried by the chain-wavefront form");
    s.batch = 16 * CU + 4;
    p = plan_match(s);
    expect(!p.carries_exchange && p.tail_batch == 4 && p.record[3] == 4 * CU + 1, "exchange not carried by a split launch");
  }
  // the speculative-carry form is only WANTED where the host has a true bound and no graph is being captured
  {
    MatchSite s = exact_batch(1, 4096, within);
    s.exact_spec = true;
    expect(plan_match(s).family == Family::kSpec, "spec wanted");
    s.capturing = true;
    expect(plan_match(s).family == Family::kExactDense, "capture takes the literal dense form");
    s.capturing = false, s.n_bound = 0;
    expect(plan_match(s).family == Family::kExactDense, "no bound takes the literal dense form");
  }
  printf("{\"cases\": %d, \"mismatches\": %d}\n", g_cases, g_bad);
  return g_bad != 0;
}

// ---- the host runtime's scan_is_read_once and choose_wps as they stood before match_plan.h, on a bag of the context's fields ----
struct OldCtx {
  int wps_override, compute_units, bpl_override, coop_min_beams, exact_dense_min;
  bool exact, auto_parity, exact_dense, exact_spec;
};
static int old_choose_wps(const OldCtx* h, int batch, int max_n) {
  if (h->wps_override > 0) return h->wps_override;
  int wps = 1;
  const long target_waves = (long)h->compute_units * 4 * 4;
  while (wps < 16 && (long)batch * wps < target_waves && 64 * wps < max_n) wps *= 2;
  int lat = 1;
  while (lat < 16 && 64 * 5 * lat < max_n) lat *= 2;
  return wps < lat ? wps : lat;
}
static bool old_wants_exact(const OldCtx* h) { return h->exact || h->auto_parity; }
static bool old_scan_is_read_once(const OldCtx* h, int n) {
  constexpr int kOldMaxRegisterResidentBeams = 16 * 64 * 17, kOldDenseRound = 64 * 15, kOldExactGroupRounds = 5;
  if (!old_wants_exact(h))
    return n <= kOldMaxRegisterResidentBeams && h->bpl_override != 0 && (n < h->coop_min_beams || h->wps_override != 0);
  const int wps = old_choose_wps(h, 1, n);
  if (wps > 1 && h->wps_override == 0 && h->exact_dense && n >= h->exact_dense_min)
    return !h->exact_spec && n <= 2 * kOldDenseRound;
  return n <= kOldExactGroupRounds * 64 * wps;
}

static int run_staging() {
  const int overrides[] = {0, 1, 2, 4, 8, 16};
  for (int wo : overrides)
    for (int exact = 0; exact < 2; ++exact)
      for (int dense = 0; dense < 2; ++dense)
        for (int spec = 0; spec < 2; ++spec)
          for (int knobs = 0; knobs < 4; ++knobs) {  // bit 0: HSM_BPL=0, bit 1: HSM_EXACT_DENSE_MIN=2048 and HSM_COOP_MIN=1024
            OldCtx o{wo, 256, (knobs & 1) ? 0 : -1, (knobs & 2) ? 1024 : 4096, (knobs & 2) ? 2048 : 4096, false, exact != 0, dense != 0, spec != 0};
            MatchSite s;
            s.batch = 1, s.exact = exact != 0, s.wps_override = wo, s.bpl_override = o.bpl_override, s.coop_min_beams = o.coop_min_beams;
            s.exact_dense = dense != 0, s.exact_dense_min = o.exact_dense_min, s.exact_spec = spec != 0, s.level0_cells = 65536;
            for (int n = 0; n <= 20000; ++n) {
              s.max_n = s.n_bound = n;
              bool same = true;
              for (int skip = 0; skip < 2; ++skip) {  // (where a scan is staged does not depend on the cooperative form's back-off)
                s.coop_skip = skip != 0;
                same = same && plan_match(s).reads_scan_once == old_scan_is_read_once(&o, n);
              }
              ++g_cases;
              if (!same && ++g_bad <= 10) fprintf(stderr, "staging differs: n %d wps %d exact %d dense %d spec %d knobs %d\n", n, wo, exact, dense, spec, knobs);
            }
          }
  printf("{\"cases\": %d, \"mismatches\": %d}\n", g_cases, g_bad);
  return g_bad != 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && strcmp(argv[1], "sites") == 0) return run_sites();
  if (argc == 2 && strcmp(argv[1], "cases") == 0) return run_cases();
  if (argc == 2 && strcmp(argv[1], "staging") == 0) return run_staging();
  fprintf(stderr, "usage: match_plan_check sites|cases|staging\n");
  return 2;
}
