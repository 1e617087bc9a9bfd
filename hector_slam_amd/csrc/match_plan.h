// match_plan.h -- which form of the matcher a launch takes: ONE decision, made on the host from plain values, before anything
// is launched.  plan_match(site) holds every rule; the three launch units (match.hip, match_teams.hip,
// match_exact_cached.hip) map the plan to their instantiations, match.hip records it (record_launch) and asks it where a
// single scan is staged (reads_scan_once).  Plain C++17, no HIP and no context: tests/cpp/match_plan_check.cpp runs it on the CPU
// against the table of tests/golden/match_forms.json.  DESIGN.md "which form runs when" is this file in prose.
#pragma once
#include <cstddef>

namespace hsm_plan {

// what the kernels fix (static_asserts in the launch units hold these equal to match_types.h, gn_step.h, gn_match_dense.h and gn_match_spec.h)
constexpr int kQuad = 1, kPlane = 2;                     // kLayoutQuad / kLayoutPlane
constexpr int kExactGroupRounds = 5;                     // rounds the exact-order team form keeps in registers
constexpr int kDenseRound = 64 * 15;                     // beams per round of the producers-ahead form
constexpr int kSpec1MaxBeams = 2048;                     // the on-chip speculative-carry form's longest scan
constexpr int kMaxRegisterResidentBeams = 16 * 64 * 17;  // 16 wavefronts x 17 beams per lane
// cached rows of the exact-order texel-cache forms: gn_match_exact.h's HSM_XBPC, HSM_XBPC_MAIN and HSM_XBPC_CW (there with the
// reasons), which a build may set with -D.  match_exact_cached.hip includes this header FIRST and then asserts them equal.
#ifdef HSM_XBPC
constexpr int kXbpc = HSM_XBPC;
#else
constexpr int kXbpc = 15;
#endif
#ifdef HSM_XBPC_MAIN
constexpr int kXbpcMain = HSM_XBPC_MAIN;
#else
constexpr int kXbpcMain = 13;
#endif
#ifdef HSM_XBPC_CW
constexpr int kXbpcCw = HSM_XBPC_CW;
#else
constexpr int kXbpcCw = 6;
#endif
enum Parity { kParityFast = 0, kParityExact = 1, kParityRelaxed = 2 };  // HSM_PARITY_* (capi.h)

// the matcher's knobs: fixed when the context is created (settings.h parse_settings, which names each one's env setting), the same
// for every launch
struct MatchKnobs {
  int wps_override = 0;          // hsm_opts::waves_per_scan, else env HSM_WPS: 1, 2, 4, 8, 16 wavefronts per scan, 0 = choose_wps
  int bpl_override = -1;         // 0 = force the memory loop (env HSM_BPL=0), -1 = auto
  bool texel_cache = true;       // env HSM_TEXEL_CACHE=0: plain gn_match_kernel for throughput launches too
  bool exact_cached = true;      // env HSM_EXACT_CACHED=0: exact-mode batches take the one-wavefront-per-scan exact form (gn_match_kernel) instead of gn_match_exact.h's
  bool exact_chain_wave = true;  // env HSM_EXACT_CHAIN_WAVE=0: no chain-only wavefront, teams of wavefronts for batches below 4096 scans (rounds 3-4)
  bool exact_split_tail = true;  // env HSM_EXACT_SPLIT_TAIL=0: one launch however the batch divides into generations
  bool exact_dense = true;       // env HSM_EXACT_DENSE=0: dense scans in exact order keep the 16-wavefront team form (gn_match_kernel<16,...,EXACT>)
  int exact_dense_min = 4096;    // env HSM_EXACT_DENSE_MIN: beams from which the producers-ahead-of-the-chain form takes over
  bool exact_spec = false;       // env HSM_EXACT_SPEC=1: one-workgroup-per-scan launches in exact order take the speculative-carry form (gn_match_spec.h:
                                 // the same bits; measured SLOWER than the literal chains on one CU -- DESIGN.md 8 -- hence opt-in)
  bool exact_spec1 = false;      // env HSM_EXACT_SPEC1=1: ONE scan of up to 2048 beams (hsm_match) in exact order takes the on-chip speculative-carry form
  int spb_large = 8;             // env HSM_SPB_LARGE=4|8: scans per workgroup of the texel-cache matcher on maps > 2^23 cells
  int coop_min_beams = 4096;     // single scans at least this long take the multi-workgroup matcher (env HSM_COOP_MIN)
};

// everything the decision reads: the knobs and the launch's own shape
struct MatchSite : MatchKnobs {
  int batch = 1;        // scans of the launch
  int max_n = 0;        // beams of the longest scan, or the caller's hint of it
  int n_bound = 0;      // a TRUE bound of the scan lengths where the host has one, else 0
  bool exact = false;   // the reference's summation order (HSM_PARITY_EXACT, and HSM_PARITY_AUTO)
  bool relaxed = false; // HSM_PARITY_RELAXED
  int layout = kQuad;
  bool batched = false;      // a begin_world array is given (the batched entries); false: hsm_match's single scan
  bool trace = false;        // the launch writes a per-step trace
  bool clock_probe = false;  // hsm_set_clock_probe
  bool capturing = false;    // the stream is being captured into a graph
  bool exchange = false;     // the launch may carry a pose-exchange step (hsm_match_batch_device_gather) ...
  int exchange_wait_blocks = 0;  // ... with this many workgroups behind the matcher's own
  int compute_units = 256;
  size_t level0_cells = 0;
  bool coop_skip = false;  // the multi-workgroup form is backing off after an exchange timeout, or could not be launched
};

enum class Family { kTeam, kTeamExact, kCached, kExactCached, kExactCachedCw, kExactDense, kSpec, kSpec1, kCoop };

struct MatchPlan {
  Family family = Family::kTeam;
  // template coordinates of the instantiation (bpc: cached rows of the exact-cached forms; coop: wps = -K workgroups)
  int wps = 1, spb = 1, bpl = 0, bpc = 0;
  bool probe = false, relaxed = false;
  int layout = kQuad;
  int block = 0, grid = 0;
  int tail_batch = 0;            // 0, or the scans of the part-filled last generation, which go out in a second launch
  bool carries_exchange = false; // the launch carries MatchParams::xp itself (grid counts its wait_blocks)
  bool reads_scan_once = false;  // a single scan may stay in pinned host memory
  bool wants_perm = false;       // the form takes its scans through a permutation (ensure_batch_perm)
  int parity = kParityFast;      // hsm_last_launch_parity
  const char* name = "";         // hsm_last_launch_kernel
  int record[6] = {0, 0, 0, 0, 0, 0};  // hsm_last_launch_config: layout, waves per scan, block, grid, beams per lane, texel cache
};

// maps whose touched region outgrows the L2s (4 MB per XCD): level 0 of more than 2^23 cells.  Measured at 4096^2 against
// 2048^2 (profiles/r03 .. r06): such a map keeps one contiguous eighth of a batch per XCD, gets the per-beam workgroup barrier,
// eight scans per workgroup in the fast texel-cache form, fifteen cached rows and no chain wavefront at three workgroups per CU
// in the exact one, and its batches are sorted by tile without being asked.
inline bool level0_outgrows_l2(size_t cells) { return cells > ((size_t)1 << 23); }

// a launch that is after throughput: a batch, and nobody watches its steps.  Only these take the texel-cache forms.
inline bool throughput_launch(const MatchSite& s) { return s.batched && !s.trace; }

// waves per scan: enough wavefronts to fill 256 CUs x 4 SIMDs x several waves, but never
// more lanes than beams
inline int choose_wps(const MatchSite& s) {
  if (s.wps_override > 0) return s.wps_override;
  int wps = 1;
  const long target_waves = (long)s.compute_units * 4 * 4;  // 4 waves per SIMD on every CU of THIS device (a partitioned device has fewer)
  while (wps < 16 && (long)s.batch * wps < target_waves && 64 * wps < s.max_n) wps *= 2;
  // ... but keep about five beams per lane: every extra wavefront adds LDS staging + a barrier to each
  // of the 14 dependent GN steps, which costs more than the beam loop saves (single 1081-beam scan on
  // MI355X: 72 / 58 / 53 / 61 / 79 us for 1 / 2 / 4 / 8 / 16 waves, profiles/r01/README.md)
  int lat = 1;
  while (lat < 16 && 64 * 5 * lat < s.max_n) lat *= 2;
  return wps < lat ? wps : lat;
}

namespace detail {

inline void finish(MatchPlan& p, const char* name, bool cached) {
  p.name = name;
  p.record[0] = p.layout, p.record[1] = p.wps, p.record[2] = p.block, p.record[3] = p.grid, p.record[4] = p.bpl, p.record[5] = cached ? 1 : 0;
}

// the team forms (gn_match_kernel) and the fast texel-cache form (gn_match_cached_kernel): `wps` wavefronts per scan, `spb` scans per
// workgroup, `bpl` beams per lane in registers (0: the endpoints stream from memory in every GN step)
inline void plan_team(const MatchSite& s, MatchPlan& p, int wps, int spb, int bpl) {
  p.wps = wps, p.spb = spb, p.bpl = bpl;
  p.block = 64 * wps * spb;
  p.grid = (s.batch + spb - 1) / spb;
  if (s.exact) {
    p.family = Family::kTeamExact;
    finish(p, "gn_match_kernel (exact order)", false);
  } else if (wps == 1 && (bpl == 9 || bpl == 17) && s.texel_cache && throughput_launch(s)) {
    // throughput launches of long scans: the texel-cache form (gn_match_cached.h)
    p.family = Family::kCached;
    p.relaxed = s.layout == kQuad && s.relaxed;
    p.wants_perm = true;  // (hsm_set_batch_order: the launch takes its scans through a permutation)
    finish(p, "gn_match_cached_kernel", true);
  } else {
    p.family = Family::kTeam;
    finish(p, "gn_match_kernel", false);
  }
}

// the texel-cache exact forms, by scan length and by how many workgroups the launch leaves a CU
inline void plan_exact_cached(const MatchSite& s, MatchPlan& p) {
  const int per_lane = (s.max_n + 63) / 64;
  // A launch that leaves every CU at most THREE workgroups takes the chain-wavefront form (gn_match_exact.h, CW): a fifth
  // wavefront per workgroup runs the chain jobs, so a round lasts max(job, production) instead of job + production --
  // 36 us against 52 for a level-0 batch of up to 2048 scans, 49 against 57 at 3072 (profiles/r05/README.md 9).  Not
  // beyond: the dispatcher places a workgroup only where EVERY SIMD has room for ceil(waves / 4) of its wavefronts
  // (tools/study/ubench_wg_placement.hip), the fourth five-wavefront workgroup of a CU waits for a whole workgroup to
  // retire, and at four per CU both forms deliver the same ~70 scans per us anyway.
  const int groups = (s.batch + 3) / 4;
  // ... and a map that outgrows the L2s (4096^2: 136 us with six cached rows against 128.5 with fifteen, at 3072 scans) keeps
  // round 3's form at three workgroups per CU; up to two per CU the chain-wavefront form has the full texel cache as well
  const bool cw2 = s.exact_chain_wave && groups <= 2 * s.compute_units;
  const bool cw = cw2 || (s.exact_chain_wave && groups <= 3 * s.compute_units && !level0_outgrows_l2(s.level0_cells));
  // (a round loop that leaves behind the longest scan's last row costs the 17-row form 8 % on full-length scans -- sixteen
  // exit edges --; a 13-row instantiation costs compile time only: a batch of 720-beam scans runs 13 rounds instead of 17)
  p.bpl = per_lane <= 5 ? 5 : per_lane <= 9 ? 9 : per_lane <= 13 ? 13 : 17;
  p.bpc = p.bpl;
  if (p.bpl == 13 && cw && !cw2) p.bpc = kXbpcCw + 1;
  if (p.bpl == 17) {
    // four workgroups per CU: the balanced schedule (13 cached rows) where level 0 fits the L2s, else round 3's (15 cached rows:
    // the gathers of a map that misses the L2 cost more than the schedule gains)
    p.bpc = cw2 ? kXbpc : cw ? kXbpcCw : level0_outgrows_l2(s.level0_cells) ? kXbpc : kXbpcMain;
    // (hsm_set_clock_probe: the headline form has an instantiation that carries the stamps)
    p.probe = !cw && p.bpc == kXbpcMain && s.clock_probe;
  }
  p.family = cw ? Family::kExactCachedCw : Family::kExactCached;
  p.wps = 1, p.spb = 4;
  p.block = 64 * (4 + (cw ? 1 : 0));
  p.grid = groups;
  // the pose exchange rides on the launch (every scan posts its pose, the workgroups behind the matcher's own unpack); the
  // chain-wavefront forms do not carry it: the caller queues the stand-alone exchange kernel
  p.carries_exchange = !cw && s.exchange;
  if (p.carries_exchange) p.grid += s.exchange_wait_blocks;
  p.wants_perm = true;  // (hsm_set_batch_order)
  finish(p, cw ? "gn_match_exact_cached_kernel (chain wavefront)" : "gn_match_exact_cached_kernel", true);
}

}  // namespace detail

// One part of a launch that plan_match split (MatchPlan::tail_batch): the whole generations, or (`is_tail`) the part-filled last
// one.  Both stay exact-order texel-cache forms whatever a launch of their own size would take -- the tail of a batch of dense
// scans is not handed to the one-workgroup-per-scan form.
inline MatchPlan plan_split_part(const MatchSite& whole, int tail_batch, bool is_tail) {
  MatchSite s = whole;
  s.batch = is_tail ? tail_batch : whole.batch - tail_batch;
  if (is_tail) s.clock_probe = false;  // (scan 0's probe belongs to the first launch)
  // (a launch that carries the pose exchange: the part-filled last generation runs in a chain-wavefront form, which does not --
  // so the whole step is left to the stand-alone exchange kernel behind both launches)
  s.exchange = false;
  MatchPlan p;
  p.layout = s.layout;
  p.parity = kParityExact;
  detail::plan_exact_cached(s, p);
  return p;
}

inline MatchPlan plan_match(const MatchSite& s) {
  MatchPlan p;
  p.layout = s.layout;
  p.parity = s.exact ? kParityExact : (s.relaxed ? kParityRelaxed : kParityFast);
  const bool throughput = throughput_launch(s);

  // one dense scan of hsm_match, tree summation: spread over K workgroups of one launch (gn_match_coop_kernel); the exact-order
  // forms keep the scan on one workgroup -- their nine summation chains are sequential anyway.  One beam per lane.  16 k beams,
  // matchData us for K = 16 / 24 / 32 / 64 workgroups: 79.8 / 71 / 66-70 / 64 with round 2's grid barrier; 70 (24) / 67-71 (31) /
  // 76 (48) / 63-64 (64) with the tagged exchange (profiles/r03/README.md).  The form re-reads the scan in every GN step, and a
  // scan it WOULD take is staged for it even while it backs off (coop_skip).
  const bool coop_wanted = !s.batched && s.max_n >= s.coop_min_beams && s.wps_override == 0 && !s.exact;
  if (coop_wanted && !s.coop_skip) {
    int K = (s.max_n + 255) / 256;
    if (K > 64) K = 64;
    if (K < 2) K = 2;
    p.family = Family::kCoop;
    p.wps = -K;  // negative: K cooperating workgroups instead of waves per scan
    p.block = 256, p.grid = K;
    p.parity = kParityFast;
    detail::finish(p, "gn_match_coop_kernel", false);
    return p;
  }

  int wps = choose_wps(s);
  // throughput launches of the quad layout in reference order: every wavefront a producer with the texel cache, four scans per
  // workgroup, one 36-lane chain job per round behind the round's barrier (gn_match_exact.h).  Measured against round 2's producer /
  // chain-wavefront form (profiles/r03/README.md): 66-69 vs 92 us on the 2048^2 headline batch, 141-143 vs 199 us on the
  // 3-level batch, 156-162 vs 291 us on the 4096^2 pyramid.  Scans longer than 17 beams per lane stream their tail rows.
  const bool exact_cached_ok = s.exact && throughput && s.layout == kQuad && s.bpl_override != 0 && s.exact_cached;
  // reference order, batches of scans of up to 17 beams per lane: ALWAYS one wavefront per scan with the texel cache.  Teams of
  // wavefronts per scan -- what choose_wps picks below 4096 scans to fill the chip -- only produce faster, and production is not
  // what bounds this form: the nine chains are.  Measured (tools/batch_size_sweep.py, level-0 batch of 1081-beam scans, us per
  // launch, teams -> one wavefront per scan + chain wavefront): 16 scans 46.7 -> 36.3, 1024: 80.3 -> 37.1, 2048: 92.4 -> 39.3,
  // 3072: 134.5 -> 48.6, 3584: 135.9 -> 60.7 (without the chain wavefront).
  // (hsm_match's single scans stay on the team form: it stops its chain at the scan's last beam and keeps the endpoints in
  // registers -- 1081 beams 94 vs 92 us per call, 720 beams 74 vs 90, 360 beams 51 vs 59 through the chain-wavefront form)
  // Longer scans (rows beyond the seventeenth stream from memory in every step, one dependent round trip per row): still one
  // wavefront per scan once the batch has more scans than the device has CUs -- 2162-beam scans, 1024 / 3072 per launch: 83 / 117 us
  // against 154 / 258 for the teams; 3243 beams: 140 / 195 against 228 / 381; up to 256 scans the 16-wavefront teams are as fast
  // or faster (110-121 against 122) -- and dense scans (>= exact_dense_min beams) keep their one-workgroup-per-scan form below.
  const bool dense = s.exact_dense && s.max_n >= s.exact_dense_min;
  if (wps > 1 && s.wps_override == 0 && exact_cached_ok && s.exact_chain_wave &&
      (s.max_n <= 17 * 64 || (s.batch > s.compute_units && !dense)))
    wps = 1;
  // exact order, a team of wavefronts per scan, and nobody asked for that width: the one-workgroup-per-scan forms may take the launch
  const bool free_team = s.exact && wps > 1 && s.wps_override == 0;

  if (free_team && dense) {
    // reference order, launches that cannot fill the chip with one wavefront per scan (single scans, small batches): one wavefront
    // adds, fifteen produce one round ahead of it (gn_match_exact_dense_kernel, gn_match_dense.h) -- a 16 k-beam match of configs[4] in
    // 0.9 instead of 1.2 ms, the nine chains' own 16 384 x 14 x 8.5 cycles being 0.8
    // Round 6, opt-in (HSM_EXACT_SPEC=1): the speculative-carry form (gn_match_spec.h) -- the same sums bit for bit, the chains cut
    // into segments that run in parallel -- whenever the host knows a true bound of the scan lengths (its product scratch is sized
    // from it).  The shift rule accepts ~97 % of the segments of real chains, but on ONE CU the form is bound by what it moves
    // (16 k texel lines + 1.2 MB of products per GN step through one L1) and by a lone workgroup's ~2 us per dependent load: 2.8 ms
    // per 16 k-beam match against 0.9 for the literal chain (profiles/r06/README.md).  A launch into a graph capture takes the
    // literal form, which needs no scratch; so does the launcher where it has no scratch block left for the stream (a ninth stream).
    const bool spec = s.exact_spec && s.n_bound > 0 && s.max_n <= s.n_bound && !s.capturing;
    p.family = spec ? Family::kSpec : Family::kExactDense;
    p.wps = 16, p.spb = 1, p.block = 1024, p.grid = s.batch;
    // the producers-ahead form keeps a scan of at most two of its rounds in registers; the speculative-carry form re-reads the
    // endpoints in every GN step
    p.reads_scan_once = !s.exact_spec && s.max_n <= 2 * kDenseRound;
    detail::finish(p, spec ? "gn_match_spec_kernel" : "gn_match_exact_dense_kernel", false);
    return p;
  }
  // Does the matcher read the endpoints of a single scan exactly ONCE?  Then they can stay in pinned, device-mapped host memory
  // (no H2D copy command in front of the kernel); otherwise -- re-read in every GN step -- they must live in device memory.
  //   tree summation: the register-resident forms, unless the multi-workgroup dense matcher takes the scan;
  //   reference order (round 5): the team form keeps a scan of at most kExactGroupRounds rounds in registers across all levels and
  //     steps (gn_match_kernel: xq_resident) -- every single scan below the dense threshold
  p.reads_scan_once = s.exact ? s.max_n <= kExactGroupRounds * 64 * wps
                              : s.max_n <= kMaxRegisterResidentBeams && s.bpl_override != 0 && !coop_wanted;
  // one scan of the node's size through hsm_match, reference order: the on-chip speculative-carry form (gn_match_spec.h)
  if (free_team && s.exact_spec1 && s.batch == 1 && !s.batched && s.n_bound > 0 && s.max_n <= s.n_bound && s.max_n <= kSpec1MaxBeams) {
    p.family = Family::kSpec1;
    p.wps = 16, p.spb = 1, p.block = 1024, p.grid = 1;
    detail::finish(p, "gn_match_spec1_kernel", false);
    return p;
  }
  if (wps > 1) {  // a team of wavefronts per scan, one scan per workgroup
    const int per_lane = (s.max_n + 64 * wps - 1) / (64 * wps);
    // (two beams per lane: only one-wavefront teams get there by themselves -- choose_wps keeps ~5 beams per lane -- so wider
    // teams, reachable through an explicit waves_per_scan only, share the three-beam instantiation)
    const int bpl = s.exact || s.bpl_override == 0 || per_lane > 17 ? 0 : per_lane <= 3 ? 3 : per_lane <= 5 ? 5 : per_lane <= 9 ? 9 : 17;
    detail::plan_team(s, p, wps, 1, bpl);
    return p;
  }
  const int per_lane = (s.max_n + 63) / 64;
  if (exact_cached_ok) {
    detail::plan_exact_cached(s, p);
    // More than one generation of workgroups (four per CU) with a remainder that the chain-wavefront form takes: the whole
    // generations go out in round 3's form, the remainder behind them in its own launch -- 5000 scans: 57 + 36 us instead of the
    // 104 a single launch takes (its last, part-filled generation runs ~47 us in the rotating-owner form).
    const int groups = (s.batch + 3) / 4, full = 4 * s.compute_units, rest = groups % full;
    if (s.exact_chain_wave && s.exact_split_tail && groups > full && rest > 0 &&
        (rest <= 2 * s.compute_units || (rest <= 3 * s.compute_units && !level0_outgrows_l2(s.level0_cells)))) {
      const int tail = s.batch - (groups - rest) * 4;
      const MatchPlan pa = plan_split_part(s, tail, false), pb = plan_split_part(s, tail, true);
      p = pa;
      p.tail_batch = tail;
      p.name = "gn_match_exact_cached_kernel + its chain-wavefront form for the last, part-filled generation";
      p.record[2] = 256;  // (hsm_last_launch_config describes the first launch; its grid counts both)
      p.record[3] = pa.grid + pb.grid;
    }
    return p;
  }
  // maps whose touched region outgrows the L2s: EIGHT consecutive scans per workgroup instead of four -- with the
  // per-beam workgroup barrier (MatchParams::wg_sync) eight waves share the texel lines in the CU's L1 (4096^2
  // pyramid: 132.8 -> 129.1 us; 16 per workgroup: 133 us; no effect on the 2048^2 workloads, which keep four)
  const bool eight = s.spb_large == 8 && level0_outgrows_l2(s.level0_cells) && !s.exact && s.texel_cache && throughput &&
                     s.bpl_override != 0 && per_lane > 5 && per_lane <= 17;
  const int bpl = s.exact || s.bpl_override == 0 || per_lane > 17 ? 0
                  : per_lane <= 2 ? 2 : per_lane <= 3 ? 3 : per_lane <= 5 ? 5 : per_lane <= 9 ? 9 : 17;
  detail::plan_team(s, p, 1, eight ? 8 : 4, bpl);
  return p;
}

}  // namespace hsm_plan
