// hsm_ctx.h -- the context of libhector_mi355.so as its translation units see it: the pyramid level, hsm_ctx, and the launch
// entry points the units implement for each other.  Internal (not installed): the public boundary is include/hector_mi355/capi.h.
// The units, and behind "=>" the members of hsm_ctx each one owns (tests/test_ctx_ownership.py has who else reaches into them):
//   hector_mi355.hip        the core: the context's life cycle and settings, the error text, the views of a level and the stream
//                           hand-over around map updates: host code only, no kernel in its include closure  => cfg, order
//   match.hip               the matcher's front door: every match, score, batch-covariance (hsm_covariance_batch*,
//                           hsm_match_cov_batch_device) and select entry, the plan of a launch and its record,
//                           the single-scan path, and the one-workgroup-per-scan and multi-workgroup matcher forms
//                           (gn_match_dense.h, gn_match_spec.h, score_kernels.h); the other forms it dispatches to the two
//                           match_* units below  => single, batch, last, retained
//   map_update.hip          every writer of the map by scans: the update entries, the movement gate, the device SLAM scan loop and
//                           the level maintenance the other units reach through this header (map_update.h, map_update_scans.h;
//                           behind them update_types.h, update_cell_rule.h, update_gate.h)  => upd
//   ingest.hip              raw sensor data: the LaserScan / point-cloud conversions of one scan and of batches, in front of
//                           the match, the update and the SLAM loop (ingest_kernels.h)  => ingest
//   occupancy.hip           a level as the node's occupancy grid, whole or its changed cells only (occupancy_kernels.h), and as
//                           what the map's consumers draw from: the hull of its known cells, a cell box as a y-flipped byte
//                           image and windows of that image around batches of poses (map_image_kernels.h)  => occ
//   probes.hip              the host-array probes (likelihood, covariance, Hessian), level downloads and uploads,
//                           the hsm_debug_* test hooks, and the kernels only these launch (probe_kernels.h)  => d_cells
//   rays.hip                what a laser would see on a level: ray distances of arrays of rays (host or device pointers) and
//                           expected scans cast from batches of poses (ray_kernels.h)
//   map_copy.hip            a pyramid, or one cell box per level, copied from another context's planes on the device
//                           (map_copy_kernels.h; the box arithmetic: map_copy_box.h), and another context's pyramid merged into
//                           this one under a rigid transform (map_merge_kernels.h; its host arithmetic: map_merge_box.h)  => copy
//   map_shift.hip           the window moved under the robot: every level's contents shifted by whole cells inside their own
//                           planes, the geometry re-derived for other start coordinates (map_shift_kernels.h; the plan:
//                           map_shift_plan.h)
//   window.hip              a window of poses around a centre scored on the device map, its K best, and the relocalisation chain
//                           behind them, for one scan and for a batch of scans in a window each (window_kernels.h; the
//                           window's arithmetic and the workspace layouts: window_grid.h); a level's occupied cells as
//                           a point set (map_points_kernels.h) and, with both, another context's map aligned to this one
//   group.hip               the multi-GPU group (hsm_group_*, hsm_shard_bounds): host code only, librccl opened on demand
//   match_exact_cached.hip  the exact-order texel-cache batch forms (gn_match_exact.h: the headline kernel and its chain-wavefront forms)
//   match_teams.hip         the team forms (gn_match_kernel, 1..16 wavefronts per scan: gn_match_teams.h) and the fast texel-cache
//                           forms (gn_match_cached.h)  => batch's perm_bufs
//   pose_exchange.hip       the device-side gather of sharded results
// This header sees the matcher's TYPES only (match_types.h): a kernel header is included by the unit that launches its kernels,
// the device primitives they share are in beam_sample.h, gn_step.h and texel_cache.h.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "hector_mi355/capi.h"
#include "hsm_host.h"
#include "match_plan.h"
#include "match_types.h"
#include "settings.h"
#include "stage_layout.h"

namespace hsm {
struct BeamRec;  // update_types.h.  The update kernels (map_update.h, map_update_scans.h) are not templates, so map_update.hip
                 // includes the update headers and no other unit does: whatever launches one of their kernels lives there
struct LevelRW;  // map_cells.h
struct UpdateBatch;  // update_types.h
struct GateState;    // map_update_scans.h
}

namespace hsm_host {

using namespace hsm;

// d_small / h_small layout (floats): [0,3) begin pose | [3,6) out pose | [6,15) out cov |
// [16,28) eval H,dTr | [kTraceOff, kTraceOff + 12 * max steps) per-step trace
constexpr int kTraceOff = 64;
constexpr int kDoneFlagOff = 32;  // one word of the pinned block: single-scan completion sequence number
constexpr int kErrFlagOff = 33;   // the next word: receives that number when the cooperative matcher's exchange timed out
constexpr int kMaxTraceSteps = 6 + 4 * (HSM_MAX_LEVELS - 1);
constexpr int kSmallFloats = kTraceOff + 12 * kMaxTraceSteps;

struct Level {
  int sx = 0, sy = 0;
  float cell_length = 0.f, scale_to_map = 0.f;
  float limx = 0.f, limy = 0.f;
  Affine2 mapTworld{}, worldTmap{};
  // device planes
  float* d_logodds = nullptr;
  int* d_update_index = nullptr;
  float* d_prob = nullptr;
  float4* d_quad = nullptr;
  unsigned int* d_key_free = nullptr;
  unsigned int* d_key_occ = nullptr;
  unsigned int* d_occ_bits = nullptr;
  unsigned char* d_free_bytes = nullptr;  // dense scans: crossed-cell byte map in 16 x 8-cell tiles (map_update.h)
  // GridMapLogOddsFunctions (GridMapLogOdds.h:200-203)
  float log_odds_free = 0.f, log_odds_occ = 0.f;
  // OccGridMapBase counters / GridMapBase::lastUpdateIndex
  int curr_update_index = 0, curr_mark_occ = -1, curr_mark_free = -1, last_update_index = -1;
  // the largest stamp hsm_upload_level last restored, -1 = none (hsm_reset).  While it is ahead of curr_update_index the
  // apply passes run their stamp-aware form (map_update.h "stored stamps"); kernels only ever store stamps below the counter
  int uploaded_stamp_max = -1;
  bool stamps_ahead() const { return uploaded_stamp_max > curr_update_index; }
  unsigned int serial = 0;  // key-plane generation (map_update.h)
  int bbox[4] = {0, 0, -1, -1};   // cell box touched by the last update
  int dirty[4] = {0, 0, -1, -1};  // union of those boxes since hsm_take_dirty_bbox was last called
  int pub[4] = {0, 0, -1, -1};    // the host's share of the publish box: the same union since the level was last exported (hsm_occupancy_changes*)
  int key_rows[2] = {0, -1};      // rows that carry keys of the current key generation (union of the boxes since the planes were last cleared)
  bool marks_pending = false;     // a mark pass was queued on this level and its apply pass has not been (scrub_marks)
  size_t cells() const { return (size_t)sx * sy; }
  int tiles_x() const { return (sx + 3) / 4; }
  int quad_texels() const { return sx * sy; }
};

// what brings level-0 end points to level l: static_cast<float>(1.0 / pow(2.0, level)) -- a power of two, exact in fp32
inline float level_factor(int l) { return (float)(1.0 / pow(2.0, (double)l)); }

inline void affine_apply_host(const Affine2& a, float x, float y, float& ox, float& oy) {
  ox = a.t0 + (a.l00 * x + a.l01 * y);
  oy = a.t1 + (a.l10 * x + a.l11 * y);
}

// the level's own OccupancyGrid metadata, as the node publishes it (HectorMappingRos.cpp:546-553), in fp32: origin =
// getWorldCoords(Vector2f::Zero()) - cell / 2 per axis, resolution = the cell length.  From the level's CURRENT transform: a
// window move (hsm_shift_map) moves the origin.  What hsm_cast_scans* (rays.hip) and hsm_map_tiles* (occupancy.hip) locate poses by
struct GridMetadata {
  float origin_x, origin_y, resolution;
};
inline GridMetadata level_grid_metadata(const Level& L) {
  float wx, wy;
  affine_apply_host(L.worldTmap, 0.0f, 0.0f, wx, wy);
  const float half = L.cell_length * 0.5f;
  return {wx - half, wy - half, L.cell_length};
}

// Teardown never stops at a failing call (everything else still has to be released), but it must not swallow one either: HIP
// keeps the last failure per thread, and the next hipGetLastError() of an unrelated call -- the launch check of the next
// hsm_create on this thread -- would report it as its own.  The first failing call is kept for hsm_last_error(), the runtime's
// per-thread state is cleared at the end (hsm_destroy).
struct TeardownLog {
  std::string first;
  void note(const char* what, hipError_t e) {
    if (e == hipSuccess || !first.empty()) return;
    first = std::string(what) + ": " + hipGetErrorString(e);
  }
};
#define TEARDOWN(log, expr) \
  do {                      \
    hipError_t e__ = (expr); \
    if (log) (log)->note(#expr, e__); \
  } while (0)

// One block that grows on demand and never shrinks: device memory, pinned host memory, or pinned host memory the device reads
// and writes in place.  Growing REPLACES the block (the contents go, and a free waits for queued work that still reads it), so
// a caller that must wait for a stream first, or has state tied to the old block, asks holds() before it reserves.
enum BufKind : unsigned char { kBufDevice, kBufPinned, kBufPinnedMapped };

struct GrowBuf {
  void* p = nullptr;
  size_t bytes = 0;
  BufKind kind = kBufDevice;
  hipError_t free_block() { return kind == kBufDevice ? hipFree(p) : hipHostFree(p); }
  int drop() {  // (a failing free leaves the block as it was)
    if (p) HIP_TRY(free_block());
    p = nullptr;
    bytes = 0;
    return HSM_OK;
  }
  int replace(size_t want_bytes) {  // null and empty after a failure
    if (int rc = drop()) return rc;
    if (kind == kBufDevice)
      HIP_TRY(hipMalloc(&p, want_bytes));
    else
      HIP_TRY(hipHostMalloc(&p, want_bytes, kind == kBufPinned ? hipHostMallocDefault : hipHostMallocMapped));
    bytes = want_bytes;
    return HSM_OK;
  }
  void release(TeardownLog* log) {
    if (p) TEARDOWN(log, free_block());
    p = nullptr;
    bytes = 0;
  }
};

// ... of elements T (char: a block carved by the byte).  `owner`: the list its context releases at teardown (hsm_ctx::bufs)
template <class T>
struct Buf : GrowBuf {
  Buf() = default;
  explicit Buf(std::vector<GrowBuf*>* owner, BufKind k = kBufDevice) {
    kind = k;
    owner->push_back(this);
  }
  operator T*() const { return static_cast<T*>(p); }
  size_t count() const { return bytes / sizeof(T); }
  bool holds(size_t n) const { return n * sizeof(T) <= bytes; }
  int reserve(size_t n, Growth g = kExact) { return holds(n) ? HSM_OK : replace(grown_capacity(n, g) * sizeof(T)); }
};

// true while the caller captures `s` into a graph (the null stream never is): what is launched then runs at the caller's replays,
// so it may neither read nor change per-stream state that eager launches rewrite or free
inline bool stream_capturing(hipStream_t s) {
  if (s == nullptr) return false;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cs) != hipSuccess) {
    (void)hipGetLastError();  // (a stream the caller destroyed: not capturing)
    return false;
  }
  return cs != hipStreamCaptureStatusNone;
}

// The copies of a host-array entry's staging block (stage_layout.h StagePlan) whose regions start at `base`, queued on `s`:
// every host array in, ahead of the entry's first launch ...
inline int stage_copy_in(const StagePlan& st, char* base, hipStream_t s) {
  for (int i = 0; i < st.n; ++i)
    if (st.r[i].src && st.r[i].bytes)
      HIP_TRY(hipMemcpyAsync(base + st.r[i].off, st.r[i].src, st.r[i].bytes, hipMemcpyHostToDevice, s));
  return HSM_OK;
}
// ... and every result out, behind its last one (the entry then waits for `s` once)
inline int stage_copy_out(const StagePlan& st, char* base, hipStream_t s) {
  for (int i = 0; i < st.n; ++i)
    if (st.r[i].dst && st.r[i].bytes)
      HIP_TRY(hipMemcpyAsync(st.r[i].dst, base + st.r[i].off, st.r[i].bytes, hipMemcpyDeviceToHost, s));
  return HSM_OK;
}
// The same two walks for a block in pinned, device-mapped host memory, which the kernels read and write where it lies: host copies,
// the second one once the caller has waited for the stream
inline void stage_fill_host(const StagePlan& st, char* base) {
  for (int i = 0; i < st.n; ++i)
    if (st.r[i].src && st.r[i].bytes) memcpy(base + st.r[i].off, st.r[i].src, st.r[i].bytes);
}
inline void stage_drain_host(const StagePlan& st, const char* base) {
  for (int i = 0; i < st.n; ++i)
    if (st.r[i].dst && st.r[i].bytes) memcpy(st.r[i].dst, base + st.r[i].off, st.r[i].bytes);
}
// the device address of a region; the three-argument form: null where the host array it stands for is absent
template <class T>
T* staged(char* base, size_t off) {
  return reinterpret_cast<T*>(base + off);
}
template <class T>
T* staged(char* base, size_t off, const void* host) {
  return host ? reinterpret_cast<T*>(base + off) : nullptr;
}

}  // namespace hsm_host

using hsm_host::Level;
using hsm::BeamRec;
using hsm::UpdateBatch;
using hsm::SpecStats;
using hsm::kLayoutQuad;

using hsm_host::Buf;
using hsm_host::kBufPinned;
using hsm_host::kBufPinnedMapped;

// The context.  What every unit may use stands at the top; the rest is grouped into member structs by the unit that owns the state,
// each under a comment that names it.  Which units reach into which member is pinned by tests/test_ctx_ownership.py: a new
// cross-unit reach fails there until it is written into that table.  A member with Buf fields starts with the owner list, so that
// its blocks enrol in hsm_ctx::bufs as they are constructed.
struct hsm_ctx {
  using Bufs = std::vector<hsm_host::GrowBuf*>;
  // ---- shared by every unit ----------------------------------------------------------------------------------------------------
  Bufs bufs;  // every Buf member below enrols here as it is constructed: hsm_destroy releases these
  int device = 0;
  int compute_units = 256;   // of this device (hsm_create)
  hsm_host::Settings cfg;    // what hsm_opts and the environment set at hsm_create, and the hsm_set_* entries since (settings.h)
  std::vector<hsm_host::Level> levels;
  float start[2] = {0.5f, 0.5f};  // the start coordinates the levels' transforms derive from (hsm_create, hsm_shift_map)
  mutable std::mutex mu;
  hipStream_t stream = nullptr;
  // scratch of whichever entry holds the mutex: single-scan staging (device) ...
  Buf<float2> d_scan{&bufs};
  // ... and batch staging for the host-pointer convenience entries
  Buf<char> d_batch{&bufs};

  // ---- hector_mi355.hip (the core) ---------------------------------------------------------------------------------------------
  // ordering between the context's stream (updates) and caller-owned streams (hsm_match_batch_device):
  // per caller stream the update epoch it has been ordered behind, and whether it may still run a match
  struct ForeignStream {
    hipStream_t s;
    unsigned long long ordered_epoch;
    bool pending;
  };
  struct Order {
    std::vector<ForeignStream> foreign;
    unsigned long long upd_epoch = 1;
    hipEvent_t evt_updates = nullptr, evt_foreign = nullptr;
    hipEvent_t evt_inputs = nullptr;     // the caller's stream at hsm_update_by_scans_device: its inputs are complete
    hipEvent_t evt_slam_done = nullptr;  // the context's stream at the end of hsm_slam_scans_device: the caller's stream waits for it
  } order;

  // ---- match.hip: the single-scan path -----------------------------------------------------------------------------------------
  struct Single {
    Bufs* bufs;
    float* d_small = nullptr;   // layout: top of this header
    float* h_small = nullptr;   // pinned mirror of d_small
    unsigned done_seq = 0;
    // single-scan fast path: endpoints staged in pinned, device-mapped host memory and read by the
    // matcher ONCE (they stay in VGPRs); results written by the kernel straight into h_small
    Buf<float2> h_scan_pinned{bufs, kBufPinnedMapped};
    // the upload of a dense scan for matchData runs on its own stream, into the OTHER of two device buffers, from a pinned
    // staging block: it overlaps the update kernels still queued on `stream` (which read the buffer of the scan before)
    // instead of waiting behind them; the match kernel waits for the copy's event (stage_scan_overlapped)
    Buf<float2> d_retained_alt{bufs};
    hipStream_t copy_stream = nullptr;
    hipEvent_t copy_evt = nullptr;
    Buf<float2> h_copy_pinned{bufs, kBufPinned};
    unsigned coop_bar_base = 0;   // value the grid-barrier counter has when the next cooperative launch starts
    float* d_partials = nullptr;  // [2][64][9] per-workgroup partial sums of gn_match_coop_kernel
    int coop_mute_block = 0;      // hsm_debug_set_coop_mute (test hook)
    unsigned coop_fallbacks = 0;  // dense single-scan matches re-run on one workgroup after an exchange timeout (match_single)
    // ... and the back-off that follows: after a timeout the multi-workgroup form is skipped for the next coop_skip matches (1, 2, 4, ...
    // up to 1024, reset by the first exchange that completes) -- on a device another process keeps busy every dense match would
    // otherwise pay the full bounded wait, a host spin and a second launch (round-5 advisor)
    unsigned coop_skip = 0, coop_backoff = 0;
  } single{&bufs};

  // ---- match.hip, match_teams.hip, match_exact_cached.hip: the batched entries --------------------------------------------------
  // One permutation buffer per stream that has launched a sorted batch (launches on one stream are ordered; a ninth stream keeps the
  // caller's order)
  struct PermBuf {
    hipStream_t s;
    Buf<int> d;  // (not enrolled: hsm_destroy walks perm_bufs)
    int batch;  // the batch size the permutation in `d` was computed for (0: none)
    int used;   // launches it has served
  };
  // gn_match_spec_kernel: products of every beam, [batch][stride] float4s -- one block per stream that has launched the form
  // (launches on one stream are ordered; a ninth stream, and any launch into a graph capture, take the literal dense form)
  struct SpecScratch {
    hipStream_t s;
    Buf<float4> d;  // (not enrolled: hsm_destroy walks spec_scratch)
  };
  struct Batch {
    Bufs* bufs;
    // the shared-scan form of the host-pointer entry (pose hypotheses of ONE scan): start poses, results and the scan in pinned, device-mapped host
    // memory -- the kernel reads each start pose once and writes each result once, straight over PCIe, no copy command either way
    Buf<char> h_hyp_pinned{bufs, kBufPinnedMapped};
    std::vector<PermBuf> perm_bufs;
    std::vector<SpecScratch> spec_scratch;
    SpecStats* d_spec_stats = nullptr; // hsm_debug_spec_stats
    unsigned long long* clock_probe = nullptr;  // hsm_set_clock_probe
    int sched_level = -1;         // hsm_debug_set_schedule (test hook): batched entries run `sched_level` only, -1 = the full schedule
    int sched_steps = 0;          //   ... with this many GN steps
    bool fused_exchange_done = false;  // the last launch_match carried MatchParams::xp itself (else the caller launches the exchange step)
  } batch{&bufs};

  // ---- the launch record: written by whichever unit launches a matcher or scorer (match.hip, match_teams.hip, rays.hip, window.hip) ----
  struct Last {
    int last_cfg[6] = {0, 0, 0, 0, 0, 0};  // MatchPlan::record of the last match launch (record_launch)
    const char* last_kernel = "";  // name of the matcher kernel the last launch used (hsm_last_launch_kernel)
    int last_parity = HSM_PARITY_FAST;  // the mode the last match launch actually ran in (hsm_last_launch_parity)
    bool last_sorted = false;
  } last;

  // ---- the hand-over between matchData (match.hip) and updateByScan (map_update.hip) ---------------------------------------------
  struct Retained {
    Bufs* bufs;
    // retained scan = MapRepMultiMap::dataContainers (level-0 units; scaled by 2^-l on use)
    std::vector<float> retained_pts;
    float retained_origo[2] = {0.f, 0.f};
    bool retained_valid = false;  // false until the first match (reference: empty containers)
    Buf<float2> d_retained{bufs};
    bool d_retained_current = false;
  } retained{&bufs};

  // ---- map_update.hip -----------------------------------------------------------------------------------------------------------
  struct Update {
    Bufs* bufs;
    Buf<BeamRec> d_beam_recs{bufs};  // dense scans: per-beam records of all levels (update_types.h BeamRec), [HSM_MAX_LEVELS][count() / HSM_MAX_LEVELS]
    // hsm_update_by_scans_device: one UpdateBatch and one cell box per level for every scan of a call, filled on the device
    // (map_update_scans.h update_prep_kernel); grown outside capture.  boxes: slot 0 the levels' running dirty boxes, slot 1 the last scan's
    Buf<UpdateBatch> d_upd_batches{bufs};
    Buf<int> d_upd_boxes{bufs};  // allocated last: non-null = both blocks serve d_upd_batches.count() scans
    bool upd_boxes_outstanding = false;  // device-side updates since the host last merged their boxes into Level::bbox / dirty
    // the movement gate of HectorSlamProcessor::update (update_gate.h; map_update_scans.h update_gate_prep_kernel): its state and the
    // count of updates it let through live on the device -- the host never learns a gated call's decisions.  Whoever needs
    // Level's update counters on the host first waits for the stream and folds that count in (fold_gate_counters), like the boxes
    hsm::GateState* d_gate = nullptr;
    float gate_min_dist = 0.4f, gate_min_angle = 0.13f;  // HectorSlamProcessor.h:62-63 (hsm_set_update_gate)
    bool gate_outstanding = false;       // gated calls since the host last folded their count into the levels' counters
    long long gate_applied_total = 0;    // updates of gated calls folded so far, since hsm_create
    // updateByScan returns when its kernels are QUEUED (Settings::Update::async_update): everything
    // that reads the map afterwards is ordered behind them on `stream`.  Host endpoints are staged in one of
    // two pinned blocks (h_upd_pinned), each guarded by the event of the update that last read it.
    Buf<char> d_upd_stage{bufs};        // hsm_update_by_scans: poses, offsets and end points of the host arrays
    Buf<float2> h_upd_pinned[2] = {Buf<float2>{bufs, kBufPinnedMapped}, Buf<float2>{bufs, kBufPinnedMapped}};
    hipEvent_t upd_evt[2] = {nullptr, nullptr};
    bool upd_busy[2] = {false, false};
    int upd_slot = 0;
    bool queued_update = false;  // an asynchronous updateByScan was queued on `stream` since the host last saw it drained
  } upd{&bufs};

  // ---- ingest.hip ---------------------------------------------------------------------------------------------------------------
  // sensor geometries of hsm_match_batch_ranges*: one immutable float2 table per (n, angle_min bits, angle_increment bits),
  // never rewritten and freed by hsm_destroy only (a queued or captured launch may read it any time before)
  struct RangesGeometry {
    int n;
    unsigned a0_bits, inc_bits;
    float2* d;
  };
  // the same for hsm_ingest_batch_ranges_tf_device / hsm_match_batch_ranges_tf: laser_geometry's double2 unit vectors
  struct RangesTfGeometry {
    int n;
    unsigned a0_bits, inc_bits;
    double2* d;
  };
  struct Ingest {
    Bufs* bufs;
    // ingested scan (hsm_ingest_laser_scan): device container + host copy, sensor trig table cache
    // (the three blocks hold d_ingest.count() beams; d_ranges: 3 floats per beam and the survivor count behind them)
    Buf<float> d_ranges{bufs};
    Buf<double2> d_trig{bufs};       // float2 (running-angle table) or double2 (laser_geometry unit vectors)
    int trig_kind = -1;
    float ingest_origo[2] = {0.f, 0.f};
    Buf<float2> d_ingest{bufs};      // allocated last: non-null = the trio is complete
    std::vector<float> h_ingest;      // endpoints as the matcher/updater see them (host copy)
    int ingest_n = -1;                // -1 = nothing ingested yet
    float trig_a0 = 0.f, trig_inc = 0.f;
    int trig_n = -1;
    std::vector<RangesGeometry> ranges_geoms;
    std::vector<RangesTfGeometry> ranges_tf_geoms;
    Buf<char> d_rbatch{bufs};  // hsm_match_batch_ranges: start poses, results, counts and the workspace of its device call
  } ingest{&bufs};

  // ---- occupancy.hip ------------------------------------------------------------------------------------------------------------
  struct Occupancy {
    Bufs* bufs;
    Buf<signed char> d_occ{bufs};    // occupancy export staging
    // the published grid (occupancy_kernels.h occupancy_prep_kernel), three rows of kMaxLevels boxes in a block of their own that no
    // growing buffer replaces: the levels' publish boxes as device-side updates widen them (never fetched), the box of the export
    // that was queued last on each level (its convert launch reads it), and the whole level as a box (written by hsm_create)
    int* d_pub_boxes = nullptr;
    // hsm_map_extents* (map_image_kernels.h): the four accumulators of the reduction, which every call leaves as it found them
    // (filled by hsm_create), and behind them the four ints the host form fetches its box from
    int* d_extents = nullptr;
  } occ{&bufs};

  // ---- map_copy.hip, map_shift.hip ----------------------------------------------------------------------------------------------
  struct Copy {
    Bufs* bufs;
    // hsm_copy_map*, hsm_merge_map (map_copy.hip).  As the destination: the staging patch of the cross-device route (4-byte elements,
    // laid out by map_copy_box.h copy_patch_at; a merge stages log-odds only, one padded box per level), and the event on the own stream behind the last read of the source, which the source's
    // stream waits for.  As the source: the event on the own stream the destination's stream waits for.
    Buf<float> d_copy_patch{bufs};
    hipEvent_t evt_copy_read = nullptr, evt_copy_src = nullptr;
  } copy{&bufs};

  // ---- probes.hip ---------------------------------------------------------------------------------------------------------------
  Buf<char> d_cells{&bufs};  // interleaved {logodds, updateIndex} staging for hsm_download_cells
};

namespace hsm_host {

using hsm_plan::MatchPlan;

// What a gated update adds to an update call (update_by_scans_device_nolock of map_update.hip; map_update_scans.h UpdateGateParams)
struct GateCall {
  const unsigned char* d_force = nullptr;
  int* d_out_applied = nullptr;
  bool slam = false;  // hsm_slam_scans_device's call for one scan: see UpdateGateParams
  float* pose_io = nullptr;
  float* cov_io = nullptr;
  const float* next_delta = nullptr;
};

// The posed scans of an update call, filled once by the entry and passed down: CSR scans (`d_offsets`) or one scan of `shared_n`
// beams at every pose; `origo` the host pair for every scan (null: zero) or `d_origos` [count * 2] on the device.  The first six
// fields are in the order of the C ABI: an entry initialises them with braces and names the rest.
struct PosedScans {
  int count = 0;
  const float* d_poses = nullptr;
  const float* d_pts = nullptr;
  const int* d_offsets = nullptr;
  int shared_n = 0, max_beams = 0;
  const float* origo = nullptr;
  const float* d_origos = nullptr;
  const GateCall* gate = nullptr;                   // the gated entries
  const char* who = "hsm_update_by_scans_device";  // the entry the caller used, for the error texts
};

// A batch of (pose, scan) pairs on the device, filled once by the entry and passed down: CSR scans (`d_offsets`) or one scan of
// `shared_n` beams at every pose.  The fields of this and the next bundles are in the order of the C ABI: an entry initialises
// them with braces.
struct ScanBatch {
  int batch = 0;
  const float* d_poses = nullptr;  // the start poses of a match, the poses to score otherwise
  const float* d_pts = nullptr;
  const int* d_offsets = nullptr;
  int shared_n = 0;  // without offsets: the beams of the one scan; with them: the matcher's sizing hint, nothing to the other kernels
  bool bad_shape() const { return batch < 0 || (!d_offsets && shared_n < 0); }
  bool points_missing() const { return batch > 0 && !d_pts && !d_offsets && shared_n > 0; }  // a scan that has beams, and no points
  int kernel_shared_n() const { return d_offsets ? 0 : shared_n; }                            // what a kernel that takes no hint receives
  ScanBatch at(const float* d_other) const { return {batch, d_other, d_pts, d_offsets, kernel_shared_n()}; }  // ... behind the match
};
// what a batched match adds to its ScanBatch
struct MatchOut {
  float* d_out_pose = nullptr;        // [batch * 3]
  float* d_out_cov = nullptr;         // [batch * 9] or null
  int n_bound = 0;                    // CSR scans: a true bound of every scan's length where the caller has one, else 0
  const ExchangeFused* xp = nullptr;  // hsm_match_batch_device_gather: the exchange step the launch may carry
};
// the outputs of a scoring step; each may be null, not all of them
struct ScoreOut {
  float *d_likelihood = nullptr, *d_residual = nullptr;
  bool none() const { return !d_likelihood && !d_residual; }
};
struct CovOut {
  float *d_cov_world = nullptr, *d_cov_map = nullptr, *d_lh7 = nullptr, *d_likelihood = nullptr;
  bool none() const { return !d_cov_world && !d_cov_map && !d_lh7 && !d_likelihood; }
};
// A scoring step, alone or as the middle of a match chain: the score, or with `covariance` the covariance estimate, of a
// ScanBatch on `level`.  `who`: the entry the caller used, for the error texts
struct ScoringStep {
  int level = 0;
  ScoreOut score;
  CovOut cov;
  bool covariance = false;
  const char* who = "hsm_match_score_batch_device";
  float* likelihood() const { return covariance ? cov.d_likelihood : score.d_likelihood; }  // what a ranking behind it ranks by
  bool no_output() const { return covariance ? cov.none() : score.none(); }
};
// The ranking request behind a scoring step: `groups` groups (0: none) of `group_size` consecutive entries, or CSR
// `group_offsets`.  Device pointers for the device entries, host pointers in match_batch_host of match.hip
struct Ranking {
  int groups = 0;
  const int* group_offsets = nullptr;
  int group_size = 0;
  int* out_index = nullptr;
  float *out_score = nullptr, *out_best_pose = nullptr;  // may be null; the pose in/out (a group without a winner keeps the caller's)
  bool bad_ranking(int batch, const void* lh) const {    // what every match -> scoring step -> winner entry refuses; `lh`: the scores
    return groups < 0 ||
           (groups > 0 && (!lh || !out_index || (!group_offsets && (group_size < 0 || (long long)groups * group_size > batch))));
  }
};

// The scan log of a SLAM call, all on the device: what steers the loop and where its results go.  Scan k's share of every array
// is sliced here and nowhere else.  (Fields in the order the entries initialise them with braces.)
struct ScanLog {
  int count = 0;
  const float* d_start_pose = nullptr;
  const float* d_hint_deltas = nullptr;  // [count * 3] or null
  const unsigned char* d_force = nullptr;  // [count] or null
  float* d_out_pose = nullptr;             // [count * 3]
  float* d_out_cov = nullptr;              // [count * 9] or null
  int* d_out_applied = nullptr;            // [count] or null
  int* d_out_counts = nullptr;             // [count] or null: the raw-scan entries' survivors per scan
  float* pose(int k) const { return d_out_pose + 3 * (size_t)k; }
  float* cov(int k) const { return d_out_cov ? d_out_cov + 9 * (size_t)k : nullptr; }
  GateCall gate(int k) const {  // scan k's gated update: it settles the scan's pose and covariance and leaves the next scan's hint
    GateCall g;
    g.d_force = d_force ? d_force + k : nullptr;
    g.d_out_applied = d_out_applied ? d_out_applied + k : nullptr;
    g.slam = true;
    g.pose_io = pose(k);
    g.cov_io = cov(k);
    g.next_delta = d_hint_deltas && k + 1 < count ? d_hint_deltas + 3 * (size_t)(k + 1) : nullptr;
    return g;
  }
};

// hector_mi355.hip, for the other units: the views of a level, the launch arithmetic, and the hand-over between a caller's stream
// and the context's around queued map updates (the definitions carry the comments).  level_factor and stream_capturing are inline above
int valid_level(const hsm_ctx* h, int level);
int select_device(const hsm_ctx* h);
bool wants_exact(const hsm_ctx* h);
int grid_for(size_t n, int block = 256);
LevelRW level_rw(const Level& L);
LevelView level_view(const Level& L, float pt_scale, int gn_steps);
void whole_level_changed(Level& L, bool mirror = true);
void set_level_transformation(Level& L, float offx, float offy, float cell_length);
int order_after_foreign_match(hsm_ctx* h);
int order_map_reader(hsm_ctx* h, hipStream_t s, const char* who, hsm_ctx::ForeignStream** mark);
int slam_refuse_capture(hsm_ctx* h, hipStream_t s, const char* who);
int wait_for_caller_inputs(hsm_ctx* h, hipStream_t s);
int slam_caller_waits(hsm_ctx* h, hipStream_t s);

// The bracket of a launch on `s` that reads the map: begin() orders it behind the map updates queued so far and can fail;
// queued(), once the launch is on the stream, leaves the mark the next update waits for -- without it that update runs under the
// reader.  `mark_now`: marked in begin() already, so that a call of several launches that fails half way leaves the next writer
// behind what it did queue.  `mark`: null where nothing is to be remembered (the context's own stream; a capture)
struct MapReader {
  hsm_ctx::ForeignStream* mark = nullptr;
  int begin(hsm_ctx* h, hipStream_t s, const char* who, bool mark_now = false) {
    const int rc = order_map_reader(h, s, who, &mark);
    if (rc == HSM_OK && mark_now) queued();
    return rc;
  }
  void queued() { if (mark) mark->pending = true; }
};
// match.hip, for the other units: the batched match behind the raw-scan, group and scan-loop entries ...
int match_batch_device_nolock(hsm_ctx* h, const ScanBatch& B, const MatchOut& M, void* stream);
// ... and the chain match -> `step` at the matched poses -> winners where R.groups > 0, which hsm_relocalize_device of window.hip
// ends in too.  Every argument is checked before the first launch
int match_chain_nolock(hsm_ctx* h, const ScanBatch& B, const MatchOut& M, const ScoringStep& step, const Ranking& R, void* stream);
// map_copy.hip, for window.hip: what two contexts must share for one's map to be merged into, or aligned to, the other's (level
// count, resolution of every level, layout); both locks held
bool merge_compatible(const hsm_ctx* a, const hsm_ctx* b);
// map_update.hip, for the other units: the level maintenance that launches map_update.h's kernels, what an entry does before it
// reads or rewrites a level's boxes and counters on the host, and the device SLAM loop over a scan log
int create_update_state(hsm_ctx* h);
int fill_level(hsm_ctx* h, Level& L);
int reset_update_gate(hsm_ctx* h);
int rebuild_probability(hsm_ctx* h, Level& L);
int scrub_pending_marks(hsm_ctx* h, Level& L);
int merge_device_boxes(hsm_ctx* h);
int fold_gate_counters(hsm_ctx* h, GateState* state = nullptr);
int slam_scans_queue(hsm_ctx* h, const ScanLog& log, const PosedScans& scans);

// f(layout, exact) with the context's texel layout and summation order as types (std::integral_constant<int, kLayout...>,
// std::bool_constant): a generic lambda launches `kernel<layout(), exact()>` and the four sampler forms need no ladder.  A kernel
// that samples in one order only ignores the second argument.
template <class F>
void with_sampler_form(const hsm_ctx* h, F&& f) {
  const bool exact = wants_exact(h);
  if (h->cfg.layout == kLayoutPlane) {
    if (exact) f(std::integral_constant<int, kLayoutPlane>{}, std::true_type{}); else f(std::integral_constant<int, kLayoutPlane>{}, std::false_type{});
  } else {
    if (exact) f(std::integral_constant<int, kLayoutQuad>{}, std::true_type{}); else f(std::integral_constant<int, kLayoutQuad>{}, std::false_type{});
  }
}

// Which form a launch takes is decided once, in match_plan.h (plan_match), by launch_match of match.hip, which also
// keeps the launch record; the other two units only map a plan to their instantiations and launch it.
// match_exact_cached.hip: reference order, batches, one wavefront per scan with the texel cache (Family::kExactCached, kExactCachedCw)
int launch_exact_cached_form(hsm_ctx* h, hsm::MatchParams P, const MatchPlan& plan, hipStream_t stream);
// match_teams.hip: `plan.wps` wavefronts per scan (1, 2, 4, 8, 16), either summation order, and the fast texel-cache form
// (Family::kTeam, kTeamExact, kCached)
int launch_team_form(hsm_ctx* h, const hsm::MatchParams& P, const MatchPlan& plan, hipStream_t stream);
// match_teams.hip: MatchParams::perm for this launch where hsm_set_batch_order asks for it (a sort kernel on `stream` in front of
// the matcher); a launch into a graph capture keeps the caller's order: no graph ever reads a stream's permutation buffer
int ensure_batch_perm(hsm_ctx* h, hsm::MatchParams& P, hipStream_t stream);
// match_teams.hip: batch_order_kernel on `stream`: perm[slot] = scan for `batch` start poses, with level 0's transform
// (hsm_debug_batch_order too)
int launch_batch_order(hsm_ctx* h, const float* begin_world, int batch, int* perm, bool detect, hipStream_t stream);

}  // namespace hsm_host
