// hector_mi355.hip -- the core of the host runtime + C ABI (include/hector_mi355/capi.h) of the
// MI355X-native hector_mapping scan matcher: the context's life cycle, its settings, the error text, the views of a level and the
// stream hand-over around map updates.  Host code only: no kernel is launched here.  The match, score and select entries and the
// plan of a matcher launch are in match.hip, the batch / team matcher forms in match_exact_cached.hip and match_teams.hip, map
// updates and the scan loop in map_update.hip, the
// probes and test hooks in probes.hip, the multi-GPU group in group.hip, raw-scan conversion in ingest.hip, the occupancy exports in
// occupancy.hip (hsm_ctx.h says which unit holds what).
//
// The context mirrors hectorslam::MapRepMultiMap (HSL/slam_main/MapRepMultiMap.h): a
// pyramid of levels, each with its grid (log-odds + update stamps), its world<->map
// transforms (HSL/map/GridMapBase.h:265-280) and the update counters of
// OccGridMapBase (HSL/map/OccGridMapBase.h:264-266).  All planes live in HBM; the
// host keeps only scalars.  There is no CPU compute path.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see build.py).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <string>
#include <vector>

#include "hector_mi355/capi.h"
#include "hsm_ctx.h"
#include "hsm_host.h"
#include "map_cells.h"

namespace {

using namespace hsm;
using namespace hsm_host;

thread_local std::string g_last_error;

}  // namespace

// every object of the library reports through this per-thread text (hsm_host.h)
int hsm_host::fail(int code, const char* what, hipError_t e) {
  char buf[512];
  if (e != hipSuccess)
    snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
  else
    snprintf(buf, sizeof buf, "%s", what);
  g_last_error = buf;
  return code;
}

int hsm_host::fail_at(int code, const char* who, const char* text, hipError_t e) {
  char buf[512];
  snprintf(buf, sizeof buf, "%s%s", who, text);
  return fail(code, buf, e);
}

void hsm_host::set_error_text(const char* text) { g_last_error = text; }

namespace {

float prob_to_log_odds(float prob) {  // GridMapLogOdds.h:196-200 (float log overload)
  float odds = prob / (1.0f - prob);
  return logf(odds);
}

// GridMapBase::setMapTransformation (GridMapBase.h:265-280) with Eigen's evaluation
// order: mapTworld = Scaling(s,s) * Translation(off); worldTmap = mapTworld.inverse()
void set_map_transformation(Level& L, float offx, float offy, float cell_length) {
  L.cell_length = cell_length;
  L.scale_to_map = 1.0f / cell_length;
  const float s = L.scale_to_map;
  Affine2 m;
  m.l00 = s;
  m.l10 = 0.0f;
  m.l01 = 0.0f;
  m.l11 = s;
  m.t0 = s * offx;
  m.t1 = s * offy;
  L.mapTworld = m;
  const float det = m.l00 * m.l11 - m.l10 * m.l01;
  const float invdet = 1.0f / det;
  Affine2 w;
  w.l00 = m.l11 * invdet;
  w.l10 = -m.l10 * invdet;
  w.l01 = -m.l01 * invdet;
  w.l11 = m.l00 * invdet;
  w.t0 = (-w.l00) * m.t0 + (-w.l01) * m.t1;
  w.t1 = (-w.l10) * m.t0 + (-w.l11) * m.t1;
  L.worldTmap = w;
}

}  // namespace

// (declared in hsm_ctx.h: the other units use these too)
namespace hsm_host {

LevelRW level_rw(const Level& L) {
  LevelRW v;
  v.logodds = L.d_logodds;
  v.update_index = L.d_update_index;
  v.prob = L.d_prob;
  v.quad = L.d_quad;
  v.key_free = L.d_key_free;
  v.key_occ = L.d_key_occ;
  v.occ_bits = L.d_occ_bits;
  v.free_bytes = L.d_free_bytes;
  v.sx = L.sx;
  v.sy = L.sy;
  v.tiles_x = L.tiles_x();
  v.kf_tiles_x = key_free_tiles_x(L.sx);
  v.quad_texels = L.quad_texels();
  return v;
}

LevelView level_view(const Level& L, float pt_scale, int gn_steps) {
  LevelView v;
  v.quad = L.d_quad;
  v.prob = L.d_prob;
  v.sx = L.sx;
  v.sy = L.sy;
  v.tiles_x = L.tiles_x();
  v.quad_texels = L.quad_texels();
  v.limx = L.limx;
  v.limy = L.limy;
  v.mapTworld = L.mapTworld;
  v.worldTmap = L.worldTmap;
  v.pt_scale = pt_scale;
  v.gn_steps = gn_steps;
  return v;
}

int grid_for(size_t n, int block) {
  size_t g = (n + block - 1) / block;
  if (g > 256 * 8) g = 256 * 8;  // grid-stride the rest (guide, Guideline 11)
  if (g < 1) g = 1;
  return (int)g;
}

// HSM_PARITY_AUTO (the default): EVERY match -- batched, single scan, dense scan, and the likelihood / covariance / Hessian
// entry points -- takes the reference's summation order: bit-identical to the reference CPU matcher on every entry point.
// History: round 3 chose exact order only on maps of more than 2^23 cells (a rule fitted to BASELINE's own scenes); round 4's scene
// sweep (tools/parity_scene_sweep.py, profiles/r04/parity_scene_sweep.jsonl) found the fast tree beyond 1e-4 m of the reference in
// every scene family for some set-up -- wherever the reference's own Gauss-Newton iteration has not settled -- and no property of
// the map or the batch known at launch separates those scans, so every batch went exact; single scans kept the tree on the evidence
// of 256 scans per family, of which the corridor family already failed (0.83 within 1e-4 m).  Round 5: the same argument holds for
// one scan as for 4096, so the default does not try there either.  HSM_PARITY_FAST / _RELAXED stay opt-in for callers who trade
// the guarantee for speed (profiles/r05/README.md has the prices: batch +34 % / +45 %, single 1081-beam scan ~35 vs ~95 us).
// AUTO and HSM_PARITY_EXACT launch the same kernels today; the distinction kept in the API is one of contract: AUTO promises the
// reference's BITS by whatever form delivers them, EXACT names the reference's order of additions.
// The effective order is an INPUT of the plan (MatchSite::exact) -- the context's flags are never changed by a launch
// (hsm_parity() reads them without the mutex) -- and is recorded for hsm_last_launch_parity().
bool wants_exact(const hsm_ctx* h) { return h->cfg.parity.exact || h->cfg.parity.auto_parity; }

// every cell of the level may have changed (create, reset, upload): host mirrors and the published grid take all of it
void whole_level_changed(Level& L, bool mirror) {
  const int all[4] = {0, 0, L.sx - 1, L.sy - 1};
  for (int k = 0; k < 4; ++k) {
    if (mirror) L.dirty[k] = all[k];
    L.pub[k] = all[k];
  }
}

int valid_level(const hsm_ctx* h, int level) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  if (level < 0 || level >= (int)h->levels.size()) return fail(HSM_ERR_INVALID, "level out of range");
  return HSM_OK;
}

int select_device(const hsm_ctx* h) {
  HIP_TRY(hipSetDevice(h->device));
  return HSM_OK;
}

}  // namespace hsm_host

namespace {

void free_level(Level& L, TeardownLog* log = nullptr) {
  TEARDOWN(log, hipFree(L.d_logodds));
  TEARDOWN(log, hipFree(L.d_update_index));
  TEARDOWN(log, hipFree(L.d_prob));
  TEARDOWN(log, hipFree(L.d_quad));
  TEARDOWN(log, hipFree(L.d_key_free));
  TEARDOWN(log, hipFree(L.d_key_occ));
  TEARDOWN(log, hipFree(L.d_occ_bits));
  TEARDOWN(log, hipFree(L.d_free_bytes));
  L = Level();
}

}  // namespace

namespace hsm_host {

// for map_shift.hip: hsm_create's transforms of a level for other offsets
void set_level_transformation(Level& L, float offx, float offy, float cell_length) { set_map_transformation(L, offx, offy, cell_length); }

// every writer of the map queues behind a batch match that a caller-owned stream may still be running, and
// bumps the epoch the next such match orders itself behind
int order_after_foreign_match(hsm_ctx* h) {
  // Refused, before anything is queued, while a caller's stream that this context has matched on is being captured into a graph:
  // a marker recorded on that stream would go into the capture, and the context's stream, waiting for it, would join the capture.
  for (const hsm_ctx::ForeignStream& f : h->order.foreign)
    if (stream_capturing(f.s))
      return fail(HSM_ERR_INVALID, "map update while a caller's stream that this context matches on is being captured into a graph: "
                                   "end the capture first (the caller orders replays against updates)");
  for (hsm_ctx::ForeignStream& f : h->order.foreign) {
    if (!f.pending) continue;
    // everything the caller has queued on that stream up to now (a superset of our matches); the wait captures
    // the event's state at this call, so one event serves all streams in turn
    if (!h->order.evt_foreign) HIP_TRY(hipEventCreateWithFlags(&h->order.evt_foreign, hipEventDisableTiming));
    if (hipEventRecord(h->order.evt_foreign, f.s) == hipSuccess) {
      HIP_TRY(hipStreamWaitEvent(h->stream, h->order.evt_foreign, 0));
    } else {  // the caller destroyed the stream meanwhile: its work has been flushed or is covered by a device sync
      (void)hipGetLastError();
      HIP_TRY(hipDeviceSynchronize());
    }
    f.pending = false;
  }
  if (h->order.foreign.size() > 16) h->order.foreign.clear();  // nothing pending any more: forget streams callers may have destroyed
  ++h->order.upd_epoch;
  return HSM_OK;
}

// the context's stream behind the caller's: the inputs are complete where `s` stands now
int wait_for_caller_inputs(hsm_ctx* h, hipStream_t s) {
  if (s == h->stream) return HSM_OK;
  if (!h->order.evt_inputs) HIP_TRY(hipEventCreateWithFlags(&h->order.evt_inputs, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(h->order.evt_inputs, s));
  HIP_TRY(hipStreamWaitEvent(h->stream, h->order.evt_inputs, 0));
  return HSM_OK;
}

// the refusals of a scan-log call, before anything is queued: `s` or a stream this context has matched on is being captured
int slam_refuse_capture(hsm_ctx* h, hipStream_t s, const char* who) {
  if (stream_capturing(s))
    return fail_at(HSM_ERR_INVALID, who, ": `stream` is being captured into a graph (map updates are not captured)");
  for (const hsm_ctx::ForeignStream& f : h->order.foreign)  // (order_after_foreign_match)
    if (stream_capturing(f.s))
      return fail_at(HSM_ERR_INVALID, who, ": a caller's stream that this context matches on is being captured into a graph");
  return HSM_OK;
}

// the caller's stream behind the context's (the results are complete where the context's stream stands now)
int slam_caller_waits(hsm_ctx* h, hipStream_t s) {
  if (s == h->stream) return HSM_OK;
  if (!h->order.evt_slam_done) HIP_TRY(hipEventCreateWithFlags(&h->order.evt_slam_done, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(h->order.evt_slam_done, h->stream));
  HIP_TRY(hipStreamWaitEvent(s, h->order.evt_slam_done, 0));
  return HSM_OK;
}

}  // namespace hsm_host

// Orders a launch on `s` that READS the map (a batched match, a batched score, the rays of rays.hip) against the map updates,
// which are queued on the context's own stream.  *mark = the stream's record where the launch has to be remembered for the next
// update (`(*mark)->pending = true` once it is queued), nullptr where nothing is to be remembered (the context's own stream; a
// capture).
int hsm_host::order_map_reader(hsm_ctx* h, hipStream_t s, const char* who, hsm_ctx::ForeignStream** mark) {
  *mark = nullptr;
  if (s == h->stream) return HSM_OK;
  // A caller-owned stream is not ordered against the context's own one, on which map updates are queued
  // (hsm_update_by_scan returns before they ran): order the launch behind the updates queued so far, and
  // leave a marker the next update waits for, so that it does not rewrite the map under a running reader.
  hsm_ctx::ForeignStream* fs = nullptr;
  for (hsm_ctx::ForeignStream& f : h->order.foreign)
    if (f.s == s) fs = &f;
  if (!fs) {
    h->order.foreign.push_back({s, 0ull, false});
    fs = &h->order.foreign.back();
  }
  if (stream_capturing(s)) {
    // A launch into a graph capture runs at the caller's replays, not now: it neither records that the stream is ordered behind
    // the updates nor leaves a marker for the next update (either would describe work only the graph holds).  The updates queued
    // so far are waited for on the host instead -- a wait node on an event recorded outside the capture would order the graph
    // but not the stream's later eager launches.  Later updates and the replays are ordered by the caller; while the capture
    // lasts, updates are refused (order_after_foreign_match).
    hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
    HIP_TRY(hipThreadExchangeStreamCaptureMode(&mode));
    const hipError_t e = hipStreamSynchronize(h->stream);
    (void)hipThreadExchangeStreamCaptureMode(&mode);
    if (e != hipSuccess) return fail_at(HSM_ERR_HIP, who, ": waiting for the queued map updates at capture", e);
    return HSM_OK;
  }
  // (what test_queued_updates_are_ordered_against_caller_streams holds)
  if (fs->ordered_epoch != h->order.upd_epoch) {  // THIS stream has not been ordered behind the latest map writes yet
    if (!h->order.evt_updates) HIP_TRY(hipEventCreateWithFlags(&h->order.evt_updates, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(h->order.evt_updates, h->stream));
    HIP_TRY(hipStreamWaitEvent(s, h->order.evt_updates, 0));
    fs->ordered_epoch = h->order.upd_epoch;
  }
  // no marker here (an event record between back-to-back launches costs 2-3 us of kernel time each): the
  // next writer of the map records one on every stream with a pending reader (order_after_foreign_match)
  *mark = fs;
  return HSM_OK;
}

extern "C" {

const char* hsm_last_error(void) { return g_last_error.c_str(); }
const char* hsm_version(void) { return "hector_mi355 0.1 (gfx950)"; }

int hsm_create(float map_resolution, int size_x, int size_y, unsigned levels, float start_x, float start_y,
               const hsm_opts* opts, hsm_ctx** out) {
  if (!out) return fail(HSM_ERR_INVALID, "hsm_create: out is null");
  *out = nullptr;
  if (levels < 1 || levels > HSM_MAX_LEVELS || size_x < 2 || size_y < 2 || !(map_resolution > 0.0f))
    return fail(HSM_ERR_INVALID, "hsm_create: bad map geometry");
  // the samplers address texels with a 32-bit byte offset (16 B per cell) and 24-bit multiplies
  if (size_x >= (1 << 24) || size_y >= (1 << 24) || ((size_t)size_x + 3) * ((size_t)size_y + 1) >= ((size_t)1 << 28))
    return fail(HSM_ERR_TOO_LARGE, "hsm_create: map larger than 2^28 cells");
  if ((size_x >> (levels - 1)) < 2 || (size_y >> (levels - 1)) < 2)
    return fail(HSM_ERR_INVALID, "hsm_create: too many levels for this map size");
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev < 1)
    return fail(HSM_ERR_NO_DEVICE, "hsm_create: no HIP device (this library has no CPU path)", e);
  hsm_ctx* h = new hsm_ctx();
  if (opts && opts->device >= 0) {
    h->device = opts->device;
  } else {
    if (hipGetDevice(&h->device) != hipSuccess) h->device = 0;
  }
  if (h->device >= ndev) {
    delete h;
    return fail(HSM_ERR_INVALID, "hsm_create: device ordinal out of range");
  }
  {  // (a partition of the device -- CPX mode -- reports its own CU count; 256 on a whole MI355X)
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) == hipSuccess && cus > 0) h->compute_units = cus;
  }
  const char* refusal = "";
  if (int rc = parse_settings(opts, [](const char* name) -> const char* { return getenv(name); }, &h->cfg, &refusal)) {  // (settings.h)
    delete h;
    return fail(rc, refusal);
  }

#define CREATE_TRY(expr)                                   \
  do {                                                     \
    hipError_t e__ = (expr);                               \
    if (e__ != hipSuccess) {                               \
      int rc__ = fail(HSM_ERR_HIP, #expr, e__);            \
      hsm_destroy(h);                                      \
      return rc__;                                         \
    }                                                      \
  } while (0)

  CREATE_TRY(hipSetDevice(h->device));
  CREATE_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  CREATE_TRY(hipMalloc((void**)&h->single.d_small, kSmallFloats * sizeof(float)));
  CREATE_TRY(hipMalloc((void**)&h->single.d_partials, 2 * 64 * 12 * sizeof(float) + 64));  // [2][64] records of 3 x {p,p,p,tag}; + the grid-barrier counter
  CREATE_TRY(hipMemset(h->single.d_partials, 0, 2 * 64 * 12 * sizeof(float) + 64));
  CREATE_TRY(hipHostMalloc((void**)&h->single.h_small, kSmallFloats * sizeof(float),
                           hipHostMallocMapped | hipHostMallocCoherent));
  memset(h->single.h_small, 0, kSmallFloats * sizeof(float));
  if (create_update_state(h) != HSM_OK) {  // (the gate's block and the publish boxes: map_update.hip)
    hsm_destroy(h);
    return HSM_ERR_HIP;
  }

  CREATE_TRY(hipMalloc((void**)&h->occ.d_extents, 8 * sizeof(int)));  // (hsm_map_extents*: map_image_kernels.h kExtentsNone)
  CREATE_TRY(hipMemsetAsync(h->occ.d_extents, 0x7f, 8 * sizeof(int), h->stream));

  // MapRepMultiMap ctor (MapRepMultiMap.h:48-72)
  int rx = size_x, ry = size_y;
  const float total_x = map_resolution * (float)size_x;
  const float mid_offset_x = total_x * start_x;
  const float total_y = map_resolution * (float)size_y;
  const float mid_offset_y = total_y * start_y;
  h->levels.resize(levels);
  h->start[0] = start_x;
  h->start[1] = start_y;
  for (unsigned i = 0; i < levels; ++i) {
    Level& L = h->levels[i];
    L.sx = rx;
    L.sy = ry;
    L.limx = (float)rx - 2.0f;  // MapDimensionProperties::setMapCellDims (:70-74)
    L.limy = (float)ry - 2.0f;
    set_map_transformation(L, mid_offset_x, mid_offset_y, map_resolution);
    L.log_odds_free = prob_to_log_odds(0.4f);  // GridMapLogOdds.h:117-118
    L.log_odds_occ = prob_to_log_odds(0.6f);
    const size_t n = L.cells();
    CREATE_TRY(hipMalloc((void**)&L.d_logodds, n * sizeof(float)));
    CREATE_TRY(hipMalloc((void**)&L.d_update_index, n * sizeof(int)));
    // the samplers point out-of-map beams at an all-zero footprint stored BEHIND the planes
    // (beam_sample.h sample_fetch): one extra texel, resp. sizeX + 2 extra cells, zeroed once here
    CREATE_TRY(hipMalloc((void**)&L.d_prob, (n + (size_t)rx + 2) * sizeof(float)));
    CREATE_TRY(hipMemsetAsync(L.d_prob + n, 0, ((size_t)rx + 2) * sizeof(float), h->stream));
    if (h->cfg.layout == kLayoutQuad) {
      // HSM_LAYOUT_PLANE samples the probability plane directly (4 gathers per beam) and keeps NO texel plane:
      // 16 B/cell less memory and one dense pass less per update -- the better trade for update-heavy use
      // (single dense scans); the quad layout is the better one for batched matching
      CREATE_TRY(hipMalloc((void**)&L.d_quad, ((size_t)L.quad_texels() + 1) * sizeof(float4)));
      CREATE_TRY(hipMemsetAsync(L.d_quad + L.quad_texels(), 0, sizeof(float4), h->stream));
    }
    CREATE_TRY(hipMalloc((void**)&L.d_key_free, key_free_cells(L.sx, L.sy) * sizeof(unsigned int)));
    CREATE_TRY(hipMalloc((void**)&L.d_key_occ, n * sizeof(unsigned int)));
    CREATE_TRY(hipMemsetAsync(L.d_key_free, 0, key_free_cells(L.sx, L.sy) * sizeof(unsigned int), h->stream));
    CREATE_TRY(hipMemsetAsync(L.d_key_occ, 0, n * sizeof(unsigned int), h->stream));
    CREATE_TRY(hipMalloc((void**)&L.d_occ_bits, ((n + 31) / 32 + 1) * sizeof(unsigned int)));
    CREATE_TRY(hipMemsetAsync(L.d_occ_bits, 0, ((n + 31) / 32 + 1) * sizeof(unsigned int), h->stream));
    CREATE_TRY(hipMalloc((void**)&L.d_free_bytes, mark_plane_bytes(L.sx, L.sy)));
    CREATE_TRY(hipMemsetAsync(L.d_free_bytes, 0, mark_plane_bytes(L.sx, L.sy), h->stream));
    if (fill_level(h, L) != HSM_OK) {
      hsm_destroy(h);
      return HSM_ERR_HIP;
    }
    whole_level_changed(L, false);  // the first export of a level is all of it (a mirror starts from the same cleared map: not dirty)
    CREATE_TRY(hipMemcpyAsync(h->occ.d_pub_boxes + (2 * kMaxLevels + i) * 4, L.pub, sizeof L.pub, hipMemcpyHostToDevice, h->stream));
    rx /= 2;
    ry /= 2;
    map_resolution *= 2.0f;
  }
  CREATE_TRY(hipStreamSynchronize(h->stream));
#undef CREATE_TRY
  *out = h;
  return HSM_OK;
}

void hsm_destroy(hsm_ctx* h) {
  if (!h) return;
  TeardownLog log_, *log = &log_;
  TEARDOWN(log, hipSetDevice(h->device));
  if (h->stream) TEARDOWN(log, hipStreamSynchronize(h->stream));
  if (h->single.copy_stream) TEARDOWN(log, hipStreamSynchronize(h->single.copy_stream));
  for (Level& L : h->levels) free_level(L, log);
  for (GrowBuf* b : h->bufs) b->release(log);  // every grow-on-demand block of the context (hsm_ctx.h)
  for (hsm_ctx::SpecScratch& b : h->batch.spec_scratch) b.d.release(log);
  for (hsm_ctx::PermBuf& b : h->batch.perm_bufs) b.d.release(log);
  for (hsm_ctx::RangesGeometry& g : h->ingest.ranges_geoms) TEARDOWN(log, hipFree(g.d));
  for (hsm_ctx::RangesTfGeometry& g : h->ingest.ranges_tf_geoms) TEARDOWN(log, hipFree(g.d));
  TEARDOWN(log, hipFree(h->batch.d_spec_stats));
  TEARDOWN(log, hipFree(h->single.d_small));
  TEARDOWN(log, hipFree(h->single.d_partials));
  TEARDOWN(log, hipFree(h->upd.d_gate));
  TEARDOWN(log, hipFree(h->occ.d_pub_boxes));
  TEARDOWN(log, hipFree(h->occ.d_extents));
  if (h->single.h_small) TEARDOWN(log, hipHostFree(h->single.h_small));
  for (hipEvent_t e : {h->single.copy_evt, h->order.evt_updates, h->order.evt_foreign, h->order.evt_inputs, h->order.evt_slam_done, h->upd.upd_evt[0], h->upd.upd_evt[1],
                       h->copy.evt_copy_read, h->copy.evt_copy_src})
    if (e) TEARDOWN(log, hipEventDestroy(e));
  if (h->single.copy_stream) TEARDOWN(log, hipStreamDestroy(h->single.copy_stream));
  if (h->stream) TEARDOWN(log, hipStreamDestroy(h->stream));
  delete h;
  if (!log_.first.empty()) {
    g_last_error = "hsm_destroy: " + log_.first;
    (void)hipGetLastError();  // consumed here, not by the next caller's launch check
  }
}

int hsm_reset(hsm_ctx* h) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  // first: it refuses a reset while a caller's stream is being captured; the folds below wait, which would invalidate that capture
  if (int rc = order_after_foreign_match(h)) return rc;
  if (h->upd.upd_boxes_outstanding)
    if (int rc = merge_device_boxes(h)) return rc;
  if (h->upd.gate_outstanding)
    if (int rc = fold_gate_counters(h)) return rc;
  if (int rc = reset_update_gate(h)) return rc;
  for (Level& L : h->levels) {
    if (int rc = fill_level(h, L)) return rc;
    L.uploaded_stamp_max = -1;  // every stamp is -1 again
    whole_level_changed(L);
  }
  HIP_TRY(hipStreamSynchronize(h->stream));
  return HSM_OK;
}

int hsm_levels(const hsm_ctx* h) { return h ? (int)h->levels.size() : 0; }
float hsm_scale_to_map(const hsm_ctx* h) { return h ? h->levels[0].scale_to_map : 0.0f; }

int hsm_set_update_factor_free(hsm_ctx* h, float f) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  std::lock_guard<std::mutex> lk(h->mu);
  for (Level& L : h->levels) L.log_odds_free = prob_to_log_odds(f);
  return HSM_OK;
}
int hsm_set_update_factor_occupied(hsm_ctx* h, float f) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  std::lock_guard<std::mutex> lk(h->mu);
  for (Level& L : h->levels) L.log_odds_occ = prob_to_log_odds(f);
  return HSM_OK;
}
int hsm_on_map_updated(hsm_ctx* h) { return h ? HSM_OK : fail(HSM_ERR_INVALID, "null context"); }

int hsm_set_parity(hsm_ctx* h, int mode) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  if (mode != HSM_PARITY_FAST && mode != HSM_PARITY_EXACT && mode != HSM_PARITY_RELAXED && mode != HSM_PARITY_AUTO)
    return fail(HSM_ERR_INVALID, "hsm_set_parity: unknown mode");
  std::lock_guard<std::mutex> lk(h->mu);
  h->cfg.parity.exact = mode == HSM_PARITY_EXACT;
  h->cfg.parity.relaxed = mode == HSM_PARITY_RELAXED;
  h->cfg.parity.auto_parity = mode == HSM_PARITY_AUTO;
  return HSM_OK;
}
int hsm_parity(const hsm_ctx* h) {
  if (!h) return HSM_PARITY_FAST;
  return h->cfg.parity.exact ? HSM_PARITY_EXACT : (h->cfg.parity.relaxed ? HSM_PARITY_RELAXED : (h->cfg.parity.auto_parity ? HSM_PARITY_AUTO : HSM_PARITY_FAST));
}

int hsm_last_launch_parity(const hsm_ctx* h) { return h ? h->last.last_parity : HSM_PARITY_FAST; }

int hsm_set_batch_order(hsm_ctx* h, int order) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  if (order != HSM_ORDER_GIVEN && order != HSM_ORDER_MORTON && order != HSM_ORDER_AUTO) return fail(HSM_ERR_INVALID, "hsm_set_batch_order: unknown order");
  std::lock_guard<std::mutex> lk(h->mu);
  h->cfg.batch.batch_order = order;
  for (hsm_ctx::PermBuf& b : h->batch.perm_bufs) b.batch = 0;
  return HSM_OK;
}
int hsm_set_batch_order_refresh(hsm_ctx* h, int launches) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  if (launches < 1) return fail(HSM_ERR_INVALID, "hsm_set_batch_order_refresh: at least 1");
  std::lock_guard<std::mutex> lk(h->mu);
  h->cfg.batch.batch_order_refresh = launches;
  for (hsm_ctx::PermBuf& b : h->batch.perm_bufs) b.batch = 0;  // (the next launch computes a fresh one)
  return HSM_OK;
}
int hsm_batch_order(const hsm_ctx* h) { return h ? h->cfg.batch.batch_order : HSM_ORDER_AUTO; }
int hsm_last_launch_sorted(const hsm_ctx* h) { return h && h->last.last_sorted ? 1 : 0; }

int hsm_set_clock_probe(hsm_ctx* h, unsigned long long* d_stamps4) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  std::lock_guard<std::mutex> lk(h->mu);
  h->batch.clock_probe = d_stamps4;
  return HSM_OK;
}

int hsm_device_info(const hsm_ctx* h, int info[4]) {
  if (!h || !info) return fail(HSM_ERR_INVALID, "null argument");
  hipDeviceProp_t p;
  HIP_TRY(hipGetDeviceProperties(&p, h->device));
  info[0] = h->device;
  info[1] = p.multiProcessorCount;
  info[2] = p.clockRate;        // kHz
  info[3] = p.memoryClockRate;  // kHz
  return HSM_OK;
}

int hsm_gn_iterations_per_match(const hsm_ctx* h) {
  return h ? 6 + 4 * ((int)h->levels.size() - 1) : 0;
}
const char* hsm_last_launch_kernel(const hsm_ctx* h) { return h ? h->last.last_kernel : ""; }
int hsm_last_launch_config(const hsm_ctx* h, int cfg[5]) {
  if (!h || !cfg) return fail(HSM_ERR_INVALID, "null argument");
  for (int i = 0; i < 5; ++i) cfg[i] = h->last.last_cfg[i];
  if (h->last.last_cfg[5]) cfg[4] = -cfg[4];  // texel-cache form: endpoints in LDS, not VGPRs
  return HSM_OK;
}

int hsm_synchronize(hsm_ctx* h) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->upd.upd_busy[0] = h->upd.upd_busy[1] = false;
  h->upd.queued_update = false;
  return HSM_OK;
}

}  // extern "C"
