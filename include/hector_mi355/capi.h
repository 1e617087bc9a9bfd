/* hector_mi355 -- C ABI of the MI355X-native scan-to-map Gauss-Newton matcher.
 *
 * This is the drop-in boundary for hector_mapping's L1 map representation
 * (SURVEY.md section 8(b)).  Every entry point names the reference interface it
 * replaces; paths are relative to
 *   /root/reference/hector_mapping/include/hector_slam_lib/        (HSL/)
 * The header facade include/hector_slam_lib/slam_main/MapRepMultiMap.h forwards
 * the reference's C++ virtuals to these functions.
 *
 * Conventions (identical to the reference):
 *   poses   float[3] = x, y, theta; world frame = metres / rad
 *   scans   a DataContainer (HSL/scan/DataPointContainer.h:36-96) is the triple
 *           (pts, n, origo): n endpoints as AoS float[2*n] in the robot frame,
 *           already multiplied by the level-0 scaleToMap (cell units), plus the
 *           laser origin `origo` in the same units
 *   cov/H   float[9], column-major 3x3 (Eigen::Matrix3f default layout)
 *   planes  row-major, index = y*sizeX + x (HSL/map/GridMapBase.h:141-144)
 *
 * Return value: 0 = HSM_OK, negative = error (hsm_last_error() has the text).
 * The reference itself has no error channel (SURVEY.md 8(b) "error conventions");
 * the facade ignores the status to stay behaviour-compatible.
 *
 * All compute runs on the GPU.  There is NO CPU fallback: without a HIP device
 * hsm_create fails with HSM_ERR_NO_DEVICE.
 */
#ifndef HECTOR_MI355_CAPI_H
#define HECTOR_MI355_CAPI_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hsm_ctx hsm_ctx;

enum {
  HSM_OK = 0,
  HSM_ERR_INVALID = -1,    /* bad argument */
  HSM_ERR_NO_DEVICE = -2,  /* no HIP device / HIP runtime error at init */
  HSM_ERR_HIP = -3,        /* HIP runtime error (text in hsm_last_error) */
  HSM_ERR_TOO_LARGE = -4   /* scan longer than HSM_MAX_UPDATE_BEAMS in update_by_scan, or map > 2^28 cells */
};

#define HSM_MAX_LEVELS 8
#define HSM_MAX_UPDATE_BEAMS 1048575

/* probability sampling layout used by the GN kernel (DESIGN.md "data layout"):
 *   QUAD  float4 texel plane {P(x,y),P(x+1,y),P(x,y+1),P(x+1,y+1)}: one 16-byte gather per beam; best for batched matching
 *   PLANE the fp32 probability plane itself, four 4-byte gathers per beam; no texel plane is kept (16 B/cell less
 *         memory, one dense pass less per update): best for update-heavy single dense scans */
enum { HSM_LAYOUT_AUTO = 0, HSM_LAYOUT_QUAD = 1, HSM_LAYOUT_PLANE = 2 };

typedef struct hsm_opts {
  int device;          /* HIP device ordinal; -1 = current device */
  int layout;          /* HSM_LAYOUT_*; AUTO honours env HSM_LAYOUT=quad|plane, default quad */
  int waves_per_scan;  /* 0 = auto (env HSM_WPS overrides), else 1,2,4,8,16 */
} hsm_opts;

/* summation order of the Hessian / gradient reduction (OccGridMapUtil.h:76-98):
 *   FAST   lane-strided partial sums + tree: the reference's per-beam products, summed in another order;
 *          poses within 1e-4 m / 1e-4 rad of the reference wherever its Gauss-Newton iteration has settled
 *   EXACT  the reference's order, beam 0 .. n-1 in nine sequential fp32 chains: H, dTr, every GN step and
 *          the final pose are BIT-IDENTICAL to the reference CPU matcher on every scan (about 2.5x the
 *          instructions per GN iteration).  sinf/cosf/expf are glibc's algorithms in every mode.
 *   RELAXED  FAST with the multiply-add pairs of the per-beam arithmetic contracted to fused operations (32 instead of
 *          51 fp32 operations per beam) in the batched throughput kernel; everything else runs as FAST.  Per-beam terms
 *          are no longer bit-exact; the bar is north_star's 1e-4 m / 1e-4 rad on the pose, measured at full size.
 *   AUTO   (default) the reference's order on EVERY entry point -- hsm_match (with and without the hook trace), hsm_match_level,
 *          hsm_match_batch*, hsm_group_match_batch*, the likelihood / covariance / Hessian probes: results bit-identical to the
 *          reference CPU matcher.  AUTO may pick any kernel form that is bit-identical to the reference's chains (today the
 *          same forms EXACT pins).  Why the default does not use the tree anywhere (rounds 4 and 5): the scene sweeps
 *          (profiles/r04/parity_scene_sweep.jsonl, profiles/r05/parity_scene_sweep_single_default.jsonl: seven scene families,
 *          three start / level set-ups, 4096 scans each) find the fast tree beyond 1e-4 m of the reference on some scans of every
 *          family wherever the reference's own iteration has not settled, and nothing known at launch separates those scans --
 *          for one scan no more than for a batch.  Price: a 1081-beam hsm_match takes 99 us instead of 33, a batch 1.3x the
 *          tree's time.  hsm_last_launch_parity() tells which order the last launch ran in.
 * env HSM_PARITY=fast|exact|relaxed|auto selects a mode at hsm_create (any other word: hsm_create fails), hsm_set_parity
 * switches at run time. */
enum { HSM_PARITY_FAST = 0, HSM_PARITY_EXACT = 1, HSM_PARITY_RELAXED = 2, HSM_PARITY_AUTO = 3 };

/* ---- construction ---------------------------------------------------------
 * replaces: MapRepMultiMap::MapRepMultiMap(mapResolution, mapSizeX, mapSizeY, numDepth,
 *           startCoords, draw, debug)                    HSL/slam_main/MapRepMultiMap.h:48-72
 * Level l has size (sx>>l, sy>>l) and cell length res*2^l; all levels share the
 * offset (res*sx*start_x, res*sy*start_y).  Update factors start at the library
 * defaults 0.4 / 0.6 (HSL/map/GridMapLogOdds.h:117-118). */
int hsm_create(float map_resolution, int size_x, int size_y, unsigned levels, float start_x,
               float start_y, const hsm_opts* opts /* may be NULL */, hsm_ctx** out);
/* replaces: MapRepMultiMap::~MapRepMultiMap                   MapRepMultiMap.h:74-81
 * Waits for the context's queued work, releases everything.  Never fails towards the caller; if a runtime call fails during
 * teardown, everything else is still released, hsm_last_error() of this thread then reads "hsm_destroy: <call>: <error>", and
 * the runtime's per-thread error state is cleared (it is not left for the next hipGetLastError() of an unrelated call). */
void hsm_destroy(hsm_ctx* h);

/* replaces: MapRepMultiMap::reset -> MapProcContainer::reset  MapRepMultiMap.h:83-90, MapProcContainer.h:67-71
 * Clears the cells, nothing else (GridMapBase::reset), on every level:
 *   cleared  log-odds 0 and stamps -1, the probability / texel planes with them (0.5); the gate's pose back to FLT_MAX three
 *            times (HectorSlamProcessor::reset); the largest restored stamp (the stamp-aware update form is deselected); the
 *            last-update box empty; the dirty box and the publish box the whole level, so the first hsm_take_dirty_bbox and the
 *            first export after it cover all of it.
 *   stays    the update counters of the maps and the gate's count of applied scans (the reference does not rewind
 *            currUpdateIndex: the first update afterwards stamps with counter + 1 / + 2), the key generation, the window start
 *            an hsm_shift_map left (reset clears cells, not geometry), the update factors, gate thresholds, parity and
 *            batch-order settings, the retained containers of the coarse levels (MapRepMultiMap::dataContainers survive: an
 *            hsm_update_by_scan with no match in between marks the coarse levels with the scan matched before the reset), the
 *            cached sensor geometries and every grown buffer.
 * What gated and device-side calls left on the device (the count of applied scans, the update boxes) is folded in first, so no
 * host query is needed in front of it.  It is a map update for ordering and capture purposes: stream-ordered behind every
 * match queued on a caller's stream, refused with HSM_ERR_INVALID while such a stream is being captured; it returns when
 * the cleared map is in place. */
int hsm_reset(hsm_ctx* h);
/* replaces: getMapLevels / getScaleToMap                      MapRepMultiMap.h:92-94 */
int hsm_levels(const hsm_ctx* h);
float hsm_scale_to_map(const hsm_ctx* h);
/* replaces: setUpdateFactorFree / setUpdateFactorOccupied     MapRepMultiMap.h:149-167 */
int hsm_set_update_factor_free(hsm_ctx* h, float free_factor);
int hsm_set_update_factor_occupied(hsm_ctx* h, float occupied_factor);
/* replaces: onMapUpdated (cache generation bump)              MapRepMultiMap.h:107-114.
 * The device probability texels are refreshed eagerly by update_by_scan, so this
 * only has to exist; it returns HSM_OK. */
int hsm_on_map_updated(hsm_ctx* h);
/* no reference counterpart: selects HSM_PARITY_FAST / _EXACT / _RELAXED / _AUTO for all later matches of the context */
int hsm_set_parity(hsm_ctx* h, int mode);
int hsm_parity(const hsm_ctx* h);
/* the order the LAST match launch of this context actually ran in (HSM_PARITY_FAST / EXACT / RELAXED); under HSM_PARITY_AUTO:
 * EXACT */
int hsm_last_launch_parity(const hsm_ctx* h);
/* no reference counterpart (the reference matches one scan at a time): the order in which a BATCH is laid out on the device.
 * Scans that are neighbours in a launch run on one XCD at the same time and share the texel lines they touch in its L2; a batch
 * whose order does not follow the map (particles of several modes, several robots) loses that -- 61 instead of 58 us on the
 * 2048^2 map, 178 instead of 145 us on the 4096^2 pyramid (profiles/r06).
 *   HSM_ORDER_MORTON: a one-workgroup counting sort in front of the matcher orders batches of at least 1024 scans by the Morton
 *     code of the 64 x 64 map tile their start poses lie in, and the matcher takes its scans through that permutation; every
 *     result still lands at the scan's own index and is bit-identical.  The sort is a 9 us kernel, so a stream's permutation
 *     serves hsm_set_batch_order_refresh launches of the same batch size (default 16; env HSM_BATCH_ORDER_REFRESH) before it is
 *     computed again: ANY permutation gives the same results, an old one only groups the scans by where they were a few
 *     launches ago.
 *   HSM_ORDER_AUTO (default; env HSM_BATCH_ORDER=auto|given|morton): that, on maps of more than 2^23 cells (the ones that outgrow
 *     the L2s), and only for a batch that does not follow the map already -- the sort kernel counts the tile changes between
 *     neighbouring scans and leaves a batch that has few of them in its own order.  Costs such a batch ~1 us per launch.
 *   HSM_ORDER_GIVEN: always the caller's order.
 * Applies to the texel-cache batch forms (every batch of the quad layout). */
enum { HSM_ORDER_GIVEN = 0, HSM_ORDER_MORTON = 1, HSM_ORDER_AUTO = 2 };
int hsm_set_batch_order(hsm_ctx* h, int order);
int hsm_set_batch_order_refresh(hsm_ctx* h, int launches);
int hsm_batch_order(const hsm_ctx* h);
/* 1 if the last batched match took its scans through a permutation (Morton order, or the identity AUTO left a batch in), else 0 */
int hsm_last_launch_sorted(const hsm_ctx* h);

/* ---- the hot path -----------------------------------------------------------
 * replaces: MapRepMultiMap::matchData(beginEstimateWorld, dataContainer, covMatrix)
 *           HSL/slam_main/MapRepMultiMap.h:116-132  (-> ScanMatcher::matchData,
 *           HSL/matcher/ScanMatcher.h:54-190, 4 GN steps per coarse level, 6 on level 0).
 * Host pointers.  n == 0: out_pose = begin, cov untouched (ScanMatcher.h:68,189).
 * Like the reference it retains the scan for the coarse levels of the next
 * hsm_update_by_scan (MapRepMultiMap.h:127,143). */
int hsm_match(hsm_ctx* h, const float begin_world[3], const float* pts_xy, int n,
              const float origo[2], float out_pose_world[3], float cov[9]);

/* hsm_match plus a per-GN-step trace for the reference's draw/debug hooks
 * (ScanMatcher.h:100-110: drawArrow(estimate) and addHessianMatrix(H) per loop iteration).
 * trace[12*k .. 12*k+11] = {map-frame estimate after step k [3], H used by step k [9] col-major},
 * steps in schedule order (coarsest level first; 4 per coarse level, 6 on level 0).
 * *steps_written = number of records (0 for an empty scan).
 * trace_cap_steps < hsm_gn_iterations_per_match() (6 + 4 * (levels - 1), 34 on 8 levels): HSM_ERR_INVALID, no match is run
 * and nothing is written, *steps_written included. */
int hsm_match_trace(hsm_ctx* h, const float begin_world[3], const float* pts_xy, int n,
                    const float origo[2], float out_pose_world[3], float cov[9], float* trace,
                    int trace_cap_steps, int* steps_written);

/* Batched extension (not in the reference): B independent (pose hypothesis, scan)
 * pairs against the read-only pyramid in ONE launch.  DEVICE pointers:
 *   d_begin_world  [B*3]       d_pts_xy [total*2]
 *   d_scan_offsets [B+1] CSR offsets into d_pts_xy in points, or NULL = every
 *                  hypothesis uses the same scan d_pts_xy[0 .. shared_n)
 *   shared_n       with CSR offsets: a sizing HINT (typical beams per scan, 0 = unknown -> 1081); it selects
 *                  the kernel form only -- scans longer than the hint are matched correctly, just slower
 *   d_out_pose     [B*3]       d_out_cov [B*9] or NULL
 * `stream` is a hipStream_t (NULL = default stream); the call is asynchronous.  The library orders it behind
 * every map update queued on the context so far, and the next map update behind it (events; no host wait),
 * per caller stream: matches may be in flight on several caller-owned streams at once.
 * Graph capture (hipStreamBeginCapture on `stream`, e.g. torch.cuda.graph): the call records kernel launches
 * only, and allocates nothing.  At capture time the host waits for the map updates queued so far, so every replay
 * sees them.  A captured launch orders nothing else: the caller orders each replay against later updates
 * (hsm_synchronize before replaying, or their own events).  While a stream that this context has matched on is
 * being captured, every map update (hsm_update_by_scan and its kin, hsm_upload_level, hsm_reset) fails with
 * HSM_ERR_INVALID and queues nothing.  Captured launches keep the caller's batch order and take the literal
 * reference-order form where HSM_EXACT_SPEC=1 would speculate: no graph reads per-stream buffers that
 * eager launches rewrite or free.  Results are the same bits.
 * Does not touch the retained-scan state. */
int hsm_match_batch_device(hsm_ctx* h, int batch, const float* d_begin_world,
                           const float* d_pts_xy, const int* d_scan_offsets, int shared_n,
                           float* d_out_pose, float* d_out_cov, void* stream);
/* same with host pointers (copies in, runs, copies out, synchronous) */
int hsm_match_batch(hsm_ctx* h, int batch, const float* begin_world, const float* pts_xy,
                    const int* scan_offsets, int shared_n, float* out_pose, float* out_cov);

/* replaces: MapRepMultiMap::updateByScan(dataContainer, robotPoseWorld)
 *           HSL/slam_main/MapRepMultiMap.h:134-147 -> OccGridMapBase::updateByScan,
 *           HSL/map/OccGridMapBase.h:121-260.  Level 0 uses (pts, n, origo); coarse
 *           levels use the scan retained by the last hsm_match, scaled by 2^-level,
 *           exactly as the reference does.
 *           Returns when the update is QUEUED on the context's stream (pts_xy has been copied and may be
 *           reused at once): every later call on this context -- matches, downloads, further updates --
 *           is ordered behind it, so results are the same as if it had completed; a device fault
 *           surfaces at the next call that waits.  hsm_synchronize() waits explicitly; the environment
 *           variable HSM_ASYNC_UPDATE=0 makes the call itself wait. */
int hsm_update_by_scan(hsm_ctx* h, const float pose_world[3], const float* pts_xy, int n,
                       const float origo[2]);
/* wait until all work queued on the context has completed (and report any device error) */
int hsm_synchronize(hsm_ctx* h);
/* one level, explicit level-scaled container (OccGridMapBase::updateByScan itself) */
int hsm_update_by_scan_level(hsm_ctx* h, int level, const float pose_world[3],
                             const float* pts_level_xy, int n, const float origo_level[2]);

/* replaces: for k = 0 .. count-1, in order: MapRepMultiMap::updateByScan(container_k, pose_k)
 *           (HSL/slam_main/MapRepMultiMap.h:134-147 -> OccGridMapBase::updateByScan, HSL/map/OccGridMapBase.h:121-260),
 *           with level l seeing container_k through DataContainer::setFrom(container_k, 1 / 2^l)
 *           (DataPointContainer.h:46-58) -- what the reference does whenever updateByScan follows the matchData
 *           of the same scan, which is always in HectorSlamProcessor::update (HectorSlamProcessor.h:78-94).
 * Poses and scans stay where the batched matchers leave them.  DEVICE pointers:
 *   d_poses_world  [count*3] WORLD poses, e.g. d_out_pose of hsm_match_batch_device or d_out_best_pose of
 *                  hsm_match_score_batch_device.  A NaN, infinite or far-away pose changes no cell (every beam fails the
 *                  reference's map test) and still counts as an update.
 *   d_pts_xy, d_scan_offsets, shared_n   as in hsm_match_batch_device: CSR offsets [count+1] in points, or NULL = every pose
 *                  integrates the one scan d_pts_xy[0 .. shared_n).  A scan of 0 beams counts as an update, like an empty
 *                  container in the reference (OccGridMapBase.h:123-167); a CSR scan of more than HSM_MAX_UPDATE_BEAMS
 *                  beams is integrated as an empty one.
 *   max_beams      a sizing HINT (typical beams per scan, 0 = unknown -> 1081): it selects launch shapes only -- a longer
 *                  scan is integrated correctly, just more slowly
 *   origo          HOST, the containers' origo (NULL = 0,0)
 * The host never learns a pose or a scan's length: one preparation launch, then two launches per scan, on the context's own
 * stream like every map writer.  `stream` is the caller's stream on which the inputs were produced (NULL = default stream):
 * the call records an event there and the context's stream waits for it; the update queues behind batched matches that
 * still read the map, and every hsm_* map reader queued later, on any stream, is ordered behind the update.  The inputs
 * must stay unchanged until the update has run: overwriting them from such later hsm_* calls needs no extra
 * synchronisation, any other writer waits (hsm_synchronize).  Returns when everything is queued.
 * HSM_ERR_INVALID, nothing queued: count < 0, max_beams < 0, a NULL pointer where data is needed, shared_n < 0 without
 * offsets, or `stream` / a stream this context has matched on is being captured into a graph (updates are not captured).
 * count == 0: HSM_OK.  hsm_update_index advances by count on every level.  Does not touch the retained or the ingested
 * scan.  hsm_last_update_bbox / hsm_take_dirty_bbox called afterwards wait for the update (the boxes are computed on the
 * device): on level 0 the box of the host path, on coarse levels a tighter one that still holds every changed cell.
 * Not replayed by hsm_group_*. */
int hsm_update_by_scans_device(hsm_ctx* h, int count, const float* d_poses_world, const float* d_pts_xy,
                               const int* d_scan_offsets, int shared_n, int max_beams, const float origo[2],
                               void* stream);
/* the same with one origo PER SCAN, on the device: a sensor whose mount moves against base_link (the node's tf path sets the
 * container's origo from the laser -> base_link translation of every scan, HectorMappingRos.cpp:517).
 *   d_origos       DEVICE [count*2] floats, scan k's origo in level-0 cell units, e.g. d_out_origo of
 *                  hsm_ingest_batch_ranges_tf_device; level l sees d_origos[k] * 2^-l (DataPointContainer.h:48).  NULL = 0,0
 *                  for every scan.  8-byte aligned (HSM_ERR_INVALID otherwise).  Complete on `stream` and unchanged until the
 *                  update has run, like the other inputs.
 * The origo is the begin cell of every Bresenham line of the scan (OccGridMapBase.h:134-137).  A NaN or infinite origo drops
 * every beam of that scan, which still counts as an update, like a NaN pose.  With every pair equal to X the call is, bit for
 * bit, hsm_update_by_scans_device with the host origo X; launches, ordering, refusals and counters are that entry's. */
int hsm_update_by_scans_device_origos(hsm_ctx* h, int count, const float* d_poses_world, const float* d_pts_xy,
                                      const int* d_scan_offsets, int shared_n, int max_beams, const float* d_origos,
                                      void* stream);
/* same with host arrays (copies in, then the same device path; returns when queued, the arrays may be reused at once):
 * builds a map from a log of posed scans in one call.  HSM_ERR_TOO_LARGE: a scan of more than HSM_MAX_UPDATE_BEAMS beams. */
int hsm_update_by_scans(hsm_ctx* h, int count, const float* poses_world, const float* pts_xy,
                        const int* scan_offsets, int shared_n, const float origo[2]);

/* ---- the movement gate of HectorSlamProcessor::update, on the device ----------------------------------------------------
 * replaces: the second half of HectorSlamProcessor::update (HSL/slam_main/HectorSlamProcessor.h:84-94):
 *             if (util::poseDifferenceLargerThan(newPose, lastMapUpdatePose, minDist, minAngle) || map_without_matching)
 *               { updateByScan; onMapUpdated; lastMapUpdatePose = newPose; }
 *           with util::poseDifferenceLargerThan (HSL/util/UtilFunctions.h:73-92) in the reference's fp32 / fp64 mix.
 * lastMapUpdatePose and the number of updates the gate has let through live in a per-context device block: the host learns
 * neither a decision nor a pose.  A NaN compares false, so a NaN in x or y leaves the angle test alone to let the pose through,
 * a NaN in theta the distance test, and an all-NaN pose is never "larger": it is not integrated and advances no counter (the
 * ungated entry counts it as an update).  An infinite pose is integrated as an update that changes no cell.
 *
 * thresholds of the gate (paramMinDistanceDiffForMapUpdate / paramMinAngleDiffForMapUpdate; 0.4 / 0.13 after hsm_create,
 * HectorSlamProcessor.h:62-63); they apply to the calls queued afterwards */
int hsm_set_update_gate(hsm_ctx* h, float min_dist, float min_angle);
/* lastMapUpdatePose = FLT_MAX three times (the next scan is integrated whatever its pose) and lastScanMatchPose = 0, as
 * HectorSlamProcessor::reset leaves them (:133-140); also done by hsm_create and hsm_reset.  Stream-ordered: queued behind the
 * gated calls made so far, no host wait.  The update counters of the maps stay. */
int hsm_reset_update_gate(hsm_ctx* h);
/* waits for the context's stream and fetches the gate's state: lastMapUpdatePose, and the number of updates gated calls have
 * applied since hsm_create.  Either pointer may be NULL. */
int hsm_update_gate_state(hsm_ctx* h, float last_update_pose[3], long long* applied_total);
/* hsm_update_by_scans_device behind the gate: for k = 0 .. count-1, in order, scan k is integrated where the gate lets pose k
 * through.  Arguments, stream rules, ordering and refusals of hsm_update_by_scans_device, plus
 *   d_force        DEVICE [count] bytes, non-zero = map_without_matching: the scan is integrated whatever the gate says
 *                  (and becomes lastMapUpdatePose).  NULL = none.
 *   d_out_applied  DEVICE [count] ints, 1 = integrated, 0 = rejected.  May be NULL.
 * One gate launch per call (the decisions are sequential: one lane walks them), then the two launches per scan of the
 * ungated entry; those of a rejected scan return at once, and it changes no cell and no counter.  An integrated scan is marked
 * with the update index that follows the last integrated one.  One key generation is spent per scan and level, integrated or
 * not.  hsm_update_index and every host-side update called afterwards first wait for the stream to learn how many scans were
 * integrated.  hsm_last_update_bbox afterwards: the box of the call's LAST scan, empty where that one was rejected.
 * HSM_ERR_INVALID, nothing queued, while `stream` or a stream this context has matched on is being captured.
 * A moving sensor mount passes its origos per scan through hsm_update_by_scans_device_gated_origos.
 * Not built: capture into graphs, replay through hsm_group_*, the byte-map (dense) form of the update. */
int hsm_update_by_scans_device_gated(hsm_ctx* h, int count, const float* d_poses_world, const float* d_pts_xy,
                                     const int* d_scan_offsets, int shared_n, int max_beams, const float origo[2],
                                     const unsigned char* d_force, int* d_out_applied, void* stream);
/* the same with d_origos as in hsm_update_by_scans_device_origos (DEVICE [count*2], NULL = 0,0): every level integrates scan k
 * at its own origo.  Everything else is hsm_update_by_scans_device_gated's. */
int hsm_update_by_scans_device_gated_origos(hsm_ctx* h, int count, const float* d_poses_world, const float* d_pts_xy,
                                            const int* d_scan_offsets, int shared_n, int max_beams, const float* d_origos,
                                            const unsigned char* d_force, int* d_out_applied, void* stream);
/* replaces: for k = 0 .. count-1, in order: HectorSlamProcessor::update(container_k, hint_k, force_k)
 *           (HSL/slam_main/HectorSlamProcessor.h:71-95): matchData, the gate, updateByScan -- a log of scans in ONE call that
 *           returns when everything is queued.  The host waits for nothing and learns nothing.  DEVICE pointers:
 *   d_start_pose   [3] hint of scan 0; NULL = lastScanMatchPose of the call before (0 after hsm_create / a reset)
 *   d_hint_deltas  [count*3] or NULL.  hint_k = pose_(k-1) + delta_k componentwise in fp32 (hint_0 = start + delta_0), e.g.
 *                  odometry increments; NULL = the pose is passed on unchanged, no addition.
 *   d_pts_xy, d_scan_offsets   CSR scans as in hsm_match_batch_device ([count+1] offsets in points; required)
 *   max_beams      sizing hint as in hsm_update_by_scans_device (0 = unknown -> 1081)
 *   origo          HOST, the containers' origo (NULL = 0,0)
 *   d_force        [count] bytes or NULL: a forced scan skips the match and takes its hint as its pose; its covariance row
 *                  repeats lastScanMatchCov, and the coarse levels integrate the containers the last MATCHED scan left there,
 *                  as the reference does (MapRepMultiMap.h:134-147).  Those containers do not outlive the call: a scan forced
 *                  before the first matched scan of a call finds them empty, as the reference does before its first match.
 *   d_out_pose     [count*3] lastScanMatchPose after each scan        d_out_cov [count*9] or NULL
 *   d_out_applied  [count] ints or NULL: 1 = the scan was integrated
 * An empty scan returns its hint as its pose, like matchData; its covariance row is what hsm_match_batch_device writes for
 * an empty scan.  Per scan the call queues one match of one scan through hsm_match_batch_device's path, the gate launch, the
 * mark and the apply launch, all on the context's stream: `stream` (the caller's, NULL = default stream) is waited for once in
 * front -- the inputs must be complete there -- and waits once behind, so work queued on it afterwards sees every result.
 * The gate's state persists on the device: two calls of 12 scans give what one call of 24 gives.
 * HSM_ERR_INVALID, nothing queued: a bad argument, or `stream` / a stream this context has matched on is being captured.
 * Does not touch the retained or the ingested scan.  A moving sensor mount passes its origos per scan through
 * hsm_slam_scans_device_origos.  Not built: capture into graphs, replay through hsm_group_*, the byte-map (dense) form of the
 * update; the C++ facade's HectorSlamProcessor.h stays reference code and does not call this. */
int hsm_slam_scans_device(hsm_ctx* h, int count, const float* d_start_pose, const float* d_hint_deltas,
                          const float* d_pts_xy, const int* d_scan_offsets, int max_beams, const float origo[2],
                          const unsigned char* d_force, float* d_out_pose, float* d_out_cov, int* d_out_applied,
                          void* stream);
/* the same with d_origos as in hsm_update_by_scans_device_origos (DEVICE [count*2], NULL = 0,0).  The origo belongs to the
 * container, so the reference's rule for a forced scan holds for it too: level 0 integrates the forced scan at its OWN origo,
 * levels >= 1 integrate the points AND the origo of the last MATCHED scan (setFrom copies both, MapRepMultiMap.h:127,143).
 * The retained origo lives in the gate's device block next to the retained scan; like it, it does not outlive the call.
 * Everything else is hsm_slam_scans_device's. */
int hsm_slam_scans_device_origos(hsm_ctx* h, int count, const float* d_start_pose, const float* d_hint_deltas,
                                 const float* d_pts_xy, const int* d_scan_offsets, int max_beams, const float* d_origos,
                                 const unsigned char* d_force, float* d_out_pose, float* d_out_cov, int* d_out_applied,
                                 void* stream);

/* ---- single-process multi-GPU group (extension; the reference has no multi-device path) ------------------
 * One replica of the pyramid per listed device (a device may be listed more than once).  Batched matching is
 * sharded contiguously over the replicas, one PERSISTENT host thread per replica (created with the group), each
 * replica on its own stream.  Two forms: host arrays in/out (hsm_group_match_batch: the "gather" of the poses is the
 * D2H copy of each shard into the caller's arrays) and device-resident shards (hsm_group_match_batch_device: the
 * gather of each shard's [n,3] poses to the root replica's device runs over xGMI, no host staging -- as ONE grouped RCCL
 * collective over the group's communicators (ncclCommInitAll on first use; librccl is dlopen'ed then, the library does
 * not link it), or as peer copies; see hsm_group_set_gather).  Map updates are replayed on every replica -- updateByScan
 * is deterministic, so the replicas stay bit-identical.
 * (bench.py's --gpus N uses the other deployment shape: one process per GPU and an RCCL all-gather of device-resident
 * poses through torch.distributed; bench.py --group N drives this one.) */
typedef struct hsm_group hsm_group;
/* how hsm_group_match_batch_device gathers.  AUTO (default; env HSM_GROUP_GATHER=auto|direct|rccl|peer at hsm_group_create):
 * DIRECT -- the device-side exchange below (hsm_exchange_*: every replica's kernel stores its rows into every replica's
 * mailbox, one launch per replica behind its match, no collective, no event; where replicas share a device, a post and a wait
 * launch per replica, the wait behind the events of that device's posts, so that no kernel polls for rows a launch queued
 * behind it has yet to store) -- whenever the replicas' devices can access
 * each other (or are the same device); else RCCL when librccl loads, every replica sits on its own device and
 * ncclCommInitAll succeeds; else peer copies (hsm_group_gather_note says why).  DIRECT or RCCL asked for explicitly fail
 * instead of falling back. */
enum { HSM_GATHER_AUTO = 0, HSM_GATHER_PEER = 1, HSM_GATHER_RCCL = 2, HSM_GATHER_DIRECT = 3 };
int hsm_group_set_gather(hsm_group* g, int mode);
/* test hook: with the RCCL gather, send EVERY shard -- the root's own too (a send to self) -- through the grouped ncclSend /
 * ncclRecv form that unequal shards take, instead of ncclAllGather.  Lets a one-device box run that form on hardware. */
int hsm_group_debug_force_p2p(hsm_group* g, int on);
/* The partitioning of `total` scans over `world` replicas (contiguous shards, the first total % world hold one more): [begin, end)
 * of shard `rank`.  Used by hsm_group_match_batch and by hector_slam_amd/sharding.py -- one rule for both transports. */
int hsm_shard_bounds(int total, int rank, int world, int* begin, int* end);
/* the mode in effect: HSM_GATHER_DIRECT, HSM_GATHER_RCCL or HSM_GATHER_PEER.  The decision -- for RCCL: dlopen of librccl and
 * ncclCommInitAll over the group's devices, SECONDS on a multi-GPU node -- is taken on first use: by this call, by hsm_group_set_gather(RCCL), or else inside the
 * first hsm_group_match_batch_device.  A latency-sensitive caller asks for the mode once right after hsm_group_create. */
int hsm_group_gather_mode(hsm_group* g);
const char* hsm_group_gather_note(const hsm_group* g);
/* the DIRECT gather, and the RCCL gather with equal shards, are all-gathers: replica i (other than the root, which received into
 * the caller's arrays) holds all poses [sum(counts) * 3] (want_cov: all Hessians [sum * 9]) in a block the group owns; NULL otherwise */
const float* hsm_group_gathered(hsm_group* g, int replica, int want_cov);
int hsm_group_create(float map_resolution, int size_x, int size_y, unsigned levels, float start_x, float start_y,
                     const int* devices, int n_devices, hsm_group** out);
void hsm_group_destroy(hsm_group* g);
int hsm_group_size(const hsm_group* g);
hsm_ctx* hsm_group_member(hsm_group* g, int i); /* replica i: uploads, downloads, queries */
int hsm_group_set_update_factors(hsm_group* g, float free_factor, float occupied_factor);
/* HectorSlamProcessor::update's two halves for ONE scan: matchData on replica 0, then -- if do_update --
 * updateByScan with the matched pose on EVERY replica (each retains the scan first, like its own matchData would) */
int hsm_group_process_scan(hsm_group* g, const float hint_world[3], const float* pts_xy, int n, const float origo[2],
                           int do_update, float out_pose_world[3], float cov[9]);
/* Device-resident sharded match: replica r matches counts[r] scans that already live on ITS device (d_begin_world[r],
 * d_pts_xy[r], d_scan_offsets[r]: CSR offsets relative to the shard, or d_scan_offsets == NULL / entries NULL for
 * pose hypotheses of one shared scan of shared_n beams per replica).  The poses of all shards are gathered, in replica
 * order, into d_out_pose_all [sum(counts) * 3] on replica `root`'s device (and the Hessians into d_out_cov_all
 * [sum * 9] unless NULL): by the device-side exchange (one launch per replica on its own stream), by a grouped ncclAllGather
 * (equal counts) / ncclSend + ncclRecv (ragged counts) on the replicas' own streams, or by hipMemcpyPeerAsync on each replica's
 * own stream (hsm_group_set_gather).  d_out_cov_all is in/out as hsm_match_batch_device's is: a scan without beams passes its
 * start estimate through and leaves its Hessian row as the caller gave it (every replica starts from the caller's rows of its
 * shard: one copy of 36 bytes per scan on the replica's stream).  Like the shards themselves, d_out_cov_all is read on the
 * replicas' streams, which are not ordered behind any stream of the caller: what the caller writes into it must be complete
 * before the call.  Asynchronous: returns when
 * everything is queued; root's context stream is ordered behind the gather (hsm_synchronize(hsm_group_member(g, root)) or
 * hsm_group_synchronize wait for it). */
int hsm_group_match_batch_device(hsm_group* g, const int* counts, const float* const* d_begin_world,
                                 const float* const* d_pts_xy, const int* const* d_scan_offsets, int shared_n, int root,
                                 float* d_out_pose_all, float* d_out_cov_all);
/* wait for all queued work of every replica */
int hsm_group_synchronize(hsm_group* g);
/* Replica `from`'s pyramid into every other replica: hsm_copy_map (boxes == NULL: the whole pyramid) or hsm_copy_map_boxes with
 * `boxes` [levels * 4, host], each queued by its replica's thread; returns when all are queued (hsm_group_synchronize waits).
 * The remedy after entries the group does not replay -- once one replica has integrated scans through hsm_update_by_scans_device*
 * or hsm_slam_*_device, pass the boxes of its hsm_take_dirty_bbox.  HSM_ERR_INVALID: a NULL group, `from` out of range, and what
 * the copies refuse. */
int hsm_group_sync_maps(hsm_group* g, int from, const int* boxes);
/* hsm_match_batch over all replicas: scans [B*r/R, B*(r+1)/R) go to replica r */
int hsm_group_match_batch(hsm_group* g, int batch, const float* begin_world, const float* pts_xy,
                          const int* scan_offsets, int shared_n, float* out_pose, float* out_cov);
/* what hsm_match does to the coarse-level containers, without matching (MapRepMultiMap.h:127) */
int hsm_retain_scan(hsm_ctx* h, const float* pts_xy, int n, const float origo[2]);

/* ---- device-side gather of sharded results (extension; the reference has no multi-device path) -------------------
 * The one exchange step of a batched matchData sharded over G GPUs (MapRepMultiMap.h:116-132 is the call being sharded;
 * SURVEY.md 8(e)): every rank ends up with every rank's [B/G, cols] rows (cols = 3 poses, 9 Hessians).  No collective library
 * on the data path: every rank owns a MAILBOX in its own HBM; a POST stores a rank's rows -- one 8-byte {value, epoch tag}
 * store per float, system scope -- into every rank's mailbox over xGMI (its own included); a WAIT polls the own mailbox until
 * every value of that epoch has arrived and unpacks it into a dense fp32 array.  One small kernel per step on the caller's
 * stream (protocol and flow control: hector_slam_amd/csrc/pose_exchange.h).  Used by hsm_group_* (HSM_GATHER_DIRECT)
 * and, one process per GPU, by hector_slam_amd/sharding.py (DirectRowGather: the handles travel once over torch.distributed,
 * the rows never do).
 *
 *   create          rank `rank` of `world` (<= 16) on `device` (-1 = current): a mailbox of `depth` buffers of
 *                   [total_rows][cols] values.  depth >= 2 + 2 * lag (lag: how many posts a rank runs ahead of its waits).
 *   handle          64-byte hipIpcMemHandle of this rank's mailbox -- hand it to the other PROCESSES (any channel)
 *   connect         handles of all ranks, world x 64 bytes in rank order (the own entry is ignored): maps the peers' mailboxes
 *   connect_local   the ranks of ONE process: ranks[r] = rank r's exchange (peer access instead of IPC)
 *   post            epoch = posted + 1: rows [first_row, first_row + n_rows) of the gathered array, from d_rows [n_rows][cols]
 *                   (device memory, written by work queued earlier on `stream`), to every rank
 *   wait            epoch = waited + 1 (must have been posted by this rank): d_out_all [total_rows][cols] holds all ranks'
 *                   rows when the launch completes (NULL: arrival only).  Bounded: values that do not arrive within
 *                   HSM_EXCHANGE_TIMEOUT_MS (default 2000) read NaN and hsm_exchange_status fails.
 *   post_wait       ONE launch: post epoch e = posted + 1 and wait for epoch e - lag (skipped while e <= lag, or when that epoch
 *                   has been waited for already)
 *   status          HSM_OK, or HSM_ERR_HIP after a timed-out wait (text in hsm_last_error)
 * Every rank calls post the same number of times; post and wait of one exchange go on ONE stream (or streams the caller orders). */
typedef struct hsm_exchange hsm_exchange;
#define HSM_EXCHANGE_HANDLE_BYTES 64
#define HSM_EXCHANGE_MAX_WORLD 16
int hsm_exchange_create(int device, int rank, int world, int total_rows, int cols, int depth, hsm_exchange** out);
void hsm_exchange_destroy(hsm_exchange* x);
int hsm_exchange_handle(hsm_exchange* x, void* handle64);
int hsm_exchange_connect(hsm_exchange* x, const void* handles);
int hsm_exchange_connect_local(hsm_exchange* x, hsm_exchange* const* ranks);
int hsm_exchange_post(hsm_exchange* x, const float* d_rows, int first_row, int n_rows, void* stream);
int hsm_exchange_wait(hsm_exchange* x, float* d_out_all, void* stream);
int hsm_exchange_post_wait(hsm_exchange* x, const float* d_rows, int first_row, int n_rows, int lag, float* d_out_all,
                           void* stream);
/* hsm_match_batch_device + one exchange step of its poses (post this rank's `batch` rows at `first_row`, wait for the epoch `lag`
 * matches back into d_out_all or NULL) as ONE call: where the matcher form can, the launch carries the exchange itself -- every
 * wavefront posts its pose from the kernel's epilogue and a few extra workgroups at the end of the grid unpack -- so nothing at all
 * runs between two matcher launches; otherwise the stand-alone exchange kernel is queued behind the matcher.  Same epochs, same
 * mailbox contents either way (hsm_exchange_wait drains what is still in flight). */
int hsm_match_batch_device_gather(hsm_ctx* h, int batch, const float* d_begin_world, const float* d_pts_xy,
                                  const int* d_scan_offsets, int shared_n, float* d_out_pose, float* d_out_cov,
                                  hsm_exchange* x, int first_row, int lag, float* d_out_all, void* stream);
int hsm_exchange_epochs(const hsm_exchange* x, unsigned long long* posted, unsigned long long* waited);
int hsm_exchange_status(hsm_exchange* x);
/* "uncached" or "fine-grained": the kind of device memory the mailbox got */
const char* hsm_exchange_memory_kind(const hsm_exchange* x);

/* ---- host mirror support: replaces getGridMap(level) cell access --------------
 * HSL/slam_main/MapRepMultiMap.h:95, HSL/map/GridMapBase.h:141-159 */
int hsm_level_info(const hsm_ctx* h, int level, int* size_x, int* size_y, float* cell_length,
                   float* scale_to_map);
/* GridMapBase::getMapCoordsPose / getWorldCoordsPose         GridMapBase.h:226-239 */
int hsm_map_coords_pose(const hsm_ctx* h, int level, const float world[3], float map[3]);
int hsm_world_coords_pose(const hsm_ctx* h, int level, const float map[3], float world[3]);
/* GridMapBase::getUpdateIndex (bumped by every update, GridMapBase.h:343-344) */
int hsm_update_index(const hsm_ctx* h, int level);
/* whole level; either pointer may be NULL */
int hsm_download_level(hsm_ctx* h, int level, float* logodds, int* update_index);
/* hsm_upload_level replaces the planes and leaves the level's update counter (currUpdateIndex) where it is, as the reference's
 * cells would be if written directly.  The reference's cell rules test each cell's stored stamp against the marks of the scan
 * being integrated (counter + 1 / + 2, OccGridMapBase.h bresenhamCellFree / bresenhamCellOcc), and so do the kernels: a cell
 * restored with a stamp at or ahead of the counter stays FROZEN -- no update touches it -- until the counter has passed its
 * stamp (the counter advances by 3 per integrated scan); a stamp equal to a scan's free mark takes unsetFree in front of that
 * scan's occupied update.  Restoring into the context the planes came from is exact.  To restore into another context and get
 * live cells, upload stamps of -1, or hsm_reset and pass update_index == NULL (which keeps the stamps that are there). */
int hsm_upload_level(hsm_ctx* h, int level, const float* logodds, const int* update_index);
/* rows [y0, y1) of the log-odds plane only (cheap mirror refresh after an update) */
int hsm_download_rows(hsm_ctx* h, int level, int y0, int y1, float* logodds_rows);
/* cells [x0..x1] x [y0..y1] (inclusive) as the reference's LogOddsCell AoS
 * {float logOddsVal; int updateIndex} (GridMapLogOdds.h:89-100), written to dst_cells (= address
 * of cell (x0,y0) in a host grid whose rows are dst_pitch_cells cells apart): the host-mirror
 * refresh behind getGridMap() */
int hsm_download_cells(hsm_ctx* h, int level, int x0, int y0, int x1, int y1, void* dst_cells,
                       int dst_pitch_cells);
/* cell bounding box {x0, y0, x1, y1} (inclusive) touched by the last update of `level`: the last SCAN integrated, so after
 * hsm_update_by_scans* of several scans the box of the last of them only (hsm_take_dirty_bbox covers the whole call);
 * x1 < x0 when nothing was touched */
int hsm_last_update_bbox(const hsm_ctx* h, int level, int bbox[4]);
/* union of the cell boxes touched on `level` since the previous call (reset/upload mark the whole level),
 * then cleared: what a host mirror has to re-download.  x1 < x0 when nothing changed. */
int hsm_take_dirty_bbox(hsm_ctx* h, int level, int bbox[4]);

/* ---- a pyramid from one context into another, on the device ----------------------------------------------------------------
 * replaces: GridMapBase's copy constructor and operator= (HSL/map/GridMapBase.h:173-205: the cells, the dimensions, the
 * transforms and the update index), for a map that lives in HBM: fork a map per hypothesis, keep a checkpoint, roll an update
 * back, bring the replicas of a group back in line.  No host trip and no host wait.
 *
 * hsm_copy_map: afterwards every level of `dst` is what it is in `src` -- the log-odds and the stamps; the probabilities (and,
 * in the quad layout, the texels), bit for bit what a rebuild from those log-odds gives; the level's update counters
 * (currUpdateIndex, currMarkOccIndex, currMarkFreeIndex, lastUpdateIndex) and whether restored stamps are still ahead of the
 * counter, so a cell frozen in `src` (hsm_upload_level) is frozen in `dst`, and every later update gives the same bits in both.
 * `dst` keeps what is its own: the update factors, the update gate's state, the retained and the ingested scan, parity, layout
 * and batch-order settings.  Every level of `dst` is marked wholly changed, for hsm_take_dirty_bbox and for
 * hsm_occupancy_changes*.
 *
 * hsm_copy_map_boxes: the same for the cells of ONE box per level, boxes[4 * level ..] = x0, y0, x1, y1 inclusive, in HOST
 * memory; a level whose box is empty (x1 < x0) copies no cell.  The counters are copied as above.  The result is the full copy
 * if -- and only if -- `dst` equalled `src` outside the boxes: the boxes hsm_take_dirty_bbox(src, level) has returned since the
 * last copy into `dst` are such boxes.  In the quad layout the texels of each box grown by one cell towards lower x and y
 * (clamped to the level) are refreshed: texel (x, y) holds P(x+1, y), P(x, y+1) and P(x+1, y+1) as well.  `dst`'s dirty box and
 * publish box widen by each copied box.
 *
 * Ordering: the copy is QUEUED on `dst`'s stream and the call returns.  It reads `src` behind every update queued on `src` so
 * far, and writes `dst` behind the batched matches callers' streams may still be running on `dst`; every later hsm_* call on
 * `dst` is ordered behind it, and `src`'s stream -- so its next update -- is ordered behind the read.  If `src` has gated updates
 * outstanding (hsm_update_by_scans_device_gated, hsm_slam_*), the call first WAITS for `src`'s stream to fetch their count;
 * likewise for `dst`.  Two threads may copy in opposite directions (the contexts' locks are taken in address order).
 *
 * HSM_ERR_INVALID, nothing queued, nothing changed: a NULL context; dst == src; contexts that differ in level count, sizes,
 * resolution, offsets or layout; a box that is not empty and reaches outside its level; boxes == NULL (hsm_copy_map_boxes); a
 * caller's stream that either context has matched on being captured into a graph (copies are not captured, like every writer).
 *
 * Contexts on the same device: the kernel reads `src`'s planes directly.  On different devices the boxes' rows are first copied
 * (hipMemcpy2DAsync, on `dst`'s stream) into a staging patch that `dst` owns and grows on demand, and the same kernel reads the
 * patch.  HSM_COPY_STAGE=1 in the environment at `dst`'s hsm_create forces that route on one device as well, and that is the only
 * way it has been exercised: the cross-device copy itself has not been run. */
int hsm_copy_map(hsm_ctx* dst, hsm_ctx* src);
int hsm_copy_map_boxes(hsm_ctx* dst, hsm_ctx* src, const int* boxes);

/* ---- two maps into one: another context's pyramid merged into this one under a rigid transform, on the device ----------------
 * No counterpart in the reference (GridMapBase can only be copied, GridMapBase.h:173-205): an extension, like the window move and
 * relocalisation, pinned by the rule below.  Two robots' pyramids, two replicas fed different scans, a stored map and a live one.
 *
 * src_in_dst = (tx, ty, theta) in HOST memory, metres and radians: the pose of `src`'s world frame in `dst`'s world frame,
 * p_dst = R(theta) p_src + t.  The contexts must agree in level count, resolution and layout; they MAY differ in size and in
 * start coordinates (a 512 x 512 local map into a 4096 x 4096 global one).  `src` is only read.
 *
 * Cell rule, per level l, for every cell (x, y) of `dst`'s box (below); cells sit AT integer map coordinates.
 *   host, in double: c = cos(theta), s = sin(theta), b_l = scale_l * (R(-theta) (-off_dst - t) + off_src), with off the fp32
 *     offsets (resolution * size) * start of hsm_create widened to double and scale_l what hsm_level_info reports; c, s and
 *     b_l are then rounded to fp32.
 *   device, in fp32, every operation rounded, nothing fused: mx = (c x + s y) + b_l.x, my = ((-s) x + c y) + b_l.y,
 *     ix = (int)floorf(mx + 0.5f), iy likewise.
 *   v = `src`'s log-odds at (ix, iy) on level l if the cell exists, else 0; a NaN or an infinite log-odds counts as 0.  Nearest
 *     neighbour: stamps are not read.
 *   d = `dst`'s log-odds of (x, y):  v == 0: the cell is not written.  v < 0: d' = d + v.
 *     v > 0: d' = d < 50.0f ? fminf(d + v, 50.0f) : d -- the reference's gate on positive evidence (GridMapLogOdds.h:135-140)
 *     and a cap at 50: two saturated cells would otherwise sum past the range of expf and put NaN into the probabilities.
 * `dst`'s stamps, update counters, mark indices and restored-stamp state do not change: frozen cells stay frozen and later scans
 * integrate under the same cell rules as before.  hsm_update_index(dst, l) advances by one on every level, as after an update.
 * The update gate, the retained and the ingested scan and all settings are untouched.  The probabilities (and, in the quad
 * layout, the texels of each box grown by one cell towards lower x and y) are bit for bit what a rebuild from the new log-odds
 * gives.
 *
 * Box, per level: the four corners of `src`'s level rectangle [-0.5, sx_src - 0.5] x [-0.5, sy_src - 0.5] through the inverse
 * affine (in double) into `dst`'s map coordinates; their bounding box, from floor of the least to ceil of the greatest
 * coordinate, grown by one cell on every side and clamped to the level; {0, 0, -1, -1} where it misses the level.  The kernel
 * visits exactly this box, and `dst`'s dirty box (hsm_take_dirty_bbox) and publish box (hsm_occupancy_changes*) widen by it;
 * hsm_last_update_bbox is left alone.  hsm_merge_map_box returns the box of `level`: a pure host function, for sizing a mirror
 * refresh.  If every level's box is empty, hsm_merge_map returns HSM_OK, queues nothing, and the update index does not advance.
 *
 * Ordering: as hsm_copy_map.  QUEUED on `dst`'s stream; reads `src` behind every update queued on `src` so far, writes `dst`
 * behind the batched matches callers' streams may still be running on it; `src`'s next update is ordered behind the read.  The
 * call waits for `dst`'s stream only to fetch the boxes and gated-update counts device-side updates left there.  The contexts'
 * locks are taken in address order.
 *
 * HSM_ERR_INVALID, nothing queued, nothing changed: a NULL context or transform (hsm_merge_map_box: or bbox, or a level out of
 * range); dst == src; a transform component that is not finite; contexts that differ in level count, resolution or layout; a
 * caller's stream that either context has matched on being captured into a graph (hsm_merge_map).
 *
 * Contexts on the same device: the kernel reads `src`'s planes directly.  On different devices the rows of the `src` box that
 * `dst`'s box maps back to (the same corner construction the other way round, grown by one, clamped) are first copied
 * (hipMemcpy2DAsync on `dst`'s stream, log-odds only) into `dst`'s staging patch, and the same kernel reads the patch.
 * HSM_COPY_STAGE=1 in the environment at `dst`'s hsm_create forces that route on one device as well, and that is the only way it
 * has been exercised: the cross-device merge itself has not been run.
 *
 * Not covered: a transform in device memory, a group-wide merge, the C++ facade, weighted or bilinear resampling, merging
 * stamps, graph capture of the call. */
int hsm_merge_map(hsm_ctx* dst, hsm_ctx* src, const float src_in_dst[3]);
int hsm_merge_map_box(const hsm_ctx* dst, const hsm_ctx* src, const float src_in_dst[3], int level, int bbox[4]);

/* ---- the map window moved under the robot, on the device -------------------------------------------------------------------
 * The reference fixes a map's window at construction (MapRepMultiMap.h:48-72); a robot that reaches its edge loses its beams.
 * hsm_shift_map moves the window so that the context's geometry becomes that of hsm_create(..., new_start_x, new_start_y): the
 * same arithmetic on offsets derived from the new start coordinates (never accumulated: repeated moves do not drift), so the
 * same bits in hsm_level_info, hsm_map_coords_pose and hsm_world_coords_pose.  Cell contents keep their WORLD position: on level
 * l they move by d_l whole cells, cells that scroll in are cleared cells (log-odds 0, update index -1), cells that scroll out
 * are gone; probabilities (and texels) are what a rebuild from the moved log-odds gives.  Afterwards the context is
 * indistinguishable from one created with the new start coordinates into which the moved cells were loaded, except that it
 * keeps its update counters, mark indices, restored-stamp state, update factors, parity mode, the update gate's state (a world
 * pose) and the retained and ingested scans (sensor frame).  Every level is marked wholly changed for hsm_take_dirty_bbox and
 * for hsm_occupancy_changes* (the host's and the device's share of the publish box); hsm_last_update_bbox is empty.
 *
 * Displacement: with off = (resolution * size) * start per axis as hsm_create computes it in fp32,
 * d_0 = nearest integer of (off' - off) / cell_0 in double, and d_l = d_0 >> l.  shift_cells (may be NULL) receives level 0's
 * {dx, dy}.  start + k * 2^(levels - 1) / size per axis moves the window by k cells of the coarsest level.
 *
 * HSM_ERR_INVALID, nothing queued, nothing changed: a NULL context; a start coordinate that is not finite; a move further than
 * 1/64 cell of level 0 from a whole number of cells on either axis; a d_0 that is no multiple of 2^(levels - 1) on either axis;
 * a caller's stream that the context has matched on being captured into a graph (a move is not captured, like every writer).
 * A zero displacement with unchanged start coordinates is HSM_OK, queues nothing and changes nothing.
 *
 * Ordering: QUEUED on the context's stream behind every update queued so far and behind the batched matches callers' streams
 * may still be running on the map; no host wait (except to fetch the box and gate counters device-side updates left on the
 * device, as hsm_copy_map does).  The cells that survive travel through a staging block the context owns and grows on demand
 * (shared with hsm_copy_map's staged route); the planes keep their addresses.
 *
 * Graphs: a graph captured from a match entry BEFORE a move carries the old transforms in its kernel arguments and would match
 * in the old frame; capture it again after the move.
 *
 * Not covered: a group-wide move (the replicas of hsm_group_member can be moved one by one; hsm_group_sync_maps refuses
 * replicas whose offsets differ), the C++ facade (its host mirrors assume the constructor's geometry), and following the robot
 * automatically inside hsm_slam_scans_device. */
int hsm_shift_map(hsm_ctx* h, float new_start_x, float new_start_y, int shift_cells[2]);
/* the start coordinates the geometry currently derives from: hsm_create's, or the last accepted hsm_shift_map's */
int hsm_map_start(const hsm_ctx* h, float start[2]);

/* ---- the rows either side of the path; reference = the ROS node,
 *      hector_mapping/src/HectorMappingRos.cpp.  Optional: the facade does not need them. ---- */
/* replaces: rosLaserScanToDataContainer (HectorMappingRos.cpp:483-507): raw LaserScan ranges ->
 * DataContainer endpoints (fp32 running angle, range gate (range_min, range_max - 0.1f), ordered
 * compaction), computed on the device; the container STAYS on the device as the "ingested scan"
 * (origo = 0,0 like the reference).  The cos/sin table of the sensor geometry (angle_min,
 * angle_increment, n) is evaluated once on the host with the float libm calls the node uses and cached.
 * out_pts_xy (host, capacity 2*n floats, may be NULL) receives the endpoints, *out_n their count. */
int hsm_ingest_laser_scan(hsm_ctx* h, const float* ranges, int n, float angle_min, float angle_increment,
                          float range_min, float range_max, float scale_to_map, float* out_pts_xy, int* out_n);
/* replaces: rosPointCloudToDataContainer (HectorMappingRos.cpp:509-542), the node's DEFAULT ingestion
 * (use_tf_scan_transformation = true, :82,:257-282): n geometry_msgs::Point32 {x,y,z} floats in the laser
 * frame + the laser->base tf::Transform as 12 doubles, rows [R | t] (tfScalar is double).  Gates as the node:
 * x*x+y*y in (sqr_laser_min_dist, sqr_laser_max_dist), x < 0 && dist_sqr < 0.5 dropped, base-frame z minus
 * t_z in (laser_z_min, laser_z_max); endpoint = float(base x,y) * scale_to_map, ordered compaction.  The
 * container stays on the device with origo = float(t_x, t_y) * scale_to_map (also written to out_origo,
 * may be NULL); out_pts_xy capacity 2*n floats, may be NULL. */
int hsm_ingest_point_cloud(hsm_ctx* h, const float* pts_xyz, int n, const double tf_rows[12],
                           float sqr_laser_min_dist, float sqr_laser_max_dist, float laser_z_min, float laser_z_max,
                           float scale_to_map, float* out_pts_xy, int* out_n, float out_origo[2]);
/* the same with the step before it fused in: laser_geometry::LaserProjection::projectLaser(scan, cloud,
 * range_cutoff) (HectorMappingRos.cpp:273; third-party package, not in the reference tree -- restated from
 * its published algorithm: point = float((double)range * (cos, sin)(angle_min + (double)i * angle_increment)),
 * kept when range < range_cutoff && range >= range_min; range_cutoff < 0 means range_max), so raw
 * LaserScan.ranges[] (4 B/beam) is the wire format on the tf path as well. */
int hsm_ingest_laser_scan_tf(hsm_ctx* h, const float* ranges, int n, float angle_min, float angle_increment,
                             float range_min, float range_max, double range_cutoff, const double tf_rows[12],
                             float sqr_laser_min_dist, float sqr_laser_max_dist, float laser_z_min,
                             float laser_z_max, float scale_to_map, float* out_pts_xy, int* out_n,
                             float out_origo[2]);
/* replaces: rosLaserScanToDataContainer (HectorMappingRos.cpp:483-507) followed by MapRepMultiMap::matchData
 *           (HSL/slam_main/MapRepMultiMap.h:116-132), for B raw scans of ONE sensor geometry at once (extension: the
 *           node converts and matches one scan per callback).  Per scan the result is bit for bit what the node's
 *           conversion (the gate, scale and products of hsm_ingest_laser_scan) and a matchData of that container give
 *           (default mode; HSM_PARITY_FAST: what hsm_match_batch_device gives on that container).
 * DEVICE pointers (or device-accessible pinned host memory for d_ranges):
 *   d_begin_world  [B*3]    d_ranges [B*n] LaserScan.ranges[] of scan b at b*n.  Pinned host memory is read exactly once
 *                  (the first kernel copies it into the workspace); device memory is read by the gate and again by the
 *                  compaction.  Either way not after the call's kernels have run
 *   d_out_pose     [B*3]    d_out_cov [B*9] or NULL (in/out)    d_out_counts [B] or NULL: beams each scan kept
 *   d_workspace    caller-owned, at least hsm_match_batch_ranges_workspace(B, n) bytes, 8-byte aligned; holds the CSR
 *                  container (counts, int32 offsets, endpoints) until the match has run -- one workspace per stream in flight
 * The (cos, sin) table of the geometry (n, angle_min, angle_increment; keyed on their bit patterns) is evaluated on the
 * host with the node's running fp32 angle, uploaded once and kept until hsm_destroy.  A geometry not seen before while
 * `stream` is being captured into a graph returns HSM_ERR_INVALID and enqueues nothing (no allocation under capture: one
 * call with that geometry before capturing).  A new geometry allocates its table and copies it on `stream`, then waits for
 * `stream`: do not introduce one while another thread captures in the global capture mode.
 * `stream` is a hipStream_t (NULL = default stream); the call is asynchronous with the ordering contract of
 * hsm_match_batch_device: behind every map update queued so far, the next update behind it.  Conversion and match are
 * one stream-ordered sequence on the device, no host round trip between them.
 * A scan that keeps no beam returns its start pose and leaves its covariance untouched (ScanMatcher.h:68,189).
 * HSM_ERR_INVALID: null pointer, batch < 0, n < 0, workspace too small; HSM_ERR_TOO_LARGE: n > HSM_MAX_UPDATE_BEAMS
 * or batch * n > INT_MAX.  Nothing is launched in either case. */
int hsm_match_batch_ranges_device(hsm_ctx* h, int batch, const float* d_begin_world, const float* d_ranges, int n,
                                  float angle_min, float angle_increment, float range_min, float range_max,
                                  float scale_to_map, float* d_out_pose, float* d_out_cov, int* d_out_counts,
                                  void* d_workspace, size_t workspace_bytes, void* stream);
/* bytes of hsm_match_batch_ranges_device's workspace for `batch` scans of n beams; 0 for sizes the entry refuses.
 * Host arithmetic only: callable without a device. */
size_t hsm_match_batch_ranges_workspace(int batch, int n);
/* the same with HOST pointers (begin_world [B*3], ranges [B*n], out_pose [B*3], out_cov [B*9] or NULL (in/out),
 * out_counts [B] or NULL): copies 4 B per beam in, one device call on the context's stream, results out; synchronous.
 * The workspace is the context's own. */
int hsm_match_batch_ranges(hsm_ctx* h, int batch, const float* begin_world, const float* ranges, int n,
                           float angle_min, float angle_increment, float range_min, float range_max, float scale_to_map,
                           float* out_pose, float* out_cov, int* out_counts);
/* replaces: the node's DEFAULT ingestion (use_tf_scan_transformation, HectorMappingRos.cpp:82,:257-282) -- projectLaser,
 *           the laser -> base_link transform and rosPointCloudToDataContainer (:509-542) -- for B raw scans of ONE sensor
 *           geometry at once, each with its own transform (extension: the node converts one scan per callback; base_link
 *           attitude from an IMU changes R every scan).  Per scan the container and its origo are bit for bit what
 *           hsm_ingest_laser_scan_tf gives: point = float((double)range * (cos, sin)(angle_min + (double)i * angle_increment)),
 *           kept when range < range_cutoff && range >= range_min (range_cutoff < 0 means range_max); x*x + y*y in
 *           (sqr_laser_min_dist, sqr_laser_max_dist), x < 0 && dist_sqr < 0.5 dropped; the transform in fp64 without FMA;
 *           base-frame z minus t_z in (laser_z_min, laser_z_max); endpoint = float(base x, y) * scale_to_map, kept beams in
 *           beam order.  CONVERSION ONLY: reads no map, touches neither the retained nor the ingested scan.
 * DEVICE pointers:
 *   d_ranges       [B*n] LaserScan.ranges[] of scan b at b*n, device-accessible; read once by each of the two passes and not
 *                  after the call's kernels have run
 *   d_tf_rows      [B*12] doubles, rows [R | t] of scan b's laser -> base transform at b*12; with shared_tf != 0 one [12] block
 *                  that every scan uses.  8-byte aligned
 *   d_out_pts_xy   caller-owned, capacity max(B*n, 1) * 2 floats (the matcher clamps an empty scan's loads to element 0)
 *   d_out_offsets  [B+1] int32 CSR offsets in points        d_out_counts [B] beams each scan kept; REQUIRED: it is the
 *                  entry's only scratch
 *   d_out_origo    [B*2] or NULL: origo of scan b = float(t_x, t_y) * scale_to_map (:517)
 * The outputs are exactly the d_pts_xy / d_scan_offsets arguments of hsm_match_batch_device, hsm_score_batch_device,
 * hsm_match_score_batch_device, hsm_update_by_scans_device[_gated][_origos] and hsm_slam_scans_device[_origos]; pass n as
 * shared_n / max_beams, it is a true bound of every scan's length, and d_out_origo as d_origos of the *_origos entries.
 * The unit-vector table of the geometry (n, angle_min, angle_increment; keyed on their bit patterns) is evaluated on the host
 * with the double cos / sin that laser_geometry uses, uploaded once and kept until hsm_destroy.  A geometry not seen before
 * while `stream` is being captured into a graph returns HSM_ERR_INVALID and enqueues nothing (no allocation under capture: one
 * call with that geometry before capturing); a new geometry allocates its table, copies it on `stream` and waits for `stream`.
 * With a known geometry a capture records three kernel launches and nothing is allocated.
 * `stream` is a hipStream_t (NULL = default stream); the call is asynchronous and ordered by `stream` alone -- it waits for
 * no map update and none waits for it.  The context lock is held for the geometry cache only.
 * HSM_ERR_INVALID, nothing launched: NULL context, batch < 0, n < 0, NULL d_ranges with batch*n > 0, NULL d_tf_rows with
 * batch > 0, NULL d_out_pts_xy / d_out_offsets / d_out_counts, an unseen geometry under capture.  HSM_ERR_TOO_LARGE:
 * n > HSM_MAX_UPDATE_BEAMS or batch * n > INT_MAX.  batch == 0: HSM_OK, nothing written.
 * Not built: a fused conversion + match device entry with a workspace (this call and hsm_match_batch_device on one stream are
 * the same launches; conversion + the whole scan loop in one call is hsm_slam_ranges_tf_device); the C++ facade; hsm_group_*. */
int hsm_ingest_batch_ranges_tf_device(hsm_ctx* h, int batch, const float* d_ranges, int n, float angle_min,
                                      float angle_increment, float range_min, float range_max, double range_cutoff,
                                      const double* d_tf_rows, int shared_tf, float sqr_laser_min_dist,
                                      float sqr_laser_max_dist, float laser_z_min, float laser_z_max, float scale_to_map,
                                      float* d_out_pts_xy, int* d_out_offsets, int* d_out_counts, float* d_out_origo,
                                      void* stream);
/* the same conversion followed by MapRepMultiMap::matchData (HSL/slam_main/MapRepMultiMap.h:116-132) per scan, with HOST
 * pointers (begin_world [B*3], ranges [B*n], tf_rows [B*12] or [12] with shared_tf, out_pose [B*3], out_cov [B*9] or NULL
 * (in/out), out_counts [B] or NULL, out_origo [B*2] or NULL): copies 4 B per beam and 96 B per scan in, runs the conversion and
 * then hsm_match_batch_device's path on the context's stream, copies the results out; synchronous.  The staging block is the
 * context's own.  The origo plays no part in a match (it is the update's); a scan that keeps no beam returns its start pose
 * and leaves its covariance untouched (ScanMatcher.h:68,189).  Errors as above, and NULL begin_world / out_pose. */
int hsm_match_batch_ranges_tf(hsm_ctx* h, int batch, const float* begin_world, const float* ranges, int n, float angle_min,
                              float angle_increment, float range_min, float range_max, double range_cutoff,
                              const double* tf_rows, int shared_tf, float sqr_laser_min_dist, float sqr_laser_max_dist,
                              float laser_z_min, float laser_z_max, float scale_to_map, float* out_pose, float* out_cov,
                              int* out_counts, float* out_origo);
/* replaces: the node's scan callback for a LOG of raw scans (HectorMappingRos.cpp:257-282 + HectorSlamProcessor.h:71-95) --
 *           hsm_ingest_batch_ranges_tf_device for the whole log, then hsm_slam_scans_device_origos on what it wrote, in ONE
 *           call: raw ranges and a transform per scan in; poses, covariances, decisions and the map out.  The host waits for
 *           nothing and learns nothing in between -- not a count, not an origo.
 * Arguments as in the two entries (DEVICE pointers; d_start_pose / d_hint_deltas / d_force / d_out_cov / d_out_applied /
 * d_out_counts may be NULL as there; d_out_counts [count] = beams each scan kept).  A scan that keeps no beam returns its hint
 * as its pose, its covariance row is what hsm_match_batch_device writes for an empty scan.
 *   d_workspace    caller-owned, 8-byte aligned, hsm_slam_ranges_tf_workspace(count, n) bytes: the conversion's counts, CSR
 *                  offsets, origos and end points; the update reads them, so it stays unchanged until the call's work has run
 * `stream` (the caller's, NULL = default stream) is waited for once in front -- the inputs must be complete there -- and waits
 * once behind; the conversion's three launches and the loop's launches all go on the context's stream.  Ordering against
 * other hsm_* calls is hsm_slam_scans_device's.  The geometry-table rules of hsm_ingest_batch_ranges_tf_device apply: a geometry
 * not seen before is uploaded before anything is queued (that one call waits for the context's stream).
 * Every argument is checked before the first launch.  HSM_ERR_INVALID, nothing queued: count < 0, n < 0, NULL d_out_pose,
 * NULL d_ranges with count*n > 0, NULL or misaligned d_tf_rows, a workspace that is NULL, misaligned or too small, `stream` / a
 * stream this context has matched on is being captured (updates are not captured; so an unseen geometry under capture is
 * refused, too).  HSM_ERR_TOO_LARGE: n > HSM_MAX_UPDATE_BEAMS or count * n > INT_MAX.  count == 0: HSM_OK, nothing written.
 * Not built: capture into graphs, replay through hsm_group_*, the byte-map (dense) form of the update, the non-tf conversion
 * (rosLaserScanToDataContainer: its origo is always 0,0 -- hsm_match_batch_ranges_device's conversion and
 * hsm_slam_scans_device cover it in two calls); the C++ facade's HectorSlamProcessor.h stays reference code. */
int hsm_slam_ranges_tf_device(hsm_ctx* h, int count, const float* d_start_pose, const float* d_hint_deltas,
                              const float* d_ranges, int n, float angle_min, float angle_increment, float range_min,
                              float range_max, double range_cutoff, const double* d_tf_rows, int shared_tf,
                              float sqr_laser_min_dist, float sqr_laser_max_dist, float laser_z_min, float laser_z_max,
                              float scale_to_map, const unsigned char* d_force, float* d_out_pose, float* d_out_cov,
                              int* d_out_applied, int* d_out_counts, void* d_workspace, size_t workspace_bytes, void* stream);
/* bytes of that workspace (0 for sizes the entry refuses).  Host arithmetic only: callable without a device. */
size_t hsm_slam_ranges_tf_workspace(int count, int n);
/* the same with HOST pointers (start_pose [3] or NULL, hint_deltas [count*3] or NULL, ranges [count*n], tf_rows [count*12] or
 * [12] with shared_tf, force [count] or NULL, out_pose [count*3], out_cov [count*9] or NULL (in/out), out_applied [count] or
 * NULL, out_counts [count] or NULL, out_origo [count*2] or NULL): copies 4 B per beam and 96 B per scan in, makes the one
 * device call on the context's stream, copies the results out; synchronous.  The staging block is the context's own. */
int hsm_slam_ranges_tf(hsm_ctx* h, int count, const float* start_pose, const float* hint_deltas, const float* ranges, int n,
                       float angle_min, float angle_increment, float range_min, float range_max, double range_cutoff,
                       const double* tf_rows, int shared_tf, float sqr_laser_min_dist, float sqr_laser_max_dist,
                       float laser_z_min, float laser_z_max, float scale_to_map, const unsigned char* force, float* out_pose,
                       float* out_cov, int* out_applied, int* out_counts, float* out_origo);
/* hsm_match / hsm_update_by_scan on the ingested scan (no endpoint upload; origo as ingested) */
int hsm_match_ingested(hsm_ctx* h, const float begin_world[3], float out_pose_world[3], float cov[9]);
int hsm_update_by_ingested(hsm_ctx* h, const float pose_world[3]);
/* replaces: OccGridMapUtil::getLikelihoodForState (HSL/map/OccGridMapUtil.h:184-214) evaluated for
 * `batch` MAP-frame states of `level` against one scan (pts: level-0 units, scaled by 2^-level here):
 * out_lh[b] = 1 - sum_i(1 - M_i)/n -- the particle-weight primitive of the batched-hypotheses use case.
 * Host pointers. */
int hsm_likelihood_states(hsm_ctx* h, int level, int batch, const float* states_map, const float* pts_xy, int n,
                          float* out_lh);
/* replaces: OccGridMapUtil::getResidualForState (HSL/map/OccGridMapUtil.h:205-221): out_residual[b] =
 * sum_i (1 - M_i), same arguments as hsm_likelihood_states. */
int hsm_residual_states(hsm_ctx* h, int level, int batch, const float* states_map, const float* pts_xy, int n,
                        float* out_residual);
/* ---- scoring and ranking a batch of pose hypotheses on the device (extension: the reference scores one state per call) ----
 * replaces: OccGridMapUtil::getLikelihoodForState / getResidualForState (HSL/map/OccGridMapUtil.h:184-221) at
 *           GridMapBase::getMapCoordsPose(pose) (HSL/map/GridMapBase.h:235-239), for B (pose, scan) pairs at once: the
 *           weighting step behind hsm_match_batch_device.  DEVICE pointers:
 *   d_poses_world  [B*3] WORLD poses -- what hsm_match_batch_device writes to d_out_pose; converted to the map frame of
 *                  `level` in the kernel
 *   d_pts_xy, d_scan_offsets, shared_n   as in hsm_match_batch_device (CSR offsets in points, or NULL = every hypothesis looks
 *                  at the one scan d_pts_xy[0 .. shared_n); with offsets shared_n is ignored).  Level-0 units, scaled by
 *                  (float)(1 / 2^level) in the kernel (DataContainer::setFrom)
 *   d_out_likelihood [B] = 1 - residual / (float)n       d_out_residual [B] = sum_i (1 - M_i); either may be NULL, not both.
 *                  A scan of 0 beams: residual +0, likelihood NaN (1 - 0/0, as the reference computes it)
 * HSM_PARITY_AUTO / _EXACT: the residual is summed in the reference's beam order, both outputs are bit-identical to the
 * reference for every hypothesis.  HSM_PARITY_FAST / _RELAXED: lane-strided partial sums + tree, as hsm_likelihood_states.
 * hsm_last_launch_parity / hsm_last_launch_kernel ("score_batch_kernel") report the launch.
 * Ordering, capture and locking: the contract of hsm_match_batch_device, through the same bookkeeping.  Asynchronous on
 * `stream` (a hipStream_t, NULL = default stream); ordered behind every map update queued on the context so far and the next
 * update behind it, per caller stream.  Under graph capture the call records one kernel launch and allocates nothing; at
 * capture time the host waits for the updates queued so far; the caller orders the replays against later updates; while a
 * stream this context has scored or matched on is being captured, every map update fails with HSM_ERR_INVALID and queues
 * nothing.  The call needs no workspace and keeps no per-stream or per-context device state.  It does not touch the retained
 * or the ingested scan.
 * HSM_ERR_INVALID (nothing launched): NULL context, level out of range, batch < 0, both outputs NULL, shared_n < 0 without
 * offsets, NULL poses, NULL points for a shared scan of shared_n > 0.  batch == 0: HSM_OK. */
int hsm_score_batch_device(hsm_ctx* h, int level, int batch, const float* d_poses_world, const float* d_pts_xy,
                           const int* d_scan_offsets, int shared_n, float* d_out_likelihood, float* d_out_residual,
                           void* stream);
/* no reference counterpart: the best hypothesis of every group (one group per physical scan / robot; one group of all
 * hypotheses is the particle-filter case).  DEVICE pointers:
 *   d_group_offsets [G+1] CSR offsets into d_scores, or NULL = G groups of group_size consecutive entries
 *   d_scores        what hsm_score_batch_device wrote (any floats)      d_poses_world [*3] or NULL
 *   d_out_index [G] index, into the whole score array, of the group's highest score.  A NaN never wins; among equal scores
 *                   (compared as floats: +0 == -0) the LOWEST index wins; an empty or all-NaN group gives -1
 *   d_out_score [G] or NULL: that score, NaN for -1
 *   d_out_pose_world [G*3] or NULL (needs d_poses_world): that hypothesis's pose, copied bit for bit; untouched for -1
 * The result is a function of the scores alone: the reduction runs on the pair (score, index), uses no atomics and does not
 * depend on the launch shape.  Reads no map, so it is ordered by `stream` only; asynchronous, allocates nothing, capturable.
 * HSM_ERR_INVALID: NULL context, groups < 0, NULL d_out_index, group_size < 0 without offsets, NULL scores where there are
 * entries, d_out_pose_world without d_poses_world.  groups == 0: HSM_OK. */
int hsm_select_best_device(hsm_ctx* h, int groups, const int* d_group_offsets, int group_size, const float* d_scores,
                           const float* d_poses_world, int* d_out_index, float* d_out_score, float* d_out_pose_world,
                           void* stream);
/* hsm_match_batch_device, then hsm_score_batch_device of its d_out_pose on score_level into d_out_likelihood / d_out_residual,
 * then -- groups > 0 -- hsm_select_best_device over d_out_likelihood and d_out_pose into d_out_index / d_out_score /
 * d_out_best_pose: queued on `stream` under ONE lock of the context, no host wait in between; the same bits as the three calls.
 * All arguments are checked before the first launch (groups > 0 needs d_out_likelihood and d_out_index, and groups * group_size
 * <= batch without group offsets). */
int hsm_match_score_batch_device(hsm_ctx* h, int batch, const float* d_begin_world, const float* d_pts_xy,
                                 const int* d_scan_offsets, int shared_n, float* d_out_pose, float* d_out_cov, int score_level,
                                 float* d_out_likelihood, float* d_out_residual, int groups, const int* d_group_offsets,
                                 int group_size, int* d_out_index, float* d_out_score, float* d_out_best_pose, void* stream);
/* the same with HOST pointers, built like hsm_match_batch (copies in, the chain on the context's stream, copies out;
 * synchronous).  out_cov, out_residual, out_score and out_best_pose may be NULL; out_best_pose is in/out (a group without a
 * winner keeps the caller's values); group offsets are checked against batch. */
int hsm_match_score_batch(hsm_ctx* h, int batch, const float* begin_world, const float* pts_xy, const int* scan_offsets,
                          int shared_n, float* out_pose, float* out_cov, int score_level, float* out_likelihood,
                          float* out_residual, int groups, const int* group_offsets, int group_size, int* out_index,
                          float* out_score, float* out_best_pose);
/* ---- sigma-point covariances of a batch of pose hypotheses on the device (extension: the reference estimates one per call) ----
 * replaces: OccGridMapUtil::getCovarianceForPose (HSL/map/OccGridMapUtil.h:106-160) followed by getCovMatrixWorldCoords
 *           (:162-188) -- the block commented out at ScanMatcher.h:134-147 -- at GridMapBase::getMapCoordsPose(pose)
 *           (HSL/map/GridMapBase.h:235-239), for B (pose, scan) pairs at once: the uncertainty behind hsm_match_batch_device,
 *           whose own d_out_cov is the Gauss-Newton Hessian.  DEVICE pointers:
 *   d_poses_world, d_pts_xy, d_scan_offsets, shared_n   as in hsm_score_batch_device (WORLD poses, converted to the map frame of
 *                  `level` in the kernel; CSR offsets in points or one shared scan; level-0 units, scaled in the kernel)
 *   d_out_cov_world [B*9], d_out_cov_map [B*9]   column major      d_out_lh7 [B*7]   the likelihoods of the seven sigma points of
 *                  :119-125 around the map-frame pose, in that order: x +- 1.5 cells, y +- 1.5 cells, angle +- 0.05 rad, the pose
 *   d_out_likelihood [B]   sigma point 6 again, contiguous: the same bits as hsm_score_batch_device's likelihood of the same
 *                  batch, so that it can go straight into hsm_select_best_device
 *   Any of the four may be NULL, not all.  A scan of 0 beams: every likelihood and every covariance entry NaN (1 - 0/0, as the
 *   reference computes it).  (The reference prints the likelihoods to stdout on every call, :136; this entry does not.)
 * HSM_PARITY_AUTO / _EXACT: every residual is summed in the reference's beam order, all outputs are bit-identical to the reference
 * for every hypothesis.  HSM_PARITY_FAST / _RELAXED: lane-strided partial sums + tree, the bits of hsm_covariance_for_poses in that
 * mode.  hsm_last_launch_parity / hsm_last_launch_kernel ("covariance_batch_kernel") report the launch.
 * Ordering, capture, locking and batch == 0: the contract of hsm_score_batch_device, through the same bookkeeping -- reads the map
 * only, needs no workspace, keeps no per-stream or per-context state, one kernel node under capture.
 * HSM_ERR_INVALID (nothing launched, hsm_last_error() names the entry): NULL context, level out of range, batch < 0, all four
 * outputs NULL, shared_n < 0 without offsets, NULL poses, NULL points for a shared scan of shared_n > 0.
 * Not built: replay through hsm_group_*, a covariance inside hsm_relocalize_device or the scan-log loop. */
int hsm_covariance_batch_device(hsm_ctx* h, int level, int batch, const float* d_poses_world, const float* d_pts_xy,
                                const int* d_scan_offsets, int shared_n, float* d_out_cov_world, float* d_out_cov_map,
                                float* d_out_lh7, float* d_out_likelihood, void* stream);
/* replaces: MapRepMultiMap::matchData followed by the covariance estimate above at every matched pose.
 * hsm_match_batch_device, then hsm_covariance_batch_device of its d_out_pose on cov_level, then -- groups > 0 --
 * hsm_select_best_device over d_out_likelihood and d_out_pose into d_out_index / d_out_score / d_out_best_pose: queued on `stream`
 * under ONE lock of the context, no host wait in between; the same bits as the three calls.  d_out_cov (the match's Hessian) stays
 * a separate, optional output.  All arguments are checked before the first launch (groups > 0 needs d_out_likelihood and
 * d_out_index, and groups * group_size <= batch without group offsets). */
int hsm_match_cov_batch_device(hsm_ctx* h, int batch, const float* d_begin_world, const float* d_pts_xy, const int* d_scan_offsets,
                               int shared_n, float* d_out_pose, float* d_out_cov, int cov_level, float* d_out_cov_world,
                               float* d_out_cov_map, float* d_out_lh7, float* d_out_likelihood, int groups,
                               const int* d_group_offsets, int group_size, int* d_out_index, float* d_out_score,
                               float* d_out_best_pose, void* stream);
/* replaces: getCovarianceForPose + getCovMatrixWorldCoords as above -- hsm_covariance_batch_device with HOST pointers: copies in,
 * the kernel on the context's stream, copies out; synchronous.  scan_offsets (host) must start at 0 and not decrease. */
int hsm_covariance_batch(hsm_ctx* h, int level, int batch, const float* poses_world, const float* pts_xy, const int* scan_offsets,
                         int shared_n, float* out_cov_world, float* out_cov_map, float* out_lh7, float* out_likelihood);
/* ---- relocalisation: one scan against a WINDOW of poses on the device map (extension: hector_mapping has no recovery once
 * the matcher has left its basin) ----
 * A window is a DEVICE centre d_center_world[3] (so that it can be the d_out_pose of a match or of hsm_slam_* without a host
 * trip), HOST steps step[3] (m, m, rad; finite) and HOST half-extents half[3] >= 0.  It holds W = (2hx+1)(2hy+1)(2ht+1)
 * hypotheses that never exist in memory; hypothesis w = (k*(2hy+1) + j)*(2hx+1) + i is, every operation fp32 and un-fused:
 *   x = cx + (float)(i - hx) * step_x;   y = cy + (float)(j - hy) * step_y;   theta = ctheta + (float)(k - ht) * step_theta
 * (theta is not normalised).
 *
 * hsm_score_window_device
 * replaces: OccGridMapUtil::getLikelihoodForState / getResidualForState (HSL/map/OccGridMapUtil.h:184-221) at
 *           GridMapBase::getMapCoordsPose(pose_w) for every pose of the window against ONE scan d_pts_xy[0 .. n) (level-0 units,
 *           scaled by (float)(1 / 2^level) in the kernel).  d_out_likelihood [W] / d_out_residual [W]: either may be NULL, not
 *           both; the same bits as hsm_score_batch_device in its reference-order mode gives on the written-out poses.  n == 0:
 *           residual +0, likelihood NaN.
 * One kernel launch in one of two forms that give the same bits -- a lane per hypothesis, each lane walking beams 0 .. n-1
 * itself, or a wavefront per hypothesis (the shape of score_batch_kernel); the entry chooses by W, env HSM_WINDOW_FORM=lane|wave
 * at hsm_create forces one, hsm_last_launch_kernel names the one that ran ("score_window_lane_kernel" /
 * "score_window_wave_kernel").  The residual is summed in the reference's beam order in EVERY parity mode (a lane owns a whole
 * chain, a tree sum would buy nothing): hsm_last_launch_parity reports HSM_PARITY_EXACT after this entry whatever hsm_set_parity
 * asked for.
 * Ordering, capture and locking: the contract of hsm_score_batch_device, through the same bookkeeping -- reads the map only,
 * needs no workspace, keeps no state, one kernel node under capture.
 * HSM_ERR_INVALID (nothing launched): NULL context, level out of range, a negative half-extent, W > INT_MAX, a non-finite step,
 * n < 0, both outputs NULL, NULL centre, steps or half-extents, NULL points where n > 0.
 * Not built: replay through hsm_group_*, a C++ facade entry, non-maximum suppression among candidates.  (A window per scan of a
 * batch of different scans: hsm_score_windows_batch_device below.) */
#define HSM_MAX_TOPK 64
int hsm_score_window_device(hsm_ctx* h, int level, const float* d_center_world, const float step[3], const int half[3],
                            const float* d_pts_xy, int n, float* d_out_likelihood, float* d_out_residual, void* stream);
/* the same with HOST pointers (the centre too): copies in, the kernel on the context's stream, copies out; synchronous. */
int hsm_score_window(hsm_ctx* h, int level, const float center_world[3], const float step[3], const int half[3],
                     const float* pts_xy, int n, float* out_likelihood, float* out_residual);
/* window indices as poses: d_out_pose[3c ..] = the world pose of hypothesis d_index[c], c < count, by the arithmetic above; an
 * index of -1 or outside [0, W) writes three quiet NaNs.  d_index == NULL: indices 0 .. count-1 (count <= W), the window written
 * out.  One small launch, ordered by `stream` alone (reads no map), capturable.  HSM_ERR_INVALID: NULL context, a bad window (as
 * above), count < 0, NULL output where count > 0, count > W without indices. */
int hsm_window_poses_device(hsm_ctx* h, const float* d_center_world, const float step[3], const int half[3], const int* d_index,
                            int count, float* d_out_pose, void* stream);
/* the K best of d_scores[0 .. count) in rank order, by the strict total order of hsm_select_best_device: a NaN never takes
 * part, the higher score first, equal scores (+0 == -0) the lower index first.  d_out_index [k]; d_out_score [k] or NULL; where
 * fewer than k entries take part the remaining places are -1 and NaN.  1 <= k <= HSM_MAX_TOPK.  The result is a function of the
 * scores alone (no float atomics, no dependence on launch shape).  Two launches: slices of the array reduced to k candidates each
 * in the caller-owned d_workspace of at least hsm_select_topk_workspace(count, k) bytes (4-byte aligned), merged by one workgroup.
 * Nothing is allocated: capturable; reads no map: ordered by `stream` alone.
 * Neighbouring cells of one peak can fill all k places: non-maximum suppression is not built.  One winner per heading slice is
 * hsm_select_best_device with group_size = (2hx+1)(2hy+1) followed by hsm_window_poses_device.
 * HSM_ERR_INVALID: NULL context, count < 0, k out of range, NULL indices, NULL scores where count > 0, a workspace that is NULL,
 * misaligned or too small. */
int hsm_select_topk_device(hsm_ctx* h, int count, const float* d_scores, int k, int* d_out_index, float* d_out_score,
                           void* d_workspace, size_t workspace_bytes, void* stream);
/* host arithmetic, callable without a device; a multiple of 8; 0 for refused sizes (count < 0, k out of range) */
size_t hsm_select_topk_workspace(int count, int k);
/* One call, everything queued on `stream` under one lock of the context, no host wait:
 *   1. hsm_score_window_device on search_level (likelihoods into the workspace)     2. hsm_select_topk_device, k
 *   3. hsm_window_poses_device of the k indices        4. hsm_match_score_batch_device on the k poses and the shared scan, with
 *   score_level 0 and one group of k;  then d_out_best_index[0], the winner's place among the k, is replaced by the WINDOW index
 *   its start came from (-1 if none).
 * The same bits as the four public calls.  d_out_cand_pose [k*3] the refined poses, d_out_cand_cov [k*9] or NULL,
 * d_out_cand_likelihood [k] on level 0, d_out_best_pose [3] (left as it is where there is no winner), d_out_best_score [1] or
 * NULL, d_out_best_index [1].  Where fewer than k window scores take part the remaining starts are NaN poses: the matcher returns
 * a non-finite pose for them, their likelihood is 0 (every beam outside the map) or NaN, and they lie behind every filled place,
 * so they never win over one.  d_workspace: at least hsm_relocalize_workspace(W, k) bytes, 8-byte aligned.
 * Every argument is checked before the first launch.  Ordering is hsm_match_batch_device's; capturable (a replay with a new
 * centre or scan written into the same buffers gives the new answer); the retained and the ingested scan are not touched.
 * HSM_ERR_INVALID: the refusals of hsm_score_window_device, k out of range, a NULL required output, a workspace that is NULL,
 * misaligned or too small. */
int hsm_relocalize_device(hsm_ctx* h, int search_level, const float* d_center_world, const float step[3], const int half[3], int k,
                          const float* d_pts_xy, int n, void* d_workspace, size_t workspace_bytes, float* d_out_cand_pose,
                          float* d_out_cand_cov, float* d_out_cand_likelihood, float* d_out_best_pose, float* d_out_best_score,
                          int* d_out_best_index, void* stream);
/* host arithmetic, callable without a device; a multiple of 8; 0 for refused sizes (window_count < 1, k out of range) */
size_t hsm_relocalize_workspace(int window_count, int k);
/* the same with HOST pointers, built like hsm_match_score_batch (copies in, the chain on the context's stream, copies out;
 * synchronous).  out_cand_cov and out_best_score may be NULL; out_best_pose is in/out. */
int hsm_relocalize(hsm_ctx* h, int search_level, const float center_world[3], const float step[3], const int half[3], int k,
                   const float* pts_xy, int n, float* out_cand_pose, float* out_cand_cov, float* out_cand_likelihood,
                   float* out_best_pose, float* out_best_score, int* out_best_index);

/* ---- relocalisation of a BATCH of scans, each in its own window of one shared shape (extension, as above: several matches that
 * left their basin at once, or a loop-closure search over old scans, against one map) ----
 * The windows share the HOST steps step[3] and half-extents half[3], so each holds the same W hypotheses; window b lies around
 * the DEVICE centre d_centers_world[3b ..] and is scored against scan b.  The scans are the pair the other batched entries take:
 * d_pts_xy with d_scan_offsets [batch + 1] (CSR, in points; they start at 0 and do not decrease), or d_scan_offsets == NULL and
 * ONE scan of shared_n beams for every window (with offsets shared_n is the matcher's sizing hint in hsm_match_batch_device and
 * is not looked at here).
 *
 * hsm_score_windows_batch_device
 * replaces: batch calls of hsm_score_window_device, window b and scan b, in ONE kernel launch.  d_out_likelihood [batch * W] /
 *           d_out_residual [batch * W], window b at [b * W, (b + 1) * W): either may be NULL, not both; the same bits as the
 *           batch calls.  A scan of 0 beams: residual +0, likelihood NaN.
 * Two forms that give the same bits -- a wavefront per hypothesis b * W + w, or a lane per hypothesis with every window padded to
 * whole wavefronts, so that the 64 lanes of a wavefront walk one scan; the entry chooses by batch * W, env HSM_WINDOW_FORM=lane|wave
 * forces one, hsm_last_launch_kernel names the one that ran ("score_windows_batch_lane_kernel" / "score_windows_batch_wave_kernel").
 * The reference's beam order in every parity mode: hsm_last_launch_parity reports HSM_PARITY_EXACT.
 * Ordering, capture and locking: the contract of hsm_score_window_device -- reads the map only, needs no workspace, keeps no
 * state, one kernel node under capture.  batch == 0: HSM_OK, nothing launched.
 * HSM_ERR_INVALID (nothing launched): the refusals of hsm_score_window_device, batch < 0, batch * W > INT_MAX, NULL centres where
 * batch > 0, shared_n < 0 without offsets, NULL points for a shared scan of shared_n > 0.
 * Not built: replay through hsm_group_*, a C++ facade entry, a window shape per scan, non-maximum suppression among candidates. */
int hsm_score_windows_batch_device(hsm_ctx* h, int level, int batch, const float* d_centers_world, const float step[3],
                                   const int half[3], const float* d_pts_xy, const int* d_scan_offsets, int shared_n,
                                   float* d_out_likelihood, float* d_out_residual, void* stream);
/* the K best of each of `groups` runs of group_size scores, d_scores[g * group_size ..]: hsm_select_topk_device's rule (a NaN
 * never takes part, the higher score first, equal scores the lower index first) for every group on its own.  d_out_index
 * [groups * k], indices RELATIVE to the group, in rank order; d_out_score [groups * k] or NULL; unfilled places -1 and NaN.  Two
 * launches however many groups: every group's slices reduced to k candidates each in the caller-owned d_workspace of at least
 * hsm_select_topk_groups_workspace(groups, group_size, k) bytes (4-byte aligned), then one workgroup per group merges them.  No
 * float atomics; a function of the scores alone; capturable; ordered by `stream` alone.  groups == 1: bit for bit
 * hsm_select_topk_device, which is this launch.  groups == 0: HSM_OK, nothing launched.
 * HSM_ERR_INVALID: NULL context, groups < 0, group_size < 0, k out of range, groups * group_size or groups * k above INT_MAX,
 * NULL indices, NULL scores where group_size > 0, a workspace that is NULL, misaligned or too small. */
int hsm_select_topk_groups_device(hsm_ctx* h, int groups, int group_size, const float* d_scores, int k, int* d_out_index,
                                  float* d_out_score, void* d_workspace, size_t workspace_bytes, void* stream);
/* host arithmetic, callable without a device; a multiple of 8; hsm_select_topk_workspace(group_size, k) for one group; 0 for
 * refused sizes and for groups == 0 */
size_t hsm_select_topk_groups_workspace(int groups, int group_size, int k);
/* One call, everything queued on `stream` under one lock of the context, no host wait:
 *   1. hsm_score_windows_batch_device on search_level (likelihoods into the workspace)
 *   2. hsm_select_topk_groups_device, groups = batch, group_size = W
 *   3. the start poses of the batch * k indices, index (b, r) around centre b (-1: three quiet NaNs)
 *   4. hsm_match_score_batch_device on the batch * k pairs, candidate (b, r) against scan b, with score_level 0 and batch groups
 *      of k;  then d_out_best_index[b] is replaced by the WINDOW index the winner's start came from (-1 if none).
 * Per scan the outputs of hsm_relocalize_device: d_out_cand_pose [batch*k*3], d_out_cand_cov [batch*k*9] or NULL,
 * d_out_cand_likelihood [batch*k], d_out_cand_index [batch*k] or NULL (the window indices of the starts, -1 for an unfilled
 * place), d_out_best_pose [batch*3] (a scan without a winner leaves its three as they are), d_out_best_score [batch] or NULL,
 * d_out_best_index [batch].  In the reference's summation order (the default) the same bits as batch calls of
 * hsm_relocalize_device; in HSM_PARITY_FAST / _RELAXED the matcher's sums are those of ONE launch of batch * k pairs, whose form
 * follows batch * k and the mean scan length -- the bits of the single calls where these plan the same form (DESIGN.md "which form
 * runs when").
 * The batch matcher takes one scan per pair, so CSR scans are first laid out k times in the workspace by a copy kernel.  The host
 * must know the bytes: total_points is the caller's statement of d_scan_offsets[batch].  The copy clamps every scan into
 * [0, total_points] and never writes beyond its region whatever the offsets hold (offsets that break the rule above give
 * meaningless candidates, nothing else).  A shared scan is not copied, and total_points is not looked at.
 * d_workspace: at least hsm_relocalize_batch_workspace(batch, W, k, total_points) bytes (total_points = 0 for a shared scan),
 * 8-byte aligned.  Every argument is checked before the first launch.  Ordering is hsm_match_batch_device's; capturable (a replay
 * with new centres or scans written into the same buffers gives the new answer).  batch == 0: HSM_OK, nothing launched.
 * HSM_ERR_INVALID (nothing launched, outputs untouched): the refusals of hsm_score_windows_batch_device and of
 * hsm_relocalize_device, batch * k > INT_MAX / 9, with offsets total_points < 0 or k * total_points > INT_MAX, a NULL required
 * output, a workspace that is NULL, misaligned or too small.
 * Not built: replay through hsm_group_*, a C++ facade entry, a window shape per scan, non-maximum suppression among candidates. */
int hsm_relocalize_batch_device(hsm_ctx* h, int search_level, int batch, const float* d_centers_world, const float step[3],
                                const int half[3], int k, const float* d_pts_xy, const int* d_scan_offsets, int shared_n,
                                int total_points, void* d_workspace, size_t workspace_bytes, float* d_out_cand_pose,
                                float* d_out_cand_cov, float* d_out_cand_likelihood, int* d_out_cand_index, float* d_out_best_pose,
                                float* d_out_best_score, int* d_out_best_index, void* stream);
/* host arithmetic, callable without a device; a multiple of 8; 0 for refused sizes (batch < 0, window_count < 1, k out of range,
 * total_points < 0, batch * window_count or k * total_points above INT_MAX, batch * k above INT_MAX / 9) */
size_t hsm_relocalize_batch_workspace(int batch, int window_count, int k, int total_points);
/* the same with HOST pointers, built like hsm_relocalize (copies in, the chain on the context's stream, copies out; synchronous).
 * scan_offsets (host) must start at 0 and not decrease; their last entry is the number of points.  out_cand_cov, out_cand_index
 * and out_best_score may be NULL; out_best_pose is in/out. */
int hsm_relocalize_batch(hsm_ctx* h, int search_level, int batch, const float* centers_world, const float step[3], const int half[3],
                         int k, const float* pts_xy, const int* scan_offsets, int shared_n, float* out_cand_pose,
                         float* out_cand_cov, float* out_cand_likelihood, int* out_cand_index, float* out_best_pose,
                         float* out_best_score, int* out_best_index);

/* ---- another context's map aligned to this one, ready to merge: occupied cells as a point set, then the relocalisation --------
 * No counterpart in the reference: an extension, like hsm_merge_map, whose src_in_dst this produces.  Two entries.
 *
 * hsm_occupied_points_device: the occupied cells of a cell box of `level` of `src`, thinned, as points in level-0 units.
 * Which cells count: a cell (x, y) of `level` inside the inclusive bbox {x0, y0, x1, y1} (NULL: the whole level) is OCCUPIED when
 *   its log-odds is > 0.0f: isOccupied of GridMapLogOdds.h:76-84, the cells hsm_occupancy_grid reports as 100.  NaN and +-0 are
 *   not occupied.  The box is clamped to the level; {0, 0, -1, -1} or a box that misses the level gives no cells.
 * Order and thinning: occupied cells are ranked in row-major order of the box, y outer and x inner, rank 0 first.  The cell of
 *   rank r is KEPT when r % every == 0, every >= 1 (by rank, not by lattice: an axis-aligned wall does not vanish).
 * Output: kept cell number j, in rank order, goes to d_out_pts_xy[2j .. 2j+1] if j < max_points; nothing beyond
 *   2 * min(kept, max_points) floats is touched.  The order depends on the map alone: no atomics on the output index, no
 *   dependence on the launch shape.
 * The point of a cell: (wx, wy) = the level's world-from-map transform applied to ((float)x, (float)y), t0 + (l00 * x + l01 * y)
 *   in fp32, every operation rounded, nothing fused, then each coordinate times hsm_scale_to_map(src) in fp32: the bits of the
 *   host's hsm_world_coords_pose(src, level, {x, y, 0}) followed by that multiplication.  (The device's and the host's form of
 *   the transform agree in operation order.)
 * Counts: d_out_count[0] the points written, d_out_count[1] the cells kept before the max_points cap: truncation shows.
 * Form: a counting pass per tile of the box, a scan of the tile counts, a scatter pass.  The tile counts live in the
 *   caller-owned d_workspace of at least hsm_occupied_points_workspace(cells of the clamped box) bytes, 8-byte aligned (the
 *   level's cell count always suffices).  Nothing is allocated: capturable, as a reader of the map.
 * Ordering and locking: the contract of hsm_score_window_device -- queued on `stream` behind every update queued on `src`, `src`'s
 *   next writer behind the read, no host wait; under capture the launches go into the graph and the caller orders replays.
 * HSM_ERR_INVALID, nothing queued, outputs untouched: NULL context, level out of range, every < 1, max_points < 0, NULL counts,
 *   NULL points where max_points > 0, a workspace that is NULL, misaligned or too small.
 *
 * hsm_occupied_points: the same with HOST pointers, on the context's stream, its device arrays and workspace staged in the
 * context's batch staging block; synchronous.  out_pts_xy receives 2 * count[0] floats and is touched no further.
 *
 * hsm_align_map: guess -> src_in_dst as hsm_merge_map defines it (p_dst = R(theta) p_src + t).  The points of `src`'s box are a
 * scan given in `src`'s world frame, and the matcher's "sensor pose" of such a scan on `dst` is src_in_dst.  Synchronous, HOST
 * pointers, one chain on `dst`'s stream:
 *   (a) hsm_occupied_points of (src, src_level, src_bbox, every, max_points) into `dst`'s staging block, ordered as a reader of
 *       `src`;
 *   (b) the 8 bytes of counts come down: THE ONE HOST WAIT of the chain, because every later entry takes n from the host;
 *   (c) hsm_relocalize on `dst` with the window (step, half) centred on the guess, k starts, n = count[0] points;
 *   (d) the winner comes down: out_src_in_dst its refined pose, out_cov[9] (or NULL) the matcher covariance of the place it took
 *       among the k, out_likelihood (or NULL) its level-0 likelihood, out_window_index (or NULL) the window index its start came
 *       from, out_counts[2] (or NULL) the counts of (a).
 * Bit for bit what hsm_occupied_points followed by hsm_relocalize with center_world = guess and out_best_pose seeded with the
 * guess give.  No winner -- no occupied cell, or every window score NaN: HSM_OK, out_src_in_dst = the guess, likelihood NaN,
 * window index -1, out_cov untouched.  Neither map is written; stamps, counters and boxes of both stay.
 * HSM_MAX_ALIGN_POINTS is the densest scan the benchmark's configurations send through the matcher; a larger max_points is
 * refused: thin with `every`.  hsm_align_map_workspace(cells, window_count, k, max_points): the bytes of `dst`'s staging block
 * the call carves (grown on demand, kept), host arithmetic, a multiple of 8, 0 for refused sizes.
 * The contexts' locks are taken in address order, as hsm_merge_map does.
 * HSM_ERR_INVALID, nothing queued: the refusals of hsm_merge_map on the pair (a NULL context, dst == src, contexts that differ in
 * level count, resolution or layout), those of hsm_relocalize, those of hsm_occupied_points, max_points > HSM_MAX_ALIGN_POINTS,
 * a NULL out_src_in_dst, contexts on different devices (hsm_merge_map's cross-device route has itself never been run).
 *
 * Not built: a device-resident count (it would free the chain of its host wait and make it capturable, and needs n in device
 * memory throughout the matcher); hsm_merge_map with the transform in device memory; alignment across devices or through
 * hsm_group_*; points weighted by log-odds; free cells as points; the C++ facade. */
#define HSM_MAX_ALIGN_POINTS 16384
/* host arithmetic, callable without a device; a multiple of 8; 0 for cells < 0 */
size_t hsm_occupied_points_workspace(int cells);
int hsm_occupied_points_device(hsm_ctx* src, int level, const int bbox[4], int every, int max_points, float* d_out_pts_xy,
                               int* d_out_count, void* d_workspace, size_t workspace_bytes, void* stream);
int hsm_occupied_points(hsm_ctx* src, int level, const int bbox[4], int every, int max_points, float* out_pts_xy, int count[2]);
size_t hsm_align_map_workspace(int cells, int window_count, int k, int max_points);
int hsm_align_map(hsm_ctx* dst, hsm_ctx* src, int src_level, const int src_bbox[4], int every, int max_points, int search_level,
                  const float guess_src_in_dst[3], const float step[3], const int half[3], int k, float out_src_in_dst[3],
                  float out_cov[9], float* out_likelihood, int out_counts[2], int* out_window_index);
/* replaces: OccGridMapUtil::getCovarianceForPose (HSL/map/OccGridMapUtil.h:106-160) and
 * getCovMatrixWorldCoords (:162-188) for `batch` MAP-frame poses of `level`: seven sigma points per pose
 * (x +- 1.5 cells, y +- 1.5 cells, angle +- 0.05 rad, the pose), likelihood-weighted sample covariance.
 * out_cov_map / out_cov_world: batch x 9 floats, column major; out_lh7: batch x 7 likelihoods in the
 * reference's sigma-point order.  Any of the three may be NULL.  (The reference prints the likelihoods to
 * stdout on every call, :136; this entry does not.) */
int hsm_covariance_for_poses(hsm_ctx* h, int level, int batch, const float* poses_map, const float* pts_xy, int n,
                             float* out_cov_map, float* out_cov_world, float* out_lh7);
/* replaces: hectormaptools::DistanceMeasurementProvider::getDist (hector_map_tools/include/hector_map_tools/
 * HectorMapTools.h:133-234, behind hector_map_server's services) for `n` rays on `level`, with the
 * OccupancyGrid metadata the node publishes (origin = getWorldCoords(0,0) - cell/2, resolution = cell length,
 * HectorMappingRos.cpp:546-553): out_dist[i] = resolution * (int) cell distance to the first occupied cell, or
 * -resolution when there is none; out_hit_xy[2i..] = its world coordinates (left untouched without a hit).
 * Host pointers; out_hit_xy may be NULL. */
int hsm_ray_distances(hsm_ctx* h, int level, float origin_x, float origin_y, float resolution, int n,
                      const float* begin_world_xy, const float* end_world_xy, float* out_dist, float* out_hit_xy);
/* ---- expected scans on the device-resident map (extension: the reference answers one ray per service call) ----
 * hsm_ray_distances with DEVICE pointers, asynchronous on `stream`: the same kernel walk and, for every ray of finite
 * coordinates, the same bits.  A ray with a non-finite end-point coordinate is "without a hit" here (-resolution, hit untouched);
 * hsm_ray_distances leaves that case to the device's float -> int conversion.  d_out_hit_xy may be NULL.
 * Ordering, capture and locking: the contract of hsm_score_batch_device, through the same bookkeeping -- reads the map only,
 * needs no workspace, keeps no per-stream or per-context device state; ordered behind every map update queued on the context so
 * far and the next update behind it; under graph capture one kernel launch and no allocation; the retained and the ingested scan
 * are not touched.  hsm_last_launch_kernel: "ray_distance_kernel".
 * HSM_ERR_INVALID (nothing launched): NULL context, level out of range, n < 0, NULL begin, end or distances where n > 0,
 * resolution not > 0.  n == 0: HSM_OK.
 * Not built: replay through hsm_group_*, a C++ facade entry. */
int hsm_ray_distances_device(hsm_ctx* h, int level, float origin_x, float origin_y, float resolution, int n,
                             const float* d_begin_world_xy, const float* d_end_world_xy, float* d_out_dist,
                             float* d_out_hit_xy, void* stream);
/* replaces: getDist for the n beams of a scan fan at each of `batch` sensor poses -- batch * n rays that never exist in memory.
 * DEVICE pointers:
 *   d_poses_world [batch*3]  the SENSOR's world pose (x, y, theta); the caller folds in any mount offset
 *   d_beam_angles [n]        sensor frame, rad -- a table, so the caller decides how the angles were accumulated (the node adds
 *                            angle_increment in fp32)
 * Beam i of pose b, every operation fp32 and un-fused, in this order:
 *   a = theta + beam_angles[i];  (s, c) = sincosf(a) (glibc's, bit for bit);
 *   begin = (px, py);  end = (px + range_max * c, py + range_max * s);  getDist(begin, end)
 * on the level's OWN OccupancyGrid metadata, computed once on the host in fp32: origin = getWorldCoords(0,0) - cell * 0.5f per
 * axis, resolution = the cell length (HectorMappingRos.cpp:546-553).
 *   d_out_ranges [batch*n]   [b*n+i] = resolution * (float)(int)|begin cell - hit cell|, or -resolution WITHOUT A HIT: no occupied
 *                            cell among the steps walked, either end point outside the level (so a beam that leaves the map
 *                            reports no hit even where it crosses a wall first -- the reference's behaviour at the map's edge),
 *                            the walk's cap of 5000 steps (bresenham2D's max_length: an occupied cell further along is not
 *                            seen), or a non-finite end-point coordinate (a non-finite pose)
 *   d_out_hit_xy [batch*n*2] or NULL: the hit cell's world coordinates; left untouched for a ray without a hit
 * One kernel launch in one of two shapes that give the same bits -- a lane per beam with 64 adjacent beams of a pose in a
 * wavefront, or a wavefront per beam for fans of fewer than 32 beams; hsm_last_launch_kernel says which ("cast_scans_lane_kernel" /
 * "cast_scans_wave_kernel"), env HSM_CAST_FORM=wave|lane at hsm_create forces one.
 * Ordering, capture and locking: as hsm_ray_distances_device.
 * HSM_ERR_INVALID (nothing launched): NULL context, level out of range, batch < 0, n < 0, batch * n > INT_MAX, range_max
 * negative or non-finite, NULL poses, angles or ranges where batch * n > 0.  batch == 0 or n == 0: HSM_OK, nothing launched.
 * Not built: replay through hsm_group_*, a C++ facade entry. */
int hsm_cast_scans_device(hsm_ctx* h, int level, int batch, const float* d_poses_world, const float* d_beam_angles, int n,
                          float range_max, float* d_out_ranges, float* d_out_hit_xy, void* stream);
/* the same with HOST pointers: copies in, the kernel on the context's stream, copies out; synchronous.  out_hit_xy is in/out
 * (a ray without a hit keeps the caller's values) and may be NULL. */
int hsm_cast_scans(hsm_ctx* h, int level, int batch, const float* poses_world, const float* beam_angles, int n,
                   float range_max, float* out_ranges, float* out_hit_xy);
/* replaces: publishMap's cell loop (HectorMappingRos.cpp:449-468) with LogOddsCell::isFree/isOccupied
 * (GridMapLogOdds.h:76-84): -1 unknown, 0 free (logOdds < 0), 100 occupied (logOdds > 0).
 * out: host, sx*sy bytes, row major. */
int hsm_occupancy_grid(hsm_ctx* h, int level, signed char* out);
/* replaces: the same loop with the grid left in DEVICE memory: d_out, sx*sy bytes, row major, any alignment.  Asynchronous:
 * the conversion runs on the context's stream, behind every update queued so far and in front of every later one; `stream`
 * (the caller's, NULL = default stream) is waited for once in front -- d_out may still be in use there -- and waits once
 * behind, so work queued on it afterwards sees the grid.  The host waits for nothing.  Leaves the publish box of
 * hsm_occupancy_changes* alone.  HSM_ERR_INVALID, nothing queued: a NULL context or grid, a level out of range, or `stream` /
 * a stream this context has matched on is being captured into a graph.
 * Not built: capture into graphs, replay through hsm_group_*, a C++ facade entry (the node's publishMap reads the host
 * mirror). */
int hsm_occupancy_grid_device(hsm_ctx* h, int level, signed char* d_out, void* stream);
/* replaces: publishMap's cell loop (HectorMappingRos.cpp:435-481) restricted to the cells that can differ from the grid
 *           published before: every level keeps a PUBLISH box, the hull of the cells whose log-odds may have changed since
 *           the level was last exported -- widened by every update, on the host or on the device, and independent of the
 *           mirror's box (hsm_take_dirty_bbox and these entries never consume each other's box).
 *   d_grid      DEVICE, the caller's persistent sx*sy byte grid of this level, row major, any alignment.  Only cells inside
 *               the exported box are written (-1 / 0 / 100 as above); every other byte keeps its value.
 *   d_out_bbox  DEVICE, 4 ints, may be NULL: the exported box x0,y0,x1,y1 (inclusive), or 0,0,-1,-1 when nothing changed.
 * After the call the level's publish box is empty.  The first export of a level is the whole level; so is the first after
 * hsm_reset, hsm_upload_level or hsm_occupancy_restart.  A scan that a gated call rejected widens nothing.  The box is a
 * hull: it holds every changed cell and may hold unchanged ones, which are written with the value they have.
 * ONE consumer per level and context: whoever calls this (or hsm_occupancy_changes) for a level empties that level's box, so
 * two grids fed from the same level would each miss the other's changes.
 * Stream rules, ordering and refusals of hsm_occupancy_grid_device; a refused call leaves the publish box as it was.  The
 * host never learns the box: one preparation launch of one wavefront, one conversion launch whose shape does not depend on it.
 * Not built: capture into graphs, replay through hsm_group_*, a C++ facade entry. */
int hsm_occupancy_changes_device(hsm_ctx* h, int level, signed char* d_grid, int* d_out_bbox, void* stream);
/* the same into a HOST grid (sx*sy bytes, row major): converts into the context's staging grid, fetches the box and copies
 * the box's rows and columns only (a 2-D copy at pitch sx); bbox[4] receives the box, 0,0,-1,-1 when nothing changed (then
 * `grid` is not written).  Synchronous: waits for the context's stream.  Shares the level's publish box with
 * hsm_occupancy_changes_device: one consumer per level. */
int hsm_occupancy_changes(hsm_ctx* h, int level, signed char* grid, int bbox[4]);
/* the next hsm_occupancy_changes* of `level` (-1 = every level) exports the whole level: for a consumer that lost or
 * replaced its grid.  Host bookkeeping only, nothing is queued. */
int hsm_occupancy_restart(hsm_ctx* h, int level);

/* ---- what the map's other consumers draw from: known extents, the map image, pose tiles ------------------------------------
 * One cell rule for the six entries below, publishMap's: a log-odds < 0 is free, > 0 occupied, anything else (+0, -0, NaN)
 * unknown.  Image bytes are map_to_image_node's: free 255, occupied 0, unknown 127.  A cell is KNOWN when it is free or
 * occupied.  On every plane without a NaN that is GridMapBase::getMapExtends's `getValue() != 0.0f`; a NaN cell is unknown here
 * because the published grid says -1 for it (the reference's float test would call it known).  Everything is integer and
 * comparison work: equal to the reference loops byte for byte and box for box.
 * The three device entries follow hsm_occupancy_grid_device: the work runs on the context's stream, behind every update queued
 * so far and in front of every later one; `stream` (the caller's, NULL = default stream) is waited for once in front and waits
 * once behind; the host waits for nothing.  HSM_ERR_INVALID, nothing queued and no output touched: a NULL context, a level
 * out of range, a NULL output where there is something to write, or `stream` / a stream this context has matched on is being
 * captured into a graph.  None of the six touches the map, its stamps, the publish box of hsm_occupancy_changes* or the
 * mirror's dirty box.
 * Not built: capture into graphs, replay through hsm_group_*, a C++ facade entry, a crop box in device memory (extents ->
 * image without the host learning the size), the GeoTIFF writer's Qt drawing, rotated tiles. */
/* replaces: GridMapBase::getMapExtends (GridMapBase.h:334-383) and HectorMapTools::getMapExtends
 *           (hector_map_tools/HectorMapTools.h:241-290; hector_geotiff's setupTransforms, geotiff_writer.cpp:129, crops
 *           everything it draws to it): the bounding box of every known cell of `level`.
 *   d_out_box  DEVICE, 4 ints: x0, y0, x1, y1, the INCLUSIVE hull -- GridMapBase's (xMin, yMin, xMax, yMax) -- or 0, 0, -1, -1
 *              without a known cell, where the reference returns false.  HectorMapTools's topLeft / bottomRight are
 *              (x0, y0) / (x1 + 1, y1 + 1).
 * One pass over the plane (16-byte loads, minima and maxima folded per wavefront and workgroup, then integer atomic minima,
 * which commute: the box does not depend on the launch shape) and one finishing launch of one thread, the only writer of
 * d_out_box. */
int hsm_map_extents_device(hsm_ctx* h, int level, int* d_out_box, void* stream);
/* the same into HOST memory; synchronous: waits for the context's stream */
int hsm_map_extents(hsm_ctx* h, int level, int box[4]);
/* replaces: map_to_image_node's full image (hector_compressed_map_transport/src/map_to_image_node.cpp:98-140) with crop ==
 *           NULL; with a crop to the extents, the cells the GeoTIFF writer draws from.
 *   crop   HOST, 4 ints, an inclusive cell box x0, y0, x1, y1, or NULL = the whole level.  It is clamped to the level; with
 *          the clamped box w = x1 - x0 + 1 and hgt = y1 - y0 + 1.  A crop that misses the level: HSM_OK, nothing written.
 *   d_out  DEVICE, w * hgt bytes, any alignment: d_out[r * w + c] = byte(logodds[(y1 - r) * sx + x0 + c]) -- image row 0 is
 *          the box's TOP map row.  No byte beyond w * hgt is touched. */
int hsm_map_image_device(hsm_ctx* h, int level, const int crop[4], unsigned char* d_out, void* stream);
/* the same into HOST memory (converted into the context's staging grid and copied); synchronous */
int hsm_map_image(hsm_ctx* h, int level, const int crop[4], unsigned char* out);
/* replaces: map_to_image_node's tile image (map_to_image_node.cpp:143-235; there one 64 x 64 window around the robot's pose)
 *           for a batch of poses: local occupancy patches around matched poses or hypotheses.
 *   d_poses_world  DEVICE [batch * 3] x, y, theta: the layout every batched entry writes.  theta is not read (the reference's
 *                  tile is not rotated).
 *   d_out_tiles    DEVICE [batch * tile_w * tile_h] bytes, any alignment, tiles contiguous:
 *                  tile b, [r * tile_w + c] = byte(logodds[(hi_y - 1 - r) * sx + lo_x + c])
 *   d_out_boxes    DEVICE [batch * 4] ints or NULL: lo_x, lo_y, hi_x - 1, hi_y - 1 of every tile
 * Per pose and axis, the reference's arithmetic in its order (:147-193), on the level's OWN OccupancyGrid metadata computed once
 * on the host in fp32 as for hsm_cast_scans_device, from the current map start (after hsm_shift_map too): origin =
 * getWorldCoords(0,0) - cell * 0.5f, inv = 1.0f / cell length;
 *   m = (int)((p - origin) * inv)  (fp32, un-fused, truncation toward zero);  lo = max(m - tile / 2, 0);  hi = lo + tile;
 *   where hi > size: lo -= hi - size, hi = size;  lo = max(lo, 0).
 * Where the reference is undefined: the map coordinate (p - origin) * inv of a finite p is clamped in float to +-2^30 in front
 * of the conversion (the clamps then give the window on the level's edge); a non-finite x or y gives a tile of 127 throughout and
 * the box 0, 0, -1, -1.
 * One launch for the whole batch, straight from the log-odds plane (no grid of the level in between): a tile's row is a
 * contiguous run of floats, read by 16-byte loads and written by packed 4-byte stores where the caller's memory is aligned, byte
 * stores for the ragged ends; narrow tiles share a wavefront by rows, a large tile is shared by several wavefronts.
 * HSM_ERR_INVALID besides the common refusals: batch < 0, tile_w < 1, tile_h < 1, tile_w > sx or tile_h > sy (the reference's
 * shrunken tile on a map smaller than the window is not built), batch * tile_w * tile_h > INT_MAX, NULL poses or tiles where
 * batch > 0.  batch == 0: HSM_OK, nothing queued. */
int hsm_map_tiles_device(hsm_ctx* h, int level, int batch, const float* d_poses_world, int tile_w, int tile_h,
                         unsigned char* d_out_tiles, int* d_out_boxes, void* stream);
/* the same with HOST pointers: poses in, the kernel on the context's stream, tiles and boxes out; synchronous */
int hsm_map_tiles(hsm_ctx* h, int level, int batch, const float* poses_world, int tile_w, int tile_h, unsigned char* out_tiles,
                  int* out_boxes);

/* ---- parity / debug entry points (used by tests, not by the facade) ------------ */
/* device probability plane p = e^l/(e^l+1) (GridMapLogOdds.h:163-166) */
int hsm_download_prob(hsm_ctx* h, int level, float* prob);
/* one evaluation of OccGridMapUtil::getCompleteHessianDerivs (OccGridMapUtil.h:64-104)
 * at a MAP-frame pose with level-scaled points */
int hsm_hessian_derivs(hsm_ctx* h, int level, const float pose_map[3], const float* pts_level_xy,
                       int n, float H[9], float dTr[3]);
/* per-beam terms of the same evaluation: out[4*i] = M, dM/dx, dM/dy, rotDeriv */
int hsm_eval_beams(hsm_ctx* h, int level, const float pose_map[3], const float* pts_level_xy,
                   int n, float* out4);
/* ScanMatcher::matchData on one level with explicit max_iterations (ScanMatcher.h:54) */
int hsm_match_level(hsm_ctx* h, int level, const float begin_world[3], const float* pts_level_xy,
                    int n, int max_iterations, float out_pose_world[3], float cov[9]);

/* test hook: set the 12-bit per-scan generation counter of `level`'s key planes (it wraps every 4095
 * updates -- 27 minutes at 40 Hz -- and the wrap path has to be exercised without running that long) */
int hsm_debug_set_update_serial(hsm_ctx* h, int level, unsigned serial);
/* test hook: out[0] = non-zero 32-bit words of `level`'s crossed-cell byte map (dense scans), out[1] = non-zero words of its
 * end-cell bitmap (scans below 4096 beams).  Both planes carry no generation tag: every update's apply pass clears exactly
 * what its mark passes set, so BETWEEN updates both counts must be 0 (waits for the queued updates first) */
int hsm_debug_marks_nonzero(hsm_ctx* h, int level, unsigned long long out[2]);
/* test hook: set the monotonic arrival counter of the cooperative matcher's grid barrier (it advances by
 * workgroups x GN steps per dense match and wraps at 2^32) */
int hsm_debug_set_coop_barrier(hsm_ctx* h, unsigned value);
/* gn_match_spec_kernel (one scan per workgroup, reference order, speculative carries: csrc/spec_chain.h): counters of its
 * stitching passes since the last call -- out[0] segments settled, [1] unused (0), [2] accepted by the shift rule, [3] re-run
 * literally.  enable != 0 keeps counting (zeroed by every call), 0 stops.  Results never
 * depend on these numbers: they only say how fast the exact form ran. */
int hsm_debug_spec_stats(hsm_ctx* h, int enable, unsigned long long out[4]);
/* test hook: workgroup `block_plus_one - 1` of the multi-workgroup dense matcher (HSM_PARITY_FAST / _RELAXED, >= 4096 beams)
 * never publishes its partial sums (0 = off) -- the exchange of every workgroup then times out, which is what a device that
 * cannot keep the K workgroups co-resident looks like.  hsm_match handles that by matching the scan again on the
 * one-workgroup matcher; hsm_debug_coop_fallbacks() counts how often it had to. */
int hsm_debug_set_coop_mute(hsm_ctx* h, int block_plus_one);
int hsm_debug_coop_fallbacks(hsm_ctx* h);
/* test hook: batched entries (hsm_match_batch, hsm_match_batch_device and the ranges entries) restrict matchData to `level`
 * with `gn_steps` steps (1 + maxIterations); level < 0 restores the schedule.  Single-scan entries are not affected. */
int hsm_debug_set_schedule(hsm_ctx* h, int level, int gn_steps);
/* test hook: the sort that hsm_set_batch_order puts in front of a batch, alone: d_perm_out[slot] = scan for `batch` start poses
 * (DEVICE pointers, asynchronous on `stream`), by the 64 x 64 level-0 tile of each start pose in Morton order; with
 * HSM_ORDER_AUTO its map-order detection may return the identity.  Runs whatever the map size and batch size; no other effect. */
int hsm_debug_batch_order(hsm_ctx* h, int batch, const float* d_begin_world, int* d_perm_out, void* stream);
/* device sincosf of n angles (glibc's algorithm, csrc/libm_exact.h) -- numerics test hook */
int hsm_debug_sincos(hsm_ctx* h, int n, const float* x, float* s, float* c);
/* device expf(x) and getGridProbability(x) = e/(e+1) of n values -- numerics test hook */
int hsm_debug_expf(hsm_ctx* h, int n, const float* x, float* out_exp, float* out_prob);

/* the context's device: {HIP ordinal, compute units, shader clock kHz, memory clock kHz} (roofline arithmetic of bench.py) */
int hsm_device_info(const hsm_ctx* h, int info[4]);

/* Measurement aid (no reference counterpart): d_stamps4 = device pointer to four 64-bit words, or NULL to switch it
 * off.  While set, a batched match by a texel-cache form (tree summation: the wavefront of scan 0; reference-order
 * summation: the first wavefront of workgroup 0 of the 4096-scan form, which launches a probed instantiation that is 0.4 us
 * slower) stores {shader-clock counter (s_memtime), 100 MHz wall clock} as taken at its start [0,1] and at its end [2,3]:
 * (s[2]-s[0]) / (s[3]-s[1]) * 100 MHz = the clock the kernel actually ran at (bench.py prices the VALU roof at it next
 * to the nominal 2.4 GHz).  The caller owns the memory. */
int hsm_set_clock_probe(hsm_ctx* h, unsigned long long* d_stamps4);
/* GN steps one full hsm_match performs per scan (4 per coarse level + 6) */
int hsm_gn_iterations_per_match(const hsm_ctx* h);
/* effective kernel configuration of the last match launch:
 * {layout, waves_per_scan, block, grid, beams_per_lane (0 = endpoints streamed from memory; negative =
 * the texel-cache form: that many beams per lane with endpoints in LDS and the last texel of every beam
 * kept in VGPRs)} */
int hsm_last_launch_config(const hsm_ctx* h, int cfg[5]);
/* name of the matcher kernel of the last match launch ("gn_match_exact_cached_kernel", "gn_match_exact_dense_kernel", ...): what
 * bench.py looks up in the rocprofv3 kernel trace; a static string */
const char* hsm_last_launch_kernel(const hsm_ctx* h);

const char* hsm_last_error(void);
const char* hsm_version(void);

#ifdef __cplusplus
}
#endif
#endif /* HECTOR_MI355_CAPI_H */
