// window.hip -- the entries of the C ABI (include/hector_mi355/capi.h) that search a window of poses around a centre on the
// device-resident map: the likelihood of one scan at every pose of the window (hsm_score_window_device, hsm_score_window), window
// indices as poses (hsm_window_poses_device), the K best of an array of scores (hsm_select_topk_device) and the chain
// window score -> top K -> poses -> match -> score on level 0 -> winner (hsm_relocalize_device, hsm_relocalize); and the same for
// a batch of scans, each in its own window of one shared shape (hsm_score_windows_batch_device, hsm_select_topk_groups_device,
// hsm_relocalize_batch_device, hsm_relocalize_batch): one launch per stage whatever the batch.  The kernels are
// in window_kernels.h (the score of one hypothesis: pose_score.h), the window's arithmetic and the workspace sizes in
// window_grid.h.  Single and batched entries differ in the score kernels they launch and in nothing else: one form rule on the
// number of hypotheses, one launch helper (window_score_launch), one chain behind the score (relocalize_after_score, one group
// or `batch` groups), one workspace layout.  The scoring entries read the map like a batched score and are ordered like one
// (MapReader of hsm_ctx.h); the chain's tail is match_chain_nolock of match.hip.
// Also here, because the chain ends in the relocalisation: a level's occupied cells as a point set (hsm_occupied_points*, the
// kernels in map_points_kernels.h) and another context's map aligned to this one (hsm_align_map): extraction from the other
// context, the counts fetched, the relocalisation of those points on this one.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>

#include <mutex>

#include "hector_mi355/capi.h"
#include "hsm_ctx.h"
#include "map_points_kernels.h"
#include "window_kernels.h"

using namespace hsm;
using namespace hsm_host;

static_assert(HSM_MAX_TOPK == kMaxTopK, "capi.h and window_grid.h disagree on K");
static_assert(HSM_MAX_ALIGN_POINTS <= HSM_MAX_UPDATE_BEAMS, "an aligned point set is a scan the matcher takes");

namespace {

// Launches of at least this many hypotheses -- W of a single window, B * W of a batch of B -- take a lane per hypothesis, smaller
// ones a wavefront per hypothesis (either gives the same bits).  A lane-per-hypothesis launch is never shorter than one lane's
// walk over one whole scan, whatever the batch; the wave form grows by 1.9 us per 1000 hypotheses.  Measured, 1081-beam scans of
// the 2048^2 pyramid, lane against wave.  One window on level 0 (profiles/r20/): 1 089 hypotheses 119 against 21 us, 4 225: 119
// against 23, 35 301: 120 against 93, 269 001: 234 against 585; they meet near 52 000.  Batches on level 2 (profiles/r30/), B * W
// hypotheses: 1 089: 137 against 18 us, 8 712: 139 against 31, 33 800: 140 against 82, 69 696: 145 against 150, 270 400: 247
// against 536, 557 568: 434 against 1 118, 2 163 200: 1 277 against 4 225; they meet near 65 000.  This is the nearest power of
// two to both.
constexpr long long kWindowLaneMin = 1ll << 16;

bool window_lane_form(const hsm_ctx* h, long long hypotheses) {
  if (h->cfg.forms.window_form >= 0) return h->cfg.forms.window_form == 1;
  return hypotheses >= kWindowLaneMin;
}

// the refusals every window entry shares; *W: the window's size
int window_refusals(const hsm_ctx* h, const float* d_center, const float step[3], const int half[3], const char* who, long long* W) {
  if (!step || !half || !d_center) return fail_at(HSM_ERR_INVALID, who, ": null centre, steps or half-extents");
  if (half[0] < 0 || half[1] < 0 || half[2] < 0) return fail_at(HSM_ERR_INVALID, who, ": negative half-extent");
  for (int a = 0; a < 3; ++a)
    if (!(fabsf(step[a]) <= 3.402823466e38f)) return fail_at(HSM_ERR_INVALID, who, ": non-finite step");
  *W = window_count(half[0], half[1], half[2]);
  if (*W > (long long)INT_MAX) return fail_at(HSM_ERR_INVALID, who, ": more than INT_MAX hypotheses");
  (void)h;
  return HSM_OK;
}

// a batch of none may come without centres: what window_refusals looks at in their place
const float* centres_or_stand_in(int batch, const float* d_centers) {
  static const float kAnyCentre[3] = {0.0f, 0.0f, 0.0f};
  return batch > 0 ? d_centers : kAnyCentre;
}

WindowGrid window_grid(const float step[3], const int half[3]) { return WindowGrid{half[0], half[1], half[2], step[0], step[1], step[2]}; }

int score_window_refusals(const hsm_ctx* h, int level, const float* d_center, const float step[3], const int half[3],
                          const void* pts, int n, const void* out_lh, const void* out_res, const char* who, long long* W) {
  if (int rc = valid_level(h, level)) return rc;
  if (int rc = window_refusals(h, d_center, step, half, who, W)) return rc;
  if (n < 0 || (!out_lh && !out_res) || (n > 0 && !pts)) return fail_at(HSM_ERR_INVALID, who, ": bad argument");
  return HSM_OK;
}

// the kernels of one window entry, single or batched: [layout is quad][lane form], and the two names hsm_last_launch_kernel gives
template <typename Params>
struct WindowKernels {
  void (*kernel[2][2])(LevelView, Params);
  const char* name[2];
};
const WindowKernels<WindowParams> kSingleKernels = {
    {{score_window_wave_kernel<kLayoutPlane>, score_window_lane_kernel<kLayoutPlane>},
     {score_window_wave_kernel<kLayoutQuad>, score_window_lane_kernel<kLayoutQuad>}},
    {"score_window_wave_kernel", "score_window_lane_kernel"}};
const WindowKernels<WindowBatchParams> kBatchKernels = {
    {{score_windows_batch_wave_kernel<kLayoutPlane>, score_windows_batch_lane_kernel<kLayoutPlane>},
     {score_windows_batch_wave_kernel<kLayoutQuad>, score_windows_batch_lane_kernel<kLayoutQuad>}},
    {"score_windows_batch_wave_kernel", "score_windows_batch_lane_kernel"}};

// one kernel on `s`, as a reader of the map: the 2 x 2 choice over layout and form, `waves` wavefronts in workgroups of four
template <typename Params>
int window_score_launch(hsm_ctx* h, int level, const WindowKernels<Params>& K, bool lane, long long waves, const Params& P,
                        const char* who, hipStream_t s) {
  MapReader reader;
  if (int rc = reader.begin(h, s, who)) return rc;
  const LevelView v = level_view(h->levels[level], level_factor(level), 1);
  hipLaunchKernelGGL(K.kernel[h->cfg.layout == kLayoutPlane ? 0 : 1][lane ? 1 : 0], dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s,
                     v, P);
  HIP_TRY(hipGetLastError());
  reader.queued();
  h->last.last_kernel = K.name[lane ? 1 : 0];
  h->last.last_parity = HSM_PARITY_EXACT;  // a lane (or lane 0) owns the whole chain: the reference's order in every mode
  return HSM_OK;
}

// the single kernels for one window; arguments checked, device selected, lock held
int score_window_launch(hsm_ctx* h, int level, const float* d_center, const WindowGrid& G, int W, const float* d_pts, int n,
                        float* d_out_lh, float* d_out_res, hipStream_t s) {
  WindowParams P;
  P.grid = G;
  P.center = d_center;
  P.count = W;
  P.pts = reinterpret_cast<const float2*>(d_pts);
  P.n = n;
  P.out_lh = d_out_lh;
  P.out_residual = d_out_res;
  const bool lane = window_lane_form(h, W);
  return window_score_launch(h, level, kSingleKernels, lane, lane ? ((long long)W + 63) / 64 : (long long)W, P,
                             "hsm_score_window_device", s);
}

// the scans of a batched window entry: ScanBatch without poses
struct WindowScans {
  const float* d_pts;
  const int* d_offsets;
  int shared_n;
  ScanBatch of(int batch) const { return {batch, nullptr, d_pts, d_offsets, shared_n}; }
};

// what the batched entries refuse on top of window_refusals: the batch's own shape.  *BW: batch * W
int window_batch_refusals(int batch, long long W, const float* d_centers, const WindowScans& S, const char* who, long long* BW) {
  if (batch < 0) return fail_at(HSM_ERR_INVALID, who, ": batch < 0");
  *BW = (long long)batch * W;
  if (*BW > (long long)INT_MAX) return fail_at(HSM_ERR_INVALID, who, ": more than INT_MAX hypotheses in all");
  if (batch > 0 && !d_centers) return fail_at(HSM_ERR_INVALID, who, ": null centres");
  if (S.of(batch).bad_shape() || S.of(batch).points_missing()) return fail_at(HSM_ERR_INVALID, who, ": bad scans");
  return HSM_OK;
}

// the batched kernels for `batch` >= 1 windows of W hypotheses; arguments checked, device selected, lock held
int score_windows_batch_launch(hsm_ctx* h, int level, int batch, const float* d_centers, const WindowGrid& G, int W,
                               const WindowScans& S, float* d_out_lh, float* d_out_res, hipStream_t s) {
  WindowBatchParams P;
  P.grid = G;
  P.centers = d_centers;
  P.batch = batch;
  P.count = W;
  P.pts = reinterpret_cast<const float2*>(S.d_pts);
  P.offsets = S.d_offsets;
  P.shared_n = S.d_offsets ? 0 : S.shared_n;
  P.out_lh = d_out_lh;
  P.out_residual = d_out_res;
  const bool lane = window_lane_form(h, (long long)batch * W);
  // (lane form: every window padded to whole wavefronts)
  return window_score_launch(h, level, kBatchKernels, lane, (long long)batch * (lane ? ((long long)W + 63) / 64 : (long long)W), P,
                             "hsm_score_windows_batch_device", s);
}

// `count` indices of windows of W hypotheses, `per_window` of them in a row for each centre
int window_poses_launch(const WindowGrid& G, int W, const float* d_centers, const int* d_index, int count, int per_window,
                        float* d_out_pose, hipStream_t s) {
  hipLaunchKernelGGL(window_poses_kernel, dim3((unsigned)(((long long)count + 255) / 256)), dim3(256), 0, s, G, W, d_centers, d_index,
                     count, per_window, d_out_pose);
  HIP_TRY(hipGetLastError());
  return HSM_OK;
}

// the K best of each of `groups` >= 1 runs of `count` scores: two launches; one group: hsm_select_topk_device
int select_topk_launch(int groups, int count, const float* d_scores, int k, int* d_out_index, float* d_out_score, void* d_workspace,
                       hipStream_t s) {
  const int slices = topk_slices(count);
  const TopKGroupsLayout L = topk_groups_layout(groups, count, k);
  float* cand_score = reinterpret_cast<float*>(static_cast<char*>(d_workspace) + L.cand_score);
  int* cand_index = reinterpret_cast<int*>(static_cast<char*>(d_workspace) + L.cand_index);
  const long long waves = (long long)groups * slices;
  hipLaunchKernelGGL(topk_slice_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, d_scores, count, k, slices, groups,
                     cand_score, cand_index);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)groups), dim3(256), 0, s, cand_score, cand_index, slices * k, k, d_out_index,
                     d_out_score);
  HIP_TRY(hipGetLastError());
  return HSM_OK;
}

int select_topk_refusals(int count, const void* scores, int k, const void* out_index, const void* ws, size_t ws_bytes) {
  if (count < 0 || k < 1 || k > HSM_MAX_TOPK || !out_index || (count > 0 && !scores) || !ws ||
      ws_bytes < topk_workspace_bytes(count, k) || ((size_t)ws & 3))
    return fail(HSM_ERR_INVALID, "hsm_select_topk_device: bad argument");
  return HSM_OK;
}

// (no groups: nothing to select, and nothing but the counts and k is looked at)
int select_topk_groups_refusals(int groups, int group_size, const void* scores, int k, const void* out_index, const void* ws,
                                size_t ws_bytes) {
  const char* who = "hsm_select_topk_groups_device";
  if (groups < 0 || group_size < 0 || k < 1 || k > HSM_MAX_TOPK) return fail_at(HSM_ERR_INVALID, who, ": bad counts or k");
  if ((long long)groups * group_size > (long long)INT_MAX || (long long)groups * k > (long long)INT_MAX)
    return fail_at(HSM_ERR_INVALID, who, ": more than INT_MAX scores or places");
  if (groups == 0) return HSM_OK;
  if (!out_index || (group_size > 0 && !scores)) return fail_at(HSM_ERR_INVALID, who, ": null scores or indices");
  if (!ws || ((size_t)ws & 3) || ws_bytes < topk_groups_workspace_bytes(groups, group_size, k))
    return fail_at(HSM_ERR_INVALID, who, ": workspace missing, misaligned or too small");
  return HSM_OK;
}

int relocalize_refusals(const hsm_ctx* h, int search_level, const float* d_center, const float step[3], const int half[3], int k,
                        const void* pts, int n, const void* cand_pose, const void* cand_lh, const void* best_pose,
                        const void* best_index, const char* who, long long* W) {
  if (int rc = valid_level(h, search_level)) return rc;
  if (int rc = window_refusals(h, d_center, step, half, who, W)) return rc;
  if (n < 0 || (n > 0 && !pts) || k < 1 || k > HSM_MAX_TOPK || !cand_pose || !cand_lh || !best_pose || !best_index)
    return fail_at(HSM_ERR_INVALID, who, ": bad argument");
  return HSM_OK;
}

// the outputs of a relocalisation, `groups` * k candidates and `groups` winners: device pointers where it is queued, host pointers
// in the batched host entry's refusals.  cand_index: the batched entries' alone
struct RelocalizeOut {
  float *cand_pose, *cand_cov, *cand_lh;
  int* cand_index;
  float *best_pose, *best_score;
  int* best_index;
};

// The chain behind the window score on `s`, for `groups` >= 1 runs of W scores at ws + L.scores, run g around centre g against
// scan g: the k best of every run, their poses, and the groups * k starts through match, likelihood on level 0 and the winner of
// every group of k (match_chain_nolock), named by its window index.  Candidate (g, r) is matched against scan g: a shared scan
// as it is; CSR scans laid out k times, since the matcher takes one scan per pair (its sizing hint: the mean length).  One
// group with a shared scan is the single relocalisation: no copy, every grid 1.
int relocalize_after_score(hsm_ctx* h, int groups, const float* d_centers, const WindowGrid& G, int W, int k, const WindowScans& S,
                           int total_points, char* ws, const RelocalizeLayout& L, const RelocalizeOut& O, hipStream_t s) {
  const int cands = groups * k;
  const float* scores = reinterpret_cast<const float*>(ws + L.scores);
  int* kindex = O.cand_index ? O.cand_index : reinterpret_cast<int*>(ws + L.index);
  float* kscore = reinterpret_cast<float*>(ws + L.kscore);
  float* kpose = reinterpret_cast<float*>(ws + L.pose);
  if (int rc = select_topk_launch(groups, W, scores, k, kindex, kscore, ws + L.topk, s)) return rc;
  if (int rc = window_poses_launch(G, W, d_centers, kindex, cands, k, kpose, s)) return rc;
  ScanBatch pairs{cands, kpose, S.d_pts, nullptr, S.shared_n};
  if (S.d_offsets) {
    int* koffsets = reinterpret_cast<int*>(ws + L.offsets);
    float2* kpts = reinterpret_cast<float2*>(ws + L.pts);
    hipLaunchKernelGGL(replicate_scans_kernel, dim3((unsigned)cands), dim3(256), 0, s, reinterpret_cast<const float2*>(S.d_pts),
                       S.d_offsets, groups, k, total_points, kpts, koffsets);
    HIP_TRY(hipGetLastError());
    pairs = ScanBatch{cands, kpose, reinterpret_cast<const float*>(kpts), koffsets, (total_points + groups - 1) / groups};
  }
  if (int rc = match_chain_nolock(h, pairs, {O.cand_pose, O.cand_cov}, {0, {O.cand_lh}},
                                  {groups, nullptr, k, O.best_index, O.best_score, O.best_pose}, s))
    return rc;
  hipLaunchKernelGGL(window_best_index_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, s, kindex, cands, groups,
                     O.best_index);
  HIP_TRY(hipGetLastError());
  return HSM_OK;
}

// the single chain on `s`: the single window score, then one group against the one scan; arguments checked, device selected,
// lock held
int relocalize_queue(hsm_ctx* h, int search_level, const float* d_center, const WindowGrid& G, int W, int k, const float* d_pts,
                     int n, char* ws, const RelocalizeOut& O, hipStream_t s) {
  const RelocalizeLayout L = relocalize_layout(W, k);
  if (int rc = score_window_launch(h, search_level, d_center, G, W, d_pts, n, reinterpret_cast<float*>(ws + L.scores), nullptr, s))
    return rc;
  return relocalize_after_score(h, 1, d_center, G, W, k, {d_pts, nullptr, n}, 0, ws, L, O, s);
}

// ---- the chain for a batch of scans, each in its own window -----------------------------------------------------------------
int relocalize_batch_refusals(const hsm_ctx* h, int search_level, int batch, const float* d_centers, const float step[3],
                              const int half[3], int k, const WindowScans& S, long long total_points, const RelocalizeOut& O,
                              const char* who, long long* W) {
  if (int rc = valid_level(h, search_level)) return rc;
  if (int rc = window_refusals(h, centres_or_stand_in(batch, d_centers), step, half, who, W)) return rc;
  long long BW = 0;
  if (int rc = window_batch_refusals(batch, *W, d_centers, S, who, &BW)) return rc;
  if (k < 1 || k > HSM_MAX_TOPK || (long long)batch * k > (long long)(INT_MAX / 9))
    return fail_at(HSM_ERR_INVALID, who, ": k out of range, or more than INT_MAX / 9 candidates");
  if (!O.cand_pose || !O.cand_lh || !O.best_pose || !O.best_index) return fail_at(HSM_ERR_INVALID, who, ": null output");
  if (S.d_offsets && (total_points < 0 || total_points * k > (long long)INT_MAX))
    return fail_at(HSM_ERR_INVALID, who, ": total_points negative, or k copies of the scans hold more than INT_MAX points");
  return HSM_OK;
}

// the batched chain on `s` for batch >= 1: the batched window score, then `batch` groups; arguments checked, device selected,
// lock held
int relocalize_batch_queue(hsm_ctx* h, int search_level, int batch, const float* d_centers, const WindowGrid& G, int W, int k,
                           const WindowScans& S, int total_points, char* ws, const RelocalizeOut& O, hipStream_t s) {
  const RelocalizeLayout L = relocalize_batch_layout(batch, W, k, S.d_offsets ? total_points : 0);
  if (int rc = score_windows_batch_launch(h, search_level, batch, d_centers, G, W, S, reinterpret_cast<float*>(ws + L.scores),
                                          nullptr, s))
    return rc;
  return relocalize_after_score(h, batch, d_centers, G, W, k, S, total_points, ws, L, O, s);
}

// ---- occupied cells as points (map_points_kernels.h) ---------------------------------------------------------------------------------
// the refusals the three entries share; the workspace is the device entry's own
int occupied_points_refusals(const hsm_ctx* h, int level, int every, int max_points, const void* pts, const void* count,
                             const char* who) {
  if (int rc = valid_level(h, level)) return rc;
  if (every < 1) return fail_at(HSM_ERR_INVALID, who, ": every < 1");
  if (max_points < 0) return fail_at(HSM_ERR_INVALID, who, ": max_points < 0");
  if (!count || (max_points > 0 && !pts)) return fail_at(HSM_ERR_INVALID, who, ": null counts or points");
  return HSM_OK;
}

// the three launches on `s`, ordered as a reader of `src`; arguments checked, device selected, lock held.  `reader`: the caller's
// bracket, marked pending here already -- before the first launch, so that a call that fails half way leaves `src`'s
// next writer behind whatever it did queue.  A caller that has waited for `s` under the lock may clear the mark again
int occupied_points_launch(hsm_ctx* src, int level, const PointsBox& B, int every, int max_points, float* d_pts, int* d_count,
                           void* d_ws, hipStream_t s, const char* who, MapReader& reader) {
  if (int rc = reader.begin(src, s, who, /*mark_now=*/true)) return rc;
  const Level& L = src->levels[level];
  MapPointsParams P;
  P.logodds = L.d_logodds;
  P.sx = L.sx;
  P.x0 = B.x0, P.y0 = B.y0, P.w = B.w;
  P.cells = B.w * B.h;
  P.tiles = points_tiles(P.cells);
  P.every = every, P.max_points = max_points;
  P.worldTmap = L.worldTmap;
  P.scale = src->levels[0].scale_to_map;  // hsm_scale_to_map
  P.out = reinterpret_cast<float2*>(d_pts);
  P.out_count = d_count;
  P.tile_counts = static_cast<int*>(d_ws);
  const bool whole = B.w == L.sx;
  const dim3 grid((unsigned)(P.tiles < 2048 ? P.tiles : 2048));
  if (P.tiles > 0) {
    if (whole) hipLaunchKernelGGL(map_points_count_kernel<true>, grid, dim3(256), 0, s, P);
    else hipLaunchKernelGGL(map_points_count_kernel<false>, grid, dim3(256), 0, s, P);
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(map_points_scan_kernel, dim3(1), dim3(kPointsScanThreads), 0, s, P);  // (an empty box: the counts alone)
  HIP_TRY(hipGetLastError());
  if (P.tiles > 0 && max_points > 0) {
    if (whole) hipLaunchKernelGGL(map_points_scatter_kernel<true>, grid, dim3(256), 0, s, P);
    else hipLaunchKernelGGL(map_points_scatter_kernel<false>, grid, dim3(256), 0, s, P);
    HIP_TRY(hipGetLastError());
  }
  return HSM_OK;
}

}  // namespace

extern "C" {

size_t hsm_select_topk_workspace(int count, int k) { return topk_workspace_bytes(count, k); }

size_t hsm_relocalize_workspace(int window_count, int k) { return relocalize_layout(window_count, k).total; }

int hsm_score_window_device(hsm_ctx* h, int level, const float* d_center_world, const float step[3], const int half[3],
                            const float* d_pts_xy, int n, float* d_out_likelihood, float* d_out_residual, void* stream) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  long long W = 0;
  if (int rc = score_window_refusals(h, level, d_center_world, step, half, d_pts_xy, n, d_out_likelihood, d_out_residual,
                                     "hsm_score_window_device", &W))
    return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  return score_window_launch(h, level, d_center_world, window_grid(step, half), (int)W, d_pts_xy, n, d_out_likelihood,
                             d_out_residual, static_cast<hipStream_t>(stream));
}

int hsm_score_window(hsm_ctx* h, int level, const float center_world[3], const float step[3], const int half[3],
                     const float* pts_xy, int n, float* out_likelihood, float* out_residual) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  long long W = 0;
  if (int rc = score_window_refusals(h, level, center_world, step, half, pts_xy, n, out_likelihood, out_residual,
                                     "hsm_score_window", &W))
    return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  const ScoreWindowStage st = score_window_stage((size_t)W, n, center_world, pts_xy, out_likelihood, out_residual);
  if (int rc = h->d_batch.reserve(st.plan.total())) return rc;
  char* base = h->d_batch;
  if (int rc = stage_copy_in(st.plan, base, h->stream)) return rc;
  if (int rc = score_window_launch(h, level, staged<float>(base, st.center), window_grid(step, half), (int)W,
                                   staged<float>(base, st.pts), n, staged<float>(base, st.lh, out_likelihood),
                                   staged<float>(base, st.res, out_residual), h->stream))
    return rc;
  if (int rc = stage_copy_out(st.plan, base, h->stream)) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  return HSM_OK;
}

int hsm_window_poses_device(hsm_ctx* h, const float* d_center_world, const float step[3], const int half[3], const int* d_index,
                            int count, float* d_out_pose, void* stream) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  long long W = 0;
  if (int rc = window_refusals(h, d_center_world, step, half, "hsm_window_poses_device", &W)) return rc;
  if (count < 0 || (count > 0 && !d_out_pose) || (!d_index && count > W))
    return fail(HSM_ERR_INVALID, "hsm_window_poses_device: bad argument");
  if (count == 0) return HSM_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  return window_poses_launch(window_grid(step, half), (int)W, d_center_world, d_index, count, count, d_out_pose,
                             static_cast<hipStream_t>(stream));
}

int hsm_select_topk_device(hsm_ctx* h, int count, const float* d_scores, int k, int* d_out_index, float* d_out_score,
                           void* d_workspace, size_t workspace_bytes, void* stream) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  if (int rc = select_topk_refusals(count, d_scores, k, d_out_index, d_workspace, workspace_bytes)) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  return select_topk_launch(1, count, d_scores, k, d_out_index, d_out_score, d_workspace, static_cast<hipStream_t>(stream));
}

size_t hsm_select_topk_groups_workspace(int groups, int group_size, int k) {
  return topk_groups_workspace_bytes(groups, group_size, k);
}

int hsm_select_topk_groups_device(hsm_ctx* h, int groups, int group_size, const float* d_scores, int k, int* d_out_index,
                                  float* d_out_score, void* d_workspace, size_t workspace_bytes, void* stream) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  if (int rc = select_topk_groups_refusals(groups, group_size, d_scores, k, d_out_index, d_workspace, workspace_bytes)) return rc;
  if (groups == 0) return HSM_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  return select_topk_launch(groups, group_size, d_scores, k, d_out_index, d_out_score, d_workspace, static_cast<hipStream_t>(stream));
}

int hsm_score_windows_batch_device(hsm_ctx* h, int level, int batch, const float* d_centers_world, const float step[3],
                                   const int half[3], const float* d_pts_xy, const int* d_scan_offsets, int shared_n,
                                   float* d_out_likelihood, float* d_out_residual, void* stream) {
  const char* who = "hsm_score_windows_batch_device";
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  if (int rc = valid_level(h, level)) return rc;
  long long W = 0, BW = 0;
  if (int rc = window_refusals(h, centres_or_stand_in(batch, d_centers_world), step, half, who, &W)) return rc;
  const WindowScans S{d_pts_xy, d_scan_offsets, shared_n};
  if (int rc = window_batch_refusals(batch, W, d_centers_world, S, who, &BW)) return rc;
  if (!d_out_likelihood && !d_out_residual) return fail_at(HSM_ERR_INVALID, who, ": both outputs are null");
  if (batch == 0) return HSM_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  return score_windows_batch_launch(h, level, batch, d_centers_world, window_grid(step, half), (int)W, S, d_out_likelihood,
                                    d_out_residual, static_cast<hipStream_t>(stream));
}

int hsm_relocalize_device(hsm_ctx* h, int search_level, const float* d_center_world, const float step[3], const int half[3], int k,
                          const float* d_pts_xy, int n, void* d_workspace, size_t workspace_bytes, float* d_out_cand_pose,
                          float* d_out_cand_cov, float* d_out_cand_likelihood, float* d_out_best_pose, float* d_out_best_score,
                          int* d_out_best_index, void* stream) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  long long W = 0;
  if (int rc = relocalize_refusals(h, search_level, d_center_world, step, half, k, d_pts_xy, n, d_out_cand_pose,
                                   d_out_cand_likelihood, d_out_best_pose, d_out_best_index, "hsm_relocalize_device", &W))
    return rc;
  if (!d_workspace || ((size_t)d_workspace & 7) || workspace_bytes < relocalize_layout(W, k).total)
    return fail(HSM_ERR_INVALID, "hsm_relocalize_device: workspace missing, misaligned or too small");
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  return relocalize_queue(h, search_level, d_center_world, window_grid(step, half), (int)W, k, d_pts_xy, n,
                          static_cast<char*>(d_workspace),
                          {d_out_cand_pose, d_out_cand_cov, d_out_cand_likelihood, nullptr, d_out_best_pose, d_out_best_score,
                           d_out_best_index},
                          static_cast<hipStream_t>(stream));
}

int hsm_relocalize(hsm_ctx* h, int search_level, const float center_world[3], const float step[3], const int half[3], int k,
                   const float* pts_xy, int n, float* out_cand_pose, float* out_cand_cov, float* out_cand_likelihood,
                   float* out_best_pose, float* out_best_score, int* out_best_index) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  long long W = 0;
  if (int rc = relocalize_refusals(h, search_level, center_world, step, half, k, pts_xy, n, out_cand_pose, out_cand_likelihood,
                                   out_best_pose, out_best_index, "hsm_relocalize", &W))
    return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  const RelocalizeStage st = relocalize_stage(k, n, relocalize_layout(W, k).total, center_world, pts_xy, out_cand_pose, out_cand_cov,
                                              out_cand_likelihood, out_best_pose, out_best_score, out_best_index);
  if (int rc = h->d_batch.reserve(st.plan.total())) return rc;
  char* base = h->d_batch;
  if (int rc = stage_copy_in(st.plan, base, h->stream)) return rc;
  if (int rc = relocalize_queue(h, search_level, staged<float>(base, st.center), window_grid(step, half), (int)W, k,
                                staged<float>(base, st.pts), n, base + st.ws,
                                {staged<float>(base, st.pose), staged<float>(base, st.cov, out_cand_cov), staged<float>(base, st.lh),
                                 nullptr, staged<float>(base, st.bpose), staged<float>(base, st.bscore, out_best_score),
                                 staged<int>(base, st.bidx)},
                                h->stream))
    return rc;
  if (int rc = stage_copy_out(st.plan, base, h->stream)) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  return HSM_OK;
}

size_t hsm_relocalize_batch_workspace(int batch, int window_count, int k, int total_points) {
  return relocalize_batch_layout(batch, window_count, k, total_points).total;
}

int hsm_relocalize_batch_device(hsm_ctx* h, int search_level, int batch, const float* d_centers_world, const float step[3],
                                const int half[3], int k, const float* d_pts_xy, const int* d_scan_offsets, int shared_n,
                                int total_points, void* d_workspace, size_t workspace_bytes, float* d_out_cand_pose,
                                float* d_out_cand_cov, float* d_out_cand_likelihood, int* d_out_cand_index, float* d_out_best_pose,
                                float* d_out_best_score, int* d_out_best_index, void* stream) {
  const char* who = "hsm_relocalize_batch_device";
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  const WindowScans S{d_pts_xy, d_scan_offsets, shared_n};
  const RelocalizeOut O{d_out_cand_pose, d_out_cand_cov, d_out_cand_likelihood, d_out_cand_index,
                             d_out_best_pose, d_out_best_score,  d_out_best_index};
  long long W = 0;
  if (int rc = relocalize_batch_refusals(h, search_level, batch, d_centers_world, step, half, k, S, total_points, O, who, &W)) return rc;
  const size_t need = relocalize_batch_layout(batch, W, k, d_scan_offsets ? total_points : 0).total;
  if (!d_workspace || ((size_t)d_workspace & 7) || need == 0 || workspace_bytes < need)
    return fail_at(HSM_ERR_INVALID, who, ": workspace missing, misaligned or too small");
  if (batch == 0) return HSM_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  return relocalize_batch_queue(h, search_level, batch, d_centers_world, window_grid(step, half), (int)W, k, S, total_points,
                                static_cast<char*>(d_workspace), O, static_cast<hipStream_t>(stream));
}

int hsm_relocalize_batch(hsm_ctx* h, int search_level, int batch, const float* centers_world, const float step[3], const int half[3],
                         int k, const float* pts_xy, const int* scan_offsets, int shared_n, float* out_cand_pose,
                         float* out_cand_cov, float* out_cand_likelihood, int* out_cand_index, float* out_best_pose,
                         float* out_best_score, int* out_best_index) {
  const char* who = "hsm_relocalize_batch";
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  // (host offsets: they start at 0 and do not decrease, and their last entry is the number of points)
  long long total = 0;
  if (scan_offsets && batch > 0) {
    if (scan_offsets[0] != 0) return fail_at(HSM_ERR_INVALID, who, ": scan_offsets[0] != 0");
    for (int b = 0; b < batch; ++b)
      if (scan_offsets[b + 1] < scan_offsets[b]) return fail_at(HSM_ERR_INVALID, who, ": scan_offsets decrease");
    total = scan_offsets[batch];
  }
  if (total > 0 && !pts_xy) return fail_at(HSM_ERR_INVALID, who, ": null points");
  const WindowScans S{pts_xy, scan_offsets, shared_n};
  const RelocalizeOut O{out_cand_pose, out_cand_cov, out_cand_likelihood, out_cand_index, out_best_pose, out_best_score, out_best_index};
  long long W = 0;
  if (int rc = relocalize_batch_refusals(h, search_level, batch, centers_world, step, half, k, S, total, O, who, &W)) return rc;
  if (batch == 0) return HSM_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  const size_t points = scan_offsets ? (size_t)total : (size_t)shared_n;
  const RelocalizeBatchStage st =
      relocalize_batch_stage(batch, k, points, relocalize_batch_layout(batch, W, k, total).total, centers_world, pts_xy, scan_offsets,
                             out_cand_pose, out_cand_cov, out_cand_likelihood, out_cand_index, out_best_pose, out_best_score,
                             out_best_index);
  if (int rc = h->d_batch.reserve(st.plan.total())) return rc;
  char* base = h->d_batch;
  if (int rc = stage_copy_in(st.plan, base, h->stream)) return rc;
  const WindowScans DS{staged<float>(base, st.pts), staged<int>(base, st.offs, scan_offsets), shared_n};
  const RelocalizeOut DO{staged<float>(base, st.pose), staged<float>(base, st.cov, out_cand_cov), staged<float>(base, st.lh),
                              staged<int>(base, st.cidx, out_cand_index), staged<float>(base, st.bpose),
                              staged<float>(base, st.bscore, out_best_score), staged<int>(base, st.bidx)};
  if (int rc = relocalize_batch_queue(h, search_level, batch, staged<float>(base, st.centers), window_grid(step, half), (int)W, k, DS,
                                      (int)total, base + st.ws, DO, h->stream))
    return rc;
  if (int rc = stage_copy_out(st.plan, base, h->stream)) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  return HSM_OK;
}

size_t hsm_occupied_points_workspace(int cells) { return points_workspace_bytes(cells); }

int hsm_occupied_points_device(hsm_ctx* src, int level, const int bbox[4], int every, int max_points, float* d_out_pts_xy,
                               int* d_out_count, void* d_workspace, size_t workspace_bytes, void* stream) {
  const char* who = "hsm_occupied_points_device";
  if (!src) return fail(HSM_ERR_INVALID, "null context");
  if (int rc = occupied_points_refusals(src, level, every, max_points, d_out_pts_xy, d_out_count, who)) return rc;
  std::lock_guard<std::mutex> lk(src->mu);  // (hsm_shift_map rewrites the geometry)
  const PointsBox B = points_clamp_box(bbox, src->levels[level].sx, src->levels[level].sy);
  if (!d_workspace || ((size_t)d_workspace & 7) || workspace_bytes < points_workspace_bytes((long long)B.w * B.h))
    return fail_at(HSM_ERR_INVALID, who, ": workspace missing, misaligned or too small");
  if (int rc = select_device(src)) return rc;
  MapReader reader;
  return occupied_points_launch(src, level, B, every, max_points, d_out_pts_xy, d_out_count, d_workspace,
                                static_cast<hipStream_t>(stream), who, reader);
}

int hsm_occupied_points(hsm_ctx* src, int level, const int bbox[4], int every, int max_points, float* out_pts_xy, int count[2]) {
  const char* who = "hsm_occupied_points";
  if (!src) return fail(HSM_ERR_INVALID, "null context");
  if (int rc = occupied_points_refusals(src, level, every, max_points, out_pts_xy, count, who)) return rc;
  std::lock_guard<std::mutex> lk(src->mu);
  if (int rc = select_device(src)) return rc;
  const PointsBox B = points_clamp_box(bbox, src->levels[level].sx, src->levels[level].sy);
  const OccupiedPointsStage st = occupied_points_stage(max_points, points_workspace_bytes((long long)B.w * B.h), count);
  if (int rc = src->d_batch.reserve(st.plan.total())) return rc;
  char* base = src->d_batch;
  MapReader reader;
  if (int rc = occupied_points_launch(src, level, B, every, max_points, staged<float>(base, st.pts), staged<int>(base, st.counts),
                                      base + st.ws, src->stream, who, reader))
    return rc;
  if (int rc = stage_copy_out(st.plan, base, src->stream)) return rc;
  HIP_TRY(hipStreamSynchronize(src->stream));
  if (count[0] > 0) {  // the points the counts name and no float behind them
    HIP_TRY(hipMemcpyAsync(out_pts_xy, base + st.pts, (size_t)count[0] * 2 * sizeof(float), hipMemcpyDeviceToHost, src->stream));
    HIP_TRY(hipStreamSynchronize(src->stream));
  }
  return HSM_OK;
}

size_t hsm_align_map_workspace(int cells, int window_count, int k, int max_points) {
  const size_t ws = relocalize_layout(window_count, k).total;
  if (cells < 0 || ws == 0 || max_points < 0 || max_points > HSM_MAX_ALIGN_POINTS) return 0;
  return align_map_stage(k, max_points, points_workspace_bytes(cells), ws, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr)
      .plan.total();
}

int hsm_align_map(hsm_ctx* dst, hsm_ctx* src, int src_level, const int src_bbox[4], int every, int max_points, int search_level,
                  const float guess_src_in_dst[3], const float step[3], const int half[3], int k, float out_src_in_dst[3],
                  float out_cov[9], float* out_likelihood, int out_counts[2], int* out_window_index) {
  const char* who = "hsm_align_map";
  if (!dst || !src) return fail(HSM_ERR_INVALID, "null context");
  if (dst == src) return fail_at(HSM_ERR_INVALID, who, ": dst and src are the same context");
  if (max_points > HSM_MAX_ALIGN_POINTS) return fail_at(HSM_ERR_INVALID, who, ": max_points above HSM_MAX_ALIGN_POINTS");
  if (!out_src_in_dst) return fail_at(HSM_ERR_INVALID, who, ": out_src_in_dst is null");
  std::unique_lock<std::mutex> lk_a(dst < src ? dst->mu : src->mu);  // (as hsm_merge_map: two calls in opposite directions)
  std::unique_lock<std::mutex> lk_b(dst < src ? src->mu : dst->mu);
  if (!merge_compatible(dst, src)) return fail_at(HSM_ERR_INVALID, who, ": the contexts differ in level count, resolution or layout");
  if (dst->device != src->device) return fail_at(HSM_ERR_INVALID, who, ": the contexts are on different devices");
  int cnt[2] = {0, 0}, kindex[HSM_MAX_TOPK], best_index = -1;
  float cand_cov[HSM_MAX_TOPK * 9], best_score = 0.0f;
  // (the points and the counts are device regions here: any address that is not null passes the shared refusals)
  if (int rc = occupied_points_refusals(src, src_level, every, max_points, cnt, cnt, who)) return rc;
  long long W = 0;
  if (int rc = relocalize_refusals(dst, search_level, guess_src_in_dst, step, half, k, cnt, max_points, cand_cov, cand_cov,
                                   out_src_in_dst, &best_index, who, &W))
    return rc;
  if (int rc = select_device(dst)) return rc;
  const Level& S = src->levels[src_level];
  const PointsBox B = points_clamp_box(src_bbox, S.sx, S.sy);
  const RelocalizeLayout RL = relocalize_layout(W, k);
  const AlignMapStage st = align_map_stage(k, max_points, points_workspace_bytes((long long)B.w * B.h), RL.total, RL.index,
                                           guess_src_in_dst, kindex, cand_cov, out_src_in_dst, &best_score, &best_index);
  if (int rc = dst->d_batch.reserve(st.plan.total())) return rc;
  char* base = dst->d_batch;
  if (int rc = stage_copy_in(st.plan, base, dst->stream)) return rc;
  // (a) `src`'s cells on `dst`'s stream, behind every update queued on `src`, marked for `src`'s next writer
  MapReader reader;
  if (int rc = occupied_points_launch(src, src_level, B, every, max_points, staged<float>(base, st.pts), staged<int>(base, st.counts),
                                      base + st.xws, dst->stream, who, reader))
    return rc;
  // (b) the chain's one host wait: every entry behind this point takes the number of points from the host
  HIP_TRY(hipMemcpyAsync(cnt, base + st.counts, sizeof cnt, hipMemcpyDeviceToHost, dst->stream));
  HIP_TRY(hipStreamSynchronize(dst->stream));
  if (reader.mark) reader.mark->pending = false;  // the read of `src` is over, under `src`'s lock: its next writer has nothing to wait for
  // (c) the points are a scan in `src`'s world frame, so the pose the matcher refines is src_in_dst
  if (int rc = relocalize_queue(dst, search_level, staged<float>(base, st.center), window_grid(step, half), (int)W, k,
                                staged<float>(base, st.pts), cnt[0], base + st.ws,
                                {staged<float>(base, st.pose), staged<float>(base, st.cov), staged<float>(base, st.lh), nullptr,
                                 staged<float>(base, st.bpose), staged<float>(base, st.bscore), staged<int>(base, st.bidx)},
                                dst->stream))
    return rc;
  // (d) the winner
  if (int rc = stage_copy_out(st.plan, base, dst->stream)) return rc;
  HIP_TRY(hipStreamSynchronize(dst->stream));
  if (out_cov && best_index >= 0)
    for (int j = 0; j < k; ++j)
      if (kindex[j] == best_index) {  // (the k window indices are distinct: the place the winner's start took)
        memcpy(out_cov, cand_cov + 9 * j, 9 * sizeof(float));
        break;
      }
  if (out_likelihood) *out_likelihood = best_score;
  if (out_counts) out_counts[0] = cnt[0], out_counts[1] = cnt[1];
  if (out_window_index) *out_window_index = best_index;
  return HSM_OK;
}

}  // extern "C"
