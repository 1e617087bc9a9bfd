// probes.hip -- the entries of the C ABI (include/hector_mi355/capi.h) that look INTO a context and are never timed: the
// host-array probes of the matcher's sums (likelihood, residual, covariance, Hessian, single beams), a level's planes down and
// up, its boxes, and the hsm_debug_* test hooks.  Each one ends in a wait for the context's stream.  Their kernels, which nothing else
// launches, are in probe_kernels.h (sampler and sums: beam_sample.h, gn_step.h).  What these entries need of the core runtime
// (hector_mi355.hip) is declared in hsm_ctx.h.  (Ray distances are in rays.hip.)
#include <hip/hip_runtime.h>
#include <math.h>

#include <mutex>

#include "hector_mi355/capi.h"
#include "hsm_ctx.h"
#include "probe_kernels.h"

using namespace hsm;
using namespace hsm_host;

extern "C" {

static int score_states(hsm_ctx* h, int level, int batch, const float* states_map, const float* pts_xy, int n,
                        float* out_lh, float* out_residual, const char* who) {
  if (int rc = valid_level(h, level)) return rc;
  if (batch < 0 || n < 0 || (batch > 0 && (!states_map || !(out_lh || out_residual))) || (n > 0 && !pts_xy))
    return fail(HSM_ERR_INVALID, who);
  if (batch == 0) return HSM_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  const ScoreStatesStage st = score_states_stage(batch, n, states_map, pts_xy, out_lh, out_residual);
  if (int rc = h->d_batch.reserve(st.plan.total())) return rc;
  char* base = h->d_batch;
  if (int rc = stage_copy_in(st.plan, base, h->stream)) return rc;
  const float factor = (float)(1.0 / pow(2.0, (double)level));
  const LevelView v = level_view(h->levels[level], factor, 1);
  const int grid = (batch + 3) / 4;
  with_sampler_form(h, [&](auto lay, auto ex) {
    hipLaunchKernelGGL((likelihood_kernel<lay(), ex()>), dim3(grid), dim3(256), 0, h->stream, v, staged<float>(base, st.states),
                       batch, staged<float2>(base, st.pts), n, factor, staged<float>(base, st.lh, out_lh),
                       staged<float>(base, st.res, out_residual));
  });
  HIP_TRY(hipGetLastError());
  if (int rc = stage_copy_out(st.plan, base, h->stream)) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  return HSM_OK;
}

int hsm_likelihood_states(hsm_ctx* h, int level, int batch, const float* states_map, const float* pts_xy, int n,
                          float* out_lh) {
  return score_states(h, level, batch, states_map, pts_xy, n, out_lh, nullptr, "hsm_likelihood_states: bad argument");
}

int hsm_residual_states(hsm_ctx* h, int level, int batch, const float* states_map, const float* pts_xy, int n,
                        float* out_residual) {
  return score_states(h, level, batch, states_map, pts_xy, n, nullptr, out_residual,
                      "hsm_residual_states: bad argument");
}

int hsm_covariance_for_poses(hsm_ctx* h, int level, int batch, const float* poses_map, const float* pts_xy, int n,
                             float* out_cov_map, float* out_cov_world, float* out_lh7) {
  if (int rc = valid_level(h, level)) return rc;
  if (batch < 0 || n < 0 || (batch > 0 && (!poses_map || !(out_cov_map || out_cov_world || out_lh7))) ||
      (n > 0 && !pts_xy))
    return fail(HSM_ERR_INVALID, "hsm_covariance_for_poses: bad argument");
  if (batch == 0) return HSM_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  const PoseCovarianceStage st = pose_covariance_stage(batch, n, poses_map, pts_xy, out_cov_map, out_cov_world, out_lh7);
  if (int rc = h->d_batch.reserve(st.plan.total())) return rc;
  char* base = h->d_batch;
  if (int rc = stage_copy_in(st.plan, base, h->stream)) return rc;
  const float factor = (float)(1.0 / pow(2.0, (double)level));
  const Level& Lv = h->levels[level];
  const LevelView v = level_view(Lv, factor, 1);
  with_sampler_form(h, [&](auto lay, auto ex) {
    hipLaunchKernelGGL((pose_covariance_kernel<lay(), ex()>), dim3(batch), dim3(448), 0, h->stream, v, staged<float>(base, st.poses),
                       batch, staged<float2>(base, st.pts), n, factor, Lv.cell_length, staged<float>(base, st.cov_map),
                       staged<float>(base, st.cov_world), staged<float>(base, st.lh7));
  });
  HIP_TRY(hipGetLastError());
  if (int rc = stage_copy_out(st.plan, base, h->stream)) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  return HSM_OK;
}

int hsm_level_info(const hsm_ctx* h, int level, int* sx, int* sy, float* cell, float* scale) {
  if (int rc = valid_level(h, level)) return rc;
  const Level& L = h->levels[level];
  if (sx) *sx = L.sx;
  if (sy) *sy = L.sy;
  if (cell) *cell = L.cell_length;
  if (scale) *scale = L.scale_to_map;
  return HSM_OK;
}
int hsm_map_coords_pose(const hsm_ctx* h, int level, const float w[3], float m[3]) {
  if (int rc = valid_level(h, level)) return rc;
  affine_apply_host(h->levels[level].mapTworld, w[0], w[1], m[0], m[1]);
  m[2] = w[2];
  return HSM_OK;
}
int hsm_world_coords_pose(const hsm_ctx* h, int level, const float m[3], float w[3]) {
  if (int rc = valid_level(h, level)) return rc;
  affine_apply_host(h->levels[level].worldTmap, m[0], m[1], w[0], w[1]);
  w[2] = m[2];
  return HSM_OK;
}
int hsm_update_index(const hsm_ctx* h, int level) {
  if (valid_level(h, level)) return -1;
  std::lock_guard<std::mutex> lk(h->mu);  // read by the facade's publisher thread while the scan thread updates
  if (h->upd.gate_outstanding)  // gated updates since the last look: wait for them and fetch their count
    if (fold_gate_counters(const_cast<hsm_ctx*>(h))) return -1;
  return h->levels[level].last_update_index;
}

int hsm_download_level(hsm_ctx* h, int level, float* logodds, int* update_index) {
  if (int rc = valid_level(h, level)) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  Level& L = h->levels[level];
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (logodds) HIP_TRY(hipMemcpy(logodds, L.d_logodds, L.cells() * sizeof(float), hipMemcpyDeviceToHost));
  if (update_index)
    HIP_TRY(hipMemcpy(update_index, L.d_update_index, L.cells() * sizeof(int), hipMemcpyDeviceToHost));
  return HSM_OK;
}
int hsm_upload_level(hsm_ctx* h, int level, const float* logodds, const int* update_index) {
  if (int rc = valid_level(h, level)) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  Level& L = h->levels[level];
  if (h->upd.upd_boxes_outstanding)
    if (int rc = merge_device_boxes(h)) return rc;
  if (h->upd.gate_outstanding)
    if (int rc = fold_gate_counters(h)) return rc;
  if (int rc = order_after_foreign_match(h)) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (logodds) HIP_TRY(hipMemcpy(L.d_logodds, logodds, L.cells() * sizeof(float), hipMemcpyHostToDevice));
  if (update_index) {
    HIP_TRY(hipMemcpy(L.d_update_index, update_index, L.cells() * sizeof(int), hipMemcpyHostToDevice));
    // the reference's cell rules read these stamps: while one is at or ahead of the counter the apply passes read them, too
    int top = -1;
    for (size_t i = 0; i < L.cells(); ++i) top = update_index[i] > top ? update_index[i] : top;
    L.uploaded_stamp_max = top;
  }
  if (int rc = rebuild_probability(h, L)) return rc;
  whole_level_changed(L);
  HIP_TRY(hipStreamSynchronize(h->stream));
  return HSM_OK;
}
int hsm_download_rows(hsm_ctx* h, int level, int y0, int y1, float* rows) {
  if (int rc = valid_level(h, level)) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  Level& L = h->levels[level];
  if (y0 < 0 || y1 > L.sy || y0 > y1 || !rows) return fail(HSM_ERR_INVALID, "hsm_download_rows: bad row range");
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (y1 > y0)
    HIP_TRY(hipMemcpy(rows, L.d_logodds + (size_t)y0 * L.sx, (size_t)(y1 - y0) * L.sx * sizeof(float),
                      hipMemcpyDeviceToHost));
  return HSM_OK;
}
int hsm_download_cells(hsm_ctx* h, int level, int x0, int y0, int x1, int y1, void* dst_cells, int dst_pitch_cells) {
  if (int rc = valid_level(h, level)) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  Level& L = h->levels[level];
  if (x0 < 0 || y0 < 0 || x1 >= L.sx || y1 >= L.sy || x1 < x0 || y1 < y0 || !dst_cells || dst_pitch_cells < x1 - x0 + 1)
    return fail(HSM_ERR_INVALID, "hsm_download_cells: bad rectangle");
  const int w = x1 - x0 + 1, hgt = y1 - y0 + 1;
  const size_t need = (size_t)w * hgt * 8;
  if (int rc = h->d_cells.reserve(need, kHalfMore)) return rc;
  hipLaunchKernelGGL(pack_cells_kernel, dim3(grid_for((size_t)w * hgt)), dim3(256), 0, h->stream, level_rw(L), x0, y0, w,
                     hgt, reinterpret_cast<int2*>(h->d_cells.p));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy2DAsync(dst_cells, (size_t)dst_pitch_cells * 8, h->d_cells, (size_t)w * 8, (size_t)w * 8, hgt,
                           hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return HSM_OK;
}
int hsm_last_update_bbox(const hsm_ctx* h, int level, int bbox[4]) {
  if (int rc = valid_level(h, level)) return rc;
  if (h->upd.upd_boxes_outstanding) {  // a device-side update since the last look: wait for it and fetch its boxes
    hsm_ctx* m = const_cast<hsm_ctx*>(h);
    std::lock_guard<std::mutex> lk(m->mu);
    if (m->upd.upd_boxes_outstanding)
      if (int rc = merge_device_boxes(m)) return rc;
  }
  for (int i = 0; i < 4; ++i) bbox[i] = h->levels[level].bbox[i];
  return HSM_OK;
}
int hsm_take_dirty_bbox(hsm_ctx* h, int level, int bbox[4]) {
  if (int rc = valid_level(h, level)) return rc;
  if (!bbox) return fail(HSM_ERR_INVALID, "hsm_take_dirty_bbox: bbox is null");
  std::lock_guard<std::mutex> lk(h->mu);
  if (h->upd.upd_boxes_outstanding)
    if (int rc = merge_device_boxes(h)) return rc;
  Level& L = h->levels[level];
  for (int i = 0; i < 4; ++i) bbox[i] = L.dirty[i];
  L.dirty[0] = L.dirty[1] = 0;
  L.dirty[2] = L.dirty[3] = -1;
  return HSM_OK;
}
int hsm_download_prob(hsm_ctx* h, int level, float* prob) {
  if (int rc = valid_level(h, level)) return rc;
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  Level& L = h->levels[level];
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(prob, L.d_prob, L.cells() * sizeof(float), hipMemcpyDeviceToHost));
  return HSM_OK;
}

int hsm_hessian_derivs(hsm_ctx* h, int level, const float pose_map[3], const float* pts, int n, float H[9],
                       float dTr[3]) {
  if (int rc = valid_level(h, level)) return rc;
  if (!pose_map || n < 0 || (n > 0 && !pts) || !H || !dTr) return fail(HSM_ERR_INVALID, "bad argument");
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  if (int rc = h->d_scan.reserve((size_t)n, kScanGrowth)) return rc;
  if (n > 0) HIP_TRY(hipMemcpyAsync(h->d_scan, pts, (size_t)n * sizeof(float2), hipMemcpyHostToDevice, h->stream));
  const LevelView v = level_view(h->levels[level], 1.0f, 1);
  float* d_out = h->single.d_small + 16;
  with_sampler_form(h, [&](auto lay, auto ex) {
    hipLaunchKernelGGL((gn_eval_kernel<lay(), ex()>), dim3(1), dim3(1024), 0, h->stream, v, h->d_scan, n,
                       pose_map[0], pose_map[1], pose_map[2], d_out);
  });
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(h->single.h_small + 16, d_out, 12 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  for (int i = 0; i < 9; ++i) H[i] = h->single.h_small[16 + i];
  for (int i = 0; i < 3; ++i) dTr[i] = h->single.h_small[25 + i];
  return HSM_OK;
}

int hsm_eval_beams(hsm_ctx* h, int level, const float pose_map[3], const float* pts, int n, float* out4) {
  if (int rc = valid_level(h, level)) return rc;
  if (!pose_map || n < 0 || (n > 0 && (!pts || !out4))) return fail(HSM_ERR_INVALID, "bad argument");
  if (n == 0) return HSM_OK;
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  if (int rc = h->d_scan.reserve((size_t)n * 3, kScanGrowth)) return rc;  // pts + float4 out
  HIP_TRY(hipMemcpyAsync(h->d_scan, pts, (size_t)n * sizeof(float2), hipMemcpyHostToDevice, h->stream));
  float4* d_out = reinterpret_cast<float4*>(h->d_scan + (((size_t)n + 1) & ~(size_t)1));
  const LevelView v = level_view(h->levels[level], 1.0f, 1);
  const int grid = (n + 255) / 256;
  with_sampler_form(h, [&](auto lay, auto) {  // (the terms of single beams: no summation order)
    hipLaunchKernelGGL((gn_beam_terms_kernel<lay()>), dim3(grid), dim3(256), 0, h->stream, v, h->d_scan, n,
                       pose_map[0], pose_map[1], pose_map[2], d_out);
  });
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out4, d_out, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return HSM_OK;
}

int hsm_debug_set_coop_barrier(hsm_ctx* h, unsigned value) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(h->single.d_partials + 2 * 64 * 12, &value, sizeof value, hipMemcpyHostToDevice));
  h->single.coop_bar_base = value;
  return HSM_OK;
}

int hsm_debug_set_coop_mute(hsm_ctx* h, int block_plus_one) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  std::lock_guard<std::mutex> lk(h->mu);
  h->single.coop_mute_block = block_plus_one;
  return HSM_OK;
}

int hsm_debug_set_schedule(hsm_ctx* h, int level, int gn_steps) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  if (level >= (int)h->levels.size() || (level >= 0 && gn_steps < 1))
    return fail(HSM_ERR_INVALID, "hsm_debug_set_schedule: level out of range or gn_steps < 1");
  std::lock_guard<std::mutex> lk(h->mu);
  h->batch.sched_level = level < 0 ? -1 : level;
  h->batch.sched_steps = level < 0 ? 0 : gn_steps;
  return HSM_OK;
}

int hsm_debug_batch_order(hsm_ctx* h, int batch, const float* d_begin_world, int* d_perm_out, void* stream) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  if (batch < 1 || !d_begin_world || !d_perm_out) return fail(HSM_ERR_INVALID, "hsm_debug_batch_order: bad argument");
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  return launch_batch_order(h, d_begin_world, batch, d_perm_out, h->cfg.batch.batch_order == HSM_ORDER_AUTO, (hipStream_t)stream);
}

int hsm_debug_spec_stats(hsm_ctx* h, int enable, unsigned long long out[4]) {
  if (!h) return fail(HSM_ERR_INVALID, "null context");
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (out) {
    out[0] = out[1] = out[2] = out[3] = 0;
    if (h->batch.d_spec_stats) HIP_TRY(hipMemcpy(out, h->batch.d_spec_stats, sizeof(SpecStats), hipMemcpyDeviceToHost));
  }
  if (enable && !h->batch.d_spec_stats) HIP_TRY(hipMalloc((void**)&h->batch.d_spec_stats, sizeof(SpecStats)));
  if (h->batch.d_spec_stats) HIP_TRY(hipMemset(h->batch.d_spec_stats, 0, sizeof(SpecStats)));
  if (!enable && h->batch.d_spec_stats) {
    HIP_TRY(hipFree(h->batch.d_spec_stats));
    h->batch.d_spec_stats = nullptr;
  }
  return HSM_OK;
}

int hsm_debug_coop_fallbacks(hsm_ctx* h) {
  if (!h) return 0;
  std::lock_guard<std::mutex> lk(h->mu);
  return (int)h->single.coop_fallbacks;
}

int hsm_debug_marks_nonzero(hsm_ctx* h, int level, unsigned long long out[2]) {
  if (int rc = valid_level(h, level)) return rc;
  if (!out) return fail(HSM_ERR_INVALID, "hsm_debug_marks_nonzero: out is null");
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  Level& L = h->levels[level];
  unsigned long long* d = nullptr;
  HIP_TRY(hipMalloc((void**)&d, 2 * sizeof(unsigned long long)));
  hipError_t e = hipMemsetAsync(d, 0, 2 * sizeof(unsigned long long), h->stream);
  if (e == hipSuccess) {
    const size_t nb = (mark_plane_bytes(L.sx, L.sy)) / 4, nw = (L.cells() + 31) / 32 + 1;
    hipLaunchKernelGGL(count_nonzero_words_kernel, dim3(grid_for(nb)), dim3(256), 0, h->stream,
                       reinterpret_cast<const unsigned int*>(L.d_free_bytes), nb, d);
    hipLaunchKernelGGL(count_nonzero_words_kernel, dim3(grid_for(nw)), dim3(256), 0, h->stream, L.d_occ_bits, nw, d + 1);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, d, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  (void)hipFree(d);
  if (e != hipSuccess) return fail(HSM_ERR_HIP, "hsm_debug_marks_nonzero", e);
  return HSM_OK;
}

int hsm_debug_set_update_serial(hsm_ctx* h, int level, unsigned serial) {
  if (int rc = valid_level(h, level)) return rc;
  if (serial > kSerialMax) return fail(HSM_ERR_INVALID, "hsm_debug_set_update_serial: serial exceeds the key generation field");
  std::lock_guard<std::mutex> lk(h->mu);
  h->levels[level].serial = serial;
  return HSM_OK;
}

// x[n] up, kernel(x, n, a, b) over n threads, a[n] and b[n] down; the scratch block is the call's own
static int debug_sweep(hsm_ctx* h, void (*kernel)(const float*, int, float*, float*), int n, const float* x, float* out_a,
                       float* out_b, const char* who) {
  std::lock_guard<std::mutex> lk(h->mu);
  if (int rc = select_device(h)) return rc;
  float* d = nullptr;
  HIP_TRY(hipMalloc((void**)&d, 3 * (size_t)n * sizeof(float)));
  hipError_t e = hipMemcpyAsync(d, x, (size_t)n * sizeof(float), hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, d, n, d + n, d + 2 * (size_t)n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out_a, d + n, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(out_b, d + 2 * (size_t)n, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  (void)hipFree(d);
  if (e != hipSuccess) return fail(HSM_ERR_HIP, who, e);
  return HSM_OK;
}

int hsm_debug_expf(hsm_ctx* h, int n, const float* x, float* out_exp, float* out_prob) {
  if (!h || n < 0 || (n > 0 && (!x || !out_exp || !out_prob))) return fail(HSM_ERR_INVALID, "hsm_debug_expf: bad argument");
  if (n == 0) return HSM_OK;
  return debug_sweep(h, expf_debug_kernel, n, x, out_exp, out_prob, "hsm_debug_expf");
}

int hsm_debug_sincos(hsm_ctx* h, int n, const float* x, float* s, float* c) {
  if (!h || n < 0 || (n > 0 && (!x || !s || !c))) return fail(HSM_ERR_INVALID, "hsm_debug_sincos: bad argument");
  if (n == 0) return HSM_OK;
  return debug_sweep(h, sincos_debug_kernel, n, x, s, c, "hsm_debug_sincos");
}


}  // extern "C"
