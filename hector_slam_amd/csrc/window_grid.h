// window_grid.h -- a window of pose hypotheses around a centre (window.hip, window_kernels.h), stated once: how many hypotheses a
// window holds, which (i, j, k) a window index stands for, and the fp32 pose of a hypothesis; and the bytes of the caller-owned
// workspaces of the top-K selection and of hsm_relocalize_device, single and batched.
// Plain C++ (no HIP header): the kernels and the host compile the same text, and tests/cpp/window_grid_check.cpp and
// relocalize_batch_check.cpp print it with the host compiler alone (tests/test_window_model.py, test_relocalize_batch_abi.py).
#pragma once
#include <limits.h>
#include <stddef.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HSM_WIN_HD __host__ __device__
#else
#define HSM_WIN_HD
#endif

namespace hsm {

// half-extents (>= 0) and steps (m, m, rad) of a window: (2hx+1)(2hy+1)(2ht+1) hypotheses, x fastest, then y, then theta
struct WindowGrid {
  int hx, hy, ht;
  float step_x, step_y, step_t;
};

// the number of hypotheses; 0 for a negative half-extent, more than INT_MAX where the window is refused for its size
HSM_WIN_HD inline long long window_count(int hx, int hy, int ht) {
  if (hx < 0 || hy < 0 || ht < 0) return 0;
  const long long nx = 2ll * hx + 1, ny = 2ll * hy + 1, nt = 2ll * ht + 1;
  const long long cap = (long long)INT_MAX + 1;
  if (nx > cap || ny > cap || nt > cap) return cap;
  const long long xy = nx * ny;  // < 2^63
  if (xy > cap) return cap;
  const long long all = xy * nt;  // <= 2^31 * (2^32 - 1) < 2^63
  return all > cap ? cap : all;
}

// w = (k * (2hy+1) + j) * (2hx+1) + i
HSM_WIN_HD inline int window_index(const WindowGrid& g, int i, int j, int k) {
  return (k * (2 * g.hy + 1) + j) * (2 * g.hx + 1) + i;
}
HSM_WIN_HD inline void window_ijk(const WindowGrid& g, int w, int& i, int& j, int& k) {
  const int nx = 2 * g.hx + 1, ny = 2 * g.hy + 1;
  const int row = w / nx;
  i = w - row * nx;
  k = row / ny;
  j = row - k * ny;
}

// The pose of hypothesis (i, j, k) around the centre (cx, cy, ct): one int -> float conversion, one multiplication and one
// addition per component, each rounded to fp32 (the library and the check are built with -ffp-contract=off: no fused
// multiply-add).  The heading is not normalised.
HSM_WIN_HD inline void window_pose_ijk(const WindowGrid& g, float cx, float cy, float ct, int i, int j, int k, float& x, float& y,
                                       float& t) {
  x = cx + (float)(i - g.hx) * g.step_x;
  y = cy + (float)(j - g.hy) * g.step_y;
  t = ct + (float)(k - g.ht) * g.step_t;
}
HSM_WIN_HD inline void window_pose(const WindowGrid& g, float cx, float cy, float ct, int w, float& x, float& y, float& t) {
  int i, j, k;
  window_ijk(g, w, i, j, k);
  window_pose_ijk(g, cx, cy, ct, i, j, k, x, y, t);
}

// ---- the top-K selection's shape and workspace -------------------------------------------------------------------------------
constexpr int kMaxTopK = 64;          // HSM_MAX_TOPK
constexpr int kTopKSliceWaves = 256;  // wavefronts of the first launch at most: each leaves K candidates (score, index)

// wavefronts the first launch uses for `count` scores: one per 64 scores, kTopKSliceWaves at most, one at least
HSM_WIN_HD inline int topk_slices(int count) {
  const int w = (count + 63) / 64;
  return w < 1 ? 1 : (w > kTopKSliceWaves ? kTopKSliceWaves : w);
}
inline size_t round_up8(size_t b) { return (b + 7) & ~(size_t)7; }
// candidates of every slice: K scores, then K indices, per slice.  0 for refused sizes
inline size_t topk_workspace_bytes(int count, int k) {
  if (count < 0 || k < 1 || k > kMaxTopK) return 0;
  return round_up8((size_t)topk_slices(count) * (size_t)k * (sizeof(float) + sizeof(int)));
}

// hsm_select_topk_groups_device: the K best of each of `groups` runs of `group_size` scores.  Every group is sliced like a single
// array of group_size scores; the candidates lie group after group, all the scores, then all the indices.  One group: the bytes
// and the layout of topk_workspace_bytes.  0 for refused sizes (a negative count, k out of range, more than INT_MAX scores or
// places in all) and for no groups
struct TopKGroupsLayout {
  size_t cand_score, cand_index, total;
};
inline TopKGroupsLayout topk_groups_layout(long long groups, long long group_size, int k) {
  TopKGroupsLayout L = {0, 0, 0};
  if (groups < 0 || group_size < 0 || k < 1 || k > kMaxTopK) return L;
  if (groups > (long long)INT_MAX || group_size > (long long)INT_MAX || groups * group_size > (long long)INT_MAX ||
      groups * k > (long long)INT_MAX)
    return L;
  const size_t cands = (size_t)groups * (size_t)topk_slices((int)group_size) * (size_t)k;
  L.cand_index = cands * sizeof(float);
  L.total = round_up8(cands * (sizeof(float) + sizeof(int)));
  return L;
}
inline size_t topk_groups_workspace_bytes(long long groups, long long group_size, int k) {
  return topk_groups_layout(groups, group_size, k).total;
}

// The relocalisation's workspace, single and batched: one layout, each region 8-byte aligned.
// hsm_relocalize_batch_device, B scans with a window of W hypotheses each: the B*W scores, the grouped top-K candidates, B*K
// indices, B*K scores, B*K start poses, and -- CSR scans -- every scan laid out K times for the matcher, which takes one scan per
// pair: B*K + 1 offsets and max(K * total_points, 1) end points (one element at least: the matcher clamps an empty scan's loads to
// element 0).  A shared scan is not copied: its caller passes total_points = 0.  A total of 0: sizes the entry refuses (B < 0,
// W < 1, k out of range, total_points < 0, B*W or K*total_points above INT_MAX, B*K above INT_MAX / 9)
struct RelocalizeLayout {
  size_t scores, topk, index, kscore, pose, offsets, pts, total;
};
using RelocalizeBatchLayout = RelocalizeLayout;
inline RelocalizeLayout relocalize_batch_layout(long long B, long long W, int k, long long total_points) {
  RelocalizeLayout L = {0, 0, 0, 0, 0, 0, 0, 0};
  if (B < 0 || W < 1 || W > (long long)INT_MAX || k < 1 || k > kMaxTopK || total_points < 0) return L;
  if (B > (long long)INT_MAX || B * W > (long long)INT_MAX || B * k > (long long)(INT_MAX / 9) ||
      total_points > (long long)INT_MAX || total_points * k > (long long)INT_MAX)
    return L;
  const size_t bk = (size_t)B * (size_t)k, copied = (size_t)total_points * (size_t)k;
  L.scores = 0;
  L.topk = round_up8((size_t)B * (size_t)W * sizeof(float));
  L.index = L.topk + topk_groups_workspace_bytes(B, W, k);
  L.kscore = L.index + round_up8(bk * sizeof(int));
  L.pose = L.kscore + round_up8(bk * sizeof(float));
  L.offsets = L.pose + round_up8(bk * 3 * sizeof(float));
  L.pts = L.offsets + round_up8((bk + 1) * sizeof(int));
  L.total = L.pts + (copied > 0 ? copied : 1) * 2 * sizeof(float);
  return L;
}

// hsm_relocalize_device: one scan in one window, never copied -- the batched layout's front (one group's W scores, top-K
// candidates, K indices, K scores, K start poses), which ends behind the start poses.  0 for refused sizes
inline RelocalizeLayout relocalize_layout(long long W, int k) {
  RelocalizeLayout L = relocalize_batch_layout(1, W, k, 0);
  L.total = L.pts = L.offsets;
  return L;
}

}  // namespace hsm
