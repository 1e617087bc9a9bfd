// map_update_scans.h -- posed scans that are already on the device (hsm_update_by_scans_device*, hsm_slam_scans_device*).
// The host knows neither a scan's pose nor its length, so everything prepare_level() / level_bbox() derive from them on the
// host is derived here:
//   update_prep_kernel        one launch per call, one wavefront per scan (lane = level): scan k's UpdateBatch, in a
//                             context-owned device array, from d_poses_world[k] -- the fp32 expressions of prepare_level()
//   update_mark_scan_kernel   update_mark_kernel's two block kinds on that UpdateBatch, read through a pointer (wave-uniform
//                             address: scalar loads); the grid is sized by the caller's hint and strides over the scan's real
//                             beam count.  Its end-cell blocks also reduce the scan's cell box (DPP min / max per wavefront,
//                             one lane's atomicMin / atomicMax) into the scan's box, the level's running dirty box and its
//                             publish box (occupancy_kernels.h).  Cell boxes: map_cells.h.
//   update_apply_scan_kernel  apply_box() over that box, in a grid sized for the whole level (the host cannot size it by a
//                             box it never sees); a later launch on the same stream, so the box is complete.
// Keyed form for every scan length (correct for any length; the byte-map form needs per-beam records sized by the host).
#pragma once
#include "update_gate.h"
#include "update_types.h"

namespace hsm {

struct UpdatePrepLevel {
  LevelRW lv;
  Affine2 mapTworld;
  float pt_scale;                 // 2^-level: DataContainer::setFrom (DataPointContainer.h:46-58)
  float origo_x, origo_y;         // the container's origo on this level (setFrom :48)
  float log_odds_free, log_odds_occ;
  unsigned int serial0;           // the level's key generation before the call: scan k takes ((serial0 + k) % kSerialMax) + 1
  int update_index0;              // currUpdateIndex before the call: scan k marks with update_index0 + 3 k + 1 / + 2
};

struct UpdatePrepParams {
  UpdatePrepLevel lv[kMaxLevels];
  int nlev, count;
  const float* poses_world;  // [count * 3]
  const float2* pts;
  const int* offsets;        // [count + 1] CSR offsets in points, or nullptr: every pose integrates pts[0 .. shared_n)
  int shared_n;
  const float2* origos;      // [count] the containers' origos in level-0 cell units, level l sees origos[k] * 2^-l (setFrom :48);
                             // or nullptr: the host pair UpdatePrepLevel::origo_x/y for every scan
  UpdateBatch* out;          // [count]
  int* boxes;                // [(count + 2) * kMaxLevels * 4]: slot 0 the running dirty boxes, slot 1 the LAST scan's, 2 + k scan k's
};

// the box slot of scan k of a call of `count` scans (the last scan's sits where the host finds it without knowing count)
__host__ __device__ __forceinline__ int update_box_slot(int k, int count) { return k == count - 1 ? 1 : 2 + k; }

// scan k's own points: [first, first + n) of A.pts
__device__ __forceinline__ void scan_range(const UpdatePrepParams& A, int k, int& first, int& n) {
  first = 0;
  n = A.shared_n;
  if (A.offsets) {
    first = A.offsets[k];
    n = A.offsets[k + 1] - first;
  }
}

// scan k's UpdateParams of level l and its (empty) box: points [first, first + n) of A.pts at `pose`, marked with
// update_index0 + 3 * rank + 1 / + 2 (currMarkFreeIndex / currMarkOccIndex, OccGridMapBase.h:123-124).  `origo`: with
// A.origos, the level-0 origo of the container this level integrates (the scan's own, or the retained scan's on the coarse
// levels of a forced scan); not read otherwise.
__device__ __forceinline__ void update_prep_scan_level(const UpdatePrepParams& A, int k, int l, float px, float py, float th,
                                                       int first, int n, int rank, float2 origo) {
  const UpdatePrepLevel& V = A.lv[l];
  UpdateParams P;
  P.lv = V.lv;
  float mx, my;
  affine_apply(V.mapTworld, px, py, mx, my);  // getMapCoordsPose
  // Translation2f(mapPose.xy) * Rotation2Df(mapPose.theta): glibc's sinf / cosf (the pair sincosf returns, libm_exact.h)
  float sinA, cosA;
  libm::sincosf_glibc<false>(th, sinA, cosA);
  P.pose.l00 = cosA;
  P.pose.l01 = -sinA;
  P.pose.l10 = sinA;
  P.pose.l11 = cosA;
  P.pose.t0 = mx;
  P.pose.t1 = my;
  // setFrom's origo * factor (DataPointContainer.h:48): one fp32 multiply per component, level 0 takes the origo as it is --
  // the expression the host evaluates for the pair it passes
  const float ox = A.origos == nullptr ? V.origo_x : (l == 0 ? origo.x : origo.x * V.pt_scale);
  const float oy = A.origos == nullptr ? V.origo_y : (l == 0 ? origo.y : origo.y * V.pt_scale);
  float bx, by;
  affine_apply(P.pose, ox, oy, bx, by);
  bx += 0.5f;
  by += 0.5f;
  // x86's truncating conversion makes a NaN or out-of-range begin coordinate INT_MIN, which fails the map test of every beam;
  // this device's makes a NaN 0, a VALID cell.  beam_line()'s finite-range test, applied to the begin cell: what it rejects is
  // outside the map in the reference too, and (-1, -1) drops every beam the same way.
  const bool finite = bx > -2.0f && bx < (float)V.lv.sx + 2.0f && by > -2.0f && by < (float)V.lv.sy + 2.0f;
  P.bx = finite ? (int)bx : -1;
  P.by = finite ? (int)by : -1;
  if (n < 0 || n > (int)kBeamMask) n = 0;  // (more beams than the key's index field holds: integrated as an empty scan)
  P.pts = A.pts + first;
  P.n = n;
  P.pt_scale = V.pt_scale;
  P.serial = (V.serial0 + (unsigned int)k) % kSerialMax + 1u;
  P.log_odds_free = V.log_odds_free;
  P.log_odds_occ = V.log_odds_occ;
  P.mark_free = V.update_index0 + 3 * rank + 1;
  P.mark_occ = V.update_index0 + 3 * rank + 2;
  P.x0 = P.y0 = kBoxEmptyLo;  // (the passes take the box from A.boxes)
  P.x1 = P.y1 = kBoxEmptyHi;
  P.recs = nullptr;
  UpdateBatch& B = A.out[k];
  B.lv[l] = P;
  if (l == 0) B.nlev = A.nlev;
  int* box = A.boxes + ((size_t)update_box_slot(k, A.count) * kMaxLevels + l) * 4;
  box[0] = box[1] = kBoxEmptyLo;
  box[2] = box[3] = kBoxEmptyHi;
}

__global__ void __launch_bounds__(64) update_prep_kernel(const UpdatePrepParams A) {
  const int k = blockIdx.x, l = threadIdx.x;
  if (l >= A.nlev) return;
  int first, n;
  scan_range(A, k, first, n);
  // every scan is integrated: scan k is update k of the call
  const float2 origo = A.origos ? A.origos[k] : make_float2(0.0f, 0.0f);
  update_prep_scan_level(A, k, l, A.poses_world[3 * k], A.poses_world[3 * k + 1], A.poses_world[3 * k + 2], first, n, k, origo);
}

// ---- the movement gate in front of them (hsm_update_by_scans_device_gated, hsm_slam_scans_device) -------------------------------
// HectorSlamProcessor::update (HectorSlamProcessor.h:71-95) integrates a scan only where util::poseDifferenceLargerThan(pose,
// lastMapUpdatePose, ..) holds or the caller forces it, and lastMapUpdatePose follows every integrated scan: the decisions of a
// call are SEQUENTIAL in k, and the host sees none of them.  So what the host derived per scan for the ungated entry -- "scan k is
// update k" -- is derived here: ONE launch per call, one workgroup.  Lane 0 walks the scans, 256 a turn (update_gate.h's
// gate_step, the text the CPU model test compiles), and leaves {integrated, rank, the coarse levels' points} per scan in LDS;
// then all lanes fill the UpdateBatch blocks as update_prep_kernel does.  A rejected scan gets n = 0 on every level and an empty
// box: update_mark_scan_kernel and update_apply_scan_kernel return after one scalar load.  The gate's state lives in a
// per-context device block and is written with ordinary stores.
struct GateState {
  float last_update_pose[3];  // lastMapUpdatePose: FLT_MAX three times until a scan is integrated
  int pending;                // updates that gated calls applied and the host has not yet folded into Level's counters
  // hsm_slam_scans_device
  float hint[3];              // start estimate of the next scan
  int retained_first;         // the scan the coarse levels retain (matchData's setFrom, MapRepMultiMap.h:143): points
  float last_pose[3];         // lastScanMatchPose                                   [retained_first, + retained_n) of this
  int retained_n;             //                                                     call's d_pts_xy
  float last_cov[9];          // lastScanMatchCov
  float retained_origo[2];    // the retained scan's origo, level-0 cell units (setFrom copies it with the points, :48); read
  int reserved[1];            // only by calls that carry per-scan origos
};
static_assert(sizeof(GateState) == 24 * 4, "GateState: six 16-byte rows");

struct UpdateGateParams {
  UpdatePrepParams prep;
  GateState* state;
  float min_dist, min_angle;
  const unsigned char* force;  // [count] map_without_matching per scan, or nullptr
  int* out_applied;            // [count], or nullptr
  // hsm_slam_scans_device's call for ONE scan (count == 1), behind its match:
  int slam;
  float* pose_io;              // [3] the matched pose; a forced scan takes its hint instead (written here)
  float* cov_io;               // [9] the match's covariance, or nullptr; a forced scan keeps the last one (written here)
  const float* next_delta;     // [3] added to the pose to give the next scan's hint, or nullptr: the pose itself
};

constexpr int kGateChunk = 256;

__global__ void __launch_bounds__(256) update_gate_prep_kernel(const UpdateGateParams G) {
  __shared__ int4 walk[kGateChunk];  // {integrated, rank, first point of the coarse levels' container, its length}
  __shared__ float2 walk_origo[kGateChunk];  // that container's origo (per-scan origos only)
  const UpdatePrepParams& A = G.prep;
  GateWalk w;
  gate_reset(w);
  GateRetained ret;
  gate_retained_reset(ret);
  if (threadIdx.x == 0) {
    w.last_update_pose[0] = G.state->last_update_pose[0];
    w.last_update_pose[1] = G.state->last_update_pose[1];
    w.last_update_pose[2] = G.state->last_update_pose[2];
    w.applied = G.state->pending;
    ret.first = G.state->retained_first;
    ret.n = G.state->retained_n;
    ret.origo[0] = G.state->retained_origo[0];
    ret.origo[1] = G.state->retained_origo[1];
  }
  for (int k0 = 0; k0 < A.count; k0 += kGateChunk) {
    const int chunk = min(kGateChunk, A.count - k0);
    if (threadIdx.x == 0) {
      for (int j = 0; j < chunk; ++j) {
        const int k = k0 + j;
        const bool force = G.force != nullptr && G.force[k] != 0;
        int first, n;
        scan_range(A, k, first, n);
        const float2 own = A.origos ? A.origos[k] : make_float2(0.0f, 0.0f);
        float pose[3];
        if (G.slam) {
          // a forced scan skips the match (HectorSlamProcessor.h:75-80): its pose is its hint, the covariance stays, and the
          // coarse levels keep the containers of the last matched scan
          for (int i = 0; i < 3; ++i) pose[i] = force ? G.state->hint[i] : G.pose_io[3 * k + i];
          if (force)
            for (int i = 0; i < 3; ++i) G.pose_io[3 * k + i] = pose[i];
          gate_retain_step(ret, force, first, n, own.x, own.y);
          if (G.cov_io) {
            for (int i = 0; i < 9; ++i) {
              if (force)
                G.cov_io[9 * k + i] = G.state->last_cov[i];
              else if (n > 0)  // (matchData leaves the covariance alone for an empty container, ScanMatcher.h:62-64)
                G.state->last_cov[i] = G.cov_io[9 * k + i];
            }
          }
          for (int i = 0; i < 3; ++i) {
            G.state->last_pose[i] = pose[i];
            G.state->hint[i] = G.next_delta ? pose[i] + G.next_delta[i] : pose[i];
          }
        } else {
          for (int i = 0; i < 3; ++i) pose[i] = A.poses_world[3 * k + i];
          gate_retain_step(ret, false, first, n, own.x, own.y);  // every level sees the scan itself, as in hsm_update_by_scans_device
        }
        int rank;
        const bool go = gate_step(w, pose, force, G.min_dist, G.min_angle, &rank);
        walk[j] = make_int4(go ? 1 : 0, rank, ret.first, ret.n);
        walk_origo[j] = make_float2(ret.origo[0], ret.origo[1]);
        if (G.out_applied) G.out_applied[k] = go ? 1 : 0;
      }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < chunk * A.nlev; t += blockDim.x) {
      const int j = t / A.nlev, l = t - j * A.nlev, k = k0 + j;
      const int4 d = walk[j];
      int first, n;
      scan_range(A, k, first, n);
      float2 origo = A.origos ? A.origos[k] : make_float2(0.0f, 0.0f);
      if (l > 0) {
        first = d.z;
        n = d.w;
        origo = walk_origo[j];
      }
      const float* pose = G.slam ? G.pose_io + 3 * k : A.poses_world + 3 * k;
      update_prep_scan_level(A, k, l, pose[0], pose[1], pose[2], first, d.x ? n : 0, d.y, origo);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    G.state->last_update_pose[0] = w.last_update_pose[0];
    G.state->last_update_pose[1] = w.last_update_pose[1];
    G.state->last_update_pose[2] = w.last_update_pose[2];
    G.state->pending = w.applied;
    G.state->retained_first = ret.first;
    G.state->retained_n = ret.n;
    G.state->retained_origo[0] = ret.origo[0];
    G.state->retained_origo[1] = ret.origo[1];
  }
}

// lastMapUpdatePose back to FLT_MAX (hsm_reset_update_gate); `all`: lastScanMatchPose and the hint back to 0 as well
// (HectorSlamProcessor::reset, HectorSlamProcessor.h:133-140).  The counters stay: the maps keep theirs.
__global__ void update_gate_reset_kernel(GateState* state) {
  if (threadIdx.x < 3) {
    state->last_update_pose[threadIdx.x] = FLT_MAX;
    state->last_pose[threadIdx.x] = 0.0f;
    state->hint[threadIdx.x] = 0.0f;
  }
}

// hsm_slam_scans_device, in front of the first scan of a call: its hint is the start pose -- or, where the caller gives none,
// the last pose of the call before -- plus delta 0; the coarse levels' containers do not outlive the call that owned their points
__global__ void slam_begin_kernel(GateState* state, const float* __restrict__ start_pose, const float* __restrict__ delta0) {
  if (threadIdx.x < 3) {
    const float p = start_pose ? start_pose[threadIdx.x] : state->last_pose[threadIdx.x];
    state->hint[threadIdx.x] = delta0 ? p + delta0[threadIdx.x] : p;
  }
  if (threadIdx.x == 0) {
    state->retained_first = 0;
    state->retained_n = 0;
    state->retained_origo[0] = state->retained_origo[1] = 0.0f;
  }
}

template <int CTRL>
__device__ __forceinline__ int dpp_i32(int v) {
  return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xf, 0xf, false);
}
// min or max over the wavefront, in every lane (all 64 lanes active): the 16-lane rows by DPP, the four rows by readlane
template <bool MAX>
__device__ __forceinline__ int wave_reduce_i32(int v) {
  auto op = [](int a, int b) { return MAX ? max(a, b) : min(a, b); };
  v = op(v, dpp_i32<0xB1>(v));   // quad_perm [1,0,3,2]
  v = op(v, dpp_i32<0x4E>(v));   // quad_perm [2,3,0,1]
  v = op(v, dpp_i32<0x141>(v));  // row_half_mirror
  v = op(v, dpp_i32<0x140>(v));  // row_mirror
  return op(op(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
            op(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}
constexpr bool kWaveMin = false, kWaveMax = true;

__device__ __forceinline__ void box_widen_atomic(int* box, int x0, int y0, int x1, int y1) {
  atomicMin(&box[0], x0);
  atomicMin(&box[1], y0);
  atomicMax(&box[2], x1);
  atomicMax(&box[3], y1);
}

// The cell box of everything beams [block * 256, block * 256 + 256) of the scan can touch: the hull of the end cells of its
// non-skipped beams and the begin cell (a Bresenham line stays inside the box of its end points) -- every cell a mark pass
// writes to, so the apply pass over it clears every mark.  level_bbox() on the host also counts beams that end IN the begin
// cell (skipped, OccGridMapBase.h:158): its box is this one, or the begin cell alone where this one is empty.
// Called by all 64 lanes of every wavefront.
__device__ __forceinline__ void mark_box_block(const UpdateParams& P, unsigned int block, int* scan_box, int* run_box,
                                               int* pub_box) {
  const int beam = block * blockDim.x + threadIdx.x;
  int x0 = kBoxEmptyLo, y0 = kBoxEmptyLo, x1 = kBoxEmptyHi, y1 = kBoxEmptyHi;
  if (beam < P.n) {
    const BeamLine b = beam_line(P, beam);
    if (b.valid) {
      x0 = x1 = b.x1;
      y0 = y1 = b.y1;
    }
  }
  x1 = wave_reduce_i32<kWaveMax>(x1);
  if (x1 < 0) return;  // wave-uniform: no beam of this wavefront ends inside the map
  x0 = min(wave_reduce_i32<kWaveMin>(x0), P.bx);
  y0 = min(wave_reduce_i32<kWaveMin>(y0), P.by);
  x1 = max(x1, P.bx);
  y1 = max(wave_reduce_i32<kWaveMax>(y1), P.by);
  if ((threadIdx.x & 63) == 0) {
    box_widen_atomic(scan_box, x0, y0, x1, y1);
    box_widen_atomic(run_box, x0, y0, x1, y1);
    box_widen_atomic(pub_box, x0, y0, x1, y1);
  }
}

// gridDim.x = occ_blocks + free_blocks, sized by the caller's hint: the first occ_blocks workgroups of a row mark end cells and
// reduce the box, 256 beams a turn, the others walk lines, 4 beams a turn, until the scan's real beam count is covered
__global__ void __launch_bounds__(256) update_mark_scan_kernel(const UpdateBatch* __restrict__ B, unsigned int occ_blocks,
                                                               int* scan_boxes, int* run_boxes, int* pub_boxes) {
  const UpdateParams P = B->lv[blockIdx.y];
  if (P.n <= 0) return;
  if (blockIdx.x < occ_blocks) {
    const unsigned int turns = ((unsigned int)P.n + 255u) / 256u;
    for (unsigned int b = blockIdx.x; b < turns; b += occ_blocks) {
      mark_occ_block(P, b);
      mark_box_block(P, b, scan_boxes + 4 * blockIdx.y, run_boxes + 4 * blockIdx.y, pub_boxes + 4 * blockIdx.y);
    }
  } else {
    const unsigned int free_blocks = gridDim.x - occ_blocks, turns = ((unsigned int)P.n + 3u) / 4u;
    for (unsigned int b = blockIdx.x - occ_blocks; b < turns; b += free_blocks) mark_free_block(P, b);
  }
}

template <bool SCATTER_TEXELS, bool STAMPED>
__global__ void __launch_bounds__(256) update_apply_scan_kernel(const UpdateBatch* __restrict__ B,
                                                                const int* __restrict__ scan_boxes) {
  const int4 box = *reinterpret_cast<const int4*>(scan_boxes + 4 * blockIdx.y);
  if (box.z < box.x) return;  // nothing of this scan on this level
  UpdateParams P = B->lv[blockIdx.y];
  P.x0 = box.x;
  P.y0 = box.y;
  P.x1 = box.z;
  P.y1 = box.w;
  apply_box<SCATTER_TEXELS, STAMPED>(P, blockIdx.x * (size_t)blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x);
}

// the running dirty boxes of all levels back to empty (after the host has merged them)
__global__ void update_boxes_clear_kernel(int* boxes, int n_boxes) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 4 * n_boxes) boxes[i] = (i & 3) < 2 ? kBoxEmptyLo : kBoxEmptyHi;
}

}  // namespace hsm
