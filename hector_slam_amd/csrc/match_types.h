// match_types.h -- the types a matcher launch is described with: the layout constants, the affine map <-> world transforms, the
// read-only view of a pyramid level and the kernel argument block.  Types only -- no device function and no kernel -- so
// hsm_ctx.h, and with it every translation unit, can include it without parsing a matcher kernel.  The device primitives that
// work on these types are in beam_sample.h (the sampler) and gn_step.h (a Gauss-Newton step); each kernel is in the header of
// the one unit that launches it (hsm_ctx.h lists them).
#pragma once
#include <hip/hip_runtime.h>

#include "pose_exchange.h"

namespace hsm {

constexpr int kMaxLevels = 8;
constexpr int kLayoutQuad = 1;
constexpr int kLayoutPlane = 2;

// Eigen::Affine2f as the reference builds it: 2x2 linear (column major) + translation.
struct Affine2 {
  float l00, l10, l01, l11, t0, t1;
};

// read-only view of one pyramid level for the matcher
struct LevelView {
  const float4* quad;  // texels {P00,P10,P01,P11}, row major (quad_index), + one all-zero texel at quad_texels
  const float* prob;   // [sy*sx] plain probability plane (row major) + sx+2 zero cells
  int sx, sy;
  int tiles_x;         // quad tiles per row = ceil(sx / 4)
  int quad_texels;     // sx * sy
  float limx, limy;    // dims - 2  (MapDimensionProperties.h:70-74)
  Affine2 mapTworld;   // GridMapBase.h:272
  Affine2 worldTmap;   // GridMapBase.h:279
  float pt_scale;      // 2^-level applied to the level-0 endpoints (DataPointContainer.h:46-58)
  int gn_steps;        // 1 + maxIterations (ScanMatcher.h:74,94-97)
};

struct SpecStats {  // optional counters of gn_match_spec_kernel: boundaries walked, candidate == carry, shifted, re-run
  unsigned long long boundaries, exact, shifted, rerun;
};

struct MatchParams {
  LevelView lv[kMaxLevels];
  int first_level;         // coarsest level to run (levels first_level .. last_level, descending)
  int last_level;
  int batch;
  const float* begin_world;  // [B*3], or nullptr: the single start estimate travels in begin_inline
  float begin_inline[3];
  const float2* pts;         // packed endpoints
  const int* offsets;        // [B+1] or nullptr (shared scan)
  int shared_n;
  float* out_pose;           // [B*3]
  float* out_cov;            // [B*9] or nullptr
  float* trace;              // nullptr, or [steps*12] per-GN-step record of scan 0 (draw/debug hooks):
                             // {map-frame estimate after the step [3], H of that step [9] col-major}
  unsigned* done_flag;       // nullptr, or a host-visible word that receives done_seq (system-scope release)
  unsigned done_seq;         // after the single-scan results are written: the host polls it instead of
                             // waiting for the end-of-kernel signal
  unsigned* err_flag;        // nullptr, or a host-visible word that receives done_seq when the cooperative matcher's
                             // exchange gave up waiting for a workgroup's record (the pose is then not to be used)
  int xcd_chunk;             // workgroup -> scan mapping (xcd_block): 0 = one contiguous eighth of the batch per XCD,
                             // c > 0 = chunks of c workgroups dealt to the XCDs in turn
  int wg_sync;               // texel-cache form: the waves of a workgroup meet at a barrier before every beam (L1 sharing)
  int coop_mute_block;       // test hook (hsm_debug_set_coop_mute): 1 + the workgroup of the multi-workgroup matcher that never
                             // publishes its records, 0 = none -- how the suite provokes the exchange timeout
  unsigned long long* clock_probe;  // nullptr, or four words the wave of scan 0 fills: shader-clock counter (s_memtime)
                                    // and 100 MHz wall clock at its first GN step [0,1] and at its end [2,3]
  float* spec_scratch;     // gn_match_spec_kernel: [batch][spec_stride] float4s for the nine products of every beam
  unsigned spec_stride;    // float4s per scan
  SpecStats* spec_stats;   // nullptr, or counters the stitching pass adds to (hsm_debug_spec_stats)
  int n_bound;             // HOST ONLY: 0 = scan lengths live on the device only (max_n is a hint), else no scan is longer than this
  const int* perm;         // nullptr, or [batch]: launch slot -> scan index (hsm_set_batch_order: the batch in Morton order of its start
                           // poses; results still land at the scan's own index).  Read by the texel-cache batch forms only
  ExchangeFused xp;        // world > 0: this launch posts its poses into an exchange and unpacks an earlier epoch (forms that support
                           // it say so by setting hsm_ctx::fused_exchange_done; the others leave both to a launch of pose_exchange.hip)
};

}  // namespace hsm
