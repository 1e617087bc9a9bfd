// match_exact_cached.hip -- launches of the exact-order texel-cache batch forms (gn_match_exact.h): the headline kernel of
// configs[2] / configs[3] and its chain-wavefront forms.  A translation unit of its own: these twelve instantiations are a third
// of the library's compile time, and the kernel is the one that gets edited.
#include "match_plan.h"  // (first: its defaults of the cached rows must be gn_match_exact.h's, asserted below)
#include "gn_match_exact.h"
#include "hsm_ctx.h"

namespace hsm_host {
namespace {

static_assert(hsm_plan::kQuad == kLayoutQuad && hsm_plan::kPlane == kLayoutPlane, "match_plan.h restates match_types.h");
static_assert(hsm_plan::kXbpc == HSM_XBPC && hsm_plan::kXbpcMain == HSM_XBPC_MAIN && hsm_plan::kXbpcCw == HSM_XBPC_CW,
              "match_plan.h restates gn_match_exact.h");

template <int BPL, int BPC = BPL, bool CW = false, bool PROBE = false>
void launch(MatchParams& P, const MatchPlan& plan, hipStream_t stream) {
  static_assert(BPC == BPL || BPC == HSM_XBPC || BPC == HSM_XBPC_MAIN || BPC == HSM_XBPC_CW || BPC == HSM_XBPC_CW + 1, "cached rows");
  hipLaunchKernelGGL((gn_match_exact_cached_kernel<4, BPL, BPC, CW, PROBE>), dim3(plan.grid), dim3(plan.block), 0, stream, P);
}

}  // namespace

// the plan's exact-order texel-cache form (match_plan.h: plan_exact_cached) -> its instantiation
int launch_exact_cached_form(hsm_ctx* h, MatchParams P, const MatchPlan& plan, hipStream_t stream) {
  const bool cw = plan.family == hsm_plan::Family::kExactCachedCw;
  if (cw) P.xp.world = 0;       // (the chain-wavefront forms do not carry it: the caller queues the stand-alone exchange kernel)
  if (plan.carries_exchange) {  // this launch carries the pose exchange: every scan posts its pose, the workgroups behind the matcher's own unpack
    P.xp.match_blocks = plan.grid - P.xp.wait_blocks;
    h->batch.fused_exchange_done = true;
  }
  // workgroup -> XCD mapping: this form runs best with one contiguous eighth of the batch per XCD on every map size (2048^2
  // headline: 57.5 us against 58.3 with the fast form's chunks of 16 workgroups dealt in turn; chunks of 8 / 32: 58.4;
  // profiles/r04/exact_kernel_param_sweep.txt) -- its rounds are paced by barriers and chain jobs, not by how long a scan's
  // gathers take, so the load balancing the chunks buy the fast form is not needed and the compacter L2 footprint wins.
  // env HSM_XCD_CHUNK_EXACT=n restores chunks of n workgroups (of four scans).
  P.xcd_chunk = h->cfg.batch.xcd_chunk_exact;
  const int bpl = plan.bpl, bpc = plan.bpc;
  if (bpl == 5) cw ? launch<5, 5, true>(P, plan, stream) : launch<5>(P, plan, stream);
  else if (bpl == 9) cw ? launch<9, 9, true>(P, plan, stream) : launch<9>(P, plan, stream);
  else if (bpl == 13 && cw) bpc == 13 ? launch<13, 13, true>(P, plan, stream) : launch<13, HSM_XBPC_CW + 1, true>(P, plan, stream);
  else if (bpl == 13) launch<13>(P, plan, stream);
  else if (cw) bpc == HSM_XBPC ? launch<17, HSM_XBPC, true>(P, plan, stream) : launch<17, HSM_XBPC_CW, true>(P, plan, stream);
  else if (bpc != HSM_XBPC_MAIN) launch<17, HSM_XBPC>(P, plan, stream);
  else if (plan.probe) launch<17, HSM_XBPC_MAIN, false, true>(P, plan, stream);
  else launch<17, HSM_XBPC_MAIN>(P, plan, stream);
  HIP_TRY(hipGetLastError());
  return HSM_OK;
}

}  // namespace hsm_host
