// match_teams.hip -- launches of the team forms of the matcher (gn_match_teams.h: gn_match_kernel on 1 .. 16 wavefronts per scan,
// either summation order) and of the fast texel-cache forms (gn_match_cached.h: gn_match_cached_kernel).  About eighty instantiations: a
// translation unit of its own so that an edit elsewhere does not rebuild them.
#include "beam_sample.h"
#include "gn_match_cached.h"
#include "gn_match_teams.h"
#include "hsm_ctx.h"

namespace hsm {
// ---- hsm_set_batch_order: the batch in Morton order of its start poses ---------------------------------------------------------
// Scans that sit next to each other in a launch run on the same XCD at the same time and share the texel lines they touch in its
// L2; a batch in an order that does not follow the map loses that (profiles/r06: +5 % on the 2048^2 map, +22 % on the 4096^2
// pyramid).  ONE workgroup: counting sort of the batch by the Morton code of the 64 x 64 level-0 tile its start pose lies in
// (4096 bins in LDS); the order inside a tile is whatever the LDS atomics make it -- any order gives the same results, a scan's
// result depends on nothing but the scan.  perm[slot] = scan.
__device__ __forceinline__ unsigned part1by1_6(unsigned v) {  // 6 bits -> every other bit
  v &= 0x3fu;
  v = (v | (v << 4)) & 0x30fu;
  v = (v | (v << 2)) & 0x333u;
  v = (v | (v << 1)) & 0x555u;
  return v;
}

// a position in bin `key` for every valid lane.  A batch that already follows the map has 64 equal keys per wavefront, which the LDS
// would serialise: a wavefront whose lanes all hold ONE key takes one atomic between them; otherwise an atomic per lane (no loop: the
// eight calls of a thread stay independent instruction streams)
__device__ __forceinline__ int bin_take(int* bins, int key, bool valid, int lane) {
  const unsigned long long todo = __ballot(valid);
  if (todo == 0ull) return 0;
  const int k = __builtin_amdgcn_readfirstlane(key);  // (the first active lane's: lanes beyond the batch sit at the end)
  const unsigned long long m = __ballot(valid && key == k);
  int pos = 0;
  if (m == todo && __builtin_amdgcn_readfirstlane((int)valid) != 0) {  // one key
    if (valid) {
      int base = 0;
      const int first = __ffsll((long long)m) - 1;
      if (lane == first) base = atomicAdd(&bins[k], (int)__popcll(m));
      pos = __shfl(base, first) + (int)__popcll(m & ((1ull << lane) - 1ull));
    }
  } else if (valid) {
    pos = atomicAdd(&bins[key], 1);
  }
  return pos;
}

// detect != 0 (HSM_ORDER_AUTO): a batch that follows the map already -- its tile changes between neighbours number no more than a
// few times its distinct tiles -- keeps its own order (the identity permutation): the order inside a tile would only get worse.
__global__ void __launch_bounds__(1024) batch_order_kernel(Affine2 mapTworld, int tile_shift, const float* __restrict__ begin_world, int batch,
                                                           int* __restrict__ perm, int detect) {
  constexpr int KPT = 8;  // scans per thread and pass: their start poses are loaded together, not one dependent round trip each
  __shared__ int bins[4096];
  __shared__ int part[1024];
  __shared__ int changes, tiles;
  const int tid = (int)threadIdx.x, lane = tid & 63;
  for (int i = tid; i < 4096; i += 1024) bins[i] = 0;
  if (tid == 0) changes = 0, tiles = 0;
  __syncthreads();
  auto keys_of = [&](int first, int (&key)[KPT]) {
    float x[KPT], y[KPT];
#pragma unroll
    for (int u = 0; u < KPT; ++u) {
      const int i = first + u * 1024 + tid;
      x[u] = i < batch ? begin_world[3 * i + 0] : 0.0f;
      y[u] = i < batch ? begin_world[3 * i + 1] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < KPT; ++u) {
      float mx, my;
      affine_apply(mapTworld, x[u], y[u], mx, my);
      // (a NaN or far-away start estimate: any tile will do)
      const int cx = mx == mx ? (int)fminf(fmaxf(mx, 0.0f), 1.0e6f) : 0, cy = my == my ? (int)fminf(fmaxf(my, 0.0f), 1.0e6f) : 0;
      const int tx = min(cx >> tile_shift, 63), ty = min(cy >> tile_shift, 63);
      key[u] = (int)(part1by1_6((unsigned)tx) | (part1by1_6((unsigned)ty) << 1));
    }
  };
  int key[KPT];
  for (int first = 0; first < batch; first += 1024 * KPT) {
    keys_of(first, key);
#pragma unroll
    for (int u = 0; u < KPT; ++u) {
      const bool valid = first + u * 1024 + tid < batch;
      bin_take(bins, key[u], valid, lane);
      if (detect) {  // neighbours in the batch are neighbours in the wavefront (the first lane's left neighbour is not looked at)
        const int left = __shfl_up(key[u], 1);
        const unsigned long long m = __ballot(valid && lane > 0 && key[u] != left);
        if (lane == 0 && m != 0ull) atomicAdd(&changes, (int)__popcll(m));
      }
    }
  }
  __syncthreads();
  const int c0 = bins[4 * tid], c1 = bins[4 * tid + 1], c2 = bins[4 * tid + 2], c3 = bins[4 * tid + 3];
  if (detect) {
    const int wave_tiles = (int)(__popcll(__ballot(c0 != 0)) + __popcll(__ballot(c1 != 0)) + __popcll(__ballot(c2 != 0)) + __popcll(__ballot(c3 != 0)));
    if (lane == 0 && wave_tiles) atomicAdd(&tiles, wave_tiles);
    __syncthreads();
    if (changes <= 4 * tiles + 16) {  // (workgroup-uniform)
      for (int i = tid; i < batch; i += 1024) perm[i] = i;
      return;
    }
  }
  // exclusive scan of the 1024 partial counts: inside the wavefront by DPP-free shuffles, then over the 16 wavefront totals
  const int mine = c0 + c1 + c2 + c3;
  int inc = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int v = __shfl_up(inc, d);
    if (lane >= d) inc += v;
  }
  if (lane == 63) part[tid >> 6] = inc;
  __syncthreads();
  int wave_base = 0;
  for (int w = 0; w < (tid >> 6); ++w) wave_base += part[w];
  const int base = wave_base + inc - mine;
  bins[4 * tid] = base, bins[4 * tid + 1] = base + c0, bins[4 * tid + 2] = base + c0 + c1, bins[4 * tid + 3] = base + c0 + c1 + c2;
  __syncthreads();
  for (int first = 0; first < batch; first += 1024 * KPT) {
    if (batch > 1024 * KPT) keys_of(first, key);  // (a batch of one pass still holds its keys)
#pragma unroll
    for (int u = 0; u < KPT; ++u) {
      const int i = first + u * 1024 + tid;
      const int pos = bin_take(bins, key[u], i < batch, lane);
      if (i < batch) perm[pos] = i;
    }
  }
}

}  // namespace hsm

namespace hsm_host {

int launch_batch_order(hsm_ctx* h, const float* begin_world, int batch, int* perm, bool detect, hipStream_t stream) {
  // 64 tiles span the longer edge of level 0
  const Level& L0 = h->levels[0];
  int shift = 0;
  while ((64 << shift) < (L0.sx > L0.sy ? L0.sx : L0.sy)) ++shift;
  hipLaunchKernelGGL(batch_order_kernel, dim3(1), dim3(1024), 0, stream, L0.mapTworld, shift, begin_world, batch, perm, detect ? 1 : 0);
  HIP_TRY(hipGetLastError());
  return HSM_OK;
}

int ensure_batch_perm(hsm_ctx* h, MatchParams& P, hipStream_t stream) {
  if (P.perm != nullptr || P.begin_world == nullptr || P.batch < h->cfg.batch.batch_order_min) return HSM_OK;
  const bool automatic = h->cfg.batch.batch_order == HSM_ORDER_AUTO;
  if (h->cfg.batch.batch_order != HSM_ORDER_MORTON && !(automatic && hsm_plan::level0_outgrows_l2(h->levels[0].cells()))) return HSM_OK;
  // A launch into a graph capture keeps the caller's order and leaves the stream's permutation as it is.  Its sort would run at
  // the replays only, while the host state below would claim it had run now (an eager launch of that size would then reuse a
  // buffer that holds another batch's permutation); and a graph that read the buffer would read it after an eager launch had
  // rewritten it or, growing it, freed it.
  if (stream_capturing(stream)) return HSM_OK;
  hsm_ctx::PermBuf* pb = nullptr;
  for (hsm_ctx::PermBuf& b : h->batch.perm_bufs)
    if (b.s == stream) pb = &b;
  if (!pb) {
    if (h->batch.perm_bufs.size() >= 8) return HSM_OK;  // (a ninth stream keeps the caller's order)
    h->batch.perm_bufs.push_back({stream, {}, 0, 0});
    pb = &h->batch.perm_bufs.back();
  }
  if (!pb->d.holds((size_t)P.batch)) pb->batch = 0;  // (the permutation goes with the block; the free waits for launches that read it)
  if (int rc = pb->d.reserve(((size_t)P.batch + 4095) / 4096 * 4096)) return rc;  // multiples of 4096 ints
  if (pb->batch == P.batch && pb->used < h->cfg.batch.batch_order_refresh) {  // the permutation of an earlier launch of this stream
    ++pb->used;
    P.perm = pb->d;
    h->last.last_sorted = true;
    return HSM_OK;
  }
  if (int rc = launch_batch_order(h, P.begin_world, P.batch, pb->d, automatic, stream)) return rc;
  pb->batch = P.batch, pb->used = 1;
  P.perm = pb->d;
  h->last.last_sorted = true;
  return HSM_OK;
}

namespace {

using hsm_plan::Family;

// gn_match_kernel<WPS, SPB, ., BPL>, and for one-wavefront teams of 9 or 17 beams per lane the fast texel-cache form next to it
template <int WPS, int SPB, int BPL>
void launch_team(const MatchParams& P, const MatchPlan& plan, hipStream_t stream) {
  const dim3 grid(plan.grid), block(plan.block);
  if constexpr (WPS == 1 && (BPL == 9 || BPL == 17)) {
    if (plan.family == Family::kCached) {
      if (plan.relaxed)
        hipLaunchKernelGGL((gn_match_cached_kernel<SPB, BPL, kLayoutQuad, 1, true>), grid, block, 0, stream, P);
      else if (plan.layout == kLayoutQuad)
        hipLaunchKernelGGL((gn_match_cached_kernel<SPB, BPL, kLayoutQuad>), grid, block, 0, stream, P);
      else
        hipLaunchKernelGGL((gn_match_cached_kernel<SPB, BPL, kLayoutPlane>), grid, block, 0, stream, P);
      return;
    }
  }
  if (plan.layout == kLayoutPlane)
    hipLaunchKernelGGL((gn_match_kernel<WPS, SPB, kLayoutPlane, BPL>), grid, block, 0, stream, P);
  else
    hipLaunchKernelGGL((gn_match_kernel<WPS, SPB, kLayoutQuad, BPL>), grid, block, 0, stream, P);
}

// gn_match_kernel<WPS, SPB, ., 0, EXACT>: the reference's summation order, endpoints streamed
template <int WPS, int SPB>
void launch_team_exact(const MatchParams& P, const MatchPlan& plan, hipStream_t stream) {
  if (plan.layout == kLayoutPlane)
    hipLaunchKernelGGL((gn_match_kernel<WPS, SPB, kLayoutPlane, 0, true>), dim3(plan.grid), dim3(plan.block), 0, stream, P);
  else
    hipLaunchKernelGGL((gn_match_kernel<WPS, SPB, kLayoutQuad, 0, true>), dim3(plan.grid), dim3(plan.block), 0, stream, P);
}

template <int WPS, int SPB>
void launch_team_w(const MatchParams& P, const MatchPlan& plan, hipStream_t stream) {
  if (plan.family == Family::kTeamExact) return launch_team_exact<WPS, SPB>(P, plan, stream);
  if (plan.bpl == 0) return launch_team<WPS, SPB, 0>(P, plan, stream);
  if constexpr (WPS == 1)  // (two beams per lane: one-wavefront teams only, match_plan.h)
    if (plan.bpl == 2) return launch_team<WPS, SPB, 2>(P, plan, stream);
  if (plan.bpl == 3) return launch_team<WPS, SPB, 3>(P, plan, stream);
  if (plan.bpl == 5) return launch_team<WPS, SPB, 5>(P, plan, stream);
  if (plan.bpl == 9) return launch_team<WPS, SPB, 9>(P, plan, stream);
  return launch_team<WPS, SPB, 17>(P, plan, stream);
}

}  // namespace

// the plan's team form or fast texel-cache form (match_plan.h: plan_team) -> its instantiation
int launch_team_form(hsm_ctx*, const MatchParams& P, const MatchPlan& plan, hipStream_t stream) {
  switch (plan.wps) {
    case 1:
      if (plan.spb == 8)
        plan.bpl == 9 ? launch_team<1, 8, 9>(P, plan, stream) : launch_team<1, 8, 17>(P, plan, stream);
      else
        launch_team_w<1, 4>(P, plan, stream);
      break;
    case 2: launch_team_w<2, 1>(P, plan, stream); break;
    case 4: launch_team_w<4, 1>(P, plan, stream); break;
    case 8: launch_team_w<8, 1>(P, plan, stream); break;
    default: launch_team_w<16, 1>(P, plan, stream); break;
  }
  HIP_TRY(hipGetLastError());
  return HSM_OK;
}

}  // namespace hsm_host
