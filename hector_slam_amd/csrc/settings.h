// settings.h -- everything hsm_opts and the environment decide about a context: the fields, their defaults, their env names, and the
// one parser that fills them (hsm_create calls it with getenv).  Plain C++17, no HIP and no context: tests/cpp/settings_check.cpp
// runs the parser on the CPU against the chain of getenv lines it replaced.  A setting's env name and meaning stand at its field,
// here (the matcher's knobs: match_plan.h MatchKnobs) and nowhere else.  HSM_GROUP_GATHER (group.hip) and HSM_EXCHANGE_TIMEOUT_MS
// (pose_exchange.hip) belong to objects other than the context and are read where those are created.
#pragma once
#include <limits.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>

#include "hector_mi355/capi.h"
#include "match_plan.h"

namespace hsm_host {

struct Settings {
  // hsm_opts::layout, else env HSM_LAYOUT=quad|plane: hsm_plan::kQuad (the default) or kPlane, which are match_types.h's kLayout*
  int layout = hsm_plan::kQuad;
  // hsm_set_parity, env HSM_PARITY=auto|fast|exact|relaxed (none of the three: HSM_PARITY_FAST)
  struct Parity {
    bool exact = false;       // HSM_PARITY_EXACT: H / dTr summed in the reference's beam order (gn_step.h exact_round)
    bool auto_parity = true;  // HSM_PARITY_AUTO (default): every entry point in the reference's summation order (wants_exact)
    bool relaxed = false;     // HSM_PARITY_RELAXED: contracted multiply-adds in the throughput kernel (gn_match_cached_kernel<.., RELAXED>)
  } parity;
  hsm_plan::MatchKnobs match;  // which form a match launch takes (match_plan.h plan_match)
  // how a batch is laid over the device (match.hip, match_teams.hip, match_exact_cached.hip)
  struct Batch {
    // hsm_set_batch_order: launch order of a batch (texel-cache batch forms)
    int batch_order = HSM_ORDER_AUTO;  // env HSM_BATCH_ORDER=auto|given|morton
    int batch_order_min = 1024;        // env HSM_BATCH_ORDER_MIN: smaller batches keep the caller's order
    int batch_order_refresh = 16;  // hsm_set_batch_order_refresh / env HSM_BATCH_ORDER_REFRESH: a stream's permutation serves that many
                                   // launches of the same batch size before it is computed again (ANY permutation gives the same
                                   // results; an old one only groups the scans by where they were)
    int xcd_chunk = 16;            // env HSM_XCD_CHUNK: workgroups per chunk of the chunked-cyclic batch mapping (0 = contiguous eighths)
    int xcd_chunk_exact = 0;       // env HSM_XCD_CHUNK_EXACT: the same for the exact-order texel-cache form (0 = contiguous eighths, its default)
    int wg_sync = -1;              // env HSM_WG_SYNC=0|1: per-beam workgroup barrier of the texel-cache matcher (-1 = for maps > 2^23 cells)
  } batch;
  // the single-scan path (match.hip)
  struct Single {
    bool coop_tagged = true;     // env HSM_COOP_TAGGED=0: the counter grid barrier instead of the tagged-record exchange
    bool spin_wait = true;       // single-scan matches: poll the kernel's completion word (env HSM_SPIN_WAIT=0: off)
    bool overlap_upload = true;  // env HSM_OVERLAP_UPLOAD=0: the copy is queued on `stream` as before
  } single;
  // map updates (map_update.hip)
  struct Update {
    bool async_update = true;          // updateByScan returns when its kernels are QUEUED (env HSM_ASYNC_UPDATE=0: wait for them)
    int update_zero_copy_max = 4096;   // env HSM_UPDATE_ZEROCOPY_MAX
    int merged_mark_max = 4096;        // scans below this take the one-launch mark pass (env HSM_MERGED_MARK_MAX, 0 = never)
    int scatter_texels_max = 1 << 30;  // quad layout: scans below this write the texels from the apply pass (env HSM_SCATTER_TEXELS_MAX, 0 = never)
    bool dense_bits = true;            // env HSM_DENSE_BITS=0: dense scans keep the keyed update (map_update.h)
  } upd;
  // the form of an entry that has two, whatever its size (-1 = by its size), and the route of a map copy
  struct Forms {
    int cast_form = -1;       // env HSM_CAST_FORM=wave|lane: hsm_cast_scans* take that walk whatever the fan (-1 = by its length, rays.hip)
    int window_form = -1;     // env HSM_WINDOW_FORM=wave|lane: hsm_score_window* take that form whatever the window (-1 = by its size, window.hip)
    bool copy_stage = false;  // env HSM_COPY_STAGE=1: copies INTO this context take the staged route from the same device too
  } forms;
};

using Env = const char* (*)(const char*);  // getenv, or a test's table

// "0" and whatever atoi reads as 0 (a word, nothing) is off, any other number on; unset keeps the default
template <class T>
inline void env_flag(Env env, const char* name, T* out) {
  if (const char* v = env(name)) *out = atoi(v) != 0;
}
// as atoi reads it, but no less than `floor`; false and *out unchanged where the name is unset
inline bool env_int(Env env, const char* name, int* out, int floor = INT_MIN) {
  const char* v = env(name);
  if (v) *out = atoi(v) < floor ? floor : atoi(v);
  return v != nullptr;
}
// the index of the value among `words`, -1 for any other value, `unset` where the name is unset
inline int env_word(Env env, const char* name, int unset, std::initializer_list<const char*> words) {
  const char* v = env(name);
  if (!v) return unset;
  int i = 0;
  for (const char* w : words) {
    if (strcmp(v, w) == 0) return i;
    ++i;
  }
  return -1;
}

// *out (defaults on entry) as `opts` (may be null) and the environment set it; hsm_opts goes before the environment for the layout and
// the waves per scan.  HSM_OK, or HSM_ERR_INVALID with *refusal the text for hsm_last_error() (*out is then half filled).
inline int parse_settings(const hsm_opts* opts, Env env, Settings* out, const char** refusal) {
  int v = 0;
  int layout = opts ? opts->layout : HSM_LAYOUT_AUTO;
  if (layout == HSM_LAYOUT_AUTO) layout = env_word(env, "HSM_LAYOUT", -1, {"plane"}) == 0 ? HSM_LAYOUT_PLANE : HSM_LAYOUT_QUAD;
  out->layout = layout == HSM_LAYOUT_PLANE ? hsm_plan::kPlane : hsm_plan::kQuad;
  hsm_plan::MatchKnobs& k = out->match;
  int wps = opts ? opts->waves_per_scan : 0;
  if (wps == 0) env_int(env, "HSM_WPS", &wps);
  if (wps != 0 && wps != 1 && wps != 2 && wps != 4 && wps != 8 && wps != 16) {
    *refusal = "hsm_create: waves_per_scan must be 0,1,2,4,8,16";
    return HSM_ERR_INVALID;
  }
  k.wps_override = wps;
  if (env_int(env, "HSM_BPL", &v)) k.bpl_override = v == 0 ? 0 : -1;
  env_int(env, "HSM_COOP_MIN", &k.coop_min_beams);
  env_flag(env, "HSM_COOP_TAGGED", &out->single.coop_tagged);
  env_flag(env, "HSM_SPIN_WAIT", &out->single.spin_wait);
  env_flag(env, "HSM_ASYNC_UPDATE", &out->upd.async_update);
  env_flag(env, "HSM_OVERLAP_UPLOAD", &out->single.overlap_upload);
  env_flag(env, "HSM_TEXEL_CACHE", &k.texel_cache);
  env_int(env, "HSM_UPDATE_ZEROCOPY_MAX", &out->upd.update_zero_copy_max);
  // only the four documented words change the mode; anything else ("Exact", "1", a typo) must not silently select the
  // fast tree: the context is refused
  const int parity = env_word(env, "HSM_PARITY", -2, {"auto", "fast", "exact", "relaxed"});
  if (parity == -1) {
    *refusal = "hsm_create: HSM_PARITY must be one of auto, fast, exact, relaxed";
    return HSM_ERR_INVALID;
  }
  if (parity >= 0) out->parity.auto_parity = parity == 0, out->parity.exact = parity == 2, out->parity.relaxed = parity == 3;
  static_assert(HSM_ORDER_GIVEN == 0 && HSM_ORDER_MORTON == 1 && HSM_ORDER_AUTO == 2, "the words below are in the order of capi.h");
  const int order = env_word(env, "HSM_BATCH_ORDER", out->batch.batch_order, {"given", "morton", "auto"});
  if (order == -1) {
    *refusal = "hsm_create: HSM_BATCH_ORDER must be one of auto, given, morton";
    return HSM_ERR_INVALID;
  }
  out->batch.batch_order = order;
  env_int(env, "HSM_BATCH_ORDER_MIN", &out->batch.batch_order_min);
  env_int(env, "HSM_BATCH_ORDER_REFRESH", &out->batch.batch_order_refresh, 1);
  env_int(env, "HSM_MERGED_MARK_MAX", &out->upd.merged_mark_max);
  env_int(env, "HSM_SCATTER_TEXELS_MAX", &out->upd.scatter_texels_max);
  env_flag(env, "HSM_DENSE_BITS", &out->upd.dense_bits);
  env_flag(env, "HSM_EXACT_CACHED", &k.exact_cached);
  env_flag(env, "HSM_EXACT_DENSE", &k.exact_dense);
  env_flag(env, "HSM_EXACT_SPEC", &k.exact_spec);
  env_flag(env, "HSM_EXACT_SPEC1", &k.exact_spec1);
  env_int(env, "HSM_EXACT_DENSE_MIN", &k.exact_dense_min);
  env_flag(env, "HSM_EXACT_CHAIN_WAVE", &k.exact_chain_wave);
  env_flag(env, "HSM_EXACT_SPLIT_TAIL", &k.exact_split_tail);
  env_flag(env, "HSM_WG_SYNC", &out->batch.wg_sync);
  if (env_int(env, "HSM_SPB_LARGE", &v)) k.spb_large = v == 8 ? 8 : 4;
  env_int(env, "HSM_XCD_CHUNK", &out->batch.xcd_chunk, 0);
  out->forms.cast_form = env_word(env, "HSM_CAST_FORM", out->forms.cast_form, {"wave", "lane"});
  out->forms.window_form = env_word(env, "HSM_WINDOW_FORM", out->forms.window_form, {"wave", "lane"});
  env_int(env, "HSM_XCD_CHUNK_EXACT", &out->batch.xcd_chunk_exact, 0);
  env_flag(env, "HSM_COPY_STAGE", &out->forms.copy_stage);
  return HSM_OK;
}

}  // namespace hsm_host
