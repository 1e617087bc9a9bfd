// settings_check.cpp -- hector_slam_amd/csrc/settings.h on the CPU (tests/test_settings.py): parse_settings against the chain of
// getenv lines hsm_create carried before it, restated literally on a plain bag of the context's fields (getenv -> env_get, the table
// below; `delete h; return fail(code, text)` -> the code and the text), over every name x every value x hsm_opts set and unset.
// Every field and every refusal (code and text) is compared.  Prints one JSON line {"cases": N, "mismatches": M}, returns M != 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "settings.h"

using hsm_host::Settings;

// ---- the injected environment ---------------------------------------------------------------------------------------------------
static const char* const kNames[] = {
    "HSM_LAYOUT", "HSM_WPS", "HSM_BPL", "HSM_COOP_MIN", "HSM_COOP_TAGGED", "HSM_SPIN_WAIT", "HSM_ASYNC_UPDATE", "HSM_OVERLAP_UPLOAD",
    "HSM_TEXEL_CACHE", "HSM_UPDATE_ZEROCOPY_MAX", "HSM_PARITY", "HSM_BATCH_ORDER", "HSM_BATCH_ORDER_MIN", "HSM_BATCH_ORDER_REFRESH",
    "HSM_MERGED_MARK_MAX", "HSM_SCATTER_TEXELS_MAX", "HSM_DENSE_BITS", "HSM_EXACT_CACHED", "HSM_EXACT_DENSE", "HSM_EXACT_SPEC",
    "HSM_EXACT_SPEC1", "HSM_EXACT_DENSE_MIN", "HSM_EXACT_CHAIN_WAVE", "HSM_EXACT_SPLIT_TAIL", "HSM_WG_SYNC", "HSM_SPB_LARGE",
    "HSM_XCD_CHUNK", "HSM_CAST_FORM", "HSM_WINDOW_FORM", "HSM_XCD_CHUNK_EXACT", "HSM_COPY_STAGE",
    // the two settings of other objects (group.hip, pose_exchange.hip): neither the chain nor the parser may read them
    "HSM_GROUP_GATHER", "HSM_EXCHANGE_TIMEOUT_MS"};
constexpr int kNameCount = sizeof kNames / sizeof kNames[0];
static_assert(kNameCount == 33, "every HSM_* setting of the library");
// (every name takes every value, the words included: a number-valued name must read a word as atoi does)
static const char* const kValues[] = {nullptr, "", "0", "1", "2", "8", "-1", "4096", "abc", "auto", "fast", "exact", "relaxed",
                                      "Exact", "given", "morton", "plane", "quad", "wave", "lane"};
constexpr int kValueCount = sizeof kValues / sizeof kValues[0];

static const char* g_env[kNameCount];
static const char* env_get(const char* name) {
  for (int i = 0; i < kNameCount; ++i)
    if (strcmp(name, kNames[i]) == 0) return g_env[i];
  fprintf(stderr, "a name this check does not know: %s\n", name);
  exit(2);
}

// ---- hsm_create's settings block as it stood, on a bag of hsm_ctx's fields with their defaults -----------------------------------
constexpr int kLayoutQuad = hsm_plan::kQuad, kLayoutPlane = hsm_plan::kPlane;
struct OldCtx {
  int layout = kLayoutQuad;
  int wps_override = 0;
  bool texel_cache = true;
  bool async_update = true;
  int update_zero_copy_max = 4096;
  int merged_mark_max = 4096;
  int scatter_texels_max = 1 << 30;
  bool spin_wait = true;
  bool overlap_upload = true;
  int coop_min_beams = 4096;
  bool coop_tagged = true;
  bool copy_stage = false;
  int bpl_override = -1;
  int xcd_chunk_exact = 0;
  int xcd_chunk = 16;
  int spb_large = 8;
  int wg_sync = -1;
  bool dense_bits = true;
  bool exact_cached = true;
  bool exact = false;
  bool auto_parity = true;
  bool relaxed = false;
  bool exact_spec = false;
  bool exact_spec1 = false;
  int batch_order = 2;
  int batch_order_min = 1024;
  int batch_order_refresh = 16;
  bool exact_dense = true;
  int exact_dense_min = 4096;
  int exact_split_tail = 1;
  int exact_chain_wave = 1;
  int cast_form = -1;
  int window_form = -1;
};

static int old_settings(const hsm_opts* opts, OldCtx* h, const char** refusal) {
  int layout = opts ? opts->layout : HSM_LAYOUT_AUTO;
  if (layout == HSM_LAYOUT_AUTO) {
    const char* env = env_get("HSM_LAYOUT");
    layout = (env && strcmp(env, "plane") == 0) ? HSM_LAYOUT_PLANE : HSM_LAYOUT_QUAD;
  }
  h->layout = layout == HSM_LAYOUT_PLANE ? kLayoutPlane : kLayoutQuad;
  int wps = opts ? opts->waves_per_scan : 0;
  if (wps == 0) {
    const char* env = env_get("HSM_WPS");
    if (env) wps = atoi(env);
  }
  if (wps != 0 && wps != 1 && wps != 2 && wps != 4 && wps != 8 && wps != 16) {
    *refusal = "hsm_create: waves_per_scan must be 0,1,2,4,8,16";
    return HSM_ERR_INVALID;
  }
  h->wps_override = wps;
  if (const char* env = env_get("HSM_BPL")) h->bpl_override = atoi(env) == 0 ? 0 : -1;
  if (const char* env = env_get("HSM_COOP_MIN")) h->coop_min_beams = atoi(env);
  if (const char* env = env_get("HSM_COOP_TAGGED")) h->coop_tagged = atoi(env) != 0;
  if (const char* env = env_get("HSM_SPIN_WAIT")) h->spin_wait = atoi(env) != 0;
  if (const char* env = env_get("HSM_ASYNC_UPDATE")) h->async_update = atoi(env) != 0;
  if (const char* env = env_get("HSM_OVERLAP_UPLOAD")) h->overlap_upload = atoi(env) != 0;
  if (const char* env = env_get("HSM_TEXEL_CACHE")) h->texel_cache = atoi(env) != 0;
  if (const char* env = env_get("HSM_UPDATE_ZEROCOPY_MAX")) h->update_zero_copy_max = atoi(env);
  if (const char* env = env_get("HSM_PARITY")) {
    const bool is_exact = strcmp(env, "exact") == 0, is_relaxed = strcmp(env, "relaxed") == 0, is_auto = strcmp(env, "auto") == 0;
    if (!is_exact && !is_relaxed && !is_auto && strcmp(env, "fast") != 0) {
      *refusal = "hsm_create: HSM_PARITY must be one of auto, fast, exact, relaxed";
      return HSM_ERR_INVALID;
    }
    h->exact = is_exact;
    h->relaxed = is_relaxed;
    h->auto_parity = is_auto;
  }
  if (const char* env = env_get("HSM_BATCH_ORDER")) {
    if (strcmp(env, "auto") == 0) h->batch_order = HSM_ORDER_AUTO;
    else if (strcmp(env, "given") == 0) h->batch_order = HSM_ORDER_GIVEN;
    else if (strcmp(env, "morton") == 0) h->batch_order = HSM_ORDER_MORTON;
    else {
      *refusal = "hsm_create: HSM_BATCH_ORDER must be one of auto, given, morton";
      return HSM_ERR_INVALID;
    }
  }
  if (const char* env = env_get("HSM_BATCH_ORDER_MIN")) h->batch_order_min = atoi(env);
  if (const char* env = env_get("HSM_BATCH_ORDER_REFRESH")) h->batch_order_refresh = atoi(env) > 0 ? atoi(env) : 1;
  if (const char* env = env_get("HSM_MERGED_MARK_MAX")) h->merged_mark_max = atoi(env);
  if (const char* env = env_get("HSM_SCATTER_TEXELS_MAX")) h->scatter_texels_max = atoi(env);
  if (const char* env = env_get("HSM_DENSE_BITS")) h->dense_bits = atoi(env) != 0;
  if (const char* env = env_get("HSM_EXACT_CACHED")) h->exact_cached = atoi(env) != 0;
  if (const char* env = env_get("HSM_EXACT_DENSE")) h->exact_dense = atoi(env) != 0;
  if (const char* env = env_get("HSM_EXACT_SPEC")) h->exact_spec = atoi(env) != 0;
  if (const char* env = env_get("HSM_EXACT_SPEC1")) h->exact_spec1 = atoi(env) != 0;
  if (const char* env = env_get("HSM_EXACT_DENSE_MIN")) h->exact_dense_min = atoi(env);
  if (const char* env = env_get("HSM_EXACT_CHAIN_WAVE")) h->exact_chain_wave = atoi(env);
  if (const char* env = env_get("HSM_EXACT_SPLIT_TAIL")) h->exact_split_tail = atoi(env);
  if (const char* env = env_get("HSM_WG_SYNC")) h->wg_sync = atoi(env) != 0;
  if (const char* env = env_get("HSM_SPB_LARGE")) h->spb_large = atoi(env) == 8 ? 8 : 4;
  if (const char* env = env_get("HSM_XCD_CHUNK")) h->xcd_chunk = atoi(env) > 0 ? atoi(env) : 0;
  if (const char* env = env_get("HSM_CAST_FORM")) h->cast_form = !strcmp(env, "wave") ? 0 : (!strcmp(env, "lane") ? 1 : -1);
  if (const char* env = env_get("HSM_WINDOW_FORM")) h->window_form = !strcmp(env, "wave") ? 0 : (!strcmp(env, "lane") ? 1 : -1);
  if (const char* env = env_get("HSM_XCD_CHUNK_EXACT")) h->xcd_chunk_exact = atoi(env) > 0 ? atoi(env) : 0;
  if (const char* env = env_get("HSM_COPY_STAGE")) h->copy_stage = atoi(env) != 0;
  return HSM_OK;
}

// ---- the comparison -------------------------------------------------------------------------------------------------------------
static int g_cases = 0, g_bad = 0;

// every field; the two flags that were ints are compared as match_site read them (!= 0)
static bool same_fields(const OldCtx& o, const Settings& s) {
  const hsm_plan::MatchKnobs& k = s.match;
  return o.layout == s.layout && o.exact == s.parity.exact && o.auto_parity == s.parity.auto_parity && o.relaxed == s.parity.relaxed &&
         o.wps_override == k.wps_override && o.bpl_override == k.bpl_override && o.texel_cache == k.texel_cache &&
         o.exact_cached == k.exact_cached && (o.exact_chain_wave != 0) == k.exact_chain_wave &&
         (o.exact_split_tail != 0) == k.exact_split_tail && o.exact_dense == k.exact_dense && o.exact_dense_min == k.exact_dense_min &&
         o.exact_spec == k.exact_spec && o.exact_spec1 == k.exact_spec1 && o.spb_large == k.spb_large &&
         o.coop_min_beams == k.coop_min_beams && o.batch_order == s.batch.batch_order && o.batch_order_min == s.batch.batch_order_min &&
         o.batch_order_refresh == s.batch.batch_order_refresh && o.xcd_chunk == s.batch.xcd_chunk &&
         o.xcd_chunk_exact == s.batch.xcd_chunk_exact && o.wg_sync == s.batch.wg_sync && o.coop_tagged == s.single.coop_tagged &&
         o.spin_wait == s.single.spin_wait && o.overlap_upload == s.single.overlap_upload && o.async_update == s.upd.async_update &&
         o.update_zero_copy_max == s.upd.update_zero_copy_max && o.merged_mark_max == s.upd.merged_mark_max &&
         o.scatter_texels_max == s.upd.scatter_texels_max && o.dense_bits == s.upd.dense_bits && o.cast_form == s.forms.cast_form &&
         o.window_form == s.forms.window_form && o.copy_stage == s.forms.copy_stage;
}

static void describe(const hsm_opts* opts) {
  if (opts) fprintf(stderr, "  opts {layout %d, waves_per_scan %d}", opts->layout, opts->waves_per_scan);
  for (int i = 0; i < kNameCount; ++i)
    if (g_env[i]) fprintf(stderr, " %s=\"%s\"", kNames[i], g_env[i]);
  fprintf(stderr, "\n");
}

static void one_case(const hsm_opts* opts) {
  OldCtx o;
  Settings s;
  const char *old_text = "", *new_text = "";
  const int old_rc = old_settings(opts, &o, &old_text);
  const int new_rc = hsm_host::parse_settings(opts, env_get, &s, &new_text);
  ++g_cases;
  // (a refused context is deleted: its fields are compared all the same, up to where the chain stopped)
  if (old_rc == new_rc && strcmp(old_text, new_text) == 0 && same_fields(o, s)) return;
  if (++g_bad <= 10) {
    fprintf(stderr, "differs: old %d \"%s\", new %d \"%s\", fields %s\n", old_rc, old_text, new_rc, new_text, same_fields(o, s) ? "same" : "differ");
    describe(opts);
  }
}

// null, and every pair of the values a caller may pass (3 and 7: what hsm_create refuses, resp. reads as the default layout)
static void with_every_opts() {
  one_case(nullptr);
  const int layouts[] = {HSM_LAYOUT_AUTO, HSM_LAYOUT_QUAD, HSM_LAYOUT_PLANE, 7}, waves[] = {0, 1, 2, 4, 8, 16, 3, -1};
  for (int layout : layouts)
    for (int w : waves) {
      const hsm_opts opts = {-1, layout, w};
      one_case(&opts);
    }
}

int main() {
  {  // the defaults are the context's
    OldCtx o;
    Settings s;
    ++g_cases;
    if (!same_fields(o, s)) ++g_bad, fprintf(stderr, "the defaults differ\n");
  }
  // one name at a time
  for (int i = 0; i < kNameCount; ++i) {
    for (int v = 0; v < kValueCount; ++v) {
      g_env[i] = kValues[v];
      with_every_opts();
    }
    g_env[i] = nullptr;
  }
  // every name at once, at the same value
  for (int v = 0; v < kValueCount; ++v) {
    for (int i = 0; i < kNameCount; ++i) g_env[i] = kValues[v];
    with_every_opts();
  }
  for (int i = 0; i < kNameCount; ++i) g_env[i] = nullptr;
  // the names that can refuse, and the layout, two at a time: which refusal comes first, and what was set before it
  const int order[] = {0, 1, 10, 11};  // HSM_LAYOUT, HSM_WPS, HSM_PARITY, HSM_BATCH_ORDER
  for (int a = 0; a < 4; ++a)
    for (int b = a + 1; b < 4; ++b)
      for (int va = 0; va < kValueCount; ++va)
        for (int vb = 0; vb < kValueCount; ++vb) {
          g_env[order[a]] = kValues[va], g_env[order[b]] = kValues[vb];
          with_every_opts();
          g_env[order[a]] = g_env[order[b]] = nullptr;
        }
  printf("{\"cases\": %d, \"mismatches\": %d}\n", g_cases, g_bad);
  return g_bad != 0;
}
