// group.hip -- the multi-GPU group of the C ABI (include/hector_mi355/capi.h: hsm_group_*, hsm_shard_bounds): one context per
// device, a worker thread per replica beyond the first, and the gather of the shards' results.  Host code only, no kernel of its
// own: it reaches the core runtime (hector_mi355.hip) through the C ABI and through select_device, fail and set_error_text, and
// the matcher (match.hip) through match_batch_device_nolock (hsm_ctx.h, hsm_host.h).
#include <dlfcn.h>
#include <hip/hip_runtime.h>
// RCCL: declarations only -- librccl is dlopen'ed by the group entry points (rccl_api), never linked.  A ROCm install without
// the RCCL development headers still builds the library: the handful of prototypes the group gather uses are then declared
// here (the stable NCCL 2.x C API; values as in nccl.h).
#if __has_include(<rccl/rccl.h>) && !defined(HSM_NO_RCCL_HEADER)
#include <rccl/rccl.h>
#else
extern "C" {
typedef struct ncclComm* ncclComm_t;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclFloat = 7 } ncclDataType_t;
ncclResult_t ncclCommInitAll(ncclComm_t* comm, int ndev, const int* devlist);
ncclResult_t ncclCommDestroy(ncclComm_t comm);
ncclResult_t ncclGroupStart(void);
ncclResult_t ncclGroupEnd(void);
ncclResult_t ncclAllGather(const void* sendbuff, void* recvbuff, size_t sendcount, ncclDataType_t datatype, ncclComm_t comm, hipStream_t stream);
ncclResult_t ncclSend(const void* sendbuff, size_t count, ncclDataType_t datatype, int peer, ncclComm_t comm, hipStream_t stream);
ncclResult_t ncclRecv(void* recvbuff, size_t count, ncclDataType_t datatype, int peer, ncclComm_t comm, hipStream_t stream);
const char* ncclGetErrorString(ncclResult_t result);
ncclResult_t ncclGetVersion(int* version);
}
#endif
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "hector_mi355/capi.h"
#include "hsm_ctx.h"

using namespace hsm_host;

// One persistent host thread per replica beyond the first (replica 0 runs on the calling thread): a job slot guarded by
// a mutex + condition variable; threads live as long as the group, so a batched match costs no thread creation.
struct GroupWorker {
  std::thread th;
  std::mutex m;
  std::condition_variable cv;
  std::function<int()> job;
  bool has_job = false, done = false, quit = false;
  int rc = HSM_OK;
  std::string err;
};

// RCCL, loaded on first use: the single-GPU library keeps its dependency set (HIP / HSA / libc), and a process that never
// gathers across devices never maps the 570 MB librccl.  In a process that has PyTorch-ROCm loaded the SONAME resolves to
// the librccl torch already brought in (one RCCL, one HIP runtime); elsewhere to /opt/rocm/lib.
struct RcclApi {
  void* lib = nullptr;
  decltype(&ncclCommInitAll) CommInitAll = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclGroupStart) GroupStart = nullptr;
  decltype(&ncclGroupEnd) GroupEnd = nullptr;
  decltype(&ncclAllGather) AllGather = nullptr;
  decltype(&ncclSend) Send = nullptr;
  decltype(&ncclRecv) Recv = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
  decltype(&ncclGetVersion) GetVersion = nullptr;
  std::string error;
};

static RcclApi* rccl_api() {
  static RcclApi api;
  static std::once_flag once;
  std::call_once(once, [] {
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      api.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
      if (api.lib) break;
    }
    if (!api.lib) {
      const char* e = dlerror();
      api.error = std::string("dlopen(librccl.so.1): ") + (e ? e : "not found");
      return;
    }
    bool ok = true;
    auto sym = [&](const char* n) -> void* {
      void* p = dlsym(api.lib, n);
      if (!p) {
        ok = false;
        api.error = std::string("librccl: missing symbol ") + n;
      }
      return p;
    };
    api.CommInitAll = reinterpret_cast<decltype(api.CommInitAll)>(sym("ncclCommInitAll"));
    api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(sym("ncclCommDestroy"));
    api.GroupStart = reinterpret_cast<decltype(api.GroupStart)>(sym("ncclGroupStart"));
    api.GroupEnd = reinterpret_cast<decltype(api.GroupEnd)>(sym("ncclGroupEnd"));
    api.AllGather = reinterpret_cast<decltype(api.AllGather)>(sym("ncclAllGather"));
    api.Send = reinterpret_cast<decltype(api.Send)>(sym("ncclSend"));
    api.Recv = reinterpret_cast<decltype(api.Recv)>(sym("ncclRecv"));
    api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(sym("ncclGetErrorString"));
    api.GetVersion = reinterpret_cast<decltype(api.GetVersion)>(sym("ncclGetVersion"));
    if (!ok) {
      dlclose(api.lib);
      api.lib = nullptr;
    }
  });
  return &api;
}

struct hsm_group {
  std::vector<hsm_ctx*> members;
  std::vector<std::unique_ptr<GroupWorker>> workers;  // workers[r - 1] serves replica r
  // device-resident gather (hsm_group_match_batch_device): per replica a result block on ITS device and an event
  std::vector<Buf<float>> d_pose, d_cov;  // (d_cov is allocated last: it holding 9 n floats says both serve n scans)
  std::vector<hipEvent_t> evt;
  // the gather itself: RCCL over the group's devices (one communicator per replica, ncclCommInitAll on first use), or
  // peer copies.  gather_pref = what was asked for (hsm_group_set_gather / env HSM_GROUP_GATHER), gather_mode = what runs.
  int gather_pref = HSM_GATHER_AUTO, gather_mode = HSM_GATHER_AUTO;
  bool force_p2p = false;  // hsm_group_debug_force_p2p: every shard, the root's too, through grouped ncclSend / ncclRecv
  std::vector<ncclComm_t> comms;
  std::vector<Buf<float>> d_all_pose, d_all_cov;  // all-gather receive blocks of the replicas other than the root (likewise)
  std::string gather_note;                    // why AUTO settled on peer copies, if it did
  // HSM_GATHER_DIRECT: one mailbox exchange per replica (pose_exchange.hip), re-made when the gathered row count changes (x_rows
  // = 0: at the next direct gather, whatever its row count)
  std::vector<hsm_exchange*> xpose, xcov;
  size_t x_rows = 0;
  bool shares_device = false;  // a device is listed more than once: the direct gather posts and waits in two rounds
  std::mutex mu;  // one group call at a time
};

#define NCCL_TRY(api, expr)                                                                     \
  do {                                                                                          \
    ncclResult_t r__ = (expr);                                                                  \
    if (r__ != ncclSuccess) {                                                                   \
      char b__[384];                                                                            \
      snprintf(b__, sizeof b__, "%s: %s", #expr, (api)->GetErrorString ? (api)->GetErrorString(r__) : "rccl error"); \
      return fail(HSM_ERR_HIP, b__);                                                            \
    }                                                                                           \
  } while (0)

// decide (once) how the group gathers: RCCL needs the library, distinct devices and a communicator per replica
static int group_ensure_gather(hsm_group* g) {
  if (g->gather_mode != HSM_GATHER_AUTO) return HSM_OK;
  const int R = (int)g->members.size();
  auto settle_peer = [&](const std::string& why) -> int {
    if (g->gather_pref == HSM_GATHER_RCCL) return fail(HSM_ERR_HIP, ("hsm_group: RCCL gather requested but unavailable: " + why).c_str());
    g->gather_note += why;
    g->gather_mode = HSM_GATHER_PEER;
    return HSM_OK;
  };
  if (g->gather_pref == HSM_GATHER_PEER) {
    g->gather_mode = HSM_GATHER_PEER;
    return HSM_OK;
  }
  std::vector<int> devs;
  for (hsm_ctx* h : g->members) devs.push_back(h->device);
  if (g->gather_pref == HSM_GATHER_AUTO || g->gather_pref == HSM_GATHER_DIRECT) {
    // the device-side exchange needs every replica's kernels to store into every other replica's HBM: the same device, or
    // peer access (xGMI on one node)
    std::string why;
    if (R > HSM_EXCHANGE_MAX_WORLD) why = "more replicas than HSM_EXCHANGE_MAX_WORLD";
    for (int a = 0; a < R && why.empty(); ++a)
      for (int b = 0; b < R && why.empty(); ++b) {
        if (devs[a] == devs[b]) continue;
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, devs[a], devs[b]) != hipSuccess || !can) {
          (void)hipGetLastError();
          why = "no peer access between devices " + std::to_string(devs[a]) + " and " + std::to_string(devs[b]);
        }
      }
    if (why.empty()) {
      g->gather_mode = HSM_GATHER_DIRECT;
      return HSM_OK;
    }
    if (g->gather_pref == HSM_GATHER_DIRECT) return fail(HSM_ERR_HIP, ("hsm_group: direct gather requested but unavailable: " + why).c_str());
    g->gather_note = "direct exchange unavailable (" + why + "); ";
  }
  for (int a = 0; a < R; ++a)
    for (int b = a + 1; b < R; ++b)
      if (devs[a] == devs[b]) return settle_peer("a device is listed more than once (one RCCL rank per device)");
  RcclApi* api = rccl_api();
  if (!api->lib) return settle_peer(api->error);
  g->comms.assign((size_t)R, nullptr);
  const ncclResult_t r = api->CommInitAll(g->comms.data(), R, devs.data());
  if (r != ncclSuccess) {
    g->comms.clear();
    return settle_peer(std::string("ncclCommInitAll: ") + api->GetErrorString(r));
  }
  g->gather_mode = HSM_GATHER_RCCL;
  return HSM_OK;
}

static void group_worker_main(GroupWorker* w) {
  std::unique_lock<std::mutex> lk(w->m);
  for (;;) {
    w->cv.wait(lk, [w] { return w->has_job || w->quit; });
    if (w->quit) return;
    std::function<int()> job = std::move(w->job);
    w->has_job = false;
    lk.unlock();
    const int rc = job();
    std::string err = rc != HSM_OK ? hsm_last_error() : "";  // thread-local text: carry it to the caller's thread
    lk.lock();
    w->rc = rc;
    w->err = std::move(err);
    w->done = true;
    w->cv.notify_all();
  }
}

// run fn(replica index) on every replica concurrently; first non-zero status wins
template <typename F>
static int group_parallel(hsm_group* g, F fn) {
  const int R = (int)g->members.size();
  for (int r = 1; r < R; ++r) {
    GroupWorker* w = g->workers[(size_t)r - 1].get();
    std::lock_guard<std::mutex> lk(w->m);
    w->job = [fn, r]() -> int { return fn(r); };
    w->has_job = true;
    w->done = false;
    w->cv.notify_all();
  }
  int rc0 = fn(0);
  int rc_out = rc0;
  std::string err_out = rc0 != HSM_OK ? std::string(hsm_last_error()) : std::string();
  for (int r = 1; r < R; ++r) {
    GroupWorker* w = g->workers[(size_t)r - 1].get();
    std::unique_lock<std::mutex> lk(w->m);
    w->cv.wait(lk, [w] { return w->done; });
    if (w->rc != HSM_OK && rc_out == HSM_OK) {
      rc_out = w->rc;
      err_out = w->err;
    }
  }
  return rc_out == HSM_OK ? HSM_OK : fail(rc_out, err_out.c_str());
}


extern "C" {

int hsm_group_create(float map_resolution, int size_x, int size_y, unsigned levels, float start_x, float start_y,
                     const int* devices, int n_devices, hsm_group** out) {
  if (!out || !devices || n_devices < 1) return fail(HSM_ERR_INVALID, "hsm_group_create: bad argument");
  *out = nullptr;
  hsm_group* g = new hsm_group();
  for (int i = 0; i < n_devices; ++i) {
    hsm_opts o;
    o.device = devices[i];
    o.layout = HSM_LAYOUT_AUTO;
    o.waves_per_scan = 0;
    hsm_ctx* h = nullptr;
    const int rc = hsm_create(map_resolution, size_x, size_y, levels, start_x, start_y, &o, &h);
    if (rc != HSM_OK) {
      hsm_group_destroy(g);
      return rc;
    }
    g->members.push_back(h);
  }
  for (int i = 1; i < n_devices; ++i) {
    g->workers.emplace_back(new GroupWorker());
    GroupWorker* w = g->workers.back().get();
    w->th = std::thread(group_worker_main, w);
  }
  for (std::vector<Buf<float>>* v : {&g->d_pose, &g->d_cov, &g->d_all_pose, &g->d_all_cov}) v->resize((size_t)n_devices);
  g->evt.assign((size_t)n_devices, nullptr);
  for (int a = 0; a < n_devices; ++a)
    for (int b = a + 1; b < n_devices; ++b) g->shares_device = g->shares_device || g->members[(size_t)a]->device == g->members[(size_t)b]->device;
  if (const char* env = getenv("HSM_GROUP_GATHER")) {
    if (strcmp(env, "rccl") == 0) g->gather_pref = HSM_GATHER_RCCL;
    else if (strcmp(env, "peer") == 0) g->gather_pref = HSM_GATHER_PEER;
    else if (strcmp(env, "direct") == 0) g->gather_pref = HSM_GATHER_DIRECT;
    else if (strcmp(env, "auto") != 0) {
      hsm_group_destroy(g);
      return fail(HSM_ERR_INVALID, "hsm_group_create: HSM_GROUP_GATHER must be one of auto, direct, rccl, peer");
    }
  }
  *out = g;
  return HSM_OK;
}

int hsm_group_set_gather(hsm_group* g, int mode) {
  if (!g) return fail(HSM_ERR_INVALID, "null group");
  if (mode != HSM_GATHER_AUTO && mode != HSM_GATHER_PEER && mode != HSM_GATHER_RCCL && mode != HSM_GATHER_DIRECT)
    return fail(HSM_ERR_INVALID, "hsm_group_set_gather: unknown mode");
  std::lock_guard<std::mutex> glk(g->mu);
  g->gather_pref = mode;
  g->gather_note.clear();
  if (mode == HSM_GATHER_PEER) {
    g->gather_mode = HSM_GATHER_PEER;
    return HSM_OK;
  }
  if (mode == HSM_GATHER_RCCL && !g->comms.empty()) {  // communicators, once made, are kept and reused
    g->gather_mode = HSM_GATHER_RCCL;
    return HSM_OK;
  }
  g->gather_mode = HSM_GATHER_AUTO;  // decide again
  return mode == HSM_GATHER_AUTO ? HSM_OK : group_ensure_gather(g);
}

int hsm_group_debug_force_p2p(hsm_group* g, int on) {
  if (!g) return fail(HSM_ERR_INVALID, "null group");
  std::lock_guard<std::mutex> glk(g->mu);
  g->force_p2p = on != 0;
  return HSM_OK;
}

int hsm_group_gather_mode(hsm_group* g) {
  if (!g) return HSM_GATHER_AUTO;
  std::lock_guard<std::mutex> glk(g->mu);
  if (group_ensure_gather(g) != HSM_OK) return HSM_GATHER_AUTO;
  return g->gather_mode;
}

const char* hsm_group_gather_note(const hsm_group* g) { return g ? g->gather_note.c_str() : ""; }

void hsm_group_destroy(hsm_group* g) {
  if (!g) return;
  for (auto& w : g->workers) {
    {
      std::lock_guard<std::mutex> lk(w->m);
      w->quit = true;
      w->cv.notify_all();
    }
    if (w->th.joinable()) w->th.join();
  }
  if (!g->comms.empty()) {
    for (hsm_ctx* h : g->members) (void)hsm_synchronize(h);
    RcclApi* api = rccl_api();
    for (ncclComm_t c : g->comms)
      if (c && api->CommDestroy) (void)api->CommDestroy(c);
  }
  if (!g->xpose.empty() || !g->xcov.empty()) {
    for (hsm_ctx* h : g->members) (void)hsm_synchronize(h);
    for (hsm_exchange* x : g->xpose) hsm_exchange_destroy(x);
    for (hsm_exchange* x : g->xcov) hsm_exchange_destroy(x);
  }
  TeardownLog log_, *log = &log_;  // (as hsm_destroy: name the first failing call, leave no error behind for the next caller)
  for (size_t r = 0; r < g->members.size(); ++r) {
    if (g->members[r]) TEARDOWN(log, hipSetDevice(g->members[r]->device));
    for (std::vector<Buf<float>>* v : {&g->d_pose, &g->d_cov, &g->d_all_pose, &g->d_all_cov})
      if (r < v->size()) (*v)[r].release(log);
    if (r < g->evt.size() && g->evt[r]) TEARDOWN(log, hipEventDestroy(g->evt[r]));
  }
  for (hsm_ctx* h : g->members) hsm_destroy(h);
  delete g;
  if (!log_.first.empty()) {
    set_error_text(("hsm_group_destroy: " + log_.first).c_str());
    (void)hipGetLastError();
  }
}

int hsm_group_size(const hsm_group* g) { return g ? (int)g->members.size() : 0; }

hsm_ctx* hsm_group_member(hsm_group* g, int i) {
  return (g && i >= 0 && i < (int)g->members.size()) ? g->members[i] : nullptr;
}

int hsm_group_set_update_factors(hsm_group* g, float free_factor, float occupied_factor) {
  if (!g) return fail(HSM_ERR_INVALID, "null group");
  for (hsm_ctx* h : g->members) {
    if (int rc = hsm_set_update_factor_free(h, free_factor)) return rc;
    if (int rc = hsm_set_update_factor_occupied(h, occupied_factor)) return rc;
  }
  return HSM_OK;
}

int hsm_group_process_scan(hsm_group* g, const float hint_world[3], const float* pts_xy, int n, const float origo[2],
                           int do_update, float out_pose_world[3], float cov[9]) {
  if (!g || g->members.empty()) return fail(HSM_ERR_INVALID, "null group");
  std::lock_guard<std::mutex> glk(g->mu);
  if (int rc = hsm_match(g->members[0], hint_world, pts_xy, n, origo, out_pose_world, cov)) return rc;
  if (!do_update) return HSM_OK;
  return group_parallel(g, [&](int r) -> int {
    hsm_ctx* h = g->members[r];
    if (r != 0)
      if (int rc = hsm_retain_scan(h, pts_xy, n, origo)) return rc;
    return hsm_update_by_scan(h, out_pose_world, pts_xy, n, origo);
  });
}

int hsm_group_match_batch_device(hsm_group* g, const int* counts, const float* const* d_begin_world,
                                 const float* const* d_pts_xy, const int* const* d_scan_offsets, int shared_n, int root,
                                 float* d_out_pose_all, float* d_out_cov_all) {
  if (!g || g->members.empty()) return fail(HSM_ERR_INVALID, "null group");
  const int R = (int)g->members.size();
  if (!counts || !d_begin_world || !d_pts_xy || !d_out_pose_all || root < 0 || root >= R)
    return fail(HSM_ERR_INVALID, "hsm_group_match_batch_device: bad argument");
  std::lock_guard<std::mutex> glk(g->mu);
  std::vector<size_t> first((size_t)R + 1, 0);
  for (int r = 0; r < R; ++r) {
    if (counts[r] < 0 || (counts[r] > 0 && (!d_begin_world[r] || !d_pts_xy[r])))
      return fail(HSM_ERR_INVALID, "hsm_group_match_batch_device: bad shard");
    first[(size_t)r + 1] = first[(size_t)r] + (size_t)counts[r];
  }
  const int root_dev = g->members[(size_t)root]->device;
  if (int rc = group_ensure_gather(g)) return rc;
  const bool rccl = g->gather_mode == HSM_GATHER_RCCL;
  const bool direct = g->gather_mode == HSM_GATHER_DIRECT;
  const size_t total = first[(size_t)R];
  if (direct && total > 0) {
    // Device-side exchange: one mailbox per replica for [total, 3] (+ one for [total, 9]), made when the gathered row count
    // changes (a particle filter keeps its particle count; anything else pays a re-allocation here)
    const bool want_cov = d_out_cov_all != nullptr;
    if (g->x_rows != total || g->xpose.empty() || (want_cov && g->xcov.empty())) {
      for (hsm_ctx* h : g->members)
        if (int rc0 = hsm_synchronize(h)) return rc0;
      const bool remake_pose = g->x_rows != total || g->xpose.empty();
      auto make = [&](std::vector<hsm_exchange*>& xs, int cols) -> int {
        for (hsm_exchange* x : xs) hsm_exchange_destroy(x);
        xs.assign((size_t)R, nullptr);
        for (int r = 0; r < R; ++r)
          if (int rc0 = hsm_exchange_create(g->members[(size_t)r]->device, r, R, (int)total, cols, 2, &xs[(size_t)r])) return rc0;
        for (int r = 0; r < R; ++r)
          if (int rc0 = hsm_exchange_connect_local(xs[(size_t)r], xs.data())) return rc0;
        return HSM_OK;
      };
      if (remake_pose) {
        if (int rc0 = make(g->xpose, 3)) return rc0;
        for (hsm_exchange* x : g->xcov) hsm_exchange_destroy(x);  // (shaped for the old row count)
        g->xcov.clear();
      }
      if (want_cov && g->xcov.empty())
        if (int rc0 = make(g->xcov, 9)) return rc0;
      g->x_rows = total;
    }
  }
  // Replicas that share a device may share a hardware queue (a process has a few, and more streams than that): a wait kernel
  // that polls for rows a later launch in the same queue has yet to post stalls until its timeout.  Such a group posts in one
  // round and waits in a second one, every wait behind the events of the posts made on its own device -- it polls only for
  // rows that other devices store.  A group of distinct devices keeps the one launch per replica.
  const bool split = direct && g->shares_device;
  bool equal = counts[0] > 0;  // ncclAllGather wants the same count from every rank
  for (int r = 1; r < R; ++r) equal = equal && counts[r] == counts[0];
  const bool self_send = rccl && g->force_p2p;  // test hook: the send / receive form for every shard, the root's own included
  if (self_send) equal = false;
  // every replica: match its shard on its own stream.  Peer gather: push the poses (and H) to the root's device with a peer
  // copy on the same stream -- 12 (+36) bytes per scan over xGMI, no host staging, no host wait.  RCCL gather: the
  // collective is queued below, behind the match, on the same streams.
  int rc = group_parallel(g, [&](int r) -> int {
    hsm_ctx* h = g->members[(size_t)r];
    const size_t n = (size_t)counts[r];
    std::lock_guard<std::mutex> lk(h->mu);
    if (int rc2 = select_device(h)) return rc2;
    if (!g->evt[(size_t)r]) HIP_TRY(hipEventCreateWithFlags(&g->evt[(size_t)r], hipEventDisableTiming));
    // a pair of result blocks for `rows` scans: the covariance block goes first and comes back last
    auto reserve_pair = [](Buf<float>& pose, Buf<float>& cov, size_t rows) -> int {
      if (cov.holds(rows * 9)) return HSM_OK;
      if (int rc2 = cov.drop()) return rc2;
      if (int rc2 = pose.replace(rows * 3 * sizeof(float))) return rc2;
      return cov.reserve(rows * 9);
    };
    if (((rccl && equal) || direct) && r != root)  // all-gather receive blocks of a non-root replica
      if (int rc2 = reserve_pair(g->d_all_pose[(size_t)r], g->d_all_cov[(size_t)r], total)) return rc2;
    if (n > 0) {
      if (int rc2 = reserve_pair(g->d_pose[(size_t)r], g->d_cov[(size_t)r], n)) return rc2;
      // the Hessians are in/out: a scan without beams leaves its row as the caller gave it (ScanMatcher.h:68,189), so the
      // shard's block starts from the caller's rows -- not from what an earlier call, or nobody, left in it
      if (d_out_cov_all)
        HIP_TRY(hipMemcpyPeerAsync(g->d_cov[(size_t)r], h->device, d_out_cov_all + 9 * first[(size_t)r], root_dev, n * 9 * sizeof(float),
                                   h->stream));
      const ScanBatch shard{(int)n, d_begin_world[r], d_pts_xy[r], d_scan_offsets ? d_scan_offsets[r] : nullptr, shared_n};
      if (int rc2 = match_batch_device_nolock(h, shard, {g->d_pose[(size_t)r], d_out_cov_all ? g->d_cov[(size_t)r] : nullptr}, h->stream))
        return rc2;
      if (direct) {
        // (below, also for a replica without scans: every replica posts every epoch)
      } else if (!rccl || (r == root && !equal && !self_send)) {  // (RCCL send/recv gather: the root's own shard is a local copy)
        HIP_TRY(hipMemcpyPeerAsync(d_out_pose_all + 3 * first[(size_t)r], root_dev, g->d_pose[(size_t)r], h->device,
                                   n * 3 * sizeof(float), h->stream));
        if (d_out_cov_all)
          HIP_TRY(hipMemcpyPeerAsync(d_out_cov_all + 9 * first[(size_t)r], root_dev, g->d_cov[(size_t)r], h->device,
                                     n * 9 * sizeof(float), h->stream));
      }
    }
    if (direct && total > 0) {
      if (split) {
        // post only; the waits follow in a round of their own, behind this event
        if (int rc2 = hsm_exchange_post(g->xpose[(size_t)r], g->d_pose[(size_t)r], (int)first[(size_t)r], (int)n, h->stream)) return rc2;
        if (d_out_cov_all)
          if (int rc2 = hsm_exchange_post(g->xcov[(size_t)r], g->d_cov[(size_t)r], (int)first[(size_t)r], (int)n, h->stream)) return rc2;
        HIP_TRY(hipEventRecord(g->evt[(size_t)r], h->stream));
        return HSM_OK;
      }
      // ONE launch on this replica's stream, behind its match: store the shard's rows into every replica's mailbox and
      // unpack all shards' rows as they arrive -- the root into the caller's arrays, the others into blocks the group
      // keeps (every replica holds all poses afterwards: hsm_group_gathered).  No collective, no event, no host wait.
      if (int rc2 = hsm_exchange_post_wait(g->xpose[(size_t)r], g->d_pose[(size_t)r], (int)first[(size_t)r], (int)n, 0,
                                           r == root ? d_out_pose_all : g->d_all_pose[(size_t)r], h->stream))
        return rc2;
      if (d_out_cov_all)
        if (int rc2 = hsm_exchange_post_wait(g->xcov[(size_t)r], g->d_cov[(size_t)r], (int)first[(size_t)r], (int)n, 0,
                                             r == root ? d_out_cov_all : g->d_all_cov[(size_t)r], h->stream))
          return rc2;
      return HSM_OK;
    }
    if (!rccl) HIP_TRY(hipEventRecord(g->evt[(size_t)r], h->stream));
    return HSM_OK;
  });
  if (rc == HSM_OK && direct && split && total > 0) {
    // the second round: every post of this epoch has been queued and its event recorded.  Each replica's stream waits for the
    // posts made on its own device, then ONE launch unpacks all shards' rows -- the root into the caller's arrays, the others
    // into blocks the group keeps -- polling only for the rows that replicas on other devices store
    rc = group_parallel(g, [&](int r) -> int {
      hsm_ctx* h = g->members[(size_t)r];
      std::lock_guard<std::mutex> lk(h->mu);
      if (int rc2 = select_device(h)) return rc2;
      for (int p = 0; p < R; ++p)
        if (p != r && g->members[(size_t)p]->device == h->device) HIP_TRY(hipStreamWaitEvent(h->stream, g->evt[(size_t)p], 0));
      if (int rc2 = hsm_exchange_wait(g->xpose[(size_t)r], r == root ? d_out_pose_all : g->d_all_pose[(size_t)r], h->stream)) return rc2;
      if (d_out_cov_all)
        if (int rc2 = hsm_exchange_wait(g->xcov[(size_t)r], r == root ? d_out_cov_all : g->d_all_cov[(size_t)r], h->stream)) return rc2;
      return HSM_OK;
    });
  }
  if (rc != HSM_OK) {
    if (direct) g->x_rows = 0;  // (the replicas' epochs may have parted: the next direct gather makes its exchanges anew)
    return rc;
  }
  if (direct) return HSM_OK;
  if (rccl) {
    // ONE grouped collective over the group's communicators, each rank's part on its replica's stream (behind its match):
    // equal shards -> ncclAllGather of [B/G, 3] (+ [B/G, 9]); the root receives straight into the caller's arrays, the
    // other replicas into blocks the group keeps (every replica then holds all poses: hsm_group_gathered).  Unequal
    // shards -> the same gather as grouped ncclSend / ncclRecv to the root.  The collective itself orders the root's
    // stream behind every shard.
    RcclApi* api = rccl_api();
    NCCL_TRY(api, api->GroupStart());
    ncclResult_t nr = ncclSuccess;
    for (int r = 0; r < R && nr == ncclSuccess; ++r) {
      hsm_ctx* h = g->members[(size_t)r];
      const size_t n = (size_t)counts[r];
      if (equal) {
        nr = api->AllGather(g->d_pose[(size_t)r], r == root ? d_out_pose_all : g->d_all_pose[(size_t)r], n * 3, ncclFloat,
                            g->comms[(size_t)r], h->stream);
        if (nr == ncclSuccess && d_out_cov_all)
          nr = api->AllGather(g->d_cov[(size_t)r], r == root ? d_out_cov_all : g->d_all_cov[(size_t)r], n * 9, ncclFloat,
                              g->comms[(size_t)r], h->stream);
      } else if ((r != root || self_send) && n > 0) {
        hsm_ctx* hr = g->members[(size_t)root];
        nr = api->Send(g->d_pose[(size_t)r], n * 3, ncclFloat, root, g->comms[(size_t)r], h->stream);
        if (nr == ncclSuccess)
          nr = api->Recv(d_out_pose_all + 3 * first[(size_t)r], n * 3, ncclFloat, r, g->comms[(size_t)root], hr->stream);
        if (nr == ncclSuccess && d_out_cov_all) {
          nr = api->Send(g->d_cov[(size_t)r], n * 9, ncclFloat, root, g->comms[(size_t)r], h->stream);
          if (nr == ncclSuccess)
            nr = api->Recv(d_out_cov_all + 9 * first[(size_t)r], n * 9, ncclFloat, r, g->comms[(size_t)root], hr->stream);
        }
      }
    }
    const ncclResult_t ne = api->GroupEnd();
    if (nr != ncclSuccess) NCCL_TRY(api, nr);
    NCCL_TRY(api, ne);
    return HSM_OK;
  }
  // the root's stream waits for every shard: work queued on it afterwards (and hsm_synchronize on the root member) sees
  // the complete gather
  hsm_ctx* hr = g->members[(size_t)root];
  std::lock_guard<std::mutex> lk(hr->mu);
  if (int rc2 = select_device(hr)) return rc2;
  for (int r = 0; r < R; ++r)
    if (r != root) HIP_TRY(hipStreamWaitEvent(hr->stream, g->evt[(size_t)r], 0));
  return HSM_OK;
}

const float* hsm_group_gathered(hsm_group* g, int replica, int want_cov) {
  if (!g || replica < 0 || replica >= (int)g->d_all_pose.size()) return nullptr;
  return want_cov ? g->d_all_cov[(size_t)replica] : g->d_all_pose[(size_t)replica];
}

// Replicas drift apart once one of them integrates scans through an entry the group does not replay (the device-resident
// writers): replica `from`'s pyramid, or one cell box per level of it, into every other replica (map_copy.hip), each copy queued
// by its replica's thread.
int hsm_group_sync_maps(hsm_group* g, int from, const int* boxes) {
  if (!g || g->members.empty()) return fail(HSM_ERR_INVALID, "null group");
  const int R = (int)g->members.size();
  if (from < 0 || from >= R) return fail(HSM_ERR_INVALID, "hsm_group_sync_maps: `from` is no replica of the group");
  std::lock_guard<std::mutex> glk(g->mu);
  hsm_ctx* src = g->members[(size_t)from];
  return group_parallel(g, [&](int r) -> int {
    if (r == from) return HSM_OK;
    return boxes ? hsm_copy_map_boxes(g->members[(size_t)r], src, boxes) : hsm_copy_map(g->members[(size_t)r], src);
  });
}

int hsm_group_synchronize(hsm_group* g) {
  if (!g) return fail(HSM_ERR_INVALID, "null group");
  for (hsm_ctx* h : g->members)
    if (int rc = hsm_synchronize(h)) return rc;
  for (hsm_exchange* x : g->xpose)  // a gather whose rows did not all arrive says so here
    if (int rc = hsm_exchange_status(x)) return rc;
  for (hsm_exchange* x : g->xcov)
    if (int rc = hsm_exchange_status(x)) return rc;
  return HSM_OK;
}

// THE partitioning of a batch over G replicas (contiguous shards): the first total % world shards hold one
// scan more.  One rule for both transports -- hsm_group_* (one process, a worker thread per device) and
// hector_slam_amd/sharding.py (one process per device under torch.distributed, which calls this function).
int hsm_shard_bounds(int total, int rank, int world, int* begin, int* end) {
  if (total < 0 || world <= 0 || rank < 0 || rank >= world || !begin || !end) return fail(HSM_ERR_INVALID, "hsm_shard_bounds: bad argument");
  const int base = total / world, rem = total % world;
  *begin = rank * base + (rank < rem ? rank : rem);
  *end = *begin + base + (rank < rem ? 1 : 0);
  return HSM_OK;
}

int hsm_group_match_batch(hsm_group* g, int batch, const float* begin_world, const float* pts_xy,
                          const int* scan_offsets, int shared_n, float* out_pose, float* out_cov) {
  if (!g || g->members.empty()) return fail(HSM_ERR_INVALID, "null group");
  if (batch < 0 || !begin_world || !out_pose) return fail(HSM_ERR_INVALID, "hsm_group_match_batch: bad argument");
  const int R = (int)g->members.size();
  std::lock_guard<std::mutex> glk(g->mu);
  return group_parallel(g, [&](int r) -> int {
    int b = 0, e = 0;
    if (int rc = hsm_shard_bounds(batch, r, R, &b, &e)) return rc;
    if (e == b) return HSM_OK;
    if (!scan_offsets)  // pose hypotheses of ONE shared scan
      return hsm_match_batch(g->members[r], e - b, begin_world + 3 * (size_t)b, pts_xy, nullptr, shared_n,
                             out_pose + 3 * (size_t)b, out_cov ? out_cov + 9 * (size_t)b : nullptr);
    std::vector<int> offs((size_t)(e - b) + 1);  // CSR offsets rebased to the shard
    for (int i = b; i <= e; ++i) offs[(size_t)(i - b)] = scan_offsets[i] - scan_offsets[b];
    return hsm_match_batch(g->members[r], e - b, begin_world + 3 * (size_t)b, pts_xy + 2 * (size_t)scan_offsets[b],
                           offs.data(), 0, out_pose + 3 * (size_t)b, out_cov ? out_cov + 9 * (size_t)b : nullptr);
  });
}

}  // extern "C"
