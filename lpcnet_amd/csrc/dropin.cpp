/*
 * dropin.cpp -- the drop-in single-stream API of include/lpcnet.h and the
 * lpcnet_mi355x_* handle and pool entry points over the batch engine
 * (engine.cpp and synth_steps.cpp, through batch.h): the handle registry and
 * placement, the StatePool of every (model, placement) with its slots and
 * work batch, and
 * the 1.6 kb/s decoder handle.  Concurrent calls coalesce into one launch
 * through the pool's flat combiner (pool_combiner.cpp, host-only), which
 * calls pool_run here.
 * Compile with -ffp-contract=off, as every translation unit.
 */
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "batch.h"
#include "pool_combiner.h"

extern "C" {

/* ======================================================================== */
/* drop-in single-stream API (include/lpcnet.h)                              */

static int pool_launch(void *pool, const std::vector<Req *> &rq, std::string &err);

/* The drop-in handles share the GPU.  Every LPCNetState bound to the same
 * model (blob bytes, resolved model constants) on the same device is a slot
 * of one StatePool: one device copy of the model, the slots' stream states
 * in one device array, and one work batch.  Concurrent calls on different
 * handles coalesce into one launch (flat combining: the first caller to find
 * the pool idle runs every request pending at that moment that has the same
 * shape -- the slots' states are gathered into the work batch, one step
 * runs, the states are scattered back), so K reference-style callers on K
 * threads get batch-K launches instead of K batch-1 engines.  Each handle's
 * results are those of its own stream alone (streams of a batch are
 * independent), i.e. the reference's. */
struct StatePool {
  /* what a request runs on its slot */
  enum Kind {
    SYNTH = 0, /* lpcnet_synthesize_impl (lpcnet.c:273-277): frame + N samples, `preload` teacher-forced */
    TAIL = 1,  /* lpcnet_synthesize_tail_impl (lpcnet.c:235-271): samples only */
    FLUSH = 2, /* run_frame_network_flush (lpcnet.c:134-144): nfr frames, conditioning discarded */
    DECODE = 3 /* lpcnet_decode (lpcnet.c:310-319): one 8-byte packet -> 4 frames */
  };
  /* the work batch (its HIP stream) and its staging, driven by the combiner */
  struct Lane {
    LPCNetBatch *work = nullptr; /* work->B >= the largest coalesced call */
    DevPtr<int> d_map;           /* [map_cap] work-batch stream -> slot */
    int map_cap = 0;
    /* pinned host staging of a launch ([map_cap] entries each), so the
     * copies are truly asynchronous: slot map, features, PCM */
    PinnedPtr<int> h_map;
    PinnedPtr<float> h_feat;
    PinnedPtr<short> h_pcm;
  };
  uint64_t key = 0;
  int device = 0;
  int place = 0; /* placement index (g_pools key) */
  std::vector<unsigned char> blob;
  bool has_codebooks = false;
  Lane lane;
  DevPtr<StreamState> d_slots;
  int cap = 0;
  std::vector<int> free_slots;
  int refs = 0; /* handles bound + transient acquisitions; changed under g_pools_mu only */
  std::mutex mu; /* slot bookkeeping (taken with the pool idle: PoolIdle) */
  /* submission, coalescing and wake-ups; its launch is pool_run on this pool */
  PoolCombiner comb{pool_launch, this};
};

static std::mutex g_pools_mu;
/* (model key, placement) -> pool: one pool per model per placement, so
 * handles spread over devices (and, for tests, over several placements of
 * one device) never share a launch across placements */
static std::map<std::pair<uint64_t, int>, StatePool *> g_pools;

/* Gather window of a combiner: before its launch it waits up to this long
 * (plus 2 us per caller expected) until as many requests have arrived as the
 * previous launch carried (a thread calling lpcnet_synthesize in a loop is
 * back within microseconds), so K looping callers keep launching together
 * instead of settling into half-size launches that alternate.  Callers that
 * stopped cost one window once: the next launch expects only those that
 * came. */
#ifndef POOL_WINDOW_US_DEFAULT
#define POOL_WINDOW_US_DEFAULT 200
#endif


static uint64_t pool_key(const unsigned char *data, int len)
{
  uint64_t h = 1469598103934665603ull;
  auto mix = [&](const void *p, size_t n) {
    for (size_t k = 0; k < n; k++) h = (h ^ ((const unsigned char *)p)[k]) * 1099511628211ull;
  };
  mix(data, (size_t)len);
  mix(&len, sizeof(len));
  /* load-time overrides change the model bound to the same bytes */
  for (const char *e : {"LPCNET_LPC_GAMMA", "LPCNET_FEATURES_DELAY", "LPCNET_END2END", "LPCNET_KERNEL", "LPCNET_RCP"}) {
    const char *v = getenv(e);
    mix(e, strlen(e));
    if (v) mix(v, strlen(v));
  }
  return h;
}

/* the pool of (blob, placement), created with its model on first use; refs+1 */
static StatePool *pool_acquire(const unsigned char *data, int len, int device, int place)
{
  if (!data || len <= 0) { set_err("lpcnet_load_model: empty blob"); return nullptr; }
  const uint64_t key = pool_key(data, len);
  std::lock_guard<std::mutex> lk(g_pools_mu);
  auto it = g_pools.find({key, place});
  if (it != g_pools.end() && it->second->blob.size() == (size_t)len && !memcmp(it->second->blob.data(), data, len)) {
    it->second->refs++;
    return it->second;
  }
  if (it != g_pools.end()) {
    /* a different blob with the same 64-bit key: refuse rather than mix models */
    set_err("lpcnet_load_model: model pool key collision between two different blobs");
    return nullptr;
  }
  LPCNetBatch *w = lpcnet_batch_create(1, device);
  if (!w) return nullptr;
  if (lpcnet_batch_load_model(w, data, len)) {
    const std::string e = last_err();
    lpcnet_batch_destroy(w);
    set_err(e);
    return nullptr;
  }
  StatePool *p = new StatePool();
  p->key = key;
  p->device = device;
  p->place = place;
  p->blob.assign(data, data + len);
  p->has_codebooks = w->has_codebooks;
  p->lane.work = w;
  p->refs = 1;
  if (const char *v = getenv("LPCNET_POOL_BROADCAST")) p->comb.broadcast = atoi(v) != 0;
  if (const char *v = getenv("LPCNET_POOL_WINDOW_US")) p->comb.window_us = std::max(0, atoi(v));
  else p->comb.window_us = POOL_WINDOW_US_DEFAULT;
  g_pools[{key, place}] = p;
  return p;
}

/* give back `slot` (if >= 0) and one reference; the last reference frees
 * the pool.  refs changes under g_pools_mu only, the lock pool_acquire holds
 * while it looks the pool up, so an acquisition and the last release can
 * never both succeed. */
static void pool_release(StatePool *p, int slot)
{
  if (slot >= 0) {
    std::unique_lock<std::mutex> lk(p->mu);
    PoolIdle idle(&p->comb, lk);
    p->free_slots.push_back(slot);
  }
  {
    std::lock_guard<std::mutex> lk(g_pools_mu);
    if (--p->refs > 0) return;
    g_pools.erase({p->key, p->place});
  }
  /* unreachable now: no handle holds it and the map no longer lists it;
   * its owners free the slots and the lane's staging on the pool's device */
  (void)hipSetDevice(p->device);
  if (p->lane.work) lpcnet_batch_destroy(p->lane.work);
  delete p;
}

/* a free slot holding `init` (a reset state when null); -1 on failure */
static int pool_alloc_slot(StatePool *p, const StreamState *init)
{
  std::unique_lock<std::mutex> lk(p->mu);
  PoolIdle idle(&p->comb, lk);
  if (hipSetDevice(p->device) != hipSuccess) { set_err("hipSetDevice failed"); return -1; }
  if (p->free_slots.empty()) {
    const int ncap = std::max(4, 2 * p->cap);
    DevPtr<StreamState> d;
    if (d.alloc((size_t)ncap)) { set_err("device allocation failed"); return -1; }
    if (p->cap && hipMemcpy(d, p->d_slots, sizeof(StreamState) * (size_t)p->cap, hipMemcpyDeviceToDevice) != hipSuccess) {
      set_err("device copy failed");
      return -1;
    }
    p->d_slots.swap(d); /* the previous slots go with d */
    for (int k = ncap - 1; k >= p->cap; k--) p->free_slots.push_back(k);
    p->cap = ncap;
  }
  const int slot = p->free_slots.back();
  StreamState s;
  if (init) s = *init;
  else host_reset_state(s);
  if (hipMemcpy(&p->d_slots[slot], &s, sizeof(s), hipMemcpyHostToDevice) != hipSuccess) { set_err("device copy failed"); return -1; }
  p->free_slots.pop_back();
  return slot;
}

static int pool_slot_io(StatePool *p, int slot, StreamState *get, const StreamState *put)
{
  std::unique_lock<std::mutex> lk(p->mu);
  PoolIdle idle(&p->comb, lk);
  if (hipSetDevice(p->device) != hipSuccess) { set_err("hipSetDevice failed"); return -1; }
  if (get && hipMemcpy(get, &p->d_slots[slot], sizeof(*get), hipMemcpyDeviceToHost) != hipSuccess) {
    set_err("device copy failed");
    return -1;
  }
  if (put && hipMemcpy(&p->d_slots[slot], put, sizeof(*put), hipMemcpyHostToDevice) != hipSuccess) {
    set_err("device copy failed");
    return -1;
  }
  return 0;
}

/* one coalesced step for requests rq (all of the same shape); the combiner
 * alone touches L */
static int pool_run(StatePool *p, StatePool::Lane &L, const std::vector<Req *> &rq)
{
  const int n = (int)rq.size();
  const Req &r0 = *rq[0];
  const int N = r0.N;
  if (!L.work || L.work->B < n) {
    int nb = 1;
    while (nb < n) nb *= 2;
    LPCNetBatch *w = lpcnet_batch_create(nb, p->device);
    if (!w) return -1;
    if (lpcnet_batch_load_model(w, p->blob.data(), (int)p->blob.size())) {
      lpcnet_batch_destroy(w);
      return -1;
    }
    if (L.work) lpcnet_batch_destroy(L.work);
    L.work = w;
  }
  LPCNetBatch *w = L.work;
  if (w->set_device()) return -1;
  if (L.map_cap < n) {
    L.d_map.reset();
    L.h_map.reset();
    L.h_feat.reset();
    L.h_pcm.reset();
    L.map_cap = 0;
    const size_t nw = (size_t)w->B;
    if (L.d_map.alloc(nw) || L.h_map.alloc(nw, false) || L.h_feat.alloc(NF * nw, false) || L.h_pcm.alloc(4 * FRAME * nw, false)) return -1;
    L.map_cap = w->B;
  }
  float *feat = L.h_feat;
  short *pcm = L.h_pcm;
  const int nout = r0.kind == StatePool::DECODE ? 4 * FRAME : N;
  /* a synthesis step's inputs go first, so the copy engine's work precedes
   * every kernel of the launch (one copy -> kernel hand-over instead of two) */
  const bool staged = r0.kind == StatePool::SYNTH;
  /* each request's features and preload into the staging (SYNTH / TAIL) */
  const auto stage = [&]() {
    for (int k = 0; k < n; k++) {
      if (r0.kind == StatePool::SYNTH) memcpy(&feat[(size_t)k * NF], rq[k]->feat, sizeof(float) * NF);
      if (r0.preload > 0) memcpy(&pcm[(size_t)k * N], rq[k]->out, sizeof(short) * std::min(r0.preload, N));
    }
  };
  if (staged) {
    stage();
    HIPCHK(hipMemcpyAsync(w->d_feat, feat, sizeof(float) * NF * n, hipMemcpyHostToDevice, w->stream));
    if (r0.preload > 0 && N > 0)
      HIPCHK(hipMemcpyAsync(w->d_pcm, pcm, sizeof(short) * N * n, hipMemcpyHostToDevice, w->stream));
  }
  for (int k = 0; k < n; k++) L.h_map[k] = rq[k]->slot;
  HIPCHK(hipMemcpyAsync(L.d_map, L.h_map, sizeof(int) * n, hipMemcpyHostToDevice, w->stream));
  if (launch_state_copy(w->d_state, p->d_slots, nullptr, L.d_map, n, w->stream)) { set_err("state gather failed"); return -1; }
  /* every stream of the work batch is this call's: the multi-frame bound is its min */
  w->min_fc = 0;
  /* the states go back to their slots right behind the step's kernels, before
   * its one synchronisation */
  const PreSync scatter = [&]() -> int {
    if (launch_state_copy(p->d_slots, w->d_state, L.d_map, nullptr, n, w->stream)) {
      set_err("state scatter failed");
      return -1;
    }
    return 0;
  };
  int rc = 0;
  switch (r0.kind) {
  case StatePool::SYNTH:
  case StatePool::TAIL:
    if (!staged) stage();
    rc = r0.kind == StatePool::SYNTH ? synth_first(w, n, feat, pcm, N, r0.preload, scatter, staged)
                                     : tail_first(w, n, pcm, N, r0.preload, scatter);
    break;
  case StatePool::FLUSH:
    for (int j = 0; j < r0.nfr && rc == 0; j++) {
      for (int k = 0; k < n; k++) memcpy(&feat[(size_t)k * NF], rq[k]->feat + (size_t)j * NF, sizeof(float) * NF);
      rc = frame_first(w, n, feat, true, j + 1 == r0.nfr ? scatter : PreSync());
    }
    break;
  case StatePool::DECODE: {
    std::vector<unsigned char> pk((size_t)n * 8);
    for (int k = 0; k < n; k++) memcpy(&pk[(size_t)k * 8], rq[k]->packet, 8);
    rc = decode_first(w, n, pk.data(), pcm, scatter);
    break;
  }
  default:
    set_err("bad request");
    rc = -1;
  }
  if (rc == 0)
    for (int k = 0; k < n; k++)
      if (nout > 0 && r0.kind != StatePool::FLUSH) memcpy(rq[k]->out, &pcm[(size_t)k * nout], sizeof(short) * nout);
  return rc;
}

/* the combiner's launch: pool_run, its error taken on the combiner's thread */
static int pool_launch(void *pool, const std::vector<Req *> &rq, std::string &err)
{
  StatePool *p = (StatePool *)pool;
  const int rc = pool_run(p, p->lane, rq);
  if (rc) err = last_err();
  return rc;
}

/* ---- handles -------------------------------------------------------------
 * An LPCNetState is caller memory (lpcnet_get_size + malloc, calloc through
 * lpcnet_create, or embedded in a larger struct as the reference's decoder
 * and PLC states embed theirs).  It holds a magic word and a 64-bit token;
 * everything else -- device, bound pool and slot, the deferred feature
 * buffer -- lives in a Handle found through the registry, so nothing read
 * from caller memory is ever dereferenced.  A registry entry whose token
 * does not match the memory at its address is stale (the memory was freed
 * without lpcnet_destroy / lpcnet_mi355x_deinit and reused): lpcnet_init
 * there drops it, releasing its slot, and starts a fresh handle. */
struct LPCNetState {
  uint32_t magic;
  uint32_t reserved;
  uint64_t token;
};
static const uint32_t kMagic = 0x4c50434eu; /* "LPCN" */

constexpr int MAX_FEATURE_BUFFER = 4; /* lpcnet_private.h:26 MAX_FEATURE_BUFFER_SIZE */

struct Handle {
  uint64_t token = 0;
  int device = 0;
  int place = 0;     /* placement index: auto placements 0.., LPCNET_DEVICE pins kPinned + device */
  unsigned place_gen = 0; /* generation of the placement list it was counted in */
  StatePool *pool = nullptr; /* bound model (nullptr: none) */
  int slot = -1;
  /* run_frame_network_deferred's buffer (lpcnet_private.h:37-38, lpcnet.c:122-132) */
  int fbuf_fill = 0;
  float fbuf[MAX_FEATURE_BUFFER][NF] = {};
};

/* A handle's complete synthesis state: lpcnet_mi355x_state_save/restore, the
 * replacement of the LPCNetState struct copies of lpcnet_plc.c:223,230. */
struct HandleSnapshot {
  StreamState s;
  int fbuf_fill;
  float fbuf[MAX_FEATURE_BUFFER][NF];
};

static_assert(sizeof(HandleSnapshot) <= LPCNET_MI355X_STATE_MAX, "LPCNET_MI355X_STATE_MAX too small");

/* the registry, sharded by address: every lpcnet_synthesize looks its
 * handle up, and one lock would serialise hundreds of calling threads */
struct LiveShard {
  std::mutex mu;
  std::unordered_map<const LPCNetState *, Handle *> map;
};
static LiveShard g_live[64];
static LiveShard &live_shard(const LPCNetState *st)
{
  const uint64_t a = (uint64_t)(uintptr_t)st;
  return g_live[((a >> 4) ^ (a >> 10) ^ (a >> 16)) & 63];
}

static uint64_t new_token()
{
  static std::atomic<uint64_t> ctr{0};
  static const uint64_t salt = (uint64_t)(uintptr_t)&ctr ^ ((uint64_t)time(nullptr) << 20);
  uint64_t z = (ctr.fetch_add(1) + 1) * 0x9E3779B97F4A7C15ull ^ salt; /* splitmix64 */
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z ? z : 1;
}

/* the live handle at st, or nullptr */
static Handle *live_handle(const LPCNetState *st)
{
  if (!st) return nullptr;
  LiveShard &sh = live_shard(st);
  std::lock_guard<std::mutex> lk(sh.mu);
  auto it = sh.map.find(st);
  if (it == sh.map.end() || st->magic != kMagic || st->token != it->second->token) return nullptr;
  return it->second;
}

/* ---- placement of drop-in handles over the visible GPUs ------------------
 * The reference's lpcnet_init/lpcnet_create take no device (lpcnet.c:184-219),
 * so placement is library policy.  By default every handle goes to one
 * device: LOCAL_RANK mod the device count in a one-process-per-GPU job
 * (torchrun ranks), device 0 otherwise -- resolved when a model is first
 * bound, so lpcnet_init/lpcnet_create never start the HIP runtime.
 * Spreading is opt-in: LPCNET_DEVICES="0,1,..." (or "all") or
 * lpcnet_mi355x_set_placement() name a list of placements, and each new
 * handle goes to the placement with the fewest live handles (one slot each
 * once a model is bound).  A list may name a device twice: two placements,
 * two pools, one GPU (the tests use this to exercise placement on a one-GPU
 * box).  LPCNET_DEVICE=d pins every new handle to device d. */
constexpr int kMaxPlace = 64;
constexpr int kPinned = 1 << 20;
constexpr int kDevDefault = -1; /* placement device resolved at the first model bind */
static std::mutex g_place_mu;
static std::vector<int> g_place_dev; /* placement -> device (empty: not set up yet) */
static int g_place_load[kMaxPlace];  /* live handles per placement (of generation g_place_gen) */
static unsigned g_place_gen = 1;     /* bumped by lpcnet_mi355x_set_placement */

static bool parse_device_list(const char *v, std::vector<int> &out)
{
  out.clear();
  while (v && *v) {
    char *end = nullptr;
    const long d = strtol(v, &end, 10);
    if (end == v || d < 0 || d > 1023) return false;
    out.push_back((int)d);
    v = end;
    while (*v == ',' || *v == ' ') v++;
  }
  return !out.empty() && out.size() <= (size_t)kMaxPlace;
}

/* the device of the default placement (starts the HIP runtime only under
 * LOCAL_RANK, to take the rank's device modulo the visible count) */
static int default_device()
{
  const char *lr = getenv("LOCAL_RANK");
  if (!lr || !*lr) return 0;
  const int r = atoi(lr), n = lpcnet_mi355x_device_count();
  return n > 0 && r > 0 ? r % n : 0;
}

/* the placement of a new handle (g_place_mu held); -1 (error set) when
 * LPCNET_DEVICES is malformed or names a device that is not visible */
static int place_new_handle(Handle *h)
{
  h->place_gen = g_place_gen;
  if (const char *d = getenv("LPCNET_DEVICE")) {
    h->device = atoi(d);
    h->place = kPinned + h->device;
    return 0;
  }
  if (g_place_dev.empty()) {
    const char *env = getenv("LPCNET_DEVICES");
    if (env && *env) {
      /* opt-in spreading: the list is checked against the visible devices
       * here, as lpcnet_mi355x_set_placement checks its own */
      std::vector<int> list;
      const int ndev = lpcnet_mi355x_device_count();
      if (strcmp(env, "all") == 0) {
        for (int k = 0; k < std::min(std::max(ndev, 1), kMaxPlace); k++) list.push_back(k);
      } else if (!parse_device_list(env, list)) {
        set_err("LPCNET_DEVICES: expected \"all\" or a comma-separated list of at most 64 device indices");
        return -1;
      }
      for (int d : list)
        if (d >= std::max(ndev, 1)) {
          set_err("LPCNET_DEVICES: device index outside the visible devices");
          return -1;
        }
      g_place_dev = list;
    } else {
      g_place_dev.assign(1, kDevDefault);
    }
  }
  int best = 0;
  for (int k = 1; k < (int)g_place_dev.size(); k++)
    if (g_place_load[k] < g_place_load[best]) best = k;
  g_place_load[best]++;
  h->place = best;
  h->device = g_place_dev[best];
  return 0;
}

static void unplace_handle(const Handle *h)
{
  std::lock_guard<std::mutex> lk(g_place_mu);
  if (h->place_gen == g_place_gen && h->place >= 0 && h->place < kMaxPlace && g_place_load[h->place] > 0)
    g_place_load[h->place]--;
}

static void handle_free(Handle *h)
{
  if (h->pool) pool_release(h->pool, h->slot);
  unplace_handle(h);
  delete h;
}

LPCNET_EXPORT int lpcnet_mi355x_set_placement(const int *devices, int n)
{
  if (n < 0 || n > kMaxPlace || (n > 0 && !devices)) { set_err("lpcnet_mi355x_set_placement: 0..64 devices"); return -1; }
  const int ndev = lpcnet_mi355x_device_count();
  for (int k = 0; k < n; k++)
    if (devices[k] < 0 || (ndev > 0 && devices[k] >= ndev)) {
      set_err("lpcnet_mi355x_set_placement: device index outside the visible devices");
      return -1;
    }
  /* live handles keep their device and pool; only handles initialised from
   * now on are counted against (and placed over) the new list */
  std::lock_guard<std::mutex> lk(g_place_mu);
  for (int k = 0; k < kMaxPlace; k++) g_place_load[k] = 0;
  g_place_gen++;
  g_place_dev.assign(devices, devices + n); /* n = 0: back to the default */
  return 0;
}

/* unregister st (if live) and release its device resources */
static void handle_deinit(LPCNetState *st)
{
  Handle *h = nullptr;
  {
    LiveShard &sh = live_shard(st);
    std::lock_guard<std::mutex> lk(sh.mu);
    auto it = sh.map.find(st);
    if (it != sh.map.end() && st->magic == kMagic && st->token == it->second->token) {
      h = it->second;
      sh.map.erase(it);
    }
  }
  if (h) handle_free(h);
  /* a later malloc may hand this block out again: leave nothing that looks live */
  st->magic = 0;
  st->token = 0;
}

LPCNET_EXPORT int lpcnet_get_size(void) { return (int)sizeof(LPCNetState); }

LPCNET_EXPORT int lpcnet_init(LPCNetState *st)
{
  if (!st) return -1;
  Handle *stale = nullptr, *live = nullptr;
  bool failed = false;
  {
    LiveShard &sh = live_shard(st);
    std::lock_guard<std::mutex> lk(sh.mu);
    auto it = sh.map.find(st);
    if (it != sh.map.end()) {
      if (st->magic == kMagic && st->token == it->second->token) {
        live = it->second;
      } else {
        stale = it->second;
        sh.map.erase(it);
      }
    }
    if (!live) {
      Handle *h = new Handle();
      h->token = new_token();
      int prc;
      {
        std::lock_guard<std::mutex> plk(g_place_mu);
        prc = place_new_handle(h);
      }
      if (prc) {
        delete h;
        st->magic = 0;
        st->token = 0;
        failed = true;
      } else {
        sh.map[st] = h;
        st->magic = kMagic;
        st->reserved = 0;
        st->token = h->token;
      }
    }
  }
  if (stale) handle_free(stale);
  if (failed) return -1;
  if (live) {
    /* src/lpcnet.c:184-200 ends with lpcnet_reset(): re-initialising a live
     * handle resets its stream and keeps its device binding and model */
    live->fbuf_fill = 0;
    if (live->pool) {
      StreamState s;
      host_reset_state(s);
      if (pool_slot_io(live->pool, live->slot, nullptr, &s)) return -1;
    }
  }
  return 0;
}

LPCNET_EXPORT LPCNetState *lpcnet_create(void)
{
  LPCNetState *st = (LPCNetState *)calloc(1, sizeof(LPCNetState));
  if (st && lpcnet_init(st) != 0) {
    free(st);
    return nullptr;
  }
  return st;
}

LPCNET_EXPORT void lpcnet_destroy(LPCNetState *st)
{
  if (!st) return;
  handle_deinit(st);
  free(st);
}

LPCNET_EXPORT void lpcnet_mi355x_deinit(LPCNetState *st)
{
  if (st) handle_deinit(st);
}

LPCNET_EXPORT void lpcnet_reset(LPCNetState *st)
{
  Handle *h = live_handle(st);
  if (!h) return;
  h->fbuf_fill = 0; /* lpcnet.c:177-179 clears from LPCNET_RESET_START, the feature buffer included */
  if (!h->pool) return;
  StreamState s;
  host_reset_state(s);
  pool_slot_io(h->pool, h->slot, nullptr, &s);
}

LPCNET_EXPORT int lpcnet_load_model(LPCNetState *st, const unsigned char *data, int len)
{
  Handle *h = live_handle(st);
  if (!h) { set_err("lpcnet_load_model: not an initialised LPCNetState"); return -1; }
  if (h->device == kDevDefault) h->device = default_device();
  /* pools per (model, placement, device): a placement index of a later
   * list may name another device */
  StatePool *p = pool_acquire(data, len, h->device, h->place >= kPinned ? h->place : h->place * 1024 + h->device);
  if (!p) return -1;
  if (p == h->pool) {
    pool_release(p, -1); /* same model: keep the binding */
    return 0;
  }
  /* the model changes, the stream state stays (lpcnet.c:202-210 only binds arrays) */
  StreamState s;
  bool have = h->pool && pool_slot_io(h->pool, h->slot, &s, nullptr) == 0;
  const int slot = pool_alloc_slot(p, have ? &s : nullptr);
  if (slot < 0) {
    pool_release(p, -1);
    return -1;
  }
  if (h->pool) pool_release(h->pool, h->slot);
  h->pool = p;
  h->slot = slot;
  return 0;
}

/* run one request on st's slot; the void entry points report failure as the
 * reference cannot: silence out, lpcnet_mi355x_last_error(), one stderr line */
static int handle_run(LPCNetState *st, Req &r, const char *what)
{
  Handle *h = live_handle(st);
  int rc;
  if (!h || !h->pool) {
    set_err(std::string(what) +
            ": no model bound (call lpcnet_load_model first; liblpcnet_mi355x has no compiled-in model)");
    rc = -1;
  } else {
    r.slot = h->slot;
    rc = pool_submit(&h->pool->comb, r);
    if (rc) set_err(r.err);
  }
  if (rc != 0) {
    static std::atomic<bool> warned{false};
    const int nout = r.kind == StatePool::DECODE ? 4 * FRAME : r.N;
    if (r.out && nout > 0 && r.kind != StatePool::FLUSH) memset(r.out, 0, sizeof(short) * nout);
    if (!warned.exchange(true)) fprintf(stderr, "liblpcnet_mi355x: %s\n", last_err().c_str());
  }
  return rc;
}

static bool req_args_ok(const float *features, const short *output, int N, int preload, bool need_features)
{
  if (N < 0 || N > FRAME || (need_features && !features) || (N > 0 && !output) || preload < 0) {
    set_err("bad arguments");
    return false;
  }
  return true;
}

LPCNET_EXPORT void lpcnet_synthesize_impl(LPCNetState *st, const float *features, short *output, int N, int preload)
{
  if (!req_args_ok(features, output, N, preload, true)) return;
  Req r{-1, StatePool::SYNTH, features, nullptr, output, N, std::min(preload, N), 0, 0, std::string()};
  handle_run(st, r, "lpcnet_synthesize_impl");
}

LPCNET_EXPORT void lpcnet_synthesize(LPCNetState *st, const float *features, short *output, int N)
{
  if (!req_args_ok(features, output, N, 0, true)) {
    if (output && N > 0 && N <= FRAME) memset(output, 0, sizeof(short) * N);
    return;
  }
  Req r{-1, StatePool::SYNTH, features, nullptr, output, N, 0, 0, 0, std::string()};
  handle_run(st, r, "lpcnet_synthesize");
}

LPCNET_EXPORT void lpcnet_synthesize_tail_impl(LPCNetState *st, short *output, int N, int preload)
{
  if (!req_args_ok(nullptr, output, N, preload, false) || N == 0) return;
  Req r{-1, StatePool::TAIL, nullptr, nullptr, output, N, std::min(preload, N), 0, 0, std::string()};
  handle_run(st, r, "lpcnet_synthesize_tail_impl");
}

/* lpcnet.c:122-132: keep the last kernel_size(conv1) + kernel_size(conv2) - 2
 * frames (4 for the 3-tap convolutions of every LPCNet model) */
LPCNET_EXPORT void run_frame_network_deferred(LPCNetState *st, const float *features)
{
  Handle *h = live_handle(st);
  if (!h || !features) return;
  if (h->fbuf_fill == MAX_FEATURE_BUFFER)
    memmove(h->fbuf[0], h->fbuf[1], sizeof(float) * NF * (MAX_FEATURE_BUFFER - 1));
  else
    h->fbuf_fill++;
  memcpy(h->fbuf[h->fbuf_fill - 1], features, sizeof(float) * NF);
}

/* lpcnet.c:134-144: the frame network of every buffered frame, outputs into
 * locals (the state's conditioning and LPC stay), then an empty buffer */
LPCNET_EXPORT void run_frame_network_flush(LPCNetState *st)
{
  Handle *h = live_handle(st);
  if (!h || h->fbuf_fill == 0) return;
  float f[MAX_FEATURE_BUFFER][NF];
  memcpy(f, h->fbuf, sizeof(f));
  Req r{-1, StatePool::FLUSH, &f[0][0], nullptr, nullptr, 0, 0, h->fbuf_fill, 0, std::string()};
  h->fbuf_fill = 0;
  handle_run(st, r, "run_frame_network_flush");
}

/* lpcnet.c:226-233 */
LPCNET_EXPORT void lpcnet_reset_signal(LPCNetState *st)
{
  Handle *h = live_handle(st);
  if (!h || !h->pool) return;
  StreamState s;
  if (pool_slot_io(h->pool, h->slot, &s, nullptr)) return;
  reset_signal(s);
  pool_slot_io(h->pool, h->slot, nullptr, &s);
}

LPCNET_EXPORT int lpcnet_mi355x_handle_placement(const LPCNetState *st, int *device, int *placement)
{
  Handle *h = live_handle(st);
  if (!h) { set_err("not an initialised LPCNetState"); return -1; }
  /* before the first model bind the default placement's device is the one
   * lpcnet_load_model will take */
  if (device) *device = h->device == kDevDefault ? default_device() : h->device;
  if (placement) *placement = h->place >= kPinned ? -1 : h->place;
  return 0;
}

LPCNET_EXPORT int lpcnet_mi355x_state_size(void) { return (int)sizeof(HandleSnapshot); }

LPCNET_EXPORT int lpcnet_mi355x_state_save(LPCNetState *st, void *buf)
{
  Handle *h = live_handle(st);
  if (!h || !h->pool || !buf) { set_err("lpcnet_mi355x_state_save: no model bound or no buffer"); return -1; }
  HandleSnapshot snap;
  memset(&snap, 0, sizeof(snap));
  if (pool_slot_io(h->pool, h->slot, &snap.s, nullptr)) return -1;
  snap.fbuf_fill = h->fbuf_fill;
  memcpy(snap.fbuf, h->fbuf, sizeof(snap.fbuf));
  memcpy(buf, &snap, sizeof(snap));
  return 0;
}

LPCNET_EXPORT int lpcnet_mi355x_state_restore(LPCNetState *st, const void *buf)
{
  Handle *h = live_handle(st);
  if (!h || !h->pool || !buf) { set_err("lpcnet_mi355x_state_restore: no model bound or no buffer"); return -1; }
  HandleSnapshot snap;
  memcpy(&snap, buf, sizeof(snap));
  if (!snapshot_ok(&snap.s)) return -1;
  if (snap.fbuf_fill < 0 || snap.fbuf_fill > MAX_FEATURE_BUFFER) {
    set_err("snapshot feature buffer fill outside [0, 4]: not a state this engine produced");
    return -1;
  }
  if (pool_slot_io(h->pool, h->slot, nullptr, &snap.s)) return -1;
  h->fbuf_fill = snap.fbuf_fill;
  memcpy(h->fbuf, snap.fbuf, sizeof(h->fbuf));
  return 0;
}

LPCNET_EXPORT double lpcnet_mi355x_pool_run_ms(const LPCNetState *st)
{
  Handle *h = live_handle(st);
  if (!h || !h->pool) return -1.0;
  std::lock_guard<std::mutex> lk(h->pool->mu);
  return h->pool->comb.run_ns.load() * 1e-6;
}

LPCNET_EXPORT int lpcnet_mi355x_pool_stats(const LPCNetState *st, long *launches, long *requests, int *streams)
{
  Handle *h = live_handle(st);
  if (!h || !h->pool) return -1;
  StatePool *p = h->pool;
  {
    std::lock_guard<std::mutex> lk(p->mu);
    if (launches) *launches = p->comb.launches.load();
    if (requests) *requests = p->comb.requests.load();
  }
  if (streams) {
    std::lock_guard<std::mutex> lk(g_pools_mu);
    *streams = p->refs;
  }
  return 0;
}

/* ---- 1.6 kb/s decoder (include/lpcnet.h:63-100 of the reference) --------
 * LPCNetDecState embeds an LPCNetState as the reference's does
 * (lpcnet_private.h:50-53); vq_mem lives with the stream's device state. */
struct LPCNetDecState {
  LPCNetState lpcnet_state;
};

LPCNET_EXPORT int lpcnet_decoder_get_size(void) { return (int)sizeof(LPCNetDecState); }

/* lpcnet.c:290-295: memset + lpcnet_init.  A never-initialised (or stale)
 * decoder is zeroed and gets a fresh handle; a live one is re-initialised in
 * place (stream reset, model kept), as below */
LPCNET_EXPORT int lpcnet_decoder_init(LPCNetDecState *st)
{
  if (!st) return -1;
  /* re-initialising a live decoder resets its stream (vq_mem included:
   * host_reset_state) and keeps its model, as lpcnet_init does for a live
   * LPCNetState; only a never-initialised (or stale) one starts from zero */
  if (live_handle(&st->lpcnet_state)) return lpcnet_init(&st->lpcnet_state);
  memset(st, 0, sizeof(*st));
  return lpcnet_init(&st->lpcnet_state);
}

LPCNET_EXPORT LPCNetDecState *lpcnet_decoder_create(void)
{
  LPCNetDecState *st = (LPCNetDecState *)malloc(sizeof(LPCNetDecState));
  if (st && lpcnet_decoder_init(st) != 0) {
    free(st);
    return nullptr;
  }
  return st;
}

LPCNET_EXPORT void lpcnet_decoder_destroy(LPCNetDecState *st)
{
  if (!st) return;
  handle_deinit(&st->lpcnet_state);
  free(st);
}

LPCNET_EXPORT int lpcnet_mi355x_decoder_load_model(LPCNetDecState *st, const unsigned char *data, int len)
{
  if (!st) return -1;
  if (lpcnet_load_model(&st->lpcnet_state, data, len)) return -1;
  Handle *h = live_handle(&st->lpcnet_state);
  if (!h || !h->pool || !h->pool->has_codebooks) {
    set_err("lpcnet_decode needs the ceps_codebook1/2/3 / ceps_codebook_diff4 records in the blob");
    return -1;
  }
  return 0;
}

/* lpcnet.c:310-319: decode_packet, then lpcnet_synthesize of the 4 frames */
LPCNET_EXPORT int lpcnet_decode(LPCNetDecState *st, const unsigned char *buf, short *pcm)
{
  if (!st || !buf || !pcm) { set_err("bad arguments"); return -1; }
  Req r{-1, StatePool::DECODE, nullptr, buf, pcm, 4 * FRAME, 0, 0, 0, std::string()};
  return handle_run(&st->lpcnet_state, r, "lpcnet_decode") ? -1 : 0;
}

}  // extern "C"
