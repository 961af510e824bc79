/*
 * pool_combiner.h -- the lock-free flat combiner of a drop-in StatePool
 * (dropin.cpp): concurrent single-stream calls coalesce into one launch.
 * Host-only, no device call: the launch is a callback given at construction,
 * so tools/pool_combiner_check.cpp drives the same code on the CPU with a
 * fake one.
 */
#ifndef LPCNET_POOL_COMBINER_H
#define LPCNET_POOL_COMBINER_H

#include <stdint.h>

#include <atomic>
#include <mutex>
#include <string>
#include <vector>

namespace lpcnet_mi355x {

/* the states of Req::state */
enum : uint32_t { REQ_WAITING = 0, REQ_DONE = 1, REQ_COMBINE = 2 };

struct Req {
  int slot;
  int kind;                    /* StatePool::Kind */
  const float *feat;           /* SYNTH [NF], FLUSH [nfr][NF] */
  const unsigned char *packet; /* DECODE [8] */
  short *out;                  /* SYNTH / TAIL [N] (the first `preload` are input), DECODE [4 * FRAME] */
  int N, preload, nfr;
  int rc = 0;
  std::string err;
  Req *next = nullptr;          /* the pool's inbox (a lock-free stack) */
  /* REQ_WAITING -> REQ_DONE (rc / err set) or REQ_COMBINE (the caller now
   * holds the pool): the caller sleeps on this word (futex), the notifier
   * stores it last */
  std::atomic<uint32_t> state{0};
  bool same_shape(const Req &o) const { return kind == o.kind && N == o.N && preload == o.preload && nfr == o.nfr; }
};

struct PoolCombiner {
  /* one coalesced step for requests rq (all of the same shape), run by the
   * combiner alone: 0, or -1 with `err` filled */
  using Launch = int (*)(void *ctx, const std::vector<Req *> &rq, std::string &err);
  PoolCombiner(Launch launch_, void *ctx_) : launch(launch_), ctx(ctx_) {}
  const Launch launch;
  void *const ctx;
  /* Submission is lock-free: a request is pushed on `inbox` and its caller
   * either takes `busy` (0 -> 1) and combines, or sleeps on its request until
   * a combiner completes it or hands it the pool.  The combiner alone drains
   * the inbox, runs the launch and updates expect_n. */
  std::atomic<Req *> inbox{nullptr};
  std::atomic<uint32_t> busy{0};       /* 1: a combiner or a slot I/O holds the pool */
  std::atomic<int> io_waiting{0};      /* slot I/O callers waiting: no new combiner takes the pool */
  std::atomic<uint32_t> arrivals{0};   /* requests pushed and not drained yet */
  std::atomic<uint32_t> win_target{0}; /* a combiner waits for this many arrivals (0: none waits) */
  int expect_n = 0;                    /* requests of the previous launch (combiner-owned) */
  /* broadcast wake-ups (LPCNET_POOL_BROADCAST): waiters sleep on wake_seq,
   * the combiner marks its completed requests and wakes them all at once */
  bool broadcast = false;
  std::atomic<uint32_t> wake_seq{0};
  int window_us = 0;                   /* LPCNET_POOL_WINDOW_US */
  /* statistics (tests / diagnostics) */
  std::atomic<long> launches{0}, requests{0};
  std::atomic<long long> run_ns{0}; /* time inside the launches themselves */
};

/* Slot I/O on an idle pool (lock held for the slot bookkeeping): takes
 * `busy` -- meanwhile no new combiner takes the pool, so a stream of
 * synthesis calls cannot starve it -- and on scope exit lets go (to any
 * requests that arrived meanwhile).  No combiner takes the pool's mutex, so
 * holding it while waiting cannot deadlock. */
struct PoolIdle {
  PoolCombiner *p;
  PoolIdle(PoolCombiner *p_, std::unique_lock<std::mutex> &);
  ~PoolIdle();
};

/* run r on the pool, in this thread's launch or another's: r.rc, with r.err
 * filled when it is not 0 */
int pool_submit(PoolCombiner *p, Req &r);

}  // namespace lpcnet_mi355x

#endif
