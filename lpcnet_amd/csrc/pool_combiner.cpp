/*
 * pool_combiner.cpp -- flat combining with a hand-off over futex words: the
 * submission side of a drop-in StatePool (pool_combiner.h).  Host-only: no
 * device call, the launch is the pool's callback.  It reports through
 * Req::rc / Req::err alone; the thread's last error is its caller's business
 * (dropin.cpp handle_run).
 */
#include "pool_combiner.h"

#include <linux/futex.h>
#include <sys/syscall.h>
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>

namespace lpcnet_mi355x {

/* Per-request wake-up: the caller sleeps on its request's state word, the
 * notifier stores the word (release) and wakes that one thread -- one
 * syscall, no lock the woken thread has to take.  The caller may return as
 * soon as it sees the store, so the wake can land on a word whose frame is
 * gone: a futex wake on a stale address wakes at most a waiter that rechecks
 * its own condition, or fails with EFAULT, both harmless. */
static void futex_wake(std::atomic<uint32_t> *w, int n)
{
  syscall(SYS_futex, (uint32_t *)w, FUTEX_WAKE_PRIVATE, n, nullptr, nullptr, 0);
}

/* sleep while *w == v, at most `ns` nanoseconds (0: no limit) */
static void futex_wait(std::atomic<uint32_t> *w, uint32_t v, long long ns = 0)
{
  struct timespec ts;
  if (ns > 0) {
    ts.tv_sec = (time_t)(ns / 1000000000);
    ts.tv_nsec = (long)(ns % 1000000000);
  }
  syscall(SYS_futex, (uint32_t *)w, FUTEX_WAIT_PRIVATE, v, ns > 0 ? &ts : nullptr, nullptr, 0);
}

static void req_post(PoolCombiner *p, Req *q, uint32_t v)
{
  std::atomic<uint32_t> *w = &q->state;
  w->store(v, std::memory_order_release);
  if (p->broadcast) {
    p->wake_seq.fetch_add(1, std::memory_order_release);
    futex_wake(&p->wake_seq, INT32_MAX);
  } else {
    futex_wake(w, 1);
  }
}

/* r's state once it leaves `from` */
static uint32_t req_wait(PoolCombiner *p, Req &r, uint32_t from = REQ_WAITING)
{
  uint32_t v;
  if (p->broadcast) {
    for (;;) {
      const uint32_t seq = p->wake_seq.load(std::memory_order_acquire);
      if ((v = r.state.load(std::memory_order_acquire)) != from) return v;
      futex_wait(&p->wake_seq, seq);
    }
  }
  while ((v = r.state.load(std::memory_order_acquire)) == from) futex_wait(&r.state, from);
  return v;
}

static void inbox_push(PoolCombiner *p, Req *q)
{
  Req *h = p->inbox.load(std::memory_order_relaxed);
  do q->next = h;
  /* seq_cst: pairs with pool_let_go's busy = 0 / inbox re-load (a
   * store-then-load hand-off on both sides; release alone would let the
   * let-go miss this push while our busy CAS still sees it held) */
  while (!p->inbox.compare_exchange_weak(h, q, std::memory_order_seq_cst, std::memory_order_relaxed));
}

/* The holder of `busy` lets go: to the slot I/O callers waiting, else to the
 * caller of the newest inbox request (REQ_COMBINE: `busy` stays held on its
 * behalf; no one else drains the inbox meanwhile), else to no one -- with a
 * recheck, since a request pushed just before the release found the pool
 * busy and sleeps. */
static void pool_let_go(PoolCombiner *p)
{
  for (;;) {
    if (p->io_waiting.load(std::memory_order_acquire) > 0) {
      p->busy.store(0, std::memory_order_release);
      futex_wake(&p->busy, INT32_MAX);
      return;
    }
    Req *h = p->inbox.load(std::memory_order_acquire);
    if (h) {
      req_post(p, h, REQ_COMBINE);
      return;
    }
    p->busy.store(0, std::memory_order_seq_cst);
    if (!p->inbox.load(std::memory_order_seq_cst)) return;
    uint32_t b = 0;
    if (!p->busy.compare_exchange_strong(b, 1, std::memory_order_seq_cst)) return; /* another caller took it */
  }
}

PoolIdle::PoolIdle(PoolCombiner *p_, std::unique_lock<std::mutex> &) : p(p_)
{
  p->io_waiting.fetch_add(1, std::memory_order_seq_cst);
  for (;;) {
    uint32_t b = 0;
    if (p->busy.compare_exchange_strong(b, 1, std::memory_order_seq_cst)) break;
    futex_wait(&p->busy, 1, 1000000); /* woken by the combiner's let-go; re-polled every ms */
  }
  p->io_waiting.fetch_sub(1, std::memory_order_seq_cst);
}

PoolIdle::~PoolIdle() { pool_let_go(p); }

/* Flat combining with a hand-off, lock-free on the submission side: the
 * caller pushes its request and either takes the idle pool or sleeps on its
 * request.  The combiner waits (the gather window) until as many requests
 * have arrived as the previous launch carried, drains the inbox, runs every
 * request of the oldest one's shape, wakes exactly the callers it completed,
 * and lets the pool go -- to the newest pending request's caller if any (the
 * GPU idles until it launches).  No mutex on this path: with hundreds of C
 * threads, waking callers that then queue on one lock costs more than the
 * launch. */
static int pool_combine(PoolCombiner *p, Req &r)
{
  while (r.state.load(std::memory_order_acquire) != REQ_DONE) {
    const int expect = p->expect_n;
    if (p->window_us > 0 && expect > 1 && (int)p->arrivals.load(std::memory_order_acquire) < expect) {
      const auto until = std::chrono::steady_clock::now() + std::chrono::microseconds(p->window_us + 2 * expect);
      p->win_target.store((uint32_t)expect, std::memory_order_seq_cst);
      for (;;) {
        const uint32_t a = p->arrivals.load(std::memory_order_seq_cst);
        if ((int)a >= expect) break;
        const long long left = std::chrono::duration_cast<std::chrono::nanoseconds>(until - std::chrono::steady_clock::now()).count();
        if (left <= 0) break;
        futex_wait(&p->arrivals, a, left);
      }
      p->win_target.store(0, std::memory_order_relaxed);
    }
    /* drain: the stack reversed is arrival order */
    Req *h = p->inbox.exchange(nullptr, std::memory_order_acquire);
    std::vector<Req *> all;
    for (; h; h = h->next) all.push_back(h);
    if (all.empty()) {
      /* r ran in the launch of the combiner that let the pool go to us: it
       * still posts r's completion, so r's frame must outlive that store */
      /* r's state is read once: the other combiner may post REQ_DONE at any
       * moment, and waiting "while state == DONE" would never end */
      const uint32_t s = r.state.load(std::memory_order_acquire);
      pool_let_go(p);
      if (s != REQ_DONE) req_wait(p, r, s);
      return r.rc;
    }
    std::reverse(all.begin(), all.end());
    p->arrivals.fetch_sub((uint32_t)all.size(), std::memory_order_acq_rel);
    std::vector<Req *> mine, rest;
    for (Req *q : all) (q->same_shape(*all[0]) ? mine : rest).push_back(q);
    /* oldest first onto the stack: the next drain's reversal gives arrival
     * order again */
    for (auto it = rest.begin(); it != rest.end(); ++it) {
      inbox_push(p, *it);
      p->arrivals.fetch_add(1, std::memory_order_acq_rel);
    }
    const auto t0 = std::chrono::steady_clock::now();
    std::string e;
    const int rc = p->launch(p->ctx, mine, e);
    p->run_ns.fetch_add(std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count());
    p->launches.fetch_add(1);
    p->requests.fetch_add((long)mine.size());
    p->expect_n = (int)mine.size();
    bool self = false;
    for (Req *q : mine) {
      q->rc = rc;
      q->err = e;
      if (q == &r) self = true;
    }
    if (self) r.state.store(REQ_DONE, std::memory_order_release);
    /* the next launch first (the GPU idles until it starts), then the
     * wake-ups: one futex call per completed caller */
    auto post_all = [&]() {
      if (p->broadcast) {
        bool any = false;
        for (Req *q : mine)
          if (q != &r) {
            q->state.store(REQ_DONE, std::memory_order_release);
            any = true;
          }
        if (any) {
          p->wake_seq.fetch_add(1, std::memory_order_release);
          futex_wake(&p->wake_seq, INT32_MAX);
        }
      } else {
        for (Req *q : mine)
          if (q != &r) req_post(p, q, REQ_DONE);
      }
    };
    if (self) {
      pool_let_go(p);
      post_all();
      return r.rc;
    }
    post_all();
  }
  pool_let_go(p);
  return r.rc;
}

int pool_submit(PoolCombiner *p, Req &r)
{
  inbox_push(p, &r);
  const uint32_t a = p->arrivals.fetch_add(1, std::memory_order_seq_cst) + 1;
  const uint32_t t = p->win_target.load(std::memory_order_seq_cst);
  if (t && a >= t) futex_wake(&p->arrivals, 1);
  if (p->io_waiting.load(std::memory_order_seq_cst) == 0) {
    uint32_t b = 0;
    if (p->busy.compare_exchange_strong(b, 1, std::memory_order_seq_cst)) return pool_combine(p, r);
  }
  if (req_wait(p, r) == REQ_DONE) return r.rc;
  return pool_combine(p, r); /* REQ_COMBINE: the pool was handed over */
}

}  // namespace lpcnet_mi355x
