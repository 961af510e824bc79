/*
 * pool_combiner_check.cpp -- the drop-in pools' flat combiner
 * (lpcnet_amd/csrc/pool_combiner.cpp) under many threads with a fake launch,
 * on the CPU.  A stand-alone program over that one host-only object:
 *
 *   make check        (builds and runs tools/pool_combiner_check)
 *   tools/pool_combiner_check [threads [calls]]      default 16 2000
 *
 * Every thread is one slot and makes `calls` calls that cycle through three
 * request shapes, one of which makes the launch fail with a fixed message;
 * thread 0 also takes the pool for slot I/O (PoolIdle) every 50th call.  The
 * launch checks that it is never entered twice at once, that it holds one
 * shape and no slot twice, bumps a plain per-slot counter into the request's
 * `out` and sleeps about 30 us.  The run repeats for (gather window us,
 * broadcast wake-ups) = (50, off), (0, off), (200, on).  It passes when every
 * call got its own rc and message and a fresh `out`, every request ran
 * exactly once, and the pool ends empty and free.  A lost wake-up would hang
 * it: a watchdog ends the program with a message instead.
 *
 * The plain counters and the variable touched under PoolIdle are what
 * ThreadSanitizer watches: a launch racing another launch, a slot I/O or a
 * caller's read of its result is a report.  Under the sanitizers:
 *
 *   mkdir -p build_san
 *   g++ -O1 -g -std=c++17 -fsanitize=thread -Ilpcnet_amd/csrc -o build_san/pool_combiner_check_tsan \
 *       tools/pool_combiner_check.cpp lpcnet_amd/csrc/pool_combiner.cpp -lpthread
 *   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -Ilpcnet_amd/csrc \
 *       -o build_san/pool_combiner_check_asan tools/pool_combiner_check.cpp lpcnet_amd/csrc/pool_combiner.cpp -lpthread
 *   build_san/pool_combiner_check_tsan && build_san/pool_combiner_check_asan
 *
 * Exit status 0 and one "pool_combiner_check ok" line when every check holds.
 */
#include <signal.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#include <atomic>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "pool_combiner.h"

using namespace lpcnet_mi355x;

/* Plain build: 0.5 s on 8 CPUs, ThreadSanitizer 3 s; a loaded machine with
 * fewer CPUs gets two orders of magnitude before a run counts as hung. */
static const unsigned kWatchdogSeconds = 300;

static const char kFailMessage[] = "fake launch: this shape fails";

static std::atomic<int> fails{0};

#define CHECK(cond, ...)                                    \
  do {                                                      \
    if (!(cond)) {                                          \
      if (fails.fetch_add(1) < 20) {                        \
        fprintf(stderr, "line %d: %s: ", __LINE__, #cond);  \
        fprintf(stderr, __VA_ARGS__);                       \
        fprintf(stderr, "\n");                              \
      }                                                     \
    }                                                       \
  } while (0)

/* shape s of a request: (kind, N); shape 2 fails */
static const int kShape[3][2] = {{0, 160}, {0, 80}, {1, 160}};

struct FakePool {
  explicit FakePool(int T) : count(T, 0) {}
  std::atomic<int> inside{0}; /* launches running now */
  std::vector<long> count;    /* launches that carried each slot: plain, the combiner's exclusion guards it */
  long touched = 0;           /* plain: every launch and every slot I/O bumps it */
  long launches = 0;
};

static int fake_launch(void *ctx, const std::vector<Req *> &rq, std::string &err)
{
  FakePool *f = (FakePool *)ctx;
  CHECK(f->inside.fetch_add(1) == 0, "two launches at once");
  CHECK(!rq.empty(), "empty launch");
  std::vector<char> seen(f->count.size(), 0);
  for (Req *q : rq) {
    CHECK(q->same_shape(*rq[0]), "two shapes in one launch");
    CHECK(q->slot >= 0 && q->slot < (int)seen.size() && !seen[q->slot], "slot %d twice in one launch", q->slot);
    seen[q->slot] = 1;
    *q->out = (short)++f->count[q->slot];
  }
  f->touched++;
  f->launches++;
  struct timespec ts = {0, 30000};
  nanosleep(&ts, nullptr);
  f->inside.fetch_sub(1);
  if (rq[0]->kind != kShape[2][0]) return 0;
  err = kFailMessage;
  return -1;
}

static void run_mode(int T, int M, int window_us, bool broadcast)
{
  FakePool f(T);
  PoolCombiner comb(fake_launch, &f);
  comb.window_us = window_us;
  comb.broadcast = broadcast;
  std::mutex mu; /* a StatePool's slot bookkeeping lock */
  std::vector<std::thread> th;
  for (int t = 0; t < T; t++)
    th.emplace_back([&, t]() {
      for (int i = 0; i < M; i++) {
        if (t == 0 && i % 50 == 49) {
          std::unique_lock<std::mutex> lk(mu);
          PoolIdle idle(&comb, lk);
          CHECK(f.inside.load() == 0, "slot I/O beside a launch");
          f.touched++;
        }
        const int *shape = kShape[(i + t) % 3];
        short out = -1;
        Req r{t, shape[0], nullptr, nullptr, &out, shape[1], 0, 0, 0, std::string()};
        const int rc = pool_submit(&comb, r);
        const bool fail = shape == kShape[2];
        CHECK(rc == (fail ? -1 : 0) && rc == r.rc, "thread %d call %d: rc %d", t, i, rc);
        CHECK(r.err == (fail ? kFailMessage : ""), "thread %d call %d: message \"%s\"", t, i, r.err.c_str());
        /* this slot's requests run once each, in order: the i-th leaves i + 1 */
        CHECK(out == (short)(i + 1), "thread %d call %d: out %d (stale, or a request ran twice)", t, i, out);
      }
    });
  for (std::thread &x : th) x.join();
  const long calls = (long)T * M;
  long sum = 0;
  for (long c : f.count) sum += c;
  CHECK(sum == calls, "%ld requests ran, %ld calls", sum, calls);
  CHECK(comb.requests.load() == calls, "requests statistic %ld, %ld calls", comb.requests.load(), calls);
  CHECK(comb.launches.load() == f.launches, "launches statistic %ld, %ld launches", comb.launches.load(), f.launches);
  CHECK(comb.inbox.load() == nullptr, "inbox not empty at the end");
  CHECK(comb.busy.load() == 0, "pool still held at the end");
  CHECK(comb.arrivals.load() == 0, "arrivals %u at the end", comb.arrivals.load());
  CHECK(f.touched == f.launches + (M / 50), "plain variable %ld, expected %ld", f.touched, f.launches + M / 50);
  printf("window %3d us broadcast %d: %ld calls in %ld launches\n", window_us, (int)broadcast, calls, f.launches);
}

static void on_alarm(int)
{
  static const char msg[] = "pool_combiner_check: watchdog: a call never returned (lost wake-up?)\n";
  if (write(2, msg, sizeof(msg) - 1)) {}
  _exit(3);
}

int main(int argc, char **argv)
{
  const int T = argc > 1 ? atoi(argv[1]) : 16, M = argc > 2 ? atoi(argv[2]) : 2000;
  if (T < 1 || T > 4096 || M < 1 || M > 30000) {
    fprintf(stderr, "usage: pool_combiner_check [threads 1..4096 [calls 1..30000]]\n");
    return 2;
  }
  signal(SIGALRM, on_alarm);
  alarm(kWatchdogSeconds);
  run_mode(T, M, 50, false);
  run_mode(T, M, 0, false);
  run_mode(T, M, 200, true);
  if (fails.load()) {
    fprintf(stderr, "pool_combiner_check: %d checks failed\n", fails.load());
    return 1;
  }
  printf("pool_combiner_check ok: %d threads x %d calls x 3 modes\n", T, M);
  return 0;
}
