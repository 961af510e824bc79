/*
 * device_mem_check.cpp -- the owners, the table uploads, the carver and the
 * state rows of lpcnet_amd/csrc/device_mem.h over a fake backend, on the CPU.
 * A stand-alone program over that one header: it defines the backend's free
 * functions itself, with malloc and free, a table of live allocations, a log
 * of every allocation's kind and size, and "fail the k-th allocation" and
 * "fail the k-th copy".
 *
 *   make check        (builds and runs tools/device_mem_check)
 *
 * It checks that
 *  - DeviceTables::upload makes one allocation per present entry, in list
 *    order, of the entry's bytes (16 for an empty entry), that every present
 *    dst receives a distinct address and the contents arrive, and that a
 *    non-present entry's dst stays as it was;
 *  - for every k, an upload whose k-th allocation, or whose k-th copy, fails
 *    returns -1, leaves as many allocations live as before the call, and
 *    leaves the tables the object already held in place with their contents;
 *    the same for zeroed();
 *  - Carver's parts are 256-byte aligned and in order, and a failed alloc
 *    leaves the planned pointers untouched and nothing live;
 *  - every owner type (DevPtr, PinnedPtr, DevStream, DevEvent, DeviceTables,
 *    a carved group, EventPool) releases each handle exactly once through
 *    moves, move assignments, swaps and resets: the fake aborts on a release
 *    of something not live, and a moved-from owner releases nothing;
 *  - rows_save then rows_restore round-trips 1, 2 and 3 parts, rows_zero of
 *    one stream leaves its neighbours alone, and rows_zero of all streams
 *    (stream < 0) covers exactly B rows;
 *  - nothing is live at the end.
 *
 * Under the sanitizers (a double free or a leak the table missed is a report):
 *
 *   mkdir -p build_san
 *   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -Ilpcnet_amd/csrc \
 *       -o build_san/device_mem_check_asan tools/device_mem_check.cpp
 *   build_san/device_mem_check_asan
 *
 * Exit status 0 and one "device_mem_check ok" line when every check holds.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "device_mem.h"

using namespace lpcnet_mi355x;

/* ---- the fake backend -------------------------------------------------------- */
namespace {

enum Kind { DEVICE, FINEGRAINED, PINNED, PINNED_MAPPED, STREAM, EVENT, EVENT_TIMING };
struct Alloc {
  Kind kind;
  size_t bytes;
};
std::map<void *, Alloc> live;
std::vector<Alloc> alloc_log;
int nalloc = 0, ncopy = 0;         /* calls so far */
int fail_alloc = -1, fail_copy = -1; /* the call (0-based, counted from arm()) that fails; -1: none */
int failures = 0;

void arm(int alloc_k, int copy_k)
{
  nalloc = ncopy = 0;
  fail_alloc = alloc_k;
  fail_copy = copy_k;
}

void *fake_alloc(Kind kind, size_t bytes)
{
  if (nalloc++ == fail_alloc) return nullptr;
  void *p = malloc(bytes ? bytes : 1);
  memset(p, 0xA5, bytes); /* device memory starts as garbage */
  live[p] = {kind, bytes};
  alloc_log.push_back({kind, bytes});
  return p;
}

void fake_free(void *p, bool pinned, bool handle)
{
  auto it = live.find(p);
  if (it == live.end()) {
    fprintf(stderr, "device_mem_check: release of %p, which is not live (double free?)\n", p);
    abort();
  }
  const Kind k = it->second.kind;
  const bool is_pinned = k == PINNED || k == PINNED_MAPPED, is_handle = k == STREAM || k == EVENT || k == EVENT_TIMING;
  if (is_pinned != pinned || is_handle != handle) {
    fprintf(stderr, "device_mem_check: %p released as the wrong kind\n", p);
    abort();
  }
  live.erase(it);
  free(p);
}

#define CHECK(c)                                                              \
  do {                                                                        \
    if (!(c)) {                                                               \
      fprintf(stderr, "device_mem_check: %s:%d: %s\n", __FILE__, __LINE__, #c); \
      failures++;                                                             \
    }                                                                         \
  } while (0)

}  // namespace

namespace lpcnet_mi355x {

void *dm_alloc(size_t bytes) { return fake_alloc(DEVICE, bytes); }
void *dm_alloc_finegrained(size_t bytes) { return fake_alloc(FINEGRAINED, bytes); }
void dm_free(void *p) { fake_free(p, false, false); }
void *dm_alloc_pinned(size_t bytes, bool mapped) { return fake_alloc(mapped ? PINNED_MAPPED : PINNED, bytes); }
void dm_free_pinned(void *p) { fake_free(p, true, false); }
int dm_upload(void *dst, const void *src, size_t bytes)
{
  if (ncopy++ == fail_copy) return -1;
  memcpy(dst, src, bytes);
  return 0;
}
int dm_download(void *dst, const void *src, size_t bytes)
{
  if (ncopy++ == fail_copy) return -1;
  memcpy(dst, src, bytes);
  return 0;
}
int dm_zero(void *dst, size_t bytes, DevStreamHandle)
{
  memset(dst, 0, bytes);
  return 0;
}
int dm_stream_sync(DevStreamHandle) { return 0; }
DevStreamHandle dm_stream_create() { return (DevStreamHandle)fake_alloc(STREAM, 1); }
void dm_stream_destroy(DevStreamHandle s) { fake_free(s, false, true); }
DevEventHandle dm_event_create(bool timing) { return (DevEventHandle)fake_alloc(timing ? EVENT_TIMING : EVENT, 1); }
void dm_event_destroy(DevEventHandle e) { fake_free(e, false, true); }

}  // namespace lpcnet_mi355x

/* ---- an upload list ------------------------------------------------------------ */
namespace {

struct Tables {
  const char *a = nullptr, *absent = (const char *)0x10, *empty = nullptr, *b = nullptr, *c = nullptr;
};
const char SRC_A[40] = "the first table of the upload list.....";
const char SRC_B[300] = "the second";
const char SRC_C[7] = "third!";

std::vector<ModelUpload> upload_list(Tables &t)
{
  return {{&t.a, SRC_A, sizeof(SRC_A), true},
          {&t.absent, SRC_A, sizeof(SRC_A), false},
          {&t.empty, nullptr, 0, true},
          {&t.b, SRC_B, sizeof(SRC_B), true},
          {&t.c, SRC_C, sizeof(SRC_C), true}};
}
constexpr int LIST_ALLOCS = 4, LIST_COPIES = 3;

bool tables_intact(const Tables &t)
{
  return t.a && t.b && t.c && t.empty && !memcmp(t.a, SRC_A, sizeof(SRC_A)) && !memcmp(t.b, SRC_B, sizeof(SRC_B)) &&
         !memcmp(t.c, SRC_C, sizeof(SRC_C));
}

void check_upload()
{
  arm(-1, -1);
  alloc_log.clear();
  {
    DeviceTables T;
    Tables t;
    CHECK(T.upload(upload_list(t)) == 0);
    CHECK(T.size() == LIST_ALLOCS && live.size() == LIST_ALLOCS);
    CHECK(tables_intact(t));
    CHECK(t.absent == (const char *)0x10);
    const char *all[4] = {t.a, t.empty, t.b, t.c};
    for (int i = 0; i < 4; i++) {
      CHECK(live.count((void *)all[i]) == 1);
      for (int j = 0; j < i; j++) CHECK(all[i] != all[j]);
    }
    /* list order, upload_model's sizes */
    const size_t want[LIST_ALLOCS] = {sizeof(SRC_A), 16, sizeof(SRC_B), sizeof(SRC_C)};
    CHECK(alloc_log.size() == LIST_ALLOCS);
    for (size_t i = 0; i < alloc_log.size() && i < LIST_ALLOCS; i++) CHECK(alloc_log[i].kind == DEVICE && alloc_log[i].bytes == want[i]);
    /* zeroed: a buffer of its own, all zero */
    const unsigned char *z = (const unsigned char *)T.zeroed(100);
    CHECK(z && T.size() == LIST_ALLOCS + 1);
    for (int i = 0; z && i < 100; i++) CHECK(z[i] == 0);
    T.clear();
    CHECK(live.empty() && T.size() == 0);
  }
  CHECK(live.empty());
}

/* the k-th allocation (copies = false) or the k-th copy of a second upload
 * fails: -1, nothing more live than before, the first upload untouched */
void check_upload_failures(bool copies)
{
  const int n = copies ? LIST_COPIES : LIST_ALLOCS;
  for (int k = 0; k < n; k++) {
    arm(-1, -1);
    DeviceTables T;
    Tables held, t;
    CHECK(T.upload(upload_list(held)) == 0);
    const size_t before = live.size();
    arm(copies ? -1 : k, copies ? k : -1);
    CHECK(T.upload(upload_list(t)) == -1);
    CHECK(live.size() == before && T.size() == LIST_ALLOCS);
    CHECK(tables_intact(held));
    CHECK(live.count((void *)held.a) && live.count((void *)held.empty) && live.count((void *)held.b) && live.count((void *)held.c));
    if (!copies) {
      arm(0, -1);
      CHECK(T.zeroed(64) == nullptr && live.size() == before && T.size() == LIST_ALLOCS);
    }
    /* and the object still takes an upload */
    arm(-1, -1);
    CHECK(T.upload(upload_list(t)) == 0 && tables_intact(t) && tables_intact(held) && live.size() == 2 * before);
  }
  CHECK(live.empty());
}

/* ---- the carver ------------------------------------------------------------------ */
struct Group {
  DevPtr<char> base;
  double *d = nullptr;
  char *c = nullptr;
  short *s = nullptr;
  float *f = nullptr;
};

void plan(Carver &c, Group &g)
{
  c.add(g.d, 3);   /* 24 bytes -> 256 */
  c.add(g.c, 257); /* -> 512 */
  c.add(g.s, 128); /* exactly 256 */
  c.add(g.f, 1);
}

void check_carver()
{
  arm(-1, -1);
  {
    Group g;
    Carver c;
    plan(c, g);
    CHECK(c.size() == 256 + 512 + 256 + 256);
    g.base = c.alloc();
    char *base = g.base;
    CHECK(base && live.size() == 1 && live.begin()->second.bytes == c.size());
    CHECK((char *)g.d == base && g.c == base + 256 && (char *)g.s == base + 768 && (char *)g.f == base + 1024);
    for (const void *p : {(const void *)g.d, (const void *)g.c, (const void *)g.s, (const void *)g.f})
      CHECK(((uintptr_t)p - (uintptr_t)base) % 256 == 0);
    /* a group is freed by assigning {} */
    g = {};
    CHECK(live.empty() && !g.base && !g.d);
  }
  {
    Group g;
    g.d = (double *)0x100;
    g.f = (float *)0x200;
    Carver c;
    plan(c, g);
    arm(0, -1);
    g.base = c.alloc();
    CHECK(!g.base && live.empty());
    CHECK(g.d == (double *)0x100 && g.f == (float *)0x200 && !g.c && !g.s);
  }
  arm(-1, -1);
}

/* ---- moves and swaps --------------------------------------------------------------- */
/* `make` fills an owner; each handle must be released exactly once (the fake
 * aborts otherwise) and at the point the test expects */
template <class O, class Make>
void check_owner(Make make)
{
  arm(-1, -1);
  {
    O a;
    CHECK(!a);
    CHECK(make(a) == 0 && a && live.size() == 1);
    void *const pa = (void *)a;
    O b(std::move(a)); /* move construction */
    CHECK(!a && (void *)b == pa && live.size() == 1);
    O c;
    c = std::move(b); /* move assignment into an empty owner */
    CHECK(!b && (void *)c == pa && live.size() == 1);
    O d;
    CHECK(make(d) == 0 && live.size() == 2);
    void *const pd = (void *)d;
    c.swap(d);
    CHECK((void *)c == pd && (void *)d == pa && live.size() == 2);
    c = std::move(d); /* move assignment over a held handle: releases pd, once */
    CHECK(!d && (void *)c == pa && live.size() == 1 && live.count(pa) == 1);
    O &self = c;
    c = std::move(self); /* self-assignment keeps it */
    CHECK((void *)c == pa && live.size() == 1);
    CHECK(make(c) == 0 && live.size() == 1 && live.count((void *)c) == 1); /* a second alloc releases the first */
    c.reset();
    CHECK(!c && live.empty());
    c.reset(); /* twice is once */
    CHECK(make(c) == 0 && live.size() == 1);
  } /* a, b, d: moved from or reset, release nothing; c releases its own */
  CHECK(live.empty());
}

void check_moves()
{
  check_owner<DevPtr<float>>([](DevPtr<float> &p) { return p.alloc(10); });
  check_owner<DevPtr<char>>([](DevPtr<char> &p) { return p.alloc_finegrained(10); });
  check_owner<PinnedPtr<short>>([](PinnedPtr<short> &p) { return p.alloc(10, true); });
  check_owner<PinnedPtr<int>>([](PinnedPtr<int> &p) { return p.alloc(10, false); });
  check_owner<DevStream>([](DevStream &s) { return s.create(); });
  check_owner<DevEvent>([](DevEvent &e) { return e.create(false); });
  /* a failed allocation leaves an empty owner */
  arm(0, -1);
  DevPtr<int> p;
  CHECK(p.alloc(4) == -1 && !p && live.empty());
  arm(-1, -1);
  /* tables: the replan's commit.  The new stand beside the old, which go
   * with the assignment; a moved-from object holds nothing */
  {
    DeviceTables cur, fresh;
    Tables t0, t1;
    CHECK(cur.upload(upload_list(t0)) == 0 && fresh.upload(upload_list(t1)) == 0 && live.size() == 2 * LIST_ALLOCS);
    cur = std::move(fresh);
    CHECK(live.size() == LIST_ALLOCS && fresh.size() == 0 && cur.size() == LIST_ALLOCS);
    CHECK(tables_intact(t1) && live.count((void *)t1.a) && !live.count((void *)t0.a));
    DeviceTables other;
    other.swap(cur);
    CHECK(cur.size() == 0 && other.size() == LIST_ALLOCS && live.size() == LIST_ALLOCS);
    DeviceTables last(std::move(other));
    CHECK(other.size() == 0 && last.size() == LIST_ALLOCS && live.size() == LIST_ALLOCS);
  }
  CHECK(live.empty());
  /* a carved group moves as a whole */
  {
    Group g, h;
    Carver c;
    plan(c, g);
    g.base = c.alloc();
    h = std::move(g);
    CHECK(!g.base && h.base && live.size() == 1);
  }
  CHECK(live.empty());
  /* the timing events: taken, recycled, reused, all destroyed with the pool */
  {
    EventPool pool;
    DevEventHandle e0 = pool.take(), e1 = pool.take();
    CHECK(e0 && e1 && e0 != e1 && live.size() == 2 && pool.taken.size() == 2);
    for (const auto &kv : live) CHECK(kv.second.kind == EVENT_TIMING);
    pool.recycle();
    CHECK(pool.taken.empty() && pool.idle.size() == 2 && live.size() == 2);
    DevEventHandle e2 = pool.take();
    CHECK((e2 == e0 || e2 == e1) && live.size() == 2 && pool.taken.size() == 1 && pool.idle.size() == 1);
    arm(0, -1);
    pool.take();                        /* the idle one: no allocation */
    CHECK(pool.take() == nullptr && pool.taken.size() == 2); /* none to be had: nothing recorded */
    arm(-1, -1);
  }
  CHECK(live.empty());
}

/* ---- state rows ---------------------------------------------------------------------- */
void check_rows()
{
  arm(-1, -1);
  const int B = 5;
  const size_t sz[3] = {12, 256, 7};
  for (int parts = 1; parts <= 3; parts++) {
    DevPtr<unsigned char> mem[3];
    std::vector<StateRows> rows;
    size_t total = 0;
    for (int k = 0; k < parts; k++) {
      CHECK(mem[k].alloc(B * sz[k]) == 0);
      for (size_t i = 0; i < B * sz[k]; i++) mem[k][i] = (unsigned char)(1 + (i * 7 + k * 31) % 250); /* never 0 */
      rows.push_back({mem[k], sz[k]});
      total += sz[k];
    }
    std::vector<unsigned char> before[3];
    for (int k = 0; k < parts; k++) before[k].assign((unsigned char *)mem[k], mem[k] + B * sz[k]);
    /* save stream 3: the parts back to back */
    std::vector<unsigned char> snap(total + 1, 0xEE);
    CHECK(rows_save(rows, 3, snap.data(), nullptr) == 0);
    size_t off = 0;
    for (int k = 0; k < parts; k++) {
      CHECK(!memcmp(&snap[off], &before[k][3 * sz[k]], sz[k]));
      off += sz[k];
    }
    CHECK(off == total && snap[total] == 0xEE);
    /* zero stream 3: its neighbours stay */
    CHECK(rows_zero(rows, 3, B, nullptr) == 0);
    for (int k = 0; k < parts; k++)
      for (size_t i = 0; i < B * sz[k]; i++) CHECK(mem[k][i] == (i / sz[k] == 3 ? 0 : before[k][i]));
    /* restore it: everything as before */
    CHECK(rows_restore(rows, 3, snap.data(), nullptr) == 0);
    for (int k = 0; k < parts; k++) CHECK(!memcmp(mem[k], before[k].data(), B * sz[k]));
    /* restore into another stream: that stream alone changes */
    CHECK(rows_restore(rows, 0, snap.data(), nullptr) == 0);
    for (int k = 0; k < parts; k++) {
      CHECK(!memcmp(mem[k], &before[k][3 * sz[k]], sz[k]));
      CHECK(!memcmp(mem[k] + sz[k], &before[k][sz[k]], (B - 1) * sz[k]));
    }
    /* a failing copy is reported */
    arm(-1, parts - 1);
    CHECK(rows_save(rows, 1, snap.data(), nullptr) == -1);
    arm(-1, 0);
    CHECK(rows_restore(rows, 1, snap.data(), nullptr) == -1);
    arm(-1, -1);
  }
  /* zero all: exactly B rows of a buffer that holds B + 1 */
  {
    DevPtr<unsigned char> m;
    const size_t row = 24;
    CHECK(m.alloc((B + 1) * row) == 0);
    memset(m, 0x5A, (B + 1) * row);
    CHECK(rows_zero({{m, row}}, -1, B, nullptr) == 0);
    for (size_t i = 0; i < (B + 1) * row; i++) CHECK(m[i] == (i < B * row ? 0 : 0x5A));
  }
  CHECK(live.empty());
}

}  // namespace

int main()
{
  check_upload();
  check_upload_failures(false);
  check_upload_failures(true);
  check_carver();
  check_moves();
  check_rows();
  CHECK(live.empty());
  if (failures) {
    fprintf(stderr, "device_mem_check: %d check(s) failed\n", failures);
    return 1;
  }
  printf("device_mem_check ok: uploads, %d + %d injected failures, carver, owners, state rows; nothing live\n", LIST_ALLOCS, LIST_COPIES);
  return 0;
}
